"""The row-wise probes of tests/rowwise_probes.py would notice the failures they target (CPU only).

Every honest oracle passes its own rule inside an intact cage, an honest fp32 emulation that reduces in another
order passes one_step, and every mutant is rejected by the rule and the family meant for it:

  reduction   one element left out / counted twice, a whole 16-byte slot left out: rejected in EVERY row of the
              spike walks (RMSNorm, LayerNorm), by construction.
  per-head    the same for the per-head RMSNorm of qknorm_rope_kv_write (128-wide heads, 8 threads a head):
              an element, a thread's share or half of it left out, an element counted twice, the divisor
              120, in every row of the 16-row walk with and without the bias; eps left out or added after the
              root in every row of the eps heads.
  divisor     d - 8: rejected by the walks at d <= 520 (the outputs move by 4 / d: 0.8 % at 512).  At d >= 4096
              the shift is below a quarter of a bf16 code, one_step cannot see it, and the ``decided`` rule on
              the random rows does (up to d = 8192, where 4 / d is still twice its margin).  Divisor rounded up
              to threads * 8: the walks at d = 520 and 1000.
  eps         left out / added after the root: the eps rows.
  rounding    norm taken from the unrounded fp32 x + r, store by truncation: the pinned rows, bitwise.  Store by
              round-half-up and a residual that is not updated: the residual rows' stream, bitwise (a tie at
              the norm's own store cannot be constructed through an rsqrt).
  mix-ups     weight read one vector over: random weights; a row normalised with its neighbour's inv: the
              spread rows.
  LayerNorm   wrong count for the mean, pre_bias dropped / added twice, residual dropped; one-pass variance:
              the offset rows 100 + 0.5 {0, 1} the GPU file runs (rejected in the rows the test prints, at least
              4 of 16 at every width used).
  RoPE        interleaved pairs, sin sign, table row +-1, table column shifted by 8, q rotated under
              rope_q=False: the exact family, bitwise; qknorm rounding to bf16 after the bias (bitwise, exact
              family) or after the norm (the model's tables, where a second rounding moves outputs two codes).
  caches      V token-major, off & 3 and off >> 2 exchanged, a padding row written to slot 0, K heads
              transposed with offsets, one stray write.
  SwiGLU      gate and up exchanged, [gate | up] read where block = 32 was asked for; sigmoid rounded to bf16
              (never two codes off: rejected by ``decided``, accepted by one_step).
  quantisers  amax over the first 2048 elements, 240 for 448, truncation, the neighbouring row's scale.

The last tests record why the probes exist: which of these mutants the N(0, 1) inputs and bounds of
tests/test_kernels_gpu.py accept."""
import functools

import pytest
import torch

from tests import rowwise_probes as rp
from tests.rowwise_probes import BF, bits, bitwise, one_step, rne

WALK_DS = [512, 520, 1000, 2048, 4096, 8192]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 17)


def _accepts(out, want, rule="one_step", mag=None, err=rp.NORM_ERR):
    cage = rp.RowCage(out.shape)
    cage.load(out)
    return not rp.violations(cage, want, rule, mag, err)


def _rows_rejected(out, want):
    return one_step(out, want).any(1)


@functools.lru_cache(maxsize=None)
def _walk(d):
    x, cols = rp.spike_walk(d)
    return x, cols, rp.weights(d, _gen(d))


@pytest.mark.parametrize("d", WALK_DS + [8, 8200, 32768])
def test_spike_walk_is_what_it_claims(d):
    chunks = rp.walk_chunks(d)
    assert sorted(s for c in chunks for s in c) == list(range(d // 8)) and max(len(c) for c in chunks) <= 512
    x, cols = rp.spike_walk(d, chunks[0])                                    # (wide walks: the first 512 rows)
    assert x.shape[0] == len(chunks[0]) and (d > 4096 or x.shape[0] == d // 8)
    assert bool(((x != 0).sum(1) == 2).all()) and bool((x[:, rp.FIXED_COL] == rp.SPIKE).all())
    assert bool((x[torch.arange(len(cols)), cols].abs() == rp.SPIKE).all())
    assert sorted(set((cols // 8).tolist())) == chunks[0]                    # one row per slot
    if d >= 64:
        assert set((cols % 8).tolist()) == set(range(8))                     # every position inside a vector
    m = rp.SPIKE
    assert m != 2.0 ** torch.tensor(m).log2().round()                        # not a power of two


@pytest.mark.parametrize("d", WALK_DS)
def test_rms_walk_rejects_reduction_mutants_in_every_row(d):
    x, cols, w = _walk(d)
    want = rp.rms(x, w, 1e-5)
    assert _accepts(rne(want), want) and _accepts(rp.rms_fp32(x, w, 1e-5), want)
    h = x.double()
    ss = (h * h).sum(1, keepdim=True)
    walker = h[torch.arange(len(cols)), cols][:, None] ** 2
    fixed = h[:, rp.FIXED_COL][:, None] ** 2
    slot = torch.stack([(h[i, (c // 8) * 8:(c // 8) * 8 + 8] ** 2).sum() for i, c in enumerate(cols.tolist())])[:, None]
    for name, ss_m in [("walker dropped", ss - walker), ("fixed dropped", ss - fixed), ("walker twice", ss + walker),
                       ("fixed twice", ss + fixed), ("slot dropped", ss - slot)]:
        out = rne(rp.rms(x, w, 1e-5, ss=ss_m))
        assert bool(_rows_rejected(out, want).all()), (name, d)
        # every non-zero output moves by at least 18 %
        nz = want != 0
        assert float(((out.double() - want).abs() / want.abs())[nz].min()) > 0.17, (name, d)


def test_rms_divisor_mutants():
    for d in (512, 520):
        x, cols, w = _walk(d)
        want = rp.rms(x, w, 1e-5)
        assert not _accepts(rne(rp.rms(x, w, 1e-5, div=d - 8)), want), d
    for d in (4096, 8192):   # a 4 / d shift is inside one code: one_step is blind to it, the decided codes are not
        x, w = rp.random_rows(5, d, _gen(d, 12)), rp.weights(d, _gen(d))
        want = rp.rms(x, w, 1e-5)
        out = rne(rp.rms(x, w, 1e-5, div=d - 8))
        assert _accepts(out, want) and not _accepts(out, want, "decided"), d
        assert _accepts(rne(want), want, "decided") and rp.decided_share(want) > 0.85
        for chunk in (8, 64):
            assert _accepts(rp.rms_fp32(x, w, 1e-5, chunk), want, "decided"), d
    for d, threads in ((520, 128), (1000, 128)):
        x, cols, w = _walk(d)
        want = rp.rms(x, w, 1e-5)
        assert bool(_rows_rejected(rne(rp.rms(x, w, 1e-5, div=threads * 8)), want).all()), d


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_eps_rows_reject_eps_mutants(eps):
    d = 512
    x, w = rp.eps_rows(5, d, _gen(d, 1)), rp.weights(d, _gen(d))
    want = rp.rms(x, w, eps)
    ms = (x.double() ** 2).mean(1, keepdim=True)
    assert float(ms.max()) < 1e-4 * eps                                      # eps is the radicand
    assert _accepts(rne(want), want) and _accepts(rp.rms_fp32(x, w, eps), want)
    assert not _accepts(rne(rp.rms(x, w, 0.0)), want)                         # eps left out
    after = x.double() / (ms.sqrt() + eps) * w.double()
    assert not _accepts(rne(after), want)                                     # eps added after the root


@pytest.mark.parametrize("d", [512, 4096, 8192])
def test_fp32_emulation_in_another_order_is_within_one_code(d):
    """The measurement the one_step rule rests on: share of outputs off by one code, none by more."""
    w = rp.weights(d, _gen(d))
    for spread in (False, True):
        x = rp.random_rows(37, d, _gen(d, spread), spread)
        want = rp.rms(x, w, 1e-5)
        for chunk in (8, 64):
            got = rp.rms_fp32(x, w, 1e-5, chunk)
            st = rp.steps(got, want)
            assert int(st.max()) <= 1 and float((st == 1).double().mean()) < 1e-3, (d, spread, chunk)


def test_residual_rows_and_stream_mutants():
    d = 512
    x, r = rp.residual_rows(7, d, _gen(d, 2))
    s64 = x.double() + r.double()
    assert bool((s64.float().double() == s64).all())                          # the fp32 sum is exact
    h = rp.stream(x, r)
    up, down = torch.arange(d) % 4 == 1, torch.arange(d) % 4 == 3
    assert bool((h[:, up].float().abs() == 1 + 2.0 ** -6).all()) and bool((h[:, down].float().abs() == 1).all())
    assert not bool(bitwise(h, h).any())
    assert bool(bitwise(rp.store_trunc(s64), h)[:, up].all())                 # truncation misses every upward tie
    assert bool(bitwise(rp.store_half_up(s64), h)[:, down].all())             # half-up every downward tie
    assert bool(bitwise(r, h).any(1).all())                                   # residual not updated
    # the norm of the stream, pinned: bitwise, and one code lower at every upward tie from the unrounded sum
    w = rp.pow2_weights(d)
    want = rp.pinned(h, w)
    eps32 = float(torch.tensor(rp.PIN_EPS, dtype=torch.float32))
    assert eps32 == rp.PIN_EPS
    honest32 = ((h.float() * torch.rsqrt(torch.tensor(eps32))) * w.float())
    assert _accepts(rne(honest32), want, "bitwise")
    assert _accepts(rne(rp.rms(h, w, rp.PIN_EPS)), want, "bitwise")
    for tilt in (1 - 2.0 ** -22, 1 + 2.0 ** -22):                             # a few ulps of rsqrt either way
        assert _accepts(rne(honest32 * tilt), want, "bitwise")
    unrounded = rne(rp.rms(s64, w, rp.PIN_EPS))
    assert bool(bitwise(unrounded, want)[:, up].all()) and _accepts(unrounded, want, "one_step")
    assert not _accepts(rp.store_trunc(rp.rms(h, w, rp.PIN_EPS)), want, "bitwise")


def test_weight_and_row_mixups():
    d = 2048
    w = rp.weights(d, _gen(d))
    x = rp.random_rows(9, d, _gen(d, 3), spread=True)
    want = rp.rms(x, w, 1e-5)
    assert not _accepts(rne(rp.rms(x, w.roll(-8), 1e-5)), want)                # weight one vector over
    inv = torch.rsqrt((x.double() ** 2).mean(1, keepdim=True) + 1e-5)
    swapped = inv.clone()
    swapped[1], swapped[2] = inv[2], inv[1]                                   # rows 1 and 2 of a 4-row workgroup
    out = rne(x.double() * swapped * w.double())
    rej = _rows_rejected(out, want)
    assert bool(rej[1]) and bool(rej[2]) and int(rej.sum()) == 2


def test_rowsumsq_family_is_exact():
    for d in (8, 520, 4096):
        x = rp.small_int_rows(5, d, _gen(d, 4))
        ss = (x.double() ** 2).sum(1)
        assert bool((ss.float().double() == ss).all()) and float(ss.max()) < 2 ** 24
        assert bool((x.float().flip(1) ** 2).sum(1).equal(ss.float()))


@pytest.mark.parametrize("d", [256, 520, 1024, 2048])
def test_layernorm_walk_and_mutants(d):
    x, cols = rp.spike_walk(d, offset=rp.LN_OFFSET)
    gen = _gen(d, 5)
    g, b = rp.weights(d, gen, 0.2), (0.2 * torch.randn(d, generator=gen)).to(BF)
    want, mag = rp.layernorm(x, g, b, 1e-12)
    assert _accepts(rne(want), want, "one_step_cond", mag)
    R = x.shape[0]
    for name, col, times in [("walker dropped", cols, 0.0), ("fixed dropped", None, 0.0), ("walker twice", cols, 2.0)]:
        # the element enters both sums ``times`` times: same as a row whose element is reweighted
        h = x.double()
        c = cols if col is not None else torch.full((R,), rp.FIXED_COL)
        e = h[torch.arange(R), c]
        s = h.sum(1) + (times - 1) * e
        mean = (s / d)[:, None]
        dev = (h - mean) ** 2
        var = (dev.sum(1) + (times - 1) * dev[torch.arange(R), c])[:, None] / d
        out = (h - mean) * torch.rsqrt(var + 1e-12) * g.double() + b.double()
        bad, _ = rp.one_step_cond(rne(out), want, mag)
        assert bool(bad.any(1).all()), (name, d)
    bad, _ = rp.one_step_cond(rne(rp.layernorm(x, g, b, 1e-12, count=d - 8)[0]), want, mag)
    assert bool(bad.any()), d


def test_layernorm_constant_rows_give_the_bias():
    d = 520
    x = torch.tensor([3.0, -5.0, 0.0, 7.0])[:, None].expand(4, d).to(BF).contiguous()
    gen = _gen(d, 6)
    g, b = rp.weights(d, gen, 0.2), (0.2 * torch.randn(d, generator=gen)).to(BF)
    want, _ = rp.layernorm(x, g, b, 1e-12)
    assert not bool(bitwise(rne(want), b.expand(4, d)).any())
    s = x.float().sum(1)
    assert bool((s / d == x[:, 0].float()).all())                             # the fp32 mean is the constant


def test_layernorm_operand_mutants():
    d, rows = 768, 5
    gen = _gen(d, 7)
    x, r = rp.random_rows(rows, d, gen), rp.random_rows(rows, d, gen)
    pb = (torch.randn(d, generator=gen)).to(BF)
    g, b = rp.weights(d, gen, 0.2), (0.2 * torch.randn(d, generator=gen)).to(BF)
    want, mag = rp.layernorm(x, g, b, 1e-12, r=r, pb=pb)
    assert _accepts(rne(want), want, "one_step_cond", mag)
    for name, kw in [("pre_bias dropped", dict(r=r)), ("pre_bias twice", dict(r=r, pb=(pb.double() * 2))),
                     ("residual dropped", dict(pb=pb))]:
        out = rne(rp.layernorm(x, g, b, 1e-12, **kw)[0])
        assert not _accepts(out, want, "one_step_cond", mag), name


@pytest.mark.parametrize("d", rp.LN_OFFSET_DS)
def test_layernorm_one_pass_variance_on_offset_rows(d):
    """The very rows the GPU file runs (rp.ln_offset_case): 16 rows 100 + 0.5 {0, 1} per width.  An fp32
    E[h^2] - mean^2 is off by more than a code in the rows the test prints, at least 4 of the 16 at every width
    used; d = 8 exposes none and is not used, nor are rows around 256, which do not expose it either."""
    rows = 16
    x, g, b = rp.ln_offset_case(d, rows)
    want, mag = rp.layernorm(x, g, b, 1e-12)
    assert _accepts(rne(want), want, "one_step_cond", mag)
    bad, _ = rp.one_step_cond(rne(rp.layernorm(x, g, b, 1e-12, one_pass=True)[0]), want, mag)
    exposed = bad.any(1).nonzero().flatten().tolist()
    assert len(exposed) >= 4, exposed
    x8, g8, b8 = rp.ln_offset_case(8)
    w8, m8 = rp.layernorm(x8, g8, b8, 1e-12)
    assert not bool(rp.one_step_cond(rne(rp.layernorm(x8, g8, b8, 1e-12, one_pass=True)[0]), w8, m8)[0].any())
    x256 = rp.offset_rows(rows, d, _gen(d, 8), base=256.0)
    w256, m256 = rp.layernorm(x256, g, b, 1e-12)
    bad256, _ = rp.one_step_cond(rne(rp.layernorm(x256, g, b, 1e-12, one_pass=True)[0]), w256, m256)
    print("d =", d, "one-pass variance exposed in rows", exposed, "of 100 + 0.5 {0, 1};", int(bad256.any(1).sum()), "rows at 256")


# ---------------------------------------------------------------------------------------------------------
# RoPE, qk-norm, caches


def _rope_case(D=128, Hq=8, Hkv=2, T=21, P=64, exact=True):
    gen = _gen(D, Hq, Hkv, T)
    W = (Hq + 2 * Hkv) * D
    qkv = rp.exact_values((T, W), gen) if exact else torch.randn(T, W, generator=gen).to(BF)
    cos, sin = rp.synthetic_tables(P, D // 2, gen)
    pos = rp.probe_positions(T, P, gen)
    return qkv, cos, sin, pos, gen


def _real_tables(P, D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).double() / D))
    ang = torch.arange(P).double()[:, None] * inv[None, :]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 2), (64, 3, 1), (16, 3, 1)])
def test_rope_exact_family_rejects_indexing_mutants(D, Hq, Hkv):
    qkv, cos, sin, pos, gen = _rope_case(D, Hq, Hkv)
    assert 0 in pos.tolist() and 1 in pos.tolist() and cos.shape[0] - 1 in pos.tolist()
    want = rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True)
    assert bool((want.qkv.float().double() == want.qkv).all())                # the rotation is exact in fp32
    assert _accepts(rne(want.qkv), want.qkv, "bitwise")
    muts = [dict(pairs="interleaved"), dict(sin_sign=-1.0), dict(row_shift=1), dict(row_shift=-1)]
    if D >= 32:
        muts.append(dict(col_shift=8))
    for mut in muts:
        out = rne(rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True, **mut).qkv)
        assert not _accepts(out, want.qkv, "bitwise"), mut
    # q rotated under rope_q=False
    want_k = rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, False)
    assert not bool(bitwise(rne(want_k.qkv[:, :Hq * D]), qkv[:, :Hq * D]).any())
    out = rne(rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, False, rotate_q_anyway=True).qkv)
    assert not _accepts(out, want_k.qkv, "bitwise")


def test_real_tables_are_well_conditioned_and_reject_mutants():
    D, Hq, Hkv, T, P = 128, 8, 2, 21, 256
    qkv, _, _, pos, gen = _rope_case(D, Hq, Hkv, T, P, exact=False)
    cos, sin = _real_tables(P, D)
    want = rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True)
    assert _accepts(rne(want.qkv), want.qkv, "one_step_cond", want.mag, rp.ROPE_ERR)
    assert _accepts(_rope_fp32(qkv, pos, cos, sin, Hq, Hkv, D), want.qkv, "one_step_cond", want.mag, rp.ROPE_ERR)
    for mut in (dict(pairs="interleaved"), dict(sin_sign=-1.0), dict(row_shift=1), dict(col_shift=8)):
        out = rne(rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True, **mut).qkv)
        assert not _accepts(out, want.qkv, "one_step_cond", want.mag, rp.ROPE_ERR), mut


def _rope_fp32(qkv, pos, cos, sin, Hq, Hkv, D):
    """rope_kv_write (rope_q, no slots) in fp32 arithmetic: two products and a sum, each rounded, one bf16 store."""
    T = qkv.shape[0]
    x = qkv.float().view(T, Hq + 2 * Hkv, D)
    c, s = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    x1, x2 = x[:, :Hq + Hkv, : D // 2], x[:, :Hq + Hkv, D // 2:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    return torch.cat([rot, x[:, Hq + Hkv:]], 1).reshape(T, -1).to(BF)


def test_fp32_emulations_break_plain_one_step_where_terms_cancel():
    """Why one_step_cond exists.  Outputs built to cancel (x1 = bf16(k sin), x2 = bf16(k cos), so x1 cos - x2 sin
    is the rounding residue; a LayerNorm bias of -bf16(t g) of row 0): an honest fp32 evaluation is several codes
    from the fp64 oracle there, and within one_step_cond everywhere."""
    D, Hq, Hkv, T, P = 128, 8, 2, 64, 256
    qkv, _, _, pos, gen = _rope_case(D, Hq, Hkv, T, P, exact=False)
    cos, sin = _real_tables(P, D)
    x = qkv.float().view(T, Hq + 2 * Hkv, D).clone()
    k = torch.randn(T, Hq + Hkv, D // 2, generator=gen)
    c, s = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    x[:, :Hq + Hkv, : D // 2] = k * s
    x[:, :Hq + Hkv, D // 2:] = k * c
    qkv = x.reshape(T, -1).to(BF)
    want = rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True)
    emu = _rope_fp32(qkv, pos, cos, sin, Hq, Hkv, D)
    far = rp.steps(emu, want.qkv)
    assert int(far.max()) > 1 and not _accepts(emu, want.qkv, "one_step")
    bad, share = rp.one_step_cond(emu, want.qkv, want.mag, rp.ROPE_ERR)
    assert not bool(bad.any())                                                 # (half the outputs cancel here)
    print("rope: fp32 emulation up to", int(far.max()), "codes off on", int((far > 1).sum()), "of", far.numel())
    # LayerNorm
    d, rows = 8192, 3
    gen = _gen(d, 13)
    xr = rp.random_rows(rows, d, gen)
    g = rp.weights(d, gen, 0.2)
    t = rp.layernorm(xr, g, torch.zeros(d, dtype=BF), 1e-12)[0]
    b = (0.2 * torch.randn(d, generator=gen)).to(BF)
    b = -rne(t[0])                                                             # row 0 cancels in every column
    want, mag = rp.layernorm(xr, g, b, 1e-12)
    h = xr.float()
    mean = h.sum(1, keepdim=True) / d
    dev = h - mean
    emu = (dev * torch.rsqrt((dev * dev).sum(1, keepdim=True) / d + torch.tensor(1e-12)) * g.float() + b.float()).to(BF)
    far = rp.steps(emu, want)
    assert int(far.max()) > 1 and not _accepts(emu, want, "one_step")
    assert not bool(rp.one_step_cond(emu, want, mag)[0].any())                 # (a third of the outputs cancel here)
    print("layernorm: fp32 emulation up to", int(far.max()), "codes off on", int((far > 1).sum()), "of", far.numel())


def test_qknorm_single_rounding_mutants():
    D, Hq, Hkv, T, P = 128, 8, 2, 21, 64
    qkv, cos, sin, pos, gen = _rope_case(D, Hq, Hkv, T, P)
    bias = rp.exact_values(((Hq + 2 * Hkv) * D,), gen)
    # bias only, exact tables: bitwise, and a rounding after the bias shows
    want = rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True, bias=bias, qknorm=True)
    assert bool((want.qkv.float().double() == want.qkv).all())
    assert _accepts(rne(want.qkv), want.qkv, "bitwise")
    twice = rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True, bias=bias, qknorm=True, round_after="bias")
    assert not _accepts(rne(twice.qkv), want.qkv, "bitwise")
    # norms, the model's tables: a rounding after the norm moves some outputs by two codes
    rcos, rsin = _real_tables(P, D)
    qw, kw = rp.weights(D, gen), rp.weights(D, gen)
    x = torch.randn(qkv.shape, generator=gen).to(BF)
    for b in (None, bias):
        want = rp.rope_want(x, pos, rcos, rsin, None, Hq, Hkv, D, True, bias=b, qw=qw, kw=kw, qknorm=True)
        assert _accepts(rne(want.qkv), want.qkv, "one_step_cond", want.mag)
        twice = rp.rope_want(x, pos, rcos, rsin, None, Hq, Hkv, D, True, bias=b, qw=qw, kw=kw, qknorm=True,
                             round_after="norm")
        assert not _accepts(rne(twice.qkv), want.qkv, "one_step_cond", want.mag)


@pytest.mark.parametrize("BS", [16, 64])
def test_cache_mutants(BS):
    D, Hq, Hkv, NB = 64, 3, 2, 4
    T = 2 * BS + 3
    qkv, cos, sin, pos, gen = _rope_case(D, Hq, Hkv, T)
    slots = rp.probe_slots(T, NB, BS, gen, "padded")
    full = rp.probe_slots(T, NB, BS, gen)
    offs = lambda blk: sorted(int(s) % BS for s in full if int(s) // BS == blk)   # noqa: E731
    assert offs(0) == list(range(BS)) and offs(NB - 1) == list(range(BS))
    assert float((full[1:] - full[:-1]).abs().float().mean()) > BS            # neighbours land far apart
    want = rp.rope_want(qkv, pos, cos, sin, slots, Hq, Hkv, D, True)
    kc, vc, km, vm = rp.scatter(want.k, want.v, slots, NB, BS)
    assert int(km.sum()) == int((slots >= 0).sum()) * Hkv * D == int(vm.sum())
    assert not rp.cache_violations(kc, kc, km) and not rp.cache_violations(vc, vc, vm)
    for mut in (dict(v_layout="token_major"), dict(swap_off=True), dict(pad_to_zero=True), dict(k_transposed=True),
                dict(stray=True)):
        kc2, vc2, _, _ = rp.scatter(want.k, want.v, slots, NB, BS, **mut)
        v = rp.cache_violations(kc2, kc, km) + rp.cache_violations(vc2, vc, vm)
        assert v, mut
    # zero-filled caches and non-zero counting (the old check) cannot see a stray write of a value into a line
    # that is written anyway, nor tell sentinel from data: here the untouched share is checked bit for bit
    assert int((bits(kc)[~km] != rp.SENTINEL).sum()) == 0


@pytest.mark.parametrize("with_bias", [False, True])
def test_per_head_walk_rejects_reduction_mutants_in_every_row(with_bias):
    """The per-head RMSNorm of qknorm_rope_kv_write at position 0 of an identity table row is rms(head + bias):
    16 walk rows, the walker in each half of each of a head's 8 threads.  An element, a thread's 16 elements or a
    thread's 8 of one half left out, or an element counted twice, is rejected in every row."""
    D = rp.HEAD_D
    x, cols = rp.spike_walk(D)
    assert x.shape[0] == 16
    units = (cols % 64) // 8
    assert sorted(zip(units.tolist(), (cols >= 64).tolist())) == [(u, hi) for u in range(8) for hi in (False, True)]
    w = rp.weights(D, _gen(D, 14))
    h = x.double() + (rp.head_bias(1, 0, _gen(1))[:D].double() if with_bias else 0.0)
    for eps in (1e-6, 1e-5):
        want = rp.rms(h, w, eps)
        assert _accepts(rne(want), want) and _accepts(rp.rms_fp32(h, w, eps), want)
        ss = (h * h).sum(1, keepdim=True)
        R = torch.arange(16)
        walker, fixed = h[R, cols][:, None] ** 2, h[:, rp.FIXED_COL][:, None] ** 2
        lane = torch.stack([(h[i, 8 * u:8 * u + 8] ** 2).sum() + (h[i, 64 + 8 * u:72 + 8 * u] ** 2).sum()
                            for i, u in enumerate(units.tolist())])[:, None]
        half = torch.stack([(h[i, (c // 8) * 8:(c // 8) * 8 + 8] ** 2).sum() for i, c in enumerate(cols.tolist())])[:, None]
        for name, ss_m in [("walker dropped", ss - walker), ("fixed dropped", ss - fixed), ("walker twice", ss + walker),
                           ("lane dropped", ss - lane), ("half lane dropped", ss - half)]:
            out = rne(rp.rms(h, w, eps, ss=ss_m))
            assert bool(_rows_rejected(out, want).all()), (name, with_bias, eps)
            assert float(((out.double() - want).abs() / want.abs())[want != 0].min()) > 0.17, (name, with_bias)
        assert bool(_rows_rejected(rne(rp.rms(h, w, eps, div=D - 8)), want).all())   # 3 % at d = 128


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_per_head_eps_rows_reject_eps_mutants_in_every_row(eps):
    D = rp.HEAD_D
    x, w = rp.eps_rows(16, D, _gen(D, 15)), rp.weights(D, _gen(D, 14))
    want = rp.rms(x, w, eps)
    ms = (x.double() ** 2).mean(1, keepdim=True)
    assert float(ms.max()) < 1e-4 * eps
    assert _accepts(rne(want), want) and _accepts(rp.rms_fp32(x, w, eps), want)
    assert bool(_rows_rejected(rne(rp.rms(x, w, 0.0)), want).all())           # eps left out
    assert bool(_rows_rejected(rne(x.double() / (ms.sqrt() + eps) * w.double()), want).all())   # after the root


def test_per_head_families_reach_every_head_and_match_the_qkv_oracle():
    """head_qkv puts every row of a family into every q and k head, and at position 0 (identity table row) the
    qknorm oracle's q and k are rms(head + bias) per head: the two tests above speak about the kernel's output."""
    D, Hq, Hkv, T = rp.HEAD_D, 3, 1, 16
    gen = _gen(D, 16)
    heads, _ = rp.spike_walk(D)
    qkv = rp.head_qkv(heads, T, Hq, Hkv, gen)
    v = qkv.view(T, Hq + 2 * Hkv, D)
    for hd in range(Hq + Hkv):
        assert sorted(bits(v[:, hd]).tolist()) == sorted(bits(heads).tolist())
    cos, sin = rp.synthetic_tables(8, D // 2, gen)
    pos = torch.zeros(T, dtype=torch.int32)
    qw, kw = rp.weights(D, gen), rp.weights(D, gen)
    for bias in (None, rp.head_bias(Hq, Hkv, gen)):
        want = rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True, bias=bias, qw=qw, kw=kw, eps=1e-6, qknorm=True)
        got = want.qkv.view(T, Hq + 2 * Hkv, D)
        hb = v.double() + (0.0 if bias is None else bias.double().view(1, -1, D))
        for hd in range(Hq + Hkv):
            ref = rp.rms(hb[:, hd], qw if hd < Hq else kw, 1e-6)
            assert float((got[:, hd] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        assert bool(rp.well_conditioned(want.qkv, want.mag).all())            # nothing cancels: plain one_step


# ---------------------------------------------------------------------------------------------------------
# SwiGLU and quantisers


def test_silu_grid_and_mutants():
    grid = rp.silu_grid()
    assert float(grid.float().abs().max()) == 64 and int((bits(grid) == -32768).sum()) == 1 and bool((grid == 0).any())
    T, F = 3, 1024
    for block in (0, 32):
        gu, gate, up = rp.silu_inputs(T, F, block)
        assert set(bits(gate).flatten().tolist()) == set(bits(grid).tolist())
        assert bool((up > 0).any()) and bool((up < 0).any())
        want = rp.silu_mul(gate, up)
        assert _accepts(rne(want), want)
        g32, u32 = gate.float(), up.float()
        honest32 = g32 * (1 / (1 + torch.exp(-g32))) * u32
        assert _accepts(rne(honest32), want)
        assert not _accepts(rne(rp.silu_mul(up, gate)), want)                 # gate and up exchanged
        other = gu.view(T, 2, F)                                              # the [gate | up] reading of the buffer
        if block:
            assert not _accepts(rne(rp.silu_mul(other[:, 0], other[:, 1])), want)
        sig_bf = rne(torch.sigmoid(gate.double())).double()
        # sigmoid rounded to bf16 first: never two codes off (one_step is blind to it), but off the decided codes
        assert _accepts(rne(gate.double() * sig_bf * up.double()), want)
        assert not _accepts(rne(gate.double() * sig_bf * up.double()), want, "decided")
        assert _accepts(rne(want), want, "decided") and _accepts(rne(honest32), want, "decided")
        assert rp.decided_share(want) > 0.85


def test_quantiser_families_and_mutants():
    for d in (2048, 2056, 16392):
        x, cols = rp.amax_walk(d, rows=37)
        assert sorted(set((cols // 8).tolist()))[0] == 0 and int(cols.max()) // 8 == d // 8 - 1
        rest = x.float().abs().clone()
        rest[torch.arange(len(cols)), cols] = 0
        assert bool((rest.amax(1) * 2 <= x.float().abs().amax(1)).all())
        s = rp.scale_ref(x)
        q = rp.e4m3_codes(x, s)
        assert int(q.view(torch.float8_e4m3fn).float().abs().max()) == 448
        if d > 2048:   # amax over the first 2048 elements only: rows whose maximum lies beyond get another scale
            s2 = rp.scale_ref(x[:, :2048])
            assert bool((rp.ulps32(s2, s) > 1)[cols >= 2048].all()) and bool((cols >= 2048).any())
        assert bool((rp.ulps32(rp.scale_ref(x, 240.0), s) > 1).all())          # 240 for 448
        assert bool((rp.e4m3_codes_trunc(x, s) != q).any(1).all())            # truncation, in every row
        assert bool((rp.e4m3_codes(x, s.roll(1)) != q).any(1).all())          # the neighbouring row's scale
    # 448 (1 + 2^-23) still converts to 448
    assert float(torch.tensor(448.0 * (1 + 2.0 ** -23)).to(torch.float8_e4m3fn).float()) == 448.0
    # ties and subnormals: the scale is a power of two, the scaled values are the midpoints themselves
    x = rp.e4m3_tie_rows(7, 2056)
    s = rp.scale_ref(x)
    assert bool((s == torch.exp2((torch.arange(7) % 7 - 3).float())).all())
    scaled = x.float() / s[:, None]
    q = rp.e4m3_codes(x, s).view(torch.float8_e4m3fn).float()
    ties = (scaled - q).abs()[:, 1:]
    assert float((ties > 0).double().mean()) > 0.9                            # nearly every value sits on a midpoint
    assert bool(((q.abs() > 0) & (q.abs() < 2.0 ** -6)).any())                # e4m3 subnormals occur
    sub = rp.subnormal_rows(3, 64, _gen(1))
    assert float(sub.float().abs().max()) < 2.0 ** -126 and bool((sub.float() != 0).all())
    assert bool((rp.scale_ref(sub) == torch.tensor(1e-12) / 448).all())
    zero = torch.zeros(2, 64, dtype=BF)
    assert bool((rp.e4m3_codes(zero, rp.scale_ref(zero)) == 0).all())


# ---------------------------------------------------------------------------------------------------------
# what the N(0, 1) inputs and bounds of tests/test_kernels_gpu.py accept


def _old_close(a, b, atol, rtol):
    a, b = a.float(), b.float()
    return bool(((a - b).abs() <= atol + rtol * b.abs()).all())


def test_old_bounds_accept_the_marked_mutants():
    """test_rmsnorm (3e-2 + 2e-2 |y|), test_silu_mul_embedding (2e-2 + 2e-2 |y|) and test_rope_kv_write
    (2e-2 + 1e-2 |y|) on their own N(0, 1) inputs: the reduction and divisor mutants of RMSNorm and the bf16
    sigmoid pass.  The two RoPE mutants do NOT pass that bound on N(0, 1) inputs with the model's tables (a
    wrong pairing or table row moves low columns by whole radians); what the old RoPE test could not see is
    the other shapes and paths, the untouched cache and the rounding, not these two.  Recorded here as found."""
    d = 4096
    gen = _gen(d, 11)
    x = torch.randn(37, d, generator=gen).to(BF)
    w = (torch.randn(d, generator=gen) * 0.5).to(BF) + 1
    ref = rp.rms(x, w, 1e-5).float()
    h = x.double()
    ss = (h * h).sum(1, keepdim=True)
    big = h.abs().argmax(1)
    e = h[torch.arange(37), big][:, None] ** 2                                # even the row's largest element
    for name, out in [("dropped", rp.rms(x, w, 1e-5, ss=ss - e)), ("twice", rp.rms(x, w, 1e-5, ss=ss + e)),
                      ("d - 8", rp.rms(x, w, 1e-5, div=d - 8))]:
        assert _old_close(rne(out), ref, 3e-2, 2e-2), name
        assert int(rp.steps(rne(out), ref.double()).max()) <= 1, name          # at most one code from the truth
    gu = torch.randn(19, 2048, generator=gen).to(BF)
    g, u = gu.float().chunk(2, -1)
    sig_bf = rne(torch.sigmoid(g.double())).double()
    assert _old_close(rne(g.double() * sig_bf * u.double()), torch.nn.functional.silu(g) * u, 2e-2, 2e-2)
    # RoPE, exactly as test_rope_kv_write compares: llama-tiny, the model's own tables, tests/torch_ref.rope as the
    # reference, positions below 200, T = 21.  Even the share of outputs past the bound is large.
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import rope_tables
    from tests import torch_ref

    cfg = decoder_config("llama-tiny")
    D, Hq, Hkv, T = cfg.head_dim, cfg.heads, cfg.kv_heads, 21
    cos, sin = rope_tables(cfg, torch.device("cpu"), 256)
    for seed in range(5):
        gen = _gen(seed, 21)
        qkv = torch.randn(T, (Hq + 2 * Hkv) * D, generator=gen).to(BF)
        pos = torch.randint(0, 200, (T,), generator=gen).to(torch.int32)
        n = (Hq + Hkv) * D
        ref = torch_ref.rope(qkv[:, :n].view(T, Hq + Hkv, D), pos, cos, sin).reshape(T, n)
        honest = rne(rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True).qkv)[:, :n]
        assert _old_close(honest, ref, 2e-2, 1e-2)                             # the emulation of the old check is sound
        for mut in (dict(pairs="interleaved"), dict(row_shift=1), dict(row_shift=-1)):
            out = rne(rp.rope_want(qkv, pos, cos, sin, None, Hq, Hkv, D, True, **mut).qkv)[:, :n]
            past = ((out.float() - ref).abs() > 2e-2 + 1e-2 * ref.abs()).double().mean()
            assert float(past) > 0.05, (mut, seed, float(past))
