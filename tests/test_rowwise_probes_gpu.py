"""The row-wise kernels between the GEMMs under the exact inputs of tests/rowwise_probes.py: rmsnorm (workgroup
and wave kernel), rmsnorm_quant_fp8, layernorm (both kernels), rms_rowsumsq, rope_kv_write,
qknorm_rope_kv_write, silu_mul, silu_mul_quant_fp8, quant_fp8_rows, embedding, kv_gather, kv_block_copy.

The N(0, 1) inputs and the 2e-2 .. 4e-2 + 1 .. 2 % bounds of tests/test_kernels_gpu.py accept an RMSNorm that
leaves an element out of its sum of squares or divides by d - 8, cannot tell RNE from truncation, run RoPE at
one shape only and count non-zeros in zero-filled caches.  Here:

  spike walks     every 16-byte vector slot of a row carries, in one row of the walk, half of the row's energy:
                  a slot, lane or reduction stage that is skipped or counted twice moves that row by >= 18 %.
                  Widths the wave kernel takes run once whole (>= 256 rows) and once in chunks of 255 rows
                  (workgroup kernel).
  random rows     under ``decided``: one code at most, and the RNE code itself wherever the fp64 value is 2^-12
                  away from a midpoint (sees a divisor off by 8 at d = 4096 and 8192).
  eps rows, residual rows (stream bitwise, ties in both directions), pinned rows (norm output bitwise: taken
                  from the bf16-rounded stream, RNE at the store).
  LayerNorm       walks on an offset, constant rows (output = bias, bit for bit), offset rows 100 + 0.5 {0, 1}
                  (a one-pass variance loses them), random rows with residual, pre_bias, both, and in place;
                  one_step_cond because ``t g + b`` may cancel.
  per-head norm   the walk and the eps rows as q and k heads through qknorm_rope_kv_write at an identity table
                  row: plain one_step.
  RoPE            tables in {0, +-1, +-0.5, +-0.25}: bitwise qkv, K cache and interleaved V cache, every element of
                  sentinel-filled caches outside the written lines intact; the model's tables under
                  one_step_cond; head_dim 128, 64 and 16, Hkv D at and above the LDS bound, T = 1, 21, 2 BS + 3,
                  BS = 16 and 64, slots over every offset of the first and last block, padding rows, no slots.
  quantisers      scale within one fp32 ulp of max(amax, 1e-12) / 448, codes = RNE_e4m3(v * (1 / s_kernel)).

Every output that is not a cache sits in a RowCage whose sentinels must survive.  tests/test_rowwise_probes.py
shows on the CPU what these comparisons reject.  Each test prints the worst distance it saw (pytest -s); under
one_step_cond both on the well-conditioned outputs and on those that cancel.

Observed on an MI355X, worst distance in bf16 codes.  Under one_step / decided (1 allowed): rmsnorm 1 on the
random / eps / residual rows of either kernel (0 at d = 8), 0 on every walk; rmsnorm_quant_fp8 1, 0 on the whole
walks; the per-head norm families through qknorm_rope_kv_write 0; silu_mul 1.  No ``decided`` output was off its
RNE code.  Under one_step_cond, on the well-conditioned outputs (1 allowed) / on the outputs that cancel (held to
the absolute bound; at most 1.2 % of a case): layernorm 1 / 13 on random rows, 1 / 1 on the offset rows, 0 / 0 on
the walks; rope_kv_write with the model's tables 1 / 2; qknorm_rope_kv_write 1 / 195 (norms, outputs next to
zero), 1 / 2 without norms; bitwise with the exact tables.  Every quantiser scale (quant_fp8_rows,
rmsnorm_quant_fp8, silu_mul_quant_fp8) was bit-equal to fp32 max(amax, 1e-12) / 448, and every e4m3 code, -0 and
the subnormal rows included, equal to torch's RNE conversion.  The file's 233 cases ran in 13 s.
"""
import pytest
import torch

from tests import rowwise_probes as rp
from tests.rowwise_probes import BF, bits, rne

pytestmark = pytest.mark.gpu

_cache = {}


def _K():
    from llm_weighted_consensus_amd import ops
    return ops.kernels()


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 29)


def _once(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _check(cage, want, rule, what, mag=None, err=rp.NORM_ERR):
    v = rp.violations(cage, want, rule, mag, err)
    assert not v, f"{what}: " + "; ".join(v)
    assert cage.unwritten() == 0, f"{what}: {cage.unwritten()} outputs never written"


def _report(name, worst, extra=""):
    print(f"\n[rowwise] {name}: worst distance {worst} code(s){extra}")


def _both(got, want, mag, err=rp.NORM_ERR):
    """(worst distance on the well-conditioned outputs, worst distance on the others, share of the others)."""
    want, mag = want.to(got.device), mag.to(got.device)
    well = rp.well_conditioned(want, mag, err)
    st = rp.steps(got, want)
    return (int(st[well].max()) if bool(well.any()) else 0, int(st[~well].max()) if bool((~well).any()) else 0,
            float((~well).double().mean()))


def _merge(a, b):
    return max(a[0], b[0]), max(a[1], b[1]), max(a[2], b[2])


def _report_cond(name, w):
    print(f"\n[rowwise] {name}: worst distance {w[0]} code(s) on well-conditioned outputs, {w[1]} on the outputs "
          f"that cancel (at most {w[2]:.4f} of a case)")


def _weights(d, gpu):
    return _once(("w", d), lambda: rp.weights(d, _gen(d)).to(gpu))


# ---------------------------------------------------------------------------------------------------------
# rmsnorm


def _rmsnorm(gpu, x, w, eps, r=None):
    """(output cage, residual cage or None) after one launch."""
    out = rp.RowCage(x.shape, gpu)
    res = None
    if r is not None:
        res = rp.RowCage(x.shape, gpu)
        res.load(r)
    _K().rmsnorm(x, None if res is None else res.view, w, out.view, float(eps))
    return out, res


def _rms_case(gpu, x, w, eps, rule, what, r=None):
    """Launch, check the stream bitwise and the output by ``rule``; returns the worst distance."""
    x = x.to(gpu)
    r = None if r is None else r.to(gpu)
    h = rp.stream(x, r)
    want = rp.pinned(h, w) if rule == "bitwise" else rp.rms(h, w, eps)
    out, res = _rmsnorm(gpu, x, w, eps, r)
    if res is not None:
        _check(res, h, "bitwise", what + " stream")
    _check(out, want, rule, what)
    return rp.worst(out.view, want)


RMS_WG = [(8, 5), (512, 5), (520, 5), (1000, 5), (4096, 37), (8192, 255), (8200, 3), (32768, 3)]
RMS_WAVE = [(d, rows) for d in (2048, 4096, 8192) for rows in (256, 257, 259)]


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("d,rows", RMS_WG + RMS_WAVE)
def test_rmsnorm_rows(gpu, d, rows, res):
    """Random rows (``decided``), eps rows at both eps, and with a residual the residual rows (stream bitwise)
    and the pinned rows (norm bitwise).  rows >= 256 at 2048 / 4096 / 8192: the wave kernel."""
    w = _weights(d, gpu)
    worst = 0
    for spread in (False, True):
        x = rp.random_rows(rows, d, _gen(d, rows, spread), spread)
        r = rp.random_rows(rows, d, _gen(d, rows, spread, 1), spread) if res else None
        worst = max(worst, _rms_case(gpu, x, w, 1e-5, "decided", f"random spread={spread}", r))
    for eps in (1e-5, 1e-6):
        x = rp.eps_rows(rows, d, _gen(d, rows, 2))
        r = rp.eps_rows(rows, d, _gen(d, rows, 3)) if res else None
        worst = max(worst, _rms_case(gpu, x, w, eps, "one_step", f"eps rows {eps}", r))
    if res:
        x, r = rp.residual_rows(rows, d, _gen(d, rows, 4))
        worst = max(worst, _rms_case(gpu, x, w, 1e-5, "one_step", "residual rows", r))
        _rms_case(gpu, x, rp.pow2_weights(d).to(gpu), rp.PIN_EPS, "bitwise", "pinned rows", r)
    _report(f"rmsnorm d={d} rows={rows} res={res}", worst)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("d", [8, 512, 520, 1000, 2048, 4096, 8192, 8200, 32768])
def test_rmsnorm_spike_walk(gpu, d, res):
    """One row per vector slot, every slot of the row at every width.  With a residual x = r = the walk (the
    stream is twice the walk, exactly)."""
    w = _weights(d, gpu)
    if d > 8200:   # 4096 rows of 64 KiB: in runs of 512 rows
        worst = 0
        for chunk in rp.walk_chunks(d):
            x = rp.spike_walk(d, chunk)[0].to(gpu)
            worst = max(worst, _rms_case(gpu, x, w, 1e-5, "one_step", f"walk slots {chunk[0]}..", x if res else None))
        _report(f"rmsnorm walk d={d} res={res}", worst)
        return
    x, _ = _once(("walk", d), lambda: rp.spike_walk(d))
    x = x.to(gpu)
    r = x if res else None
    worst = _rms_case(gpu, x, w, 1e-5, "one_step", "walk", r)
    if d in (2048, 4096, 8192):   # whole: the wave kernel; chunks of at most 255 rows: the workgroup kernel
        assert x.shape[0] >= 256
        for i in range(0, x.shape[0], 255):
            c = x[i:i + 255].contiguous()
            worst = max(worst, _rms_case(gpu, c, w, 1e-5, "one_step", f"walk rows {i}..", c if res else None))
    _report(f"rmsnorm walk d={d} res={res}", worst)


@pytest.mark.parametrize("d", [12, 32776])
def test_rmsnorm_refuses(gpu, d):
    x = torch.zeros(2, d, dtype=BF, device=gpu)
    with pytest.raises(RuntimeError, match="rmsnorm"):
        _K().rmsnorm(x, None, torch.ones(d, dtype=BF, device=gpu), torch.empty_like(x), 1e-5)


def _quant_checks(v_bf16, q_cage, s_cage, what):
    """The quantiser rules against the bf16 values ``v_bf16`` the kernel quantised; returns whether the scales
    are bit-equal to the fp32 reference."""
    assert q_cage.outside_touched() == 0 and s_cage.outside_touched() == 0, what
    s = s_cage.view.cpu()
    ref = rp.scale_ref(v_bf16.cpu())
    ul = rp.ulps32(s, ref)
    assert int(ul.max()) <= 1, f"{what}: scale {int(ul.max())} ulps from max(amax, 1e-12) / 448"
    want = rp.e4m3_codes(v_bf16.cpu(), s)
    got = q_cage.view.cpu().view(torch.uint8)
    bad = got != want
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} e4m3 codes differ; first at "
                                 f"{bad.nonzero()[0].tolist()}: got {int(got[tuple(bad.nonzero()[0])])} want "
                                 f"{int(want[tuple(bad.nonzero()[0])])}")
    return bool((ul == 0).all())


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("d", [2048, 4096, 8192])
def test_rmsnorm_quant_fp8(gpu, d, rows, res):
    """The walk (its first ``rows`` rows, cyclically) and random rows: the bf16 output by one_step / decided, q
    and s against that output by the quantiser rules; keep_bf16=False gives the same q and s."""
    walk, _ = _once(("walk", d), lambda: rp.spike_walk(d))
    walk = walk[torch.arange(rows) % walk.shape[0]].contiguous()
    worst, equal = _rq_cases(gpu, d, res, (("walk", walk, "one_step"),
                                           ("random", rp.random_rows(rows, d, _gen(d, rows, 5), True), "decided")))
    _report(f"rmsnorm_quant_fp8 d={d} rows={rows} res={res}", worst, f", scales bit-equal: {equal}")


@pytest.mark.parametrize("d", [2048, 4096, 8192])
def test_rmsnorm_quant_fp8_whole_walk(gpu, d):
    """Every vector slot of the row carries the spike (and with it the row's amax) once through the quantising
    instantiation: all VPL vectors of every lane, in the sum of squares and in the amax / wave_max pass."""
    walk, _ = _once(("walk", d), lambda: rp.spike_walk(d))
    assert walk.shape[0] == d // 8
    worst, equal = _rq_cases(gpu, d, False, (("whole walk", walk, "one_step"),))
    _report(f"rmsnorm_quant_fp8 whole walk d={d}", worst, f", scales bit-equal: {equal}")


def _rq_cases(gpu, d, res, cases):
    w = _weights(d, gpu)
    worst, equal = 0, True
    for name, x, rule in cases:
        rows = x.shape[0]
        x = x.to(gpu)
        r = x.clone() if res else None
        h = rp.stream(x, r)
        want = rp.rms(h, w, 1e-5)
        runs = []
        for keep in (True, False):
            y = rp.RowCage(x.shape, gpu)
            q = rp.RowCage(x.shape, gpu, torch.float8_e4m3fn)
            s = rp.RowCage((rows,), gpu, torch.float32)
            rc = rp.RowCage(x.shape, gpu)
            if res:
                rc.load(r)
            _K().rmsnorm_quant_fp8(x, rc.view if res else None, w, y.view if keep else None, q.view, s.view, 1e-5)
            if res:
                _check(rc, h, "bitwise", f"{name} stream")
            if keep:
                _check(y, want, rule, f"{name} bf16 output")
                worst = max(worst, rp.worst(y.view, want))
                equal &= _quant_checks(y.view, q, s, f"{name} keep_bf16")
            else:
                assert y.unwritten() == y.n and y.outside_touched() == 0
            runs.append((q.view.view(torch.uint8).clone(), s.view.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{name}: keep_bf16"
    return worst, equal


@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("d", [8, 520, 4096])
def test_rms_rowsumsq_exact(gpu, d, rows):
    x = rp.small_int_rows(rows, d, _gen(d, rows, 6)).to(gpu)
    ss = rp.RowCage((rows,), gpu, torch.float32)
    _K().rms_rowsumsq(x, ss.view)
    want = (x.double() ** 2).sum(1).float()
    assert ss.outside_touched() == 0 and ss.unwritten() == 0
    assert torch.equal(ss.view.view(torch.int32), want.view(torch.int32)), (ss.view - want).abs().max()


# ---------------------------------------------------------------------------------------------------------
# layernorm


def _ln_params(d, gpu):
    def build():
        gen = _gen(d, 7)
        return (rp.weights(d, gen, 0.2).to(gpu), (0.2 * torch.randn(d, generator=gen)).to(BF).to(gpu),
                torch.randn(d, generator=gen).to(BF).to(gpu))
    return _once(("ln", d), build)


LN_DS = [8, 256, 520, 768, 1024, 1032, 2048, 32768]


@pytest.mark.parametrize("rows", [1, 5, 53])
@pytest.mark.parametrize("d", LN_DS)
def test_layernorm_rows(gpu, d, rows):
    """d <= 1024: the wave kernel (in place allowed); above: the workgroup kernel (in place refused)."""
    g, b, pb = _ln_params(d, gpu)
    x = rp.random_rows(rows, d, _gen(d, rows, 8)).to(gpu)
    r = rp.random_rows(rows, d, _gen(d, rows, 9)).to(gpu)
    worst = (0, 0, 0.0)
    for use_r, use_pb in ((False, False), (True, False), (False, True), (True, True)):
        want, mag = rp.layernorm(x, g, b, 1e-12, r=r if use_r else None, pb=pb if use_pb else None)
        places = (False, True) if d <= 1024 else (False,)
        for in_place in places:
            out = rp.RowCage(x.shape, gpu)
            src = out.load(x) if in_place else x
            _K().layernorm(src, r if use_r else None, g, b, out.view, 1e-12, pb if use_pb else None)
            _check(out, want, "one_step_cond", f"res={use_r} pre_bias={use_pb} in_place={in_place}", mag)
            worst = _merge(worst, _both(out.view, want, mag))
    # constant rows: zero variance, the output is the bias
    c = torch.tensor([3.0, -5.0, 0.0, 7.0, 2.0])[torch.arange(rows) % 5][:, None].expand(rows, d).to(BF).contiguous().to(gpu)
    out = rp.RowCage(c.shape, gpu)
    _K().layernorm(c, None, g, b, out.view, 1e-12, None)
    _check(out, b.expand(rows, d), "bitwise", "constant rows")
    if d > 1024:
        with pytest.raises(RuntimeError, match="layernorm"):
            _K().layernorm(x, None, g, b, x, 1e-12, None)
    _report_cond(f"layernorm d={d} rows={rows}", worst)


@pytest.mark.parametrize("d", rp.LN_OFFSET_DS)
def test_layernorm_offset_rows(gpu, d):
    """The 16 rows 100 + 0.5 {0, 1} of rp.ln_offset_case(d): tests/test_rowwise_probes.py shows that a one-pass
    E[h^2] - mean^2 variance in fp32 is rejected on these very rows at every width run here.  (Sums of multiples
    of 0.5 are exact; the mean's own rounding, 2^-25 * 100 against deviations of 0.25, is 1.2e-5.)"""
    x, g, b = (t.to(gpu) for t in rp.ln_offset_case(d))
    want, mag = rp.layernorm(x, g, b, 1e-12)
    out = rp.RowCage(x.shape, gpu)
    _K().layernorm(x, None, g, b, out.view, 1e-12, None)
    _check(out, want, "one_step_cond", "offset rows", mag)
    _report_cond(f"layernorm offset rows d={d}", _both(out.view, want, mag))


@pytest.mark.parametrize("d", LN_DS)
def test_layernorm_spike_walk(gpu, d):
    """Every slot of the row; at 32768 in runs of 512 rows."""
    g, b, _ = _ln_params(d, gpu)
    worst = (0, 0, 0.0)
    for chunk in rp.walk_chunks(d):
        x = rp.spike_walk(d, chunk, offset=rp.LN_OFFSET)[0].to(gpu)
        want, mag = rp.layernorm(x, g, b, 1e-12)
        out = rp.RowCage(x.shape, gpu)
        _K().layernorm(x, None, g, b, out.view, 1e-12, None)
        _check(out, want, "one_step_cond", f"walk slots {chunk[0]}..", mag)
        worst = _merge(worst, _both(out.view, want, mag))
    _report_cond(f"layernorm walk d={d}", worst)


# ---------------------------------------------------------------------------------------------------------
# rope_kv_write / qknorm_rope_kv_write


def _real_tables(P, D):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import rope_tables

    def build():
        cfg = decoder_config("llama-tiny")
        assert cfg.head_dim == 128
        cos, sin = rope_tables(cfg, torch.device("cpu"), P)
        return cos.contiguous(), sin.contiguous()
    if D == 128:
        return _once(("tables", P), build)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).double() / D))
    ang = torch.arange(P).double()[:, None] * inv[None, :]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def _rope_launch(gpu, qkv, pos, slots, cos, sin, NB, BS, Hq, Hkv, D, rope_q, feats=None):
    """One launch on fresh sentinel caches; returns (qkv cage, k cache, v cache)."""
    cage = rp.RowCage(qkv.shape, gpu)
    cage.load(qkv.to(gpu))
    kc = rp.sentinel_cache((NB, Hkv, BS, D), gpu)
    vc = rp.sentinel_cache((NB, Hkv, BS // 4, D, 4), gpu)
    sl = None if slots is None else slots.to(gpu)
    if feats is None:
        _K().rope_kv_write(cage.view, pos.to(gpu), sl, cos.to(gpu), sin.to(gpu), kc, vc, Hq, Hkv, D, rope_q)
    else:
        bias, qw, kw, eps = feats
        dev = lambda t: None if t is None else t.to(gpu)   # noqa: E731
        _K().qknorm_rope_kv_write(cage.view, pos.to(gpu), sl, cos.to(gpu), sin.to(gpu), kc, vc, Hq, Hkv, D, rope_q,
                                  dev(bias), dev(qw), dev(kw), eps)
    return cage, kc, vc


def _rope_check(cage, kc, vc, want, slots, NB, BS, exact, what, err=rp.NORM_ERR):
    """qkv, the K cache and the V cache against the oracle; returns the worst distances (see _both)."""
    if exact:
        _check(cage, want.qkv, "bitwise", what + " qkv")
    else:
        _check(cage, want.qkv, "one_step_cond", what + " qkv", want.mag, err)
    kw_, vw_, km, vm = rp.scatter(want.k, want.v, slots, NB, BS)
    v = rp.cache_violations(vc, vw_, vm)                      # V is a copy (qknorm: one exact add): bitwise always
    if exact:
        v += rp.cache_violations(kc, kw_, km)
    else:
        n = int((bits(kc)[~km.to(kc.device)] != rp.SENTINEL).sum())
        if n:
            v.append(f"{n} K cache elements outside the written lines overwritten")
        if slots is not None and bool((slots >= 0).any()):
            real = (slots >= 0).nonzero().flatten()
            blk, off = (slots[real] // BS).long(), (slots[real] % BS).long()
            lines = kc[blk.to(kc.device), :, off.to(kc.device)]
            bad, _ = rp.one_step_cond(lines, want.k[real].to(kc.device), want.kmag[real].to(kc.device), err)
            if bool(bad.any()):
                v.append(rp.describe(bad, lines, want.k[real].to(kc.device), "one_step_cond (K cache)"))
    assert not v, f"{what}: " + "; ".join(v)
    return _both(cage.view, want.qkv, want.mag, err)


ROPE_HEADS = [(128, 3, 1), (128, 8, 2), (128, 40, 8), (128, 32, 32), (128, 40, 40), (64, 3, 1), (64, 8, 2),
              (64, 40, 8), (16, 3, 1)]
VARIANTS = ("slots", "padded", "allpad", "none")


def _rope_sweep(gpu, D, Hq, Hkv, BS, feats_of=None, tables=("exact", "real")):
    NB, P, W = 4, 96, (Hq + 2 * Hkv) * D
    worst = (0, 0, 0.0)
    for T in (1, 21, 2 * BS + 3):
        gen = _gen(D, Hq, Hkv, BS, T)
        pos = rp.probe_positions(T, P, gen)
        for kind in tables:
            exact = kind == "exact"
            cos, sin = rp.synthetic_tables(P, D // 2, gen) if exact else _real_tables(P, D)
            qkv = rp.exact_values((T, W), gen) if exact else torch.randn(T, W, generator=gen).to(BF)
            feats = None if feats_of is None else feats_of(gen, exact)
            kw = {} if feats is None else dict(bias=feats[0], qw=feats[1], kw=feats[2], eps=feats[3], qknorm=True)
            bitwise_ok = exact and (feats is None or (feats[1] is None and feats[2] is None))
            err = rp.ROPE_ERR if feats is None or (feats[1] is None and feats[2] is None) else rp.NORM_ERR
            for variant in VARIANTS:
                slots = rp.probe_slots(T, NB, BS, gen, variant)
                caches = {}
                for rope_q in (True, False):
                    what = f"T={T} {kind} {variant} rope_q={rope_q}"
                    want = rp.rope_want(qkv, pos, cos, sin, slots, Hq, Hkv, D, rope_q, **kw)
                    cage, kc, vc = _rope_launch(gpu, qkv, pos, slots, cos, sin, NB, BS, Hq, Hkv, D, rope_q, feats)
                    worst = _merge(worst, _rope_check(cage, kc, vc, want, slots, NB, BS, bitwise_ok, what, err))
                    q_unchanged = feats is None or all(f is None for f in feats[:3])
                    if not rope_q and q_unchanged:   # q is untouched, bit for bit
                        assert torch.equal(bits(cage.view[:, :Hq * D]), bits(qkv[:, :Hq * D].to(gpu))), what
                    if not rope_q and slots is not None and feats is None:   # k, v not written back at real slots
                        real = (slots >= 0).to(gpu)
                        assert torch.equal(bits(cage.view[real][:, Hq * D:]), bits(qkv.to(gpu)[real][:, Hq * D:])), what
                    caches[rope_q] = (kc, vc)
                for a, b in zip(caches[True], caches[False]):   # the caches do not depend on rope_q
                    assert torch.equal(bits(a), bits(b)), f"T={T} {kind} {variant}: caches differ between modes"
    return worst


@pytest.mark.parametrize("D,Hq,Hkv,BS", [h + (bs,) for h in ROPE_HEADS for bs in (16, 64) if (h[0], bs) != (16, 64)])
def test_rope_kv_write(gpu, D, Hq, Hkv, BS):
    """Hkv D = 4096 is the last V row staged in LDS, 5120 takes the direct path; D = 16 (one unit per head) runs
    once, at BS = 16."""
    _report_cond(f"rope_kv_write D={D} Hq={Hq} Hkv={Hkv} BS={BS}", _rope_sweep(gpu, D, Hq, Hkv, BS))


@pytest.mark.parametrize("BS", [16, 64])
@pytest.mark.parametrize("feature", ["none", "bias", "norms", "both"])
@pytest.mark.parametrize("Hq,Hkv", [(3, 1), (8, 2), (40, 8), (32, 32)])
def test_qknorm_rope_kv_write(gpu, Hq, Hkv, feature, BS):
    """Single rounding: bias, per-head norm and rotation in fp32 (oracle: fp64), one RNE at the store."""
    D = 128

    def feats(gen, exact):
        bias = qw = kw = None
        if feature in ("bias", "both"):
            n = (Hq + 2 * Hkv) * D
            bias = rp.exact_values((n,), gen) if exact else torch.randn(n, generator=gen).to(BF)
        if feature in ("norms", "both"):
            qw, kw = rp.weights(D, gen), rp.weights(D, gen)
        return bias, qw, kw, 1e-6
    tables = ("exact", "real") if feature in ("none", "bias") else ("real",)
    _report_cond(f"qknorm_rope_kv_write Hq={Hq} Hkv={Hkv} {feature} BS={BS}",
                 _rope_sweep(gpu, D, Hq, Hkv, BS, feats, tables))


@pytest.mark.parametrize("family", ["walk", "walk+bias", "eps 1e-5", "eps 1e-6"])
@pytest.mark.parametrize("Hq,Hkv", [(3, 1), (8, 2), (40, 8), (32, 32)])
def test_qknorm_per_head_norm_families(gpu, Hq, Hkv, family):
    """The spike walk and the eps rows through the per-head RMSNorm (the 8-lane DPP sum, * 1/128 + eps, rsqrt):
    every q and k head of 16 tokens takes every one of 16 rows, all tokens at position 0 of a table whose row 0
    is the identity, so the output of a head is rms(head + bias, w, eps) and nothing cancels: plain one_step.
    walk: the walker sits in each half of each of a head's 8 threads once per head (an element or a lane left
    out of the sum, or counted twice, moves that row by more than 17 %); eps rows (|x| ~ 2^-20): eps left out or
    added after the root shows.  q and k weights differ.  Both rope_q modes; K cache lines within one code, V
    bitwise, everything else in the caches untouched."""
    D, T, NB, BS = rp.HEAD_D, 16, 4, 16
    gen = _gen(Hq, Hkv, len(family))
    heads = rp.spike_walk(D)[0] if family.startswith("walk") else rp.eps_rows(16, D, gen)
    qkv = rp.head_qkv(heads, T, Hq, Hkv, gen)
    bias = rp.head_bias(Hq, Hkv, gen) if family == "walk+bias" else None
    eps = 1e-5 if family == "eps 1e-5" else 1e-6
    qw, kw = rp.weights(D, gen), rp.weights(D, gen)
    cos, sin = rp.synthetic_tables(8, D // 2, gen)
    pos = torch.zeros(T, dtype=torch.int32)
    slots = rp.probe_slots(T, NB, BS, gen)
    worst = 0
    for rope_q in (True, False):
        what = f"{family} rope_q={rope_q}"
        want = rp.rope_want(qkv, pos, cos, sin, slots, Hq, Hkv, D, rope_q, bias=bias, qw=qw, kw=kw, eps=eps, qknorm=True)
        assert bool(rp.well_conditioned(want.qkv, want.mag).all())
        cage, kc, vc = _rope_launch(gpu, qkv, pos, slots, cos, sin, NB, BS, Hq, Hkv, D, rope_q, (bias, qw, kw, eps))
        _check(cage, want.qkv, "one_step", what + " qkv")
        kw_, vw_, km, vm = rp.scatter(want.k, want.v, slots, NB, BS)
        v = rp.cache_violations(vc, vw_, vm) + rp.cache_violations(kc, kw_, km, "one_step")
        assert not v, f"{what}: " + "; ".join(v)
        nz = (want.k != 0).to(gpu)
        lines = kc[(slots // BS).long().to(gpu), :, (slots % BS).long().to(gpu)]
        assert bool(((lines != 0) == nz).all()), what + ": zeros of the walk must stay zero in the K cache"
        worst = max(worst, rp.worst(cage.view, want.qkv))
    _report(f"qknorm per-head norm Hq={Hq} Hkv={Hkv} {family}", worst)


def _rope_args(gpu, Hq=8, Hkv=2, D=128, T=5, BS=16, NB=4, P=32):
    gen = _gen(1)
    cos, sin = rp.synthetic_tables(P, D // 2, gen)
    return dict(qkv=rp.exact_values((T, (Hq + 2 * Hkv) * D), gen).to(gpu), positions=rp.probe_positions(T, P, gen).to(gpu),
                slots=rp.probe_slots(T, NB, BS, gen).to(gpu), cos_t=cos.to(gpu), sin_t=sin.to(gpu),
                k_cache=rp.sentinel_cache((NB, Hkv, BS, D), gpu), v_cache=rp.sentinel_cache((NB, Hkv, BS // 4, D, 4), gpu))


def _call_rope(a, Hq=8, Hkv=2, D=128):
    _K().rope_kv_write(a["qkv"], a["positions"], a["slots"], a["cos_t"], a["sin_t"], a["k_cache"], a["v_cache"],
                       Hq, Hkv, D, True)


@pytest.mark.parametrize("arg,how", [("slots", "cpu"), ("positions", "cpu"), ("cos_t", "cpu"), ("sin_t", "cpu"),
                                     ("slots", "strided"), ("positions", "strided"), ("cos_t", "strided"),
                                     ("sin_t", "strided"), ("k_cache", "strided"), ("sin_t", "rows"), ("qkv", "3d")])
def test_rope_kv_write_refuses(gpu, arg, how):
    """The binding checks what qknorm_rope_kv_write's checks, and names the argument."""
    a = _rope_args(gpu)
    _call_rope(a)                                             # the arguments are fine as they are
    t = a[arg]
    if how == "cpu":
        a[arg] = t.cpu()
    elif how == "strided":
        wide = torch.cat([t, t], -1) if t.dim() > 1 else torch.stack([t, t], -1).reshape(-1)
        a[arg] = wide[..., : t.shape[-1]] if t.dim() > 1 else wide[::2]
        assert a[arg].shape == t.shape and not a[arg].is_contiguous()
    elif how == "rows":
        a[arg] = t[:-1].contiguous()
    else:
        a[arg] = t.view(1, *t.shape)
    name = "cos/sin" if how == "rows" else arg
    with pytest.raises(RuntimeError, match=name):
        _call_rope(a)


def test_qknorm_refuses_33_kv_heads(gpu):
    a = _rope_args(gpu, Hq=33, Hkv=33)
    with pytest.raises(RuntimeError, match="Hkv"):
        _K().qknorm_rope_kv_write(a["qkv"], a["positions"], a["slots"], a["cos_t"], a["sin_t"], a["k_cache"],
                                  a["v_cache"], 33, 33, 128, True, None, None, None, 1e-6)


# ---------------------------------------------------------------------------------------------------------
# SwiGLU and the quantisers


@pytest.mark.parametrize("block", [0, 32])
@pytest.mark.parametrize("T,F", [(1, 8), (19, 8), (1, 1024), (19, 1024), (1, 28672), (19, 28672), (2049, 4096)])
def test_silu_mul_grid(gpu, T, F, block):
    """Gates on the +-64 grid, ups of both signs, ``decided``.  [2049, 4096] is 4096 * 256 + 512 vectors: the
    grid-stride loop takes a second trip."""
    if F % max(block, 8) != 0:
        with pytest.raises(RuntimeError, match="block"):
            _K().silu_mul(torch.zeros(T, 2 * F, dtype=BF, device=gpu), torch.zeros(T, F, dtype=BF, device=gpu), block)
        return
    gu, gate, up = rp.silu_inputs(T, F, block)
    want = rp.silu_mul(gate.to(gpu), up.to(gpu))
    out = rp.RowCage((T, F), gpu)
    _K().silu_mul(gu.to(gpu), out.view, block)
    _check(out, want, "decided", f"silu_mul block={block}")
    _report(f"silu_mul T={T} F={F} block={block}", rp.worst(out.view, want))


@pytest.mark.parametrize("F,block", [(16384, 0), (16384, 32), (16392, 0), (16392, 8)])
def test_silu_mul_quant_fp8(gpu, F, block):
    """16384 is the last width held in registers, 16392 the first that recomputes (16392 % 32 != 0: block 8).
    Bitwise against quant_fp8_rows(silu_mul(..)), and the quantiser rules against silu_mul's own output."""
    T = 3
    gu, gate, up = rp.silu_inputs(T, F, block)
    gu = gu.to(gpu)
    act = rp.RowCage((T, F), gpu)
    _K().silu_mul(gu, act.view, block)
    _check(act, rp.silu_mul(gate.to(gpu), up.to(gpu)), "decided", "silu_mul")
    q0, s0 = rp.RowCage((T, F), gpu, torch.float8_e4m3fn), rp.RowCage((T,), gpu, torch.float32)
    _K().quant_fp8_rows(act.view, q0.view, s0.view)
    q1, s1 = rp.RowCage((T, F), gpu, torch.float8_e4m3fn), rp.RowCage((T,), gpu, torch.float32)
    _K().silu_mul_quant_fp8(gu, q1.view, s1.view, block)
    equal = _quant_checks(act.view, q1, s1, "fused")
    assert torch.equal(q0.view.view(torch.uint8), q1.view.view(torch.uint8)) and torch.equal(s0.view, s1.view)
    _report(f"silu_mul_quant_fp8 F={F} block={block}", 0, f", scales bit-equal: {equal}")


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("d", [8, 2048, 2056, 16392])
def test_quant_fp8_rows(gpu, d, rows):
    equal = True
    fams = {"amax walk": rp.amax_walk(d, rows)[0], "zero": torch.zeros(rows, d, dtype=BF),
            "subnormal": rp.subnormal_rows(rows, d, _gen(d, rows, 10)), "e4m3 ties": rp.e4m3_tie_rows(rows, d),
            "random": rp.random_rows(rows, d, _gen(d, rows, 11), True)}
    for name, x in fams.items():
        assert x.shape == (rows, d), name
        x = x.to(gpu)
        q, s = rp.RowCage((rows, d), gpu, torch.float8_e4m3fn), rp.RowCage((rows,), gpu, torch.float32)
        _K().quant_fp8_rows(x, q.view, s.view)
        equal &= _quant_checks(x, q, s, name)
    _report(f"quant_fp8_rows d={d} rows={rows}", 0, f", scales bit-equal: {equal}")


# ---------------------------------------------------------------------------------------------------------
# copies


@pytest.mark.parametrize("d", [8, 1032])
def test_embedding_bitwise(gpu, d):
    """ids at 0 and V - 1, out of range on both sides (clamped to the table's ends, as the kernel documents),
    and repeated."""
    V = 50
    table = rp.distinct((V, d)).to(gpu)
    ids = torch.tensor([0, V - 1, V + 5, -3, 7, 7, 0, 2 ** 31 - 1, 31], dtype=torch.int32)
    out = rp.RowCage((ids.numel(), d), gpu)
    _K().embedding(table, ids.to(gpu), out.view)
    _check(out, table[ids.long().clamp(0, V - 1).to(gpu)], "bitwise", "embedding")


@pytest.mark.parametrize("BS", [16, 64])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_gather_bitwise(gpu, D, BS):
    NB, Hkv = 4, 2
    kc = rp.distinct((NB, Hkv, BS, D)).to(gpu)
    vc = rp.distinct((NB, Hkv, BS // 4, D, 4), start=5).to(gpu)
    slots = rp.probe_slots(2 * BS + 3, NB, BS, _gen(D, BS)).long()
    ko, vo = rp.RowCage((slots.numel(), Hkv * D), gpu), rp.RowCage((slots.numel(), Hkv * D), gpu)
    _K().kv_gather(kc, vc, slots.to(gpu), ko.view, vo.view)
    blk, off = (slots // BS).to(gpu), (slots % BS).to(gpu)
    _check(ko, kc[blk, :, off].reshape(-1, Hkv * D), "bitwise", "k")
    _check(vo, vc[blk, :, off // 4, :, off % 4].reshape(-1, Hkv * D), "bitwise", "v")


def test_kv_block_copy_bitwise(gpu):
    LK, NB, shape = 4, 8, (2, 16, 64)
    cache = rp.sentinel_cache((LK, NB) + shape)
    src, dst = [1, 2], [5, 6]
    cache[:, src] = rp.distinct((LK, 2) + shape)
    want = cache.clone()
    want[:, dst] = want[:, src]
    cage = rp.RowCage(cache.shape, gpu)
    cage.load(cache.to(gpu))
    _K().kv_block_copy(cage.view, torch.tensor([[1, 5], [2, 6]], dtype=torch.int32, device=gpu))
    assert cage.outside_touched() == 0
    assert torch.equal(bits(cage.view).cpu(), bits(want))
    assert int((bits(cage.view)[:, [0, 3, 4, 7]] != rp.SENTINEL).sum()) == 0
