"""The GEMM probes of tests/gemm_probes.py would notice the failures they target (CPU only).

For every K of tests/test_gemm_probes_gpu.py the honest oracle passes its own rule inside intact surroundings
and the conditions the GPU tests assert from the reference hold; every mutant — a k dropped or counted twice,
an 8-wide k group from the neighbouring row, a truncating or round-half-up store, a split whose partial went
through bf16, a residual or bias added after the bf16 rounding, an unwritten 16-column tail, a row written
past M — is rejected by the rule and the family its GPU tests use.  The last test records why the probes exist:
the random inputs and the bound of test_kernels_gpu.py::test_gemm4w accept three of those mutants."""
import functools

import pytest
import torch

from tests import gemm_probes as gp

# every K of tests/test_gemm_probes_gpu.py (bf16 kernels), and the e4m3 ones
KS = [64, 128, 192, 256, 384, 512, 1024, 2048, 4096, 14336]
KS8 = [128, 256, 512]
M, N = 257, 264          # the K-loop shape of the GPU tests: a 1-row and an 8-column tail


@functools.lru_cache(maxsize=None)
def _fam(family, K):
    """(A, W, fp64 accumulator, unit) of a family at [M, N, K]; built once and shared (no test writes to it)."""
    gen = torch.Generator().manual_seed(K + len(family))
    if family == "onehot":
        A, W, _ = gp.one_hot(M, N, K, gen)
    elif family == "wide":
        A, W = gp.wide(M, N, K, gen)
    else:
        A, W = gp.sign(M, N, K, gen, scaled=family == "scaled")
    return A, W, gp.exact(A, W), gp.unit(M, N, family == "scaled")


@functools.lru_cache(maxsize=None)
def _operands(kind):
    gen = torch.Generator().manual_seed(len(kind))
    if kind == "bias":
        return gp.quarters((N,), gen)
    return gp.quarters((M, N), gen) if kind == "res" else gp.big_integers((M, N), gen)


def _accepted(out, want, rule="bitwise", **kw):
    """Whether a kernel that stored ``out`` passes the GPU tests' check against ``want``."""
    return not gp.violations(gp.write(gp.Cage(M, N), out, **kw), want, rule)


@pytest.mark.parametrize("K", KS)
def test_conditions_hold_and_oracle_passes(K):
    """The 95 % condition (|accumulator| <= 255 products) holds for the sign families, the honest store passes
    bitwise and one_step inside intact surroundings, and every operand is what the derivations assume."""
    for family in ("sign", "scaled", "wide", "onehot"):
        A, W, acc, unit = _fam(family, K)
        if family in ("sign", "scaled"):
            assert gp.unit_visible(acc, unit) >= 0.95, (family, K, gp.unit_visible(acc, unit))
            assert bool(((acc / unit) % 2 == 0).all())                # even sums: one unit error makes them odd
        if family != "onehot":
            assert bool((acc.float().double() == acc).all())          # exact in fp32
        else:
            assert bool(((A != 0).sum(1) == 1).all())
        for kind in (None, "res", "resbig", "bias"):
            op = None if kind is None else _operands(kind)
            want = acc if op is None else acc + op.double()
            if family != "onehot":
                assert bool((want.float().double() == want).all())    # accumulator + operand exact in fp32
            assert _accepted(gp.rne(want), want) and _accepted(gp.rne(want), want, "one_step")
    assert bool((_operands("res").float() * 4 % 1 == 0).all()) and float(_operands("res").abs().max()) <= 64
    big = _operands("resbig").float().abs()
    assert bool((big % 1 == 0).all()) and 256 <= float(big.min()) and float(big.max()) <= 1024


def test_one_hot_walk_covers_the_tiles():
    for K in KS:
        ks = gp.probe_ks(K, shares=8 if K % 2048 == 0 else 1)
        assert len(set(ks)) == len(ks) and all(0 <= k < K for k in ks)
        want = set(range(min(64, K))) | set(range(K - 64, K))
        for b in range(32, K, 32):
            want |= {b - 1, b}
        if K % 2048 == 0:   # the skinny kernel's 8 waves own K / 8 each
            want |= {w * K // 8 for w in range(8)} | {(w + 1) * K // 8 - 1 for w in range(8)}
            assert set(ks[:16]) == {w * K // 8 for w in range(8)} | {(w + 1) * K // 8 - 1 for w in range(8)}
        assert want <= set(ks)
    # the GPU tests' 257 rows hold the whole walk at their one-hot K
    assert all(len(gp.probe_ks(K)) <= M for K in (64, 128, 192, 256, 384))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("family", ["sign", "scaled"])
def test_dropped_and_doubled_k_are_rejected(family, K):
    """One k missing from, or counted twice in, a 16 x 16 block: rejected by bitwise, at every output of the
    block whose honest and wrong sums both stay within 255 products."""
    A, W, acc, unit = _fam(family, K)
    for mutant in (gp.drop_k, gp.double_k):
        for k, r0, c0 in ((0, 0, 0), (K - 1, M - 16, N - 16), (K // 2, 100, 64)):
            wrong = mutant(acc, A, W, k, r0, c0)
            assert not _accepted(gp.rne(wrong), acc)
            blk = (slice(r0, r0 + 16), slice(c0, c0 + 16))
            seen = gp.bitwise(gp.rne(wrong), acc)[blk]
            sure = (torch.maximum(acc.abs(), wrong.abs()) <= gp.EXACT_MAX * unit)[blk]
            assert bool(seen[sure].all()) and int(sure.sum()) >= 0.9 * 256, (family, K, int(sure.sum()))
            # with the residual epilogues the stored sums are no longer bf16 integers, yet the block shows
            for kind in ("res", "resbig"):
                R = _operands(kind).double()
                assert not _accepted(gp.rne(wrong + R), acc + R)


@pytest.mark.parametrize("K", KS)
def test_k_group_from_the_neighbouring_row_is_rejected(K):
    """An 8-wide k group read from the next row of A.  Where the two rows happen to hold the same signs there,
    the plain sign family forgives it; the stair of scales does not."""
    k0 = 8 * (K // 16)
    for family in ("sign", "scaled", "onehot"):
        A, W, acc, _ = _fam(family, K)
        m, g0 = (3, int(A[3].nonzero()[0]) // 8 * 8) if family == "onehot" else (16, k0)
        assert not _accepted(gp.rne(gp.group_from_row(acc, A, W, m, g0, m + 1)), acc)
    gen = torch.Generator().manual_seed(K)
    for scaled in (False, True):
        A, W = gp.sign(M, N, K, gen, scaled=scaled)
        rs = gp.row_scales(M) if scaled else torch.ones(M)
        A = A.float()
        A[17, k0:k0 + 8] = A[16, k0:k0 + 8] / rs[16] * rs[17]    # the same signs in both rows
        A = A.to(torch.bfloat16)
        acc = gp.exact(A, W)
        assert _accepted(gp.rne(gp.group_from_row(acc, A, W, 16, k0, 17)), acc) == (not scaled)


@pytest.mark.parametrize("K", KS)
def test_wrong_stores_are_rejected(K):
    """Truncation and round-half-up: by one-hot (full-mantissa products, ties among them) with every epilogue,
    and by the sign families under the big-integer residual, whose sums land where bf16 steps are 2 and 4."""
    for family, kinds in (("onehot", (None, "res", "bias")), ("sign", ("resbig",)), ("scaled", ("resbig",))):
        _, _, acc, _ = _fam(family, K)
        for kind in kinds:
            want = acc if kind is None else acc + _operands(kind).double()
            assert not _accepted(gp.store_trunc(want), want), (family, kind)
            if family != "onehot" or kind is None:   # (one-hot + operand: 24-bit sums, ties are 2^-16 rare)
                assert not _accepted(gp.store_half_up(want), want), (family, kind)
    # what the plain sign family cannot see, and why the other cases exist: its outputs are bf16 integers
    if K <= 1024:
        _, _, acc, _ = _fam("sign", K)
        assert _accepted(gp.store_trunc(acc), acc)


@pytest.mark.parametrize("K", [512, 1024, 4096])
@pytest.mark.parametrize("splits", [2, 3, 4, 7])
def test_bf16_partial_is_rejected(K, splits):
    """A split-K partial that went through bf16: rejected by the wide family (partial sums need more than 8
    bits); invisible to the sign family, whose partial sums are integers below 256."""
    A, W, acc, _ = _fam("wide", K)
    wrong = gp.split_bf16_partial(A, W, splits)
    assert not _accepted(gp.rne(wrong), acc)
    R = _operands("res").double()
    assert not _accepted(gp.rne(wrong + R), acc + R)
    if K <= 1024:
        A, W, acc, _ = _fam("sign", K)
        assert _accepted(gp.rne(gp.split_bf16_partial(A, W, splits)), acc)


@pytest.mark.parametrize("K", KS)
def test_operand_added_after_rounding_is_rejected(K):
    """A residual or a bias added to the bf16-rounded product instead of the fp32 accumulator: rejected by
    one-hot (the product is not a bf16 number) and by the wide family."""
    for family in ("onehot", "wide"):
        _, _, acc, _ = _fam(family, K)
        for kind in ("res", "resbig", "bias"):
            op = _operands(kind)
            if family == "onehot" and kind == "resbig":
                continue   # |product| << the operand's bf16 step: both orders store the operand
            assert not _accepted(gp.residual_after_rounding(acc, op), acc + op.double()), (family, kind)


@pytest.mark.parametrize("rule", ["bitwise", "one_step"])
def test_unwritten_tail_and_stray_row_are_rejected(rule):
    _, _, acc, _ = _fam("sign", 128)
    out = gp.rne(acc)
    assert _accepted(out, acc, rule)
    assert not _accepted(out, acc, rule, skip_tail=(M - 1, 1))     # the ragged last row's 16-column tail
    assert not _accepted(out, acc, rule, skip_tail=(32, 16))
    assert not _accepted(out, acc, rule, row_past_m=True)
    cage = gp.write(gp.Cage(M, N), out)
    cage.buf[3, N] = 1.0                                             # a store past column N
    assert gp.violations(cage, acc, rule)
    # an in-place residual epilogue that skips a tail leaves finite values there: the rule rejects them
    R = _operands("res")
    cage = gp.Cage(M, N)
    cage.load(R)
    gp.write(cage, gp.rne(acc + R.double()), skip_tail=(32, 16))
    assert gp.violations(cage, acc + R.double(), rule)


def test_poisoned_operands_keep_their_values():
    A, W, _, _ = _fam("sign", 64)
    Ap, Wp = gp.poison_a(A), gp.poison_w(W)
    assert torch.equal(Ap, A) and torch.equal(Wp, W) and Wp.is_contiguous()
    assert Ap.stride() == (64 + 64, 1) and Ap.stride(0) % 8 == 0
    a8, w8, a_s, w_s = gp.fp8_operands(5, 24, 128, torch.Generator().manual_seed(0))
    a8p = gp.poison_a(a8)
    assert torch.equal(a8p.view(torch.uint8), a8.view(torch.uint8)) and a8p.stride(0) % 16 == 0
    w3 = gp.poison_w(w8.view(2, 12, 128))
    assert w3.shape == (2, 12, 128) and w3.is_contiguous()
    # what lies behind the views is NaN
    base = torch.empty(0, dtype=torch.bfloat16).set_(Ap.untyped_storage(), 0, (257 + 8, 128), (128, 1))
    assert bool(torch.isnan(base[:, 64:].float()).all()) and bool(torch.isnan(base[257:].float()).all())
    basew = torch.empty(0, dtype=torch.bfloat16).set_(Wp.untyped_storage(), 0, (264 + 16, 64), (64, 1))
    assert bool(torch.isnan(basew[264:].float()).all())


@pytest.mark.parametrize("K", KS8)
def test_fp8_family_is_exact_and_sees_a_unit_error(K):
    gen = torch.Generator().manual_seed(K)
    A, W, a_s, w_s = gp.fp8_operands(M, N, K, gen)
    acc = gp.exact(A.float(), W.float())
    scale = (a_s[:, None] * w_s[None, :]).double()
    want = acc * scale
    assert bool((want.float().double() == want).all()) and float(acc.abs().max()) <= 4 * K
    assert gp.unit_visible(acc) >= 0.95
    assert _accepted(gp.rne(want), want)
    wrong = gp.drop_k(acc, A.float(), W.float(), K - 1, M - 16, N - 16) * scale
    assert not _accepted(gp.rne(wrong), want)
    # (the sums are bf16 integers, like the sign family's: this family does not pin the store's rounding)


def _swiglu_case(K, F=288):
    gen = torch.Generator().manual_seed(K)
    A, W = gp.swiglu_sign(M, F, K, gen)
    acc = gp.exact(A, W)
    return A, W, acc[:, :F], acc[:, F:]


@pytest.mark.parametrize("K", [128, 192, 2048, 4096])
def test_swiglu_probe_rejects_unit_errors(K):
    """SwiGLU probe under one_step.  |gate| <= 32 by construction.  A unit error in the up sum u moves
    silu(g) * u by |value| / |u|: more than one bf16 step (2^-7 of the value at most) wherever |u| < 128 — the
    band, which holds >= 90 % of the outputs — and at least two steps, hence a code distance >= 2 at that very
    output, wherever |u| <= 32.  A unit error in the gate sum moves silu's argument by 2^-shift; silu is flat
    near g = -1.28, so single outputs may forgive it, a 16 x 16 block does not."""
    A, W, gate, up = _swiglu_case(K)
    F = up.shape[1]
    shift = gp.swiglu_gate_shift(K)
    assert float(gate.abs().max()) <= 32 and bool((gate * 2.0 ** shift % 2 == 0).all())
    assert gp.in_band(up) >= 0.90, gp.in_band(up)
    want = gp.silu_mul(gate, up)
    assert _accepted_f(gp.rne(want), want, F)
    blk = (slice(32, 48), slice(64, 80))
    for k in (0, K - 1):
        wrong_up = gp.drop_k(up, A, W[F:], k, 32, 64)
        wrong_gate = gp.drop_k(gate, A, W[:F], k, 32, 64)
        assert bool((wrong_up - up)[blk].abs().eq(1).all())
        assert bool((wrong_gate - gate)[blk].abs().eq(2.0 ** -shift).all())
        bad = gp.one_step(gp.rne(gp.silu_mul(gate, wrong_up)), want)
        sure = (torch.maximum(up.abs(), wrong_up.abs()) <= gp.SURE) & (want != 0)
        assert bool(bad[blk].any()) and bool(bad[blk][sure[blk]].all())
        assert bool(gp.one_step(gp.rne(gp.silu_mul(wrong_gate, up)), want)[blk].any())


def _accepted_f(out, want, F):
    return not gp.violations(gp.write(gp.Cage(M, F), out), want, "one_step")


@pytest.mark.parametrize("K", [128, 512, 4096])
def test_rowscale_probe_rejects_unit_errors(K):
    """RS 1 probe under one_step: value = sum * rsqrt(ss / K + eps).  A unit error in the accumulator moves it
    by |value| / |sum|, as for SwiGLU's up half: the same band and the same guarantee."""
    A, W, acc, _ = _fam("sign", K)
    gen = torch.Generator().manual_seed(K)
    r = torch.rsqrt((torch.rand(M, generator=gen) * K + 0.01).double() / K + 1e-5)
    want = acc * r[:, None]
    assert gp.in_band(acc) >= 0.90, gp.in_band(acc)
    assert _accepted(gp.rne(want), want, "one_step")
    blk = (slice(M - 16, M), slice(N - 16, N))
    wrong = gp.drop_k(acc, A, W, K - 1, M - 16, N - 16)
    bad = gp.one_step(gp.rne(wrong * r[:, None]), want)
    sure = (torch.maximum(acc.abs(), wrong.abs()) <= gp.SURE) & (want != 0)
    assert bool(bad[blk].any()) and bool(bad[blk][sure[blk]].all())


def _close_ok(a, b, atol=3e-2, rtol=1e-2):
    """The check of tests/test_kernels_gpu.py (_close) as a predicate."""
    a, b = a.float(), b.float()
    return bool(torch.isfinite(a).all()) and bool(((a - b).abs() <= atol + rtol * b.abs()).all())


@pytest.mark.parametrize("K", [1024, 4096])
def test_random_inputs_and_the_loose_bound_accept_these_mutants(K):
    """Why this file exists: with the randn operands and _close(out, ref, 3e-2, 1e-2) of test_gemm4w, at
    M, N = 300, 520, a truncating store, a split-K whose first partial went through bf16, and a 16-column tail
    that is never stored over memory still holding an earlier launch's result all pass."""
    torch.manual_seed(300 + 520 + K + 256)
    A = torch.randn(300, K).to(torch.bfloat16)
    W = (torch.randn(520, K) / K ** 0.5).to(torch.bfloat16)
    ref = A.float() @ W.float().t()
    acc = gp.exact(A, W)
    assert _close_ok(gp.store_trunc(acc), ref)
    assert _close_ok(gp.rne(gp.split_bf16_partial(A, W, 2)), ref)
    stale = gp.rne(acc).clone()            # the allocator hands the second launch the first one's buffer
    second = stale.clone()
    second[:, :520 - 16] = gp.rne(acc)[:, :520 - 16]
    assert _close_ok(second, ref)
    # the probes' rule on the same outputs
    assert bool(gp.bitwise(gp.store_trunc(acc), acc).any())
    assert bool(gp.bitwise(gp.rne(gp.split_bf16_partial(A, W, 2)), acc).any())
