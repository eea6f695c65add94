"""Dense and grouped GEMM kernels under exact inputs (tests/gemm_probes.py): bitwise outputs inside poisoned
surroundings, for gemm4w, gemm8p, the skinny GEMM, the grouped bf16 GEMM, the fp8 8-phase core and, as a
control, the library GEMM the planner also uses.

The random inputs and the 3e-2 / 1 % bound of tests/test_kernels_gpu.py accept a truncating store, a bf16
split-K partial, an epilogue operand added after rounding and a dropped k at large K, and cannot see an unwritten
tail, a store past M or N, or an operand read past its K columns or N rows.  Here every product and partial sum
is exact in fp32, so the output is determined bit for bit whatever the order of summation:

  sign     +-1 operands: one dropped, doubled or misread k element makes an even sum odd, and where
           |sum| <= 255 (asserted from the reference for >= 95 % of the outputs) that changes the stored bits.
  scaled   sign with stairs of powers of two down the rows of A and W: a row / column mix-up shows even where
           the signs agree.
  wide     integers of magnitude 1..8 (split-K cases): the partial sums need more than 8 bits, so a partial
           that went through bf16 shows.
  one-hot  one N(0, 1) value per row of A, walking every k of the first and the last K tile, both sides of
           every 32-k and 64-k boundary (and of every wave's K share in the skinny kernel): the accumulator is
           a 16-bit product, which pins round-to-nearest-even on full-mantissa values and ties, the k every lane
           reads, and an epilogue that adds its operand after rounding the product.
  epilogue operands  multiples of 0.25 within +-64 (the fp32 add is exact), and integers of magnitude 256..1024
           (the sums land where bf16 steps are 2 and 4, so the store meets ties).
  SwiGLU, row scale (RS 1)  under one_step: at most one bf16 code from the RNE code of the fp64 reference,
           exact zeros stay zero; the SwiGLU gate rows are scaled so |gate| <= 32.
  RS 2     C and the partial row sums of squares are bitwise (integers below 2^24); rows past M untouched.

A is the [:M, :K] view of a NaN buffer, W is followed by 16 NaN rows, and the output is the [:M, :NC] view of a
buffer filled with a NaN bit pattern that must be intact after EVERY launch; each case is launched two or
three times with the output poisoned again (an in-place residual: loaded again) in between, and split-K /
stream-K counters and flags must end zero.  tests/test_gemm_probes.py shows on the CPU that these checks reject
the failures listed above.

References are fp64 matmuls on the device, computed once per case and shared by the parametrisations.

Observed on an MI355X, worst distance of the one_step cases in bf16 codes (the rule allows 1): gemm4w RS 1 plain
1 (at the 4352-row shape, 0 elsewhere), gemm4w SwiGLU 0, split two ways 0, through RS 1 1; gemm8p SwiGLU 0;
skinny SwiGLU 0; fp8 core SwiGLU 0.  The one-hot residual cases are the ones that found gemm4w's block-staged
(schedule 32) and gemm8p's residual epilogues adding the residual to the bf16-rounded product."""
import numpy as np
import pytest
import torch

from tests import gemm_probes as gp

pytestmark = pytest.mark.gpu

_cases = {}


def _case(key, build):
    if key not in _cases:
        _cases[key] = build()
    return _cases[key]


def _operands(family, M, N, K, gpu, shares=1, start=0):
    """Poisoned A / W on the device, the fp64 accumulator, and (sign families) the asserted 95 % condition."""
    def build():
        gen = torch.Generator().manual_seed(M * 3 + N * 5 + K + len(family))
        unit = None
        if family == "onehot":
            A, W, _ = gp.one_hot(M, N, K, gen, gp.probe_ks(K, shares), start)
        elif family == "wide":
            A, W = gp.wide(M, N, K, gen)
        else:
            A, W = gp.sign(M, N, K, gen, scaled=family == "scaled")
            unit = gp.unit(M, N, family == "scaled")
        Ad, Wd = gp.poison_a(A, gpu), gp.poison_w(W, gpu)
        acc = gp.exact(Ad, Wd)
        if unit is not None:
            assert gp.unit_visible(acc, unit) >= 0.95, (family, M, N, K, gp.unit_visible(acc, unit))
        return Ad, Wd, acc
    return _case((family, M, N, K, shares, start), build)


def _epi_operand(kind, M, N, gpu):
    def build():
        gen = torch.Generator().manual_seed(M + N + len(kind))
        if kind == "bias":
            return gp.quarters((N,), gen).to(gpu)
        return (gp.quarters if kind == "res" else gp.big_integers)((M, N), gen).to(gpu)
    return _case((kind, M, N), build)


def _run_epilogues(call, acc, M, N, gpu, epilogues, launches=2, what=""):
    """``call(out, residual, bias)`` for every epilogue, ``launches`` times each, into a cage that is poisoned
    (residual: loaded) again before every launch and checked bitwise after every launch."""
    cage = gp.Cage(M, N, gpu)
    for epi in epilogues:
        op = None if epi == "plain" else _epi_operand(epi, M, N, gpu)
        want = gp.rne(acc if op is None else acc + op.double())
        for it in range(launches):
            if epi in ("res", "resbig"):
                out = cage.load(op)
                call(out, out, None)
            else:
                cage.poison()
                call(cage.view, None, op)
            torch.cuda.synchronize()
            gp.check(cage, want, "bitwise", f"{what} {epi} launch {it}")


def _run_one_step(call, want, M, NC, gpu, tag, launches=2):
    cage = gp.Cage(M, NC, gpu)
    for it in range(launches):
        cage.poison()
        call(cage.view)
        torch.cuda.synchronize()
        print(f"ONE_STEP {tag}: worst distance {int(gp.steps(cage.view, want).max())} bf16 codes")
        gp.check(cage, want, "one_step", f"{tag} launch {it}")


# ---------------------------------------------------------------------------------------------------------
# gemm4w


@pytest.mark.parametrize("var", [32, 64])
@pytest.mark.parametrize("bn", [256, 192])
@pytest.mark.parametrize("family", ["sign", "scaled", "onehot"])
@pytest.mark.parametrize("K", [64, 128, 192, 256, 384])
def test_gemm4w_k_loop(gpu, K, family, bn, var):
    """One K tile, prologue + peel only, odd K tile counts (VAR 32 fallback) and the first main-loop iterations,
    at a 1-row and an 8-column tail: plain, bias and both in-place residual epilogues, bitwise."""
    from llm_weighted_consensus_amd import ops

    M, N = 257, 264
    A, W, acc = _operands(family, M, N, K, gpu)
    _run_epilogues(lambda out, R, b: ops.gemm4w(A, W, residual=R, out=out, bias=b, bn=bn, var=var), acc, M, N, gpu,
                   ("plain", "bias", "res", "resbig"), what=f"gemm4w {family} K={K} bn={bn} var={var}")


@pytest.mark.parametrize("var", [32, 64])
@pytest.mark.parametrize("bn", [256, 192])
@pytest.mark.parametrize("M,N,K", [(256, 256, 14336), (300, 520, 4096)])
def test_gemm4w_long_loop(gpu, M, N, K, bn, var):
    from llm_weighted_consensus_amd import ops

    A, W, acc = _operands("sign", M, N, K, gpu)
    _run_epilogues(lambda out, R, b: ops.gemm4w(A, W, residual=R, out=out, bias=b, bn=bn, var=var), acc, M, N, gpu,
                   ("plain", "res"), what=f"gemm4w sign {M}x{N}x{K} bn={bn} var={var}")


@pytest.mark.parametrize("var", [32, 64])
@pytest.mark.parametrize("bn", [256, 192])
@pytest.mark.parametrize("gm", [0, 1, 8])
@pytest.mark.parametrize("family", ["sign", "onehot"])
def test_gemm4w_persistent_rounds(gpu, family, gm, bn, var):
    """272 (bn 256) / 374 (bn 192) tiles over 256 workgroups: every epilogue across persistent rounds, where
    VAR 64 prefetches the next tile under the epilogue, for three tile orders."""
    from llm_weighted_consensus_amd import ops

    M, N, K = 4352, 4096, 128
    A, W, acc = _operands(family, M, N, K, gpu)
    _run_epilogues(lambda out, R, b: ops.gemm4w(A, W, residual=R, out=out, bias=b, bn=bn, var=var, gm=gm), acc, M, N,
                   gpu, ("plain", "bias", "res", "resbig"), what=f"gemm4w rounds bn={bn} var={var} gm={gm}")


def _split_counters_zero(ops, M, N, bn, splits, split_from, dev):
    torch.cuda.synchronize()
    _, cnt = ops.split_workspace(M, N, bn, splits, split_from, dev)
    assert int(cnt.abs().sum()) == 0, "split-K counters left set"


@pytest.mark.parametrize("family", ["sign", "wide", "onehot"])
@pytest.mark.parametrize("split_from", [0, 4])
@pytest.mark.parametrize("splits", [2, 3, 4])
def test_gemm4w_split_k(gpu, splits, split_from, family, bn=256):
    """Split-K is bitwise: fp32 partials of exact sums add to the exact sum.  Whole and split tiles in one
    launch (split_from 4), plain and in-place residual, three launches; the counters end zero.  (The split-K
    builds are bn 256; the kernel refuses bn 192.)"""
    from llm_weighted_consensus_amd import ops

    M, N, K = 700, 520, 512
    A, W, acc = _operands(family, M, N, K, gpu)
    _run_epilogues(lambda out, R, b: ops.gemm4w(A, W, residual=R, out=out, bn=bn, var=64, splits=splits,
                                                split_from=split_from), acc, M, N, gpu, ("plain", "res"), launches=3,
                   what=f"gemm4w split {family} S={splits} from={split_from} bn={bn}")
    _split_counters_zero(ops, M, N, bn, splits, split_from, A.device)


@pytest.mark.parametrize("family", ["sign", "wide"])
def test_gemm4w_split_k_past_one_round(gpu, family):
    """160 tiles x 7 uneven units: more units than one round of workgroups."""
    from llm_weighted_consensus_amd import ops

    M, N, K, S = 2560, 4096, 1024, 7
    A, W, acc = _operands(family, M, N, K, gpu)
    _run_epilogues(lambda out, R, b: ops.gemm4w(A, W, residual=R, out=out, var=64, splits=S), acc, M, N, gpu,
                   ("plain", "res"), launches=3, what=f"gemm4w split {family} S=7")
    _split_counters_zero(ops, M, N, 256, S, 0, A.device)


# (split-K is a VAR 64 schedule and needs K / 128 >= splits: of these shapes, K = 512)
@pytest.mark.parametrize("M,N,K,splits,var", [(300, 520, 128, 1, 32), (300, 520, 128, 1, 64), (300, 4096, 512, 1, 32),
                                              (300, 4096, 512, 1, 64), (4352, 4096, 128, 1, 32),
                                              (4352, 4096, 128, 1, 64), (300, 4096, 512, 2, 64)])
def test_gemm4w_residual_rowsum_exact(gpu, M, N, K, splits, var):
    """RS 2, the residual producer of the folded RMSNorm: C bitwise, and the N / 256 partial row sums of squares
    of the stored bf16 values bitwise — they are integers with |C| <= 320 (asserted), so every partial is an
    integer of at most 256 * 320^2 < 2^24, exact in fp32 in any order.  Rows of ss past M are untouched."""
    from llm_weighted_consensus_amd import ops

    A, W, acc = _operands("sign", M, N, K, gpu)
    gen = torch.Generator().manual_seed(M + N)
    R = torch.randint(-64, 65, (M, N), generator=gen).to(torch.bfloat16).to(gpu)
    want = gp.rne(acc + R.double())
    assert float(want.float().abs().max()) <= 320 and bool((want.float() % 1 == 0).all())
    P = (N + 255) // 256
    pad = torch.zeros(M, P * 256, dtype=torch.float64, device=gpu)
    pad[:, :N] = want.double()
    parts = pad.pow(2).view(M, P, 256).sum(-1).t().float()
    chain = ops.NormChain(M + 64, 4096, 1e-5, gpu)
    cage = gp.Cage(M, N, gpu)
    for it in range(3):
        chain.ss.fill_(-7.0)
        out = cage.load(R)
        ops.gemm4w(A, W, residual=out, out=out, chain=chain, var=var, splits=splits)
        torch.cuda.synchronize()
        gp.check(cage, want, "bitwise", f"RS 2 launch {it}")
        assert chain.P == P
        assert torch.equal(chain.ss[:P, :M], parts), (it, (chain.ss[:P, :M] - parts).abs().max())
        assert bool((chain.ss[:P, M:] == -7.0).all()) and bool((chain.ss[P:] == -7.0).all())
    if splits > 1:
        _split_counters_zero(ops, M, N, 256, splits, 0, A.device)


def _chain_with_partials(ops, M, K, P, gpu, lo=0.01):
    """A chain whose P partials per row are random fp32 (>= ``lo``); partials the call does not use are NaN.
    -> (chain, fp64 row scales rsqrt(sum / K + eps))."""
    chain = ops.NormChain(M + 64, 4096, 1e-5, gpu)
    gen = torch.Generator().manual_seed(M + K + P)
    chain.ss.fill_(float("nan"))
    chain.ss[:P] = 0.0         # (a tile's DMA reads the partials of all its 256 rows, past M too)
    chain.ss[:P, :M] = (torch.rand(P, M, generator=gen) * K / P + lo).to(gpu)
    chain.P = P
    return chain, torch.rsqrt(chain.ss[:P, :M].double().sum(0) / K + 1e-5)


@pytest.mark.parametrize("M,N,K,P,bn,splits,var", [
    (257, 264, 128, 3, 256, 1, 32), (257, 264, 128, 3, 256, 1, 64), (257, 264, 192, 1, 192, 1, 32),
    (257, 264, 256, 2, 192, 1, 64), (4352, 4096, 128, 16, 256, 1, 32), (4352, 4096, 128, 16, 256, 1, 64),
    (4352, 4096, 128, 16, 192, 1, 32), (4352, 4096, 128, 16, 192, 1, 64), (300, 520, 512, 3, 256, 2, 64)])
def test_gemm4w_rowscale_one_step(gpu, M, N, K, P, bn, splits, var):
    """RS 1, the row-scaled consumer, plain epilogue: random fp32 partials, output within one bf16 code of the
    fp64 reference sum * rsqrt(partials / K + eps); >= 90 % of the sums lie in the band |sum| < 128 where a
    unit error moves the value by more than a step."""
    from llm_weighted_consensus_amd import ops

    A, W, acc = _operands("sign", M, N, K, gpu)
    assert gp.in_band(acc) >= 0.90
    chain, r = _chain_with_partials(ops, M, K, P, gpu)
    _run_one_step(lambda out: ops.gemm4w(A, W, out=out, bn=bn, chain=chain, var=var, splits=splits),
                  acc * r[:, None], M, N, gpu, f"gemm4w rs1 bn={bn} var={var} S={splits}")
    if splits > 1:
        _split_counters_zero(ops, M, N, bn, splits, 0, A.device)


def _swiglu_operands(ops, M, F, K, gpu):
    def build():
        gen = torch.Generator().manual_seed(M + F + K)
        A, W = gp.swiglu_sign(M, F, K, gen)
        Ad, Wd = gp.poison_a(A, gpu), gp.poison_w(ops.swiglu_interleave(W), gpu)
        acc = gp.exact(Ad, W.to(gpu))
        gate, up = acc[:, :F], acc[:, F:]
        assert float(gate.abs().max()) <= 32 and gp.in_band(up) >= 0.90
        return Ad, Wd, gate, up
    return _case(("swiglu", M, F, K), build)


@pytest.mark.parametrize("M,N,K,mode,var", [
    (257, 576, 128, "plain", 32), (257, 576, 128, "plain", 64), (257, 576, 192, "plain", 32),
    (257, 576, 192, "plain", 64), (257, 576, 4096, "plain", 32), (257, 576, 4096, "plain", 64),
    (4352, 4096, 128, "plain", 32), (4352, 4096, 128, "plain", 64), (257, 576, 4096, "split2", 64),
    (4352, 4096, 256, "split2", 64), (257, 576, 128, "rs1", 32), (257, 576, 4096, "rs1", 64),
    (4352, 4096, 128, "rs1", 32), (4352, 4096, 128, "rs1", 64)])
def test_gemm4w_swiglu_one_step(gpu, M, N, K, mode, var):
    """SwiGLU epilogue (bn 256) over interleaved gate|up sign rows with |gate| <= 32: within one bf16 code of
    fp64 silu(gate) * up; also split two ways, and through the row-scaled consumer (RS 1: the reference
    scales gate and up by the row's rsqrt first; partials >= K / P keep the scale <= 1 and |gate| <= 32)."""
    from llm_weighted_consensus_amd import ops

    F = N // 2
    A, W, gate, up = _swiglu_operands(ops, M, F, K, gpu)
    kw = {}
    if mode == "rs1":
        chain, r = _chain_with_partials(ops, M, K, 3, gpu, lo=K / 3)
        assert float(r.max()) <= 1.0
        gate, up, kw = gate * r[:, None], up * r[:, None], {"chain": chain}
    elif mode == "split2":
        kw = {"splits": 2}
    _run_one_step(lambda out: ops.gemm4w(A, W, out=out, swiglu=True, var=var, **kw), gp.silu_mul(gate, up), M, F,
                  gpu, f"gemm4w swiglu {mode} var={var}")
    if mode == "split2":
        _split_counters_zero(ops, M, N, 256, 2, 0, A.device)


# ---------------------------------------------------------------------------------------------------------
# gemm8p


@pytest.mark.parametrize("family", ["sign", "scaled", "onehot"])
@pytest.mark.parametrize("M,N,K", [(200, 8, 64), (300, 520, 128), (700, 256, 512), (3072, 6144, 256)])
def test_gemm8p_bitwise(gpu, M, N, K, family):
    """One partial tile of one K tile; ragged tails; 3 tiles over 8 workgroups (every tile split mid-K by
    stream-K); 288 tiles (stream-K plus data-parallel rounds).  Plain, bias and both in-place residuals, each
    launched twice; the stream-K flags end zero."""
    from llm_weighted_consensus_amd import ops

    A, W, acc = _operands(family, M, N, K, gpu)
    _run_epilogues(lambda out, R, b: ops.gemm8p(A, W, residual=R, out=out, bias=b), acc, M, N, gpu,
                   ("plain", "res", "resbig", "bias"), what=f"gemm8p {family} {M}x{N}x{K}")
    torch.cuda.synchronize()
    assert int(ops.gemm8p_workspace(A.device)[1].abs().sum()) == 0, "stream-K flags left set"


@pytest.mark.parametrize("M,N,K", [(700, 256, 512), (3072, 6144, 256), (257, 576, 4096)])
def test_gemm8p_swiglu_one_step(gpu, M, N, K):
    from llm_weighted_consensus_amd import ops

    A, W, gate, up = _swiglu_operands(ops, M, N // 2, K, gpu)
    _run_one_step(lambda out: ops.gemm8p(A, W, out=out, swiglu=True), gp.silu_mul(gate, up), M, N // 2, gpu,
                  "gemm8p swiglu")
    assert int(ops.gemm8p_workspace(A.device)[1].abs().sum()) == 0, "stream-K flags left set"


# ---------------------------------------------------------------------------------------------------------
# skinny GEMM


@pytest.mark.parametrize("family", ["sign", "scaled", "onehot"])
@pytest.mark.parametrize("N,K", [(16, 2048), (1040, 2048), (64, 4096)])
@pytest.mark.parametrize("M", [1, 7, 16, 17, 33, 64])
def test_skinny_bitwise(gpu, M, N, K, family):
    """Every m-tile count with ragged rows, one workgroup / 65 workgroups, plain and in-place residual.  The
    one-hot k starts with the first and last k of each of the 8 waves' K shares, then both sides of every
    64-k and 32-k boundary; each M continues the walk where the smaller M stopped."""
    from llm_weighted_consensus_amd import ops

    start = {1: 0, 7: 1, 16: 8, 17: 24, 33: 41, 64: 74}[M]
    A, W, acc = _operands(family, M, N, K, gpu, shares=8, start=start)
    _run_epilogues(lambda out, R, b: ops.skinny_gemm(A, W, residual=R, out=out), acc, M, N, gpu,
                   ("plain", "res", "resbig"), what=f"skinny {family} {M}x{N}x{K}")


@pytest.mark.parametrize("N,K", [(64, 4096), (1088, 2048)])
@pytest.mark.parametrize("M", [1, 7, 16, 17, 33, 64])
def test_skinny_swiglu_one_step(gpu, M, N, K):
    from llm_weighted_consensus_amd import ops

    A, W, gate, up = _swiglu_operands(ops, M, N // 2, K, gpu)
    _run_one_step(lambda out: ops.skinny_gemm(A, W, out=out, swiglu=True), gp.silu_mul(gate, up), M, N // 2, gpu,
                  "skinny swiglu")


# ---------------------------------------------------------------------------------------------------------
# grouped bf16 GEMM


@pytest.mark.parametrize("family", ["sign", "onehot"])
@pytest.mark.parametrize("splits", [None, 3])
def test_grouped_gemm_bitwise(gpu, splits, family):
    """Expert segments incl. an empty and a 7-row group, bias in multiples of 0.25, one workgroup per tile or
    split three ways over K (fp32 atomics: exact sums add in any order): bitwise per group; the rows around
    the empty group hold their own groups' values and nothing outside the output is touched."""
    from llm_weighted_consensus_amd import ops

    G, N, K = 4, 384, 256
    sizes = [130, 0, 7, 300]
    rows = sum(sizes)
    o = [0] + [int(v) for v in np.cumsum(sizes)]
    off = torch.tensor(o, dtype=torch.int32, device=gpu)
    A, _, _ = _operands(family, rows, 8, K, gpu)
    gen = torch.Generator().manual_seed(K + len(family))
    if family == "sign":
        W = torch.stack([gp.sign(8, N, K, gen)[1] for _ in range(G)])
    else:
        W = (torch.randn(G, N, K, generator=gen) / K ** 0.5).to(torch.bfloat16)
    W = gp.poison_w(W, gpu)
    bias = gp.quarters((G, N), gen).to(gpu)
    want = torch.zeros(rows, N, dtype=torch.float64, device=gpu)
    for g in range(G):
        acc = gp.exact(A[o[g]:o[g + 1]], W[g])
        assert family != "sign" or o[g + 1] == o[g] or gp.unit_visible(acc) >= 0.95
        want[o[g]:o[g + 1]] = acc + bias[g].double()
    cage = gp.Cage(rows, N, gpu)
    for it in range(2):
        cage.poison()
        ops.grouped_gemm(A, W, off, out=cage.view, bias=bias, splits=splits)
        torch.cuda.synchronize()
        gp.check(cage, want, "bitwise", f"grouped {family} splits={splits} launch {it}")


# ---------------------------------------------------------------------------------------------------------
# fp8 8-phase core


def _fp8_case(M, N, K, gpu, swiglu=False):
    def build():
        from llm_weighted_consensus_amd import ops

        gen = torch.Generator().manual_seed(M + N + K + swiglu)
        A, W, a_s, w_s = gp.fp8_operands(M, N, K, gen)
        if swiglu:   # |gate| <= 4 K * 1 * 2^-ceil(log2(K / 8)) <= 32
            a_s = a_s.clamp(0.5, 1.0)
            w_s[:N // 2] = 2.0 ** -max(0, (K // 8 - 1).bit_length())
        acc = gp.exact(A.float().to(gpu), W.float().to(gpu))
        assert gp.unit_visible(acc) >= 0.95
        want = acc * (a_s[:, None] * w_s[None, :]).double().to(gpu)
        Wq, ws = W.float(), w_s
        if swiglu:
            F = N // 2
            Wq = ops.swiglu_interleave(Wq)
            ws = ops.swiglu_interleave(w_s.view(-1, 1)).view(-1)
            assert float(want[:, :F].abs().max()) <= 32
            want = gp.silu_mul(want[:, :F], want[:, F:])
        w = ops.Fp8Weight.__new__(ops.Fp8Weight)   # fields set directly: quant_fp8_weight's scales are not exact
        w.q = gp.poison_w(Wq.to(torch.float8_e4m3fn), gpu)
        w.s = ws.view(1, -1).contiguous().to(gpu)
        w.shape = (N, K)
        return gp.poison_a(A, gpu), a_s.to(gpu), w, want
    return _case(("fp8", M, N, K, swiglu), build)


@pytest.mark.parametrize("M,N,K", [(1, 512, 256), (255, 640, 512), (513, 264, 128)])
def test_gemm8g_dense_bitwise(gpu, M, N, K):
    """e4m3 operands in {+-1, +-2}, power-of-two row and channel scales set directly on an Fp8Weight: the fp32
    accumulator and both scalings are exact, so the bf16 output is bitwise."""
    from llm_weighted_consensus_amd import ops

    A, a_s, w, want = _fp8_case(M, N, K, gpu)
    cage = gp.Cage(M, N, gpu)
    for it in range(2):
        cage.poison()
        ops.gemm8g_dense(A, a_s, w, out=cage.view)
        torch.cuda.synchronize()
        gp.check(cage, want, "bitwise", f"gemm8g dense launch {it}")


@pytest.mark.parametrize("M,N,K", [(1, 512, 256), (255, 640, 512)])
def test_gemm8g_dense_swiglu_one_step(gpu, M, N, K):
    from llm_weighted_consensus_amd import ops

    A, a_s, w, want = _fp8_case(M, N, K, gpu, swiglu=True)
    _run_one_step(lambda out: ops.gemm8g_dense(A, a_s, w, out=out, swiglu=True), want, M, N // 2, gpu,
                  "gemm8g swiglu")


@pytest.mark.parametrize("gather", [False, True])
def test_gemm8g_grouped_bitwise(gpu, gather):
    """The grouped call of test_gemm8g_grouped_fp8_matches_reference (empty, < one tile, several tiles, a partial
    last tile), with and without the A-row gather; the A rows no output row names are NaN."""
    from llm_weighted_consensus_amd import ops

    G, N, K = 5, 640, 512
    sizes = [300, 0, 17, 700, 256]
    rows = sum(sizes)
    o = [0] + [int(v) for v in np.cumsum(sizes)]
    off = torch.tensor(o, dtype=torch.int32, device=gpu)
    gen = torch.Generator().manual_seed(11)
    rows_a = rows + 37 if gather else rows
    A, _, a_s, _ = gp.fp8_operands(rows_a, 8, K, gen)
    W, _, w_s, _ = gp.fp8_operands(G * N, 8, K, gen)
    a_rows = torch.randperm(rows_a, generator=gen)[:rows].to(torch.int32) if gather else None
    src = a_rows.long() if gather else torch.arange(rows)
    Af, asf = A.float()[src].to(gpu), a_s[src].double().to(gpu)
    if gather:
        unused = torch.ones(rows_a, dtype=torch.bool)
        unused[src] = False
        A.view(torch.uint8)[unused] = gp.SENTINEL8
    want = torch.zeros(rows, N, dtype=torch.float64, device=gpu)
    Wf, wsf = W.float().view(G, N, K).to(gpu), w_s.view(G, N).double().to(gpu)
    for g in range(G):
        sl = slice(o[g], o[g + 1])
        want[sl] = gp.exact(Af[sl], Wf[g]) * asf[sl, None] * wsf[g][None, :]
    Ad, Wd = gp.poison_a(A, gpu), gp.poison_w(W.view(G, N, K), gpu)
    a_rows_d = a_rows.to(gpu) if gather else None
    a_s_d, w_s_d = a_s.to(gpu).contiguous(), w_s.to(gpu).contiguous()
    cage = gp.Cage(rows, N, gpu)
    for it in range(2):
        cage.poison()
        ops.kernels().gemm8g_fp8(Ad, Wd, cage.view, off, -(-rows // 256) + G, a_rows_d, a_s_d, w_s_d, 0, None, None)
        torch.cuda.synchronize()
        gp.check(cage, want, "bitwise", f"gemm8g grouped gather={gather} launch {it}")


# ---------------------------------------------------------------------------------------------------------
# control


@pytest.mark.parametrize("family", ["sign", "onehot"])
@pytest.mark.parametrize("M,N,K", [(257, 264, 64), (257, 264, 384), (300, 520, 4096), (256, 256, 14336)])
def test_library_gemm_meets_the_premise(gpu, M, N, K, family):
    """Control: torch.nn.functional.linear in bf16 (the library GEMM the planner also uses) on the plain cases
    under the same bitwise rule — exact fp32 accumulation with a round-to-nearest-even store is not a property
    of the hand-written kernels alone."""
    A, W, acc = _operands(family, M, N, K, gpu)
    out = torch.nn.functional.linear(A, W)
    bad = gp.bitwise(out, acc)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} outputs differ"
