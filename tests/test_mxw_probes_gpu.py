"""The four readers of an MXFP4 weight under exact probes (tests/mxw_probes.py): mxfp4_dequant, skinny_mxfp4,
moe_skinny_mxfp4 and gemm_mxfp4_a8.

The tolerance tests of test_mxfp4_gpu.py, test_moe_mxfp4_gpu.py and test_mxfp4_a8_gpu.py (atol 3e-2, rtol 1e-2 on
dense operands; one-hot rows over scales within 2^-12 .. 2^0) accept a dropped or doubled 128-k batch of one wave
at most row counts, never read a scale byte near either end of the e8m0 range, and compare the grouped kernel with
the dense one only.  Here:

  range     the host function ``dequant_mxfp4`` is the law on every (code, byte) the format admits: the dequantiser
            bit for bit on all 16 x 255 pairs (-0, the subnormal results of bytes 0 and 1, the inf of bytes 253 and
            254), the three GEMM readers on one-hot rows over the pairs that stay finite, with unit row scales and
            with 2^(m % 5 - 2).
  dense     random codes against rows of +-1 at one k of every 8: every partial sum is exact in fp32 in any order, so
            the output is RNE(exact fp64 product) bit for bit; every m-tile count of the weight stream, the 32-column
            workgroups, K = 256 and 512 on the W4A8 pipeline, and the dequantise path.
  segments  moe_skinny_mxfp4 against the fp64 product per expert (not against the dense kernel), segment lengths
            33, 48, 0, 49, 63, 1, 64, 17, 80, plain and SwiGLU, gathered and expert-major.
  swiglu    the three epilogues on zero, moderate and saturated gates (+-96, +-200).

Every output sits in a ``Cage``; bf16 and e4m3 activations are views into NaN-filled buffers (row stride K + 64).
tests/test_mxw_probes.py shows on the CPU which family rejects which broken reader.

What the probes found on an MI355X: every family is bitwise and no sentinel is touched; no kernel needed a fix and
the admitted bytes stay 0 to 254.  ``e8m0()`` hands the convert the float ``s << 23``, which is 0.0 for byte 0; the
convert still scales by 2^-127, so it reads the operand's exponent field; the block-scaled MFMA, which is handed the
byte itself, scales by 2^-127 as well.
bf16-subnormal results (bytes 0 and 1) are kept by the convert, by both MFMAs, by the fp32 row scale and by the bf16
store; bytes 253 and 254 give inf exactly where the host function does.  One law was narrower than first written:
a GEMM reader turns a -0 weight (code 8) into +0, because its accumulator starts at +0 and (+0) + (-0) = +0; the
sign of a zero weight is the dequantiser's to show (``wp.one_hot_law``).  The +-1 rows cannot see a partial sum
that went through bf16 (a wave's partial is a bf16 number there), so the weight stream also runs on ``wide`` rows."""
import pytest
import torch

from tests import gemm_probes as gp
from tests import mxw_probes as wp

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn
_cases = {}


def _case(key, build):
    if key not in _cases:
        _cases[key] = build()
    return _cases[key]


def _weight(gpu, q, s):
    from llm_weighted_consensus_amd import ops

    return ops.Mxfp4Weight.from_packed(q.to(gpu), s.to(gpu))


def _stack(gpu, q, s):
    from llm_weighted_consensus_amd import ops

    for e in range(q.shape[0]):
        ops.check_mxfp4(q[e], s[e])
    st = ops.Mxfp4Experts.__new__(ops.Mxfp4Experts)
    st.q, st.s = q.to(gpu).contiguous(), s.to(gpu).contiguous()
    st.shape = (q.shape[0], q.shape[1], q.shape[2] * 2)
    return st


def _row_off(gpu, *lens):
    return torch.tensor((0,) + lens, device=gpu).cumsum(0).to(torch.int32)


# ---------------------------------------------------------------------------------------------------------
# 1  range


def test_range_dequant_is_bitwise_the_host_function_on_every_pair(gpu):
    from llm_weighted_consensus_amd import ops

    rw = wp.range_weight("full")
    law = ops.dequant_mxfp4(rw.q, rw.s)
    assert torch.equal(gp.bits(law), gp.bits(gp.rne(rw.W)))
    N, K = law.shape
    buf = torch.full((N * K + 64,), gp.SENTINEL, dtype=torch.int16, device=gpu).view(torch.bfloat16)
    out = ops.mxfp4_dequant(_weight(gpu, rw.q, rw.s), buf[:N * K].view(N, K))
    bad = (gp.bits(out.cpu()) != gp.bits(law)).nonzero()
    if bad.numel():
        n, k = bad[0].tolist()
        bytes_ = sorted({int(rw.s[r, c // 32]) for r, c in bad.tolist()})
        raise AssertionError(f"{len(bad)} of {N * K} values differ under bytes {bytes_}; first at (row {n}, k {k}, "
                             f"byte {int(rw.s[n, k // 32])}, code {int(rw.codes[n, k])}): got "
                             f"0x{int(gp.bits(out)[n, k]) & 0xFFFF:04x} want 0x{int(gp.bits(law)[n, k]) & 0xFFFF:04x}")
    assert bool((gp.bits(buf)[N * K:] == gp.SENTINEL).all())


def _range(gpu):
    def build():
        rw = wp.range_weight("finite")
        ks = wp.range_ks()
        return rw, ks, _weight(gpu, rw.q, rw.s), _stack(gpu, rw.q[None], rw.s[None])
    return _case("range", build)


def _one_hot(ks, K, at):
    A = torch.zeros(len(ks), K)
    A[torch.arange(len(ks)), torch.tensor(ks)] = at
    return A


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "stairs"])
@pytest.mark.parametrize("reader", ["skinny", "moe", "a8"])
def test_range_one_hot_rows_read_every_finite_pair_exactly(gpu, reader, scaled):
    """out[m, n] = RNE(W[n, k_m] * a_scale[m]): a product of one weight and a power of two, with zeros added.  The
    stairs move the subnormal results and push the top bytes over fp32's range, where the law is inf.  A -0 weight
    gives +0: the accumulator starts at +0, and (+0) + (-0) is +0 (``wp.one_hot_law``)."""
    from llm_weighted_consensus_amd import ops

    rw, ks, mw, st = _range(gpu)
    M, (N, K) = len(ks), rw.W.shape
    a = wp.a_scales(M) if scaled else torch.ones(M)
    want = wp.one_hot_law(rw.W, ks, a)
    what = f"{reader}, {'a_scale 2^(m % 5 - 2)' if scaled else 'unit a_scale'}"
    if reader == "skinny":
        A = _one_hot(ks, K, a).to(torch.bfloat16)
        for r0 in (0, 64):
            cage = gp.Cage(64, N, gpu)
            ops.skinny_mxfp4(gp.poison_a(A[r0:r0 + 64], gpu), mw, out=cage.view)
            v = wp.bit_violations(cage, want[r0:r0 + 64], ks[r0:r0 + 64], rw.s)
            assert not v, f"{what}, rows {r0}..: " + "; ".join(v)
        return
    cage = gp.Cage(M, N, gpu)
    if reader == "moe":
        A = gp.poison_a(_one_hot(ks, K, a).to(torch.bfloat16), gpu)
        ops.moe_skinny_mxfp4(A, st, _row_off(gpu, M), out=cage.view)
    else:
        A = gp.poison_a(_one_hot(ks, K, 1.0).to(E4M3), gpu)
        ops.gemm_mxfp4_a8(A, a.to(gpu), mw, out=cage.view)
    v = wp.bit_violations(cage, want, ks, rw.s)
    assert not v, f"{what}: " + "; ".join(v)


# ---------------------------------------------------------------------------------------------------------
# 2  dense


def _dense(gpu, N, K, rows, wide=False):
    def build():
        d = wp.dense_case(N, K, rows, wide)
        return d, _weight(gpu, d.q, d.s), d.want.to(gpu)
    return _case(("dense", N, K, rows, wide), build)


def _skinny_dense(gpu, N, K, M, wide=False):
    from llm_weighted_consensus_amd import ops

    d, mw, want = _dense(gpu, N, K, max(wp.SKINNY_M), wide)
    for s in wp.shifts(M):
        A = gp.poison_a(d.A[s:s + M].to(torch.bfloat16), gpu)
        cage = gp.Cage(M, N, gpu)
        ops.skinny_mxfp4(A, mw, out=cage.view)
        gp.check(cage, want[s:s + M], "bitwise", f"skinny_mxfp4 M={M} N={N} K={K} rows {s}.. wide={wide}")


@pytest.mark.parametrize("M", wp.SKINNY_M)
@pytest.mark.parametrize("N,K", wp.SKINNY_SHAPES)
def test_dense_weight_stream_is_bitwise_the_exact_product(gpu, N, K, M):
    """MT = 1 (two-batch register sets, the ``past`` branch at an odd batch count: every wave at K = 128 and 1152),
    MT = 2, MT = 4, ragged last tiles; 16 and 32 columns per workgroup."""
    _skinny_dense(gpu, N, K, M)


@pytest.mark.parametrize("N,K", wp.WIDE_SHAPES)
def test_dense_weight_stream_on_wide_rows(gpu, N, K):
    """Rows whose sums need more than 8 bits: a partial that went through bf16 before the cross-wave sum shows."""
    for M in wp.SKINNY_M:
        _skinny_dense(gpu, N, K, M, wide=True)


@pytest.mark.parametrize("M", wp.A8_M)
@pytest.mark.parametrize("N,K", wp.A8_SHAPES)
def test_dense_w4a8_is_bitwise_the_exact_product(gpu, N, K, M):
    """KT = 1, 2 (the second register stage filled once, no refill), 3, 4 and 9; one, two and three m-tiles with ragged
    ends; N below, at and past an n-tile.  Aq is a view of row stride K + 64 whose tail is e4m3 NaN."""
    from llm_weighted_consensus_amd import ops

    d, mw, want = _dense(gpu, N, K, max(wp.A8_M))
    for s in wp.shifts(M):
        A = d.A[s:s + M].to(E4M3)
        for a in (torch.ones(M), wp.a_scales(M)):
            cage = gp.Cage(M, N, gpu)
            ops.gemm_mxfp4_a8(gp.poison_a(A, gpu), a.to(gpu), mw, out=cage.view)
            ref = gp.rne(d.acc[s:s + M] * a.double()[:, None]).to(gpu)
            gp.check(cage, ref, "bitwise", f"gemm_mxfp4_a8 M={M} N={N} K={K} rows {s}.. a_scale {a[:5].tolist()}")
    if M == 129:   # contiguous rows take the same path
        cage = gp.Cage(M, N, gpu)
        ops.gemm_mxfp4_a8(d.A[:M].to(E4M3).to(gpu), torch.ones(M, device=gpu), mw, out=cage.view)
        gp.check(cage, want[:M], "bitwise", f"gemm_mxfp4_a8 M={M} N={N} K={K} contiguous")


def test_dense_dequantise_path_gives_the_same_bits(gpu):
    """linear_mxfp4 at 65 rows: the weight through the scratch, then the bf16 GEMM."""
    from llm_weighted_consensus_amd import ops

    N, K, M = 1040, 384, 65
    d, mw, want = _dense(gpu, N, K, max(wp.A8_M))
    scratch = torch.empty(N * K, dtype=torch.bfloat16, device=gpu)
    out = ops.linear_mxfp4(d.A[:M].to(torch.bfloat16).to(gpu), mw, scratch)
    bad = gp.bitwise(out, want[:M])
    assert not bool(bad.any()), f"{int(bad.sum())} outputs differ, first at {bad.nonzero()[0].tolist()}"
    assert torch.equal(scratch.view(N, K).double().cpu(), d.W)


# ---------------------------------------------------------------------------------------------------------
# 3  segments


def _segments(gpu, N, K, swiglu):
    def build():
        sg = wp.segments(N, K, torch.Generator().manual_seed(N + K + swiglu), swiglu_=swiglu)
        return sg, _stack(gpu, sg.q, sg.s)
    return _case(("segments", N, K, swiglu), build)


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "rows"])
@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("N,K", [(64, 384), (128, 1152)])
def test_segments_are_bitwise_the_exact_product_of_their_own_expert(gpu, N, K, swiglu, gather):
    """33 and 48 rows: four m-tiles of which one is wholly past the segment's end, where the next expert's rows
    lie; 49 and 63: a ragged fourth tile; 64 and 80: a whole chunk, and one more tile.  The SwiGLU stacks hold zero
    and saturated gates only, where the epilogue is exact."""
    from llm_weighted_consensus_amd import ops

    sg, st = _segments(gpu, N, K, swiglu)
    src = sg.A if gather else sg.A_em
    A = gp.poison_a(src.to(torch.bfloat16), gpu)
    NC = N // 2 if swiglu else N
    cage = gp.Cage(sg.rows, NC, gpu)
    ops.moe_skinny_mxfp4(A, st, sg.row_off.to(gpu), a_rows=sg.a_rows.to(gpu) if gather else None, rows=sg.rows,
                         out=cage.view, swiglu=swiglu)
    what = f"moe_skinny_mxfp4 N={N} K={K} swiglu={swiglu} gather={gather}"
    if swiglu:
        v = wp.swiglu_violations(cage.view, sg.gate, sg.up)
        assert not v and not cage.outside_touched(), f"{what}: " + "; ".join(v) + f"; {cage.outside_touched()} outside"
    else:
        gp.check(cage, sg.acc.to(gpu), "bitwise", what)


# ---------------------------------------------------------------------------------------------------------
# 4  swiglu

SW_ROWS, SW_F, SW_K = 136, 96, 384


def _swiglu(gpu):
    def build():
        sw = wp.swiglu(SW_ROWS, SW_F, SW_K, torch.Generator().manual_seed(9))
        return sw, _weight(gpu, sw.q, sw.s), _stack(gpu, sw.q[None], sw.s[None])
    return _case("swiglu", build)


@pytest.mark.parametrize("reader", ["skinny", "moe", "a8"])
def test_swiglu_epilogues_on_zero_moderate_and_saturated_gates(gpu, reader):
    """A zero gate gives 0 * up bit for bit (a zero with up's sign); gates of 96 and 200 give RNE(gate * up) bit for
    bit; gates of -96 and -200, where exp(-gate) is inf in fp32, give a zero; nothing is non-finite.  Moderate gates
    are within one bf16 step of the fp64 value: the sums are exact, ``__expf`` and ``rcp`` are off by a few fp32 ulps,
    far below half a bf16 step."""
    from llm_weighted_consensus_amd import ops

    sw, mw, st = _swiglu(gpu)
    runs = [(0, M) for M in (7, 17, 40, 64)] + [(72, 64)] if reader == "skinny" else [(0, SW_ROWS)]
    for r0, M in runs:
        rows = slice(r0, r0 + M)
        cage = gp.Cage(M, SW_F, gpu)
        if reader == "a8":
            ops.gemm_mxfp4_a8(gp.poison_a(sw.A[rows].to(E4M3), gpu), torch.ones(M, device=gpu), mw, out=cage.view,
                              swiglu=True)
        else:
            A = gp.poison_a(sw.A[rows].to(torch.bfloat16), gpu)
            if reader == "skinny":
                ops.skinny_mxfp4(A, mw, out=cage.view, swiglu=True)
            else:
                ops.moe_skinny_mxfp4(A, st, _row_off(gpu, M), out=cage.view, swiglu=True)
        v = wp.swiglu_violations(cage.view, sw.gate[rows], sw.up[rows])
        assert not v and not cage.outside_touched(), (f"{reader} rows {r0}..{r0 + M}: " + "; ".join(v)
                                                      + f"; {cage.outside_touched()} sentinels outside overwritten")
