"""MXFP4 MoE experts with e4m3 activations on the GPU (csrc/kernels/moe_mxfp4_a8.hip, ``expert_act="e4m3"``).

Kernel: the grouped W4A8 GEMM bit for bit against the dense kernel on every segment, with poisoned surroundings;
exact one-hot rows through the gather; the exact fp64 product of the quantised operands; segment bounds and gather
straight from ``ops.route`` at 128 experts; row independence; device-side bounds under a captured graph; the host
refusals.  Model, at ``qwen3-moe-tiny`` and ``mixtral-tiny``: one layer and the whole model against the emulated fp32
oracle (tests/moe_mxfp4_a8_ref.py) and the unquantised twin, what the model keeps resident, the engine and the worker
factory."""
import copy

import pytest
import torch

from tests import moe_mxfp4_a8_ref, qwen_moe_ref
from tests import torch_ref as ref
from tests.qwen_ref import row_cosines
from tests.test_moe_mxfp4_gpu import _row_off, _stack, _twin_layer
from tests.test_mxfp4_a8_gpu import _acts, _bits, _close, _exact, _i32, _probe_columns, _weight

pytestmark = pytest.mark.gpu

# Whole-model bounds.  Against the unquantised twin (the fp32 oracle on the dequantised experts): the fp8 decoders'
# 0.99.  Against the emulated oracle (the same, with the MoE MLP's input rows and SwiGLU output row-quantised to e4m3):
# 1 - 4 * (largest measured 1 - cos over seeds 2, 3, 4 and every compared logits row: the prefill's last token and 7
# decode steps, every step on the W4A8 kernel), never below 0.99.
# Measured on an MI355X, largest 1 - cos for seeds 2, 3, 4:
#   qwen3-moe-tiny  3.385e-4, 3.077e-4, 2.601e-4   ->  1 - 4 * 3.385e-4 = 0.99865
#   mixtral-tiny    1.704e-4, 1.288e-4, 1.453e-4   ->  1 - 4 * 1.704e-4 = 0.99932
# (against the unquantised twin, same seeds: 3.024e-4, 3.508e-4, 8.094e-5 and 1.510e-4, 1.360e-4, 1.230e-4.  The
# emulated oracle is no nearer than the twin: it quantises the fp32 forward's rows, the model its bf16 rows, and a row
# that differs in its last bits falls on other e4m3 codes.  One layer on the same rows agrees to the bf16 bound:
# test_one_moe_layer.)
MEASURED = {"qwen3-moe-tiny": 3.385e-4, "mixtral-tiny": 1.704e-4}
COS_BOUND = {a: max(0.99, 1 - 4 * v) for a, v in MEASURED.items()}
COS_PLAIN = 0.99

LENS = {"short": [0, 1, 17, 128, 0], "long": [129, 0, 300, 16, 1]}


def _take(aq, idx):
    """Rows ``idx`` of an e4m3 tensor (gathered as bytes), contiguous."""
    return aq.view(torch.uint8)[idx.long()].contiguous().view(torch.float8_e4m3fn)


def _src(a_rows, lo, hi, dev):
    return a_rows[lo:hi].long() if a_rows is not None else torch.arange(lo, hi, device=dev)


def _check_segments(st, aq, xs, a_rows, row_off, out, swiglu):
    """Every expert's segment equals the dense kernel on those rows (and their scales), by bit pattern."""
    from llm_weighted_consensus_amd import ops

    ro = row_off.tolist()
    for e in range(st.shape[0]):
        if ro[e + 1] == ro[e]:
            continue
        idx = _src(a_rows, ro[e], ro[e + 1], out.device)
        want = ops.gemm_mxfp4_a8(_take(aq, idx), xs[idx].contiguous(), st.expert(e), swiglu=swiglu)
        bad = (_bits(out[ro[e]:ro[e + 1]]) != _bits(want)).nonzero()
        assert bad.numel() == 0, f"expert {e} ({ro[e + 1] - ro[e]} rows): first mismatch {bad[0].tolist()}"


def _run_poisoned(gpu, st, aq, xs, row_off, a_rows, rows, swiglu):
    """The op into a view of a 123.0-filled buffer; the padding stays untouched."""
    from llm_weighted_consensus_amd import ops

    NC = st.shape[1] // 2 if swiglu else st.shape[1]
    buf = torch.full((rows + 3, NC + 16), 123.0, dtype=torch.bfloat16, device=gpu)
    out = ops.moe_gemm_mxfp4_a8(aq, xs, st, row_off, a_rows=a_rows, rows=rows, out=buf[:rows, :NC], swiglu=swiglu)
    assert out.data_ptr() == buf.data_ptr() and out.shape == (rows, NC)
    assert bool(torch.isfinite(out.float()).all())
    assert bool((buf[rows:] == 123.0).all()) and bool((buf[:, NC:] == 123.0).all())
    return out


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("gather", [True, False], ids=["gather", "rows"])
@pytest.mark.parametrize("lens", ["short", "long"])
@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("N,K", [(64, 384), (128, 1152)])
def test_bitwise_the_dense_kernel_and_nothing_else_written(gpu, N, K, swiglu, lens, gather):
    """An empty segment, one row, a ragged tile, exactly one tile, a tile plus one row, several tiles.  ``Aq`` is a
    view with ``lda = K + 64`` whose padding holds e4m3 3.0; the gather repeats source rows, as a token in k experts
    does; ``out`` is a view into a buffer filled with 123.0."""
    lens = LENS[lens]
    st = _stack(gpu, 5, N, K, swiglu)
    rows, row_off = sum(lens), _row_off(gpu, lens)
    T = 23 if gather else rows
    aq, xs = _acts(gpu, T, K, N + K + rows, lda=K + 64)
    assert aq.stride(0) == K + 64
    a_rows = ((torch.arange(rows, device=gpu) * 7 + 3) % T).to(torch.int32) if gather else None
    out = _run_poisoned(gpu, st, aq, xs, row_off, a_rows, rows, swiglu)
    _check_segments(st, aq, xs, a_rows, row_off, out, swiglu)


def test_bitwise_the_dense_kernel_at_a_ragged_column_tile(gpu):
    """N = 1040 = 8 x 128 + 16: the ninth n-tile (the first of XCD 0's second round) holds 16 live columns."""
    K, lens = 384, LENS["long"]
    st = _stack(gpu, 5, 1040, K)
    rows, row_off = sum(lens), _row_off(gpu, lens)
    aq, xs = _acts(gpu, 23, K, 1040, lda=K + 64)
    a_rows = ((torch.arange(rows, device=gpu) * 7 + 3) % 23).to(torch.int32)
    out = _run_poisoned(gpu, st, aq, xs, row_off, a_rows, rows, False)
    _check_segments(st, aq, xs, a_rows, row_off, out, False)


def test_onehot_rows_through_the_gather_read_single_weights_exactly(gpu):
    """Token row m is e4m3 1.0 at one k_m (``_probe_columns``), over a stack whose scales cover 13 exponents, a
    different one per (expert, row, block): out[r, n] is dq[e(r), n, k_src(r)] bit for bit (the product and the sums
    with zeros are exact, the value is a bf16), then times the token's scale 2^(m % 5 - 2), still exact.  Pins which k
    meets which code and scale byte of which expert, and that the scale is the token's, without the dense kernel."""
    from llm_weighted_consensus_amd import ops

    E, N, K, M = 5, 64, 1152, 80
    dq = _weight(gpu, E * N, K, "spread")[1].view(E, N, K)
    st = ops.Mxfp4Experts(dq)
    assert torch.equal(_bits(st.dequant()), _bits(dq))  # (quantising the dequantised stack changes nothing)
    lens = [17, 0, 130, 12, 1]
    rows, row_off = sum(lens), _row_off(gpu, lens)
    a_rows = ((torch.arange(rows, device=gpu) * 7 + 3) % M).to(torch.int32)
    src = a_rows.long()
    expert = torch.repeat_interleave(torch.arange(E, device=gpu), torch.tensor(lens, device=gpu))
    m = torch.arange(M, device=gpu)
    for launch in range(3):
        ks = torch.tensor(_probe_columns(K, launch), device=gpu)
        A = torch.zeros(M, K, device=gpu)
        A[m, ks] = 1.0
        Aq = A.to(torch.float8_e4m3fn)
        for what, sc in (("unit", torch.ones(M, device=gpu)), ("power-of-two", torch.exp2(((m % 5) - 2).float()))):
            out = ops.moe_gemm_mxfp4_a8(Aq, sc, st, row_off, a_rows=a_rows, rows=rows)
            exact = dq[expert, :, ks[src]].float() * sc[src].view(-1, 1)
            want = exact.to(torch.bfloat16)
            assert torch.equal(want.float(), exact)  # (the reference is exact)
            bad = (_bits(out) != _bits(want)).nonzero()
            assert bad.numel() == 0, (f"launch {launch}, {what} row scales: {bad.shape[0]} mismatches, first (r, n) = "
                                      f"{bad[0].tolist()}, token {int(src[bad[0][0]])}, k {int(ks[src[bad[0][0]]])}")


def _deinterleave(y):
    """[M, 2F] in the 32-row gate|up interleave -> (gate [M, F], up [M, F])."""
    M, F_ = y.shape[0], y.shape[1] // 2
    y = y.view(M, F_ // 32, 2, 32)
    return y[:, :, 0].reshape(M, F_), y[:, :, 1].reshape(M, F_)


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
def test_matches_the_exact_product_of_the_quantised_operands(gpu, swiglu):
    """Both operands are exact in fp32, so kernel and fp64 reference differ by the accumulation order and one bf16
    rounding: the dense test's bound."""
    from llm_weighted_consensus_amd import ops

    N, K, lens = 128, 1152, LENS["long"]
    st = _stack(gpu, 5, N, K, swiglu)
    dq = st.dequant()
    rows, row_off = sum(lens), _row_off(gpu, lens)
    aq, xs = _acts(gpu, 40, K, 3)
    a_rows = ((torch.arange(rows, device=gpu) * 11 + 1) % 40).to(torch.int32)
    out = ops.moe_gemm_mxfp4_a8(aq, xs, st, row_off, a_rows=a_rows, rows=rows, swiglu=swiglu)
    ro = row_off.tolist()
    want = []
    for e in range(5):
        idx = a_rows[ro[e]:ro[e + 1]].long()
        y = _exact(_take(aq, idx), xs[idx], dq[e])
        if swiglu:
            g, u = _deinterleave(y)
            y = torch.nn.functional.silu(g) * u
        want.append(y)
    _close(out, torch.cat(want), 3e-2, 1e-2)


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
def test_wide_and_sparse_bounds_from_the_router(gpu, swiglu):
    """E = 128 (two steps of the 64-lane search), 40 rows (T = 5, k = 8) with ``row_off`` and the gather as
    ``ops.route`` returns them: at least 88 experts idle.  Then all 40 rows in expert 77, the first and the last
    expert empty."""
    from llm_weighted_consensus_amd import ops

    E, N, K, T, k = 128, 64, 384, 5, 8
    st = _stack(gpu, E, N, K, swiglu)
    h = torch.randn(T, K, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16).to(gpu)
    router = torch.randn(E, K, generator=torch.Generator().manual_seed(12)).to(torch.bfloat16).to(gpu)
    _, _, row_off, src, _ = ops.route(h, router, k)
    assert row_off.dtype == torch.int32 and row_off.shape == (E + 1,) and int(row_off[-1]) == T * k
    one = torch.zeros(E + 1, dtype=torch.int32, device=gpu)
    one[78:] = T * k
    aq, xs = ops.quant_fp8_rows(h)
    for ro in (row_off, one):
        out = _run_poisoned(gpu, st, aq, xs, ro, src, T * k, swiglu)
        _check_segments(st, aq, xs, src, ro, out, swiglu)


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
def test_a_row_does_not_depend_on_its_neighbours(gpu, swiglu):
    """One token through expert 2: routed alone, as row 127 of a 128-row tile, and as row 129 of a 140-row segment
    (in its second tile, with other experts' rows around): the same bits each time, those of the dense kernel."""
    from llm_weighted_consensus_amd import ops

    N, K = 128, 1152
    st = _stack(gpu, 5, N, K, swiglu)
    aq, xs = _acts(gpu, 160, K, 5)  # row 0 is the probe
    got = []
    for lens, pos in (([0, 0, 1, 0, 0], 0), ([3, 0, 128, 2, 0], 3 + 127), ([7, 1, 140, 0, 5], 8 + 129)):
        rows = sum(lens)
        a_rows = torch.arange(1, rows + 1, dtype=torch.int32, device=gpu)
        a_rows[pos] = 0
        out = ops.moe_gemm_mxfp4_a8(aq, xs, st, _row_off(gpu, lens), a_rows=a_rows, rows=rows, swiglu=swiglu)
        got.append(_bits(out[pos]).clone())
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    assert torch.equal(got[0], _bits(ops.gemm_mxfp4_a8(aq[:1], xs[:1], st.expert(2), swiglu=swiglu)[0]))


def test_bounds_are_read_on_the_device_under_a_graph(gpu):
    """The op captured once (a single chain); ``row_off`` and ``a_rows`` rewritten in place; the replay equals an
    eager call on the new values, bit for bit."""
    from llm_weighted_consensus_amd import ops

    st = _stack(gpu, 5, 128, 1152, True)
    rows = 300
    aq, xs = _acts(gpu, 16, 1152, 31)
    row_off = _row_off(gpu, [60, 60, 60, 60, 60])
    a_rows = (torch.arange(rows, device=gpu) % 16).to(torch.int32)
    out = torch.zeros(rows, 64, dtype=torch.bfloat16, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        ops.moe_gemm_mxfp4_a8(aq, xs, st, row_off, a_rows=a_rows, rows=rows, out=out, swiglu=True)
    torch.cuda.current_stream(gpu).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.moe_gemm_mxfp4_a8(aq, xs, st, row_off, a_rows=a_rows, rows=rows, out=out, swiglu=True)
    first = out.clone()
    row_off.copy_(_row_off(gpu, [0, 257, 0, 1, 42]))
    a_rows.copy_(((torch.arange(rows, device=gpu) * 5 + 2) % 16).to(torch.int32))
    out.zero_()
    g.replay()
    torch.cuda.synchronize(gpu)
    eager = ops.moe_gemm_mxfp4_a8(aq, xs, st, row_off, a_rows=a_rows, rows=rows, swiglu=True)
    assert torch.equal(_bits(out), _bits(eager)) and not torch.equal(_bits(out), _bits(first))


def test_wrappers_quantise_tokens_once_and_take_pairs(gpu):
    """``moe_swiglu_mxfp4_a8`` on bf16 token rows, a QAct and an (xq, xs) pair; ``moe_linear_mxfp4_a8`` on bf16 rows:
    the bits of the op on ``quant_fp8_rows`` of those rows."""
    from llm_weighted_consensus_amd import ops

    w13, w2 = _stack(gpu, 5, 128, 1152, True), _stack(gpu, 5, 64, 384)
    lens = LENS["long"]
    rows, row_off = sum(lens), _row_off(gpu, lens)
    x = torch.randn(50, 1152, generator=torch.Generator().manual_seed(21)).to(torch.bfloat16).to(gpu)
    a_rows = ((torch.arange(rows, device=gpu) * 3 + 2) % 50).to(torch.int32)
    xq, xs = ops.quant_fp8_rows(x)
    want = ops.moe_gemm_mxfp4_a8(xq, xs, w13, row_off, a_rows=a_rows, rows=rows, swiglu=True)
    assert want.shape == (rows, 64) and want.dtype == torch.bfloat16
    for arg in (x, ops.QAct(None, xq, xs), (xq, xs)):
        assert torch.equal(_bits(ops.moe_swiglu_mxfp4_a8(arg, w13, row_off, a_rows, rows)), _bits(want))
    a2 = torch.randn(rows, 384, generator=torch.Generator().manual_seed(22)).to(torch.bfloat16).to(gpu)
    want = ops.moe_gemm_mxfp4_a8(*ops.quant_fp8_rows(a2), w2, row_off)
    assert want.shape == (rows, 64)
    assert torch.equal(_bits(ops.moe_linear_mxfp4_a8(a2, w2, row_off)), _bits(want))
    assert torch.equal(_bits(ops.moe_linear_mxfp4_a8(ops.quant_fp8_rows(a2), w2, row_off)), _bits(want))


def test_refusals_on_the_host(gpu):
    from llm_weighted_consensus_amd import ops

    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=gpu)  # noqa: E731
    q = lambda *s: torch.zeros(*s, device=gpu).to(torch.float8_e4m3fn)  # noqa: E731
    one = lambda n: torch.ones(n, device=gpu)  # noqa: E731
    ro = _row_off(gpu, [2, 2])
    bad = ops.Mxfp4Experts(z(2, 16, 160))
    assert not ops.moe_mxfp4_a8_ok(4, 160, 4, bad)
    with pytest.raises(RuntimeError, match="K % 128 == 0.*got K = 160"):
        ops.moe_gemm_mxfp4_a8(q(4, 160), one(4), bad, ro)
    bad = ops.Mxfp4Experts(z(2, 32, 128))
    assert ops.moe_mxfp4_a8_ok(4, 128, 4, bad) and not ops.moe_mxfp4_a8_ok(4, 128, 4, bad, swiglu=True)
    with pytest.raises(RuntimeError, match="SwiGLU: N % 64 == 0.*got K = 128, N = 32"):
        ops.moe_gemm_mxfp4_a8(q(4, 128), one(4), bad, ro, swiglu=True)
    bad = ops.Mxfp4Experts(z(2, 24, 128))
    assert not ops.moe_mxfp4_a8_ok(4, 128, 4, bad)
    with pytest.raises(RuntimeError, match="N % 16 == 0.*got K = 128, N = 24"):
        ops.moe_gemm_mxfp4_a8(q(4, 128), one(4), bad, ro)
    st = ops.Mxfp4Experts(z(2, 16, 128))
    assert ops.moe_mxfp4_a8_ok(4, 128, 4, st)
    for dt in (torch.bfloat16, torch.float8_e5m2):
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            ops.moe_gemm_mxfp4_a8(torch.zeros(4, 128, device=gpu).to(dt), one(4), st, ro)
    with pytest.raises(RuntimeError, match="a_scale must hold one scale per row of A \\(4\\), got 3"):
        ops.moe_gemm_mxfp4_a8(q(4, 128), one(3), st, ro)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.moe_gemm_mxfp4_a8(q(4, 256), one(4), st, ro)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.moe_gemm_mxfp4_a8(q(4, 128), one(4), st, ro, out=z(4, 8))
    with pytest.raises(RuntimeError, match="row_off has dtype"):
        ops.moe_gemm_mxfp4_a8(q(4, 128), one(4), st, ro.long())
    with pytest.raises(RuntimeError, match="row_off has 4 elements, expected 3"):
        ops.moe_gemm_mxfp4_a8(q(4, 128), one(4), st, _row_off(gpu, [2, 1, 1]))
    with pytest.raises(RuntimeError, match="a_rows has dtype"):
        ops.moe_gemm_mxfp4_a8(q(4, 128), one(4), st, ro, a_rows=torch.zeros(4, dtype=torch.int64, device=gpu), rows=4)
    with pytest.raises(RuntimeError, match="a_rows has 3 elements, expected 4"):
        ops.moe_gemm_mxfp4_a8(q(4, 128), one(4), st, ro, a_rows=torch.zeros(3, dtype=torch.int32, device=gpu), rows=4)
    with pytest.raises(RuntimeError, match="without a_rows"):
        ops.moe_gemm_mxfp4_a8(q(3, 128), one(3), st, ro, rows=4)
    assert not ops.moe_mxfp4_a8_ok(4, 136, 4, st)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.moe_gemm_mxfp4_a8(q(4, 136)[:, :128], one(4), st, ro)


# ------------------------------------------------------------------ model
ARCHS = ["qwen3-moe-tiny", "mixtral-tiny"]


def _model(gpu, arch, seed=2, **kw):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    cfg = decoder_config(arch)
    cls = Qwen3MoeModel if cfg.qk_norm else MixtralModel
    return cls(cfg, device=gpu, seed=seed, max_position=1024, expert_weights="mxfp4", expert_act="e4m3", **kw)


def _twin(m):
    t = copy.copy(m)
    t.layers = [_twin_layer(L) for L in m.layers]
    return t


@pytest.fixture(scope="module", params=ARCHS)
def model(request, gpu):
    return _model(gpu, request.param)


def _count(monkeypatch):
    """Counts the calls of the W4A8 op, the weight stream and the dequantisation."""
    from llm_weighted_consensus_amd import ops

    calls = {"a8": 0, "stream": 0, "dequant": 0}

    def wrap(name, key):
        real = getattr(ops, name)

        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)

        monkeypatch.setattr(ops, name, f)

    wrap("moe_gemm_mxfp4_a8", "a8")
    wrap("moe_skinny_mxfp4", "stream")
    wrap("moe_dequant_mxfp4", "dequant")
    return calls


@pytest.mark.parametrize("T", ["5", "limit", "past"])
def test_one_moe_layer(model, gpu, T, monkeypatch):
    """``model._mlp`` on N(0, 1) rows.  At 5 tokens and at the last token count of the weight stream: that path,
    bf16 activations, against the fp32 MLP of the dequantised experts.  One token further: the W4A8 kernel, against
    the same MLP with its input rows and its SwiGLU output row-quantised, for the experts and weights ``ops.route``
    chose; the bound of test_moe_mxfp4_gpu.test_one_moe_layer.  Nothing is dequantised on either route."""
    from llm_weighted_consensus_amd import ops

    m, L = model, model.layers[1]
    k, E = m.full_cfg.experts_per_token, m.full_cfg.num_experts
    lim = ops.MOE_MXFP4_STREAM_AVG_ROWS * E // k
    T = {"5": 5, "limit": lim, "past": lim + 1}[T]
    a8 = T * k > ops.MOE_MXFP4_STREAM_AVG_ROWS * E
    assert a8 == (T > lim)
    h = torch.randn(T, m.cfg.hidden, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16).to(gpu)
    ids, w, _, _, _ = ops.route(h, L.router, k)
    calls = _count(monkeypatch)
    got = m._mlp(h, L).float()
    assert calls == ({"a8": 2, "stream": 0, "dequant": 0} if a8 else {"a8": 0, "stream": 2, "dequant": 0})
    if a8:
        want = moe_mxfp4_a8_ref.moe_mlp_given_a8(_twin_layer(L), h, ids, w)
    else:
        want = qwen_moe_ref.moe_mlp_given(_twin_layer(L), h, ids, w)
    err = (got - want).abs()
    print(f"\n[moe-mxfp4-a8] {m.cfg.name} layer T={T} ({'W4A8' if a8 else 'stream'}): max err "
          f"{float(err.max()):.3g}, max |ref| {float(want.abs().max()):.3g}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= 2e-2 * want.abs().max() + 2e-2 * want.abs()).all())


def _model_cosines(m, gpu):
    """Prefill of 37 tokens and 7 decode steps: the cosines of every compared logits row with the emulated oracle's
    and with the unquantised twin's."""
    from llm_weighted_consensus_amd.models.llama import KVCache

    P, N = 37, 44
    toks = torch.randint(0, m.cfg.vocab_size, (N,), generator=torch.Generator().manual_seed(1)).to(gpu)
    twin = _twin(m)
    emu = moe_mxfp4_a8_ref.a8_forward(twin, toks)
    plain = (qwen_moe_ref.qwen_moe_forward if m.cfg.qk_norm else ref.llama_forward)(twin, toks)
    cache = KVCache(m.cfg, 16, 16, gpu)
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    lg = m.prefill(toks[:P].int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    rows = [(lg[:1], P - 1)]
    bt = torch.arange(4, dtype=torch.int32, device=gpu).view(1, 4)
    for t in range(P, N):
        dl = m.decode(toks[t:t + 1].int(), _i32(gpu, t), _i32(gpu, t), bt, _i32(gpu, t + 1), cache, num_splits=2)
        rows.append((dl[:1], t))
    return ([float(row_cosines(r, emu[t:t + 1])[0]) for r, t in rows],
            [float(row_cosines(r, plain[t:t + 1])[0]) for r, t in rows])


def test_whole_model_matches_its_oracles_and_the_engine(model, gpu, monkeypatch):
    """With the weight stream's row limit at 0 every step — the 37-token prefill, its last layer on the one kept row,
    the 7 decode steps — takes the W4A8 kernel.  Logit cosines against the emulated fp32 oracle and the unquantised
    twin; no scratch exists and nothing is dequantised; then greedy generation of 130 children through the engine
    (captured graphs): all children agree and every block is freed."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    m = model
    assert m.expert_act == "e4m3" and m.expert_weights == "mxfp4" and m.moe_scratch is None and m.graph_safe
    monkeypatch.setattr(ops, "MOE_MXFP4_STREAM_AVG_ROWS", 0)
    calls = _count(monkeypatch)
    emu, plain = _model_cosines(m, gpu)
    assert calls == {"a8": 2 * m.cfg.layers * 8, "stream": 0, "dequant": 0}
    print(f"\n[moe-mxfp4-a8] {m.cfg.name} seed 2: largest 1 - cos {1 - min(emu):.3e} against the emulated oracle "
          f"(prefill {emu[0]:.6f}), {1 - min(plain):.3e} against the unquantised twin")
    assert min(emu) > COS_BOUND[m.cfg.name], emu
    assert min(plain) > COS_PLAIN, plain
    tok = ByteTokenizer(m.cfg.vocab_size)
    eng = LLMEngine(m, tok, num_blocks=1024, max_batch=160, max_model_len=512, cascade_min_batch=1)
    outs = eng.generate([tok.encode("a wide mixture of experts " * 3)],
                        SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True), n=130)
    assert len(outs[0]) == 130 and all(o == outs[0][0] for o in outs[0])
    assert eng.bm.num_free == 1024
    assert calls["stream"] == 0 and calls["dequant"] == 0 and m.moe_scratch is None


def test_what_the_model_keeps_resident(model, gpu):
    """The packed stacks and no bf16 buffer of a stack's size: no scratch.  The same model without the keyword keeps
    today's scratch."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config

    m = model
    c = m.full_cfg
    E, F_, d = c.num_experts, c.ffn, c.hidden
    for L in m.layers:
        assert isinstance(L.w13, ops.Mxfp4Experts) and isinstance(L.w2, ops.Mxfp4Experts) and L.gu_block == 32
        assert m._a8_stacks_ok(L)
    assert m.moe_scratch is None
    held = [n for n, v in vars(m).items() if isinstance(v, torch.Tensor) and v.numel() >= E * 2 * F_ * d
            and n not in ("embed", "lm_head")]
    assert held == [], held
    old = type(m)(decoder_config(c.name), device=gpu, seed=2, max_position=1024, expert_weights="mxfp4")
    assert old.expert_act == "bf16" and old.moe_scratch.numel() == E * 2 * F_ * d


@pytest.mark.parametrize("arch", ARCHS)
def test_served_through_the_worker_factory(gpu, arch):
    """``build_engine`` with the spec key builds the model and completes one greedy chat request."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.chat.local import render_chat_prompt, template_for
    from llm_weighted_consensus_amd.engine.group import build_engine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.schema import chat as C

    msgs = [C.SystemMessage(content="You are one voter among several. Answer briefly."),
            C.UserMessage(content="Which of the candidate answers is the most complete one, and why?")]
    eng = build_engine({"arch": arch, "weights": "random:3", "max_model_len": 512, "max_batch": 16,
                        "kv_fraction": 0.02, "device": gpu.index or 0, "expert_weights": "mxfp4",
                        "expert_act": "e4m3"}, 0)
    assert eng.model.expert_act == "e4m3" and eng.model.moe_scratch is None
    assert isinstance(eng.model.layers[0].w13, ops.Mxfp4Experts)
    prompt = eng.tokenizer.encode(render_chat_prompt(msgs, None, template_for(eng.model.cfg.name)))
    free = eng.bm.num_free
    out = eng.generate([prompt], SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True), n=1)
    assert len(out[0][0]) == 8 and eng.bm.num_free == free
    del eng
    torch.cuda.empty_cache()
