"""MoE decoders with MXFP4 experts on the GPU (csrc/kernels/moe_mxfp4.hip, ``expert_weights="mxfp4"``).

Kernel: the grouped weight stream bit for bit against the dense kernel on every chunk, with sentinel surroundings;
segment bounds and gather straight from ``ops.route`` at 128 experts; row independence; fp32; both paths of the two
wrappers; device-side bounds under a captured graph; the host refusals.  Model, at ``qwen3-moe-tiny`` and
``mixtral-tiny``: one layer and the whole model against the fp32 oracles on a twin holding the dequantised experts,
what the model keeps resident, and the engine."""
import copy
import dataclasses

import pytest
import torch

from tests import qwen_moe_ref
from tests import torch_ref as ref
from tests.qwen_ref import row_cosines
from tests.test_mxfp4_gpu import _bits, _close, _i32, _weight

pytestmark = pytest.mark.gpu

# Whole-model bounds: 1 - 4 * (largest measured 1 - cos over seeds 2, 3, 4 and every compared logits row: the
# prefill's last token and 7 decode steps, against the fp32 oracle run on the dequantised twin), never below 0.99.
# Measured on an MI355X, largest 1 - cos for seeds 2, 3, 4:
#   qwen3-moe-tiny  2.763e-4, 2.074e-4, 3.976e-5   ->  1 - 4 * 2.763e-4 = 0.99889
#   mixtral-tiny    1.413e-5, 1.514e-5, 1.425e-5   ->  1 - 4 * 1.514e-5 = 0.99994
MEASURED = {"qwen3-moe-tiny": 2.763e-4, "mixtral-tiny": 1.514e-5}
COS_BOUND = {a: max(0.99, 1 - 4 * v) for a, v in MEASURED.items()}

_S = {}  # (E, N, K, swiglu) -> Mxfp4Experts: built once, never changed


def _stack(gpu, E, N, K, swiglu=False):
    """E experts cut from one ``_weight(E * N, K, "plain")`` (randn / sqrt(K), one all-zero row and one all-zero
    block in expert 0); ``swiglu``: each expert quantised after its 32-row gate|up interleave."""
    from llm_weighted_consensus_amd import ops

    key = (E, N, K, swiglu)
    if key not in _S:
        w = _weight(gpu, E * N, K, "plain")[1].view(E, N, K)
        if swiglu:
            w = torch.stack([ops.swiglu_interleave(w[e]) for e in range(E)])
        _S[key] = ops.Mxfp4Experts(w)
    return _S[key]


def _row_off(gpu, lens):
    return torch.tensor([0] + list(lens), device=gpu).cumsum(0).to(torch.int32)


def _in_nan(gpu, rows, K, seed):
    """N(0, 1) bf16 rows as a view into a NaN-filled buffer (row stride K + 32): a live lane that read outside its
    rows shows as NaN in the output."""
    buf = torch.full((rows + 4, K + 32), float("nan"), dtype=torch.bfloat16, device=gpu)
    A = buf[2:2 + rows, :K]
    A.copy_(torch.randn(rows, K, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16))
    return A


def _fp32(st, e, x, swiglu):
    """fp32 result of expert e on rows x from the stack's exact dequantisation."""
    w = st.expert(e).dequant().float()
    y = x.float() @ w.t()
    if not swiglu:
        return y
    M, F_ = y.shape[0], y.shape[1] // 2  # (explicit sizes: an empty segment has no rows to infer one from)
    y = y.view(M, F_ // 32, 2, 32)
    return torch.nn.functional.silu(y[:, :, 0].reshape(M, F_)) * y[:, :, 1].reshape(M, F_)


def _check_chunks(st, A, a_rows, row_off, out, swiglu):
    """Every chunk of at most 64 rows of every segment equals the dense kernel on those rows, by bit pattern."""
    from llm_weighted_consensus_amd import ops

    ro = row_off.tolist()
    for e in range(st.shape[0]):
        for c0 in range(ro[e], ro[e + 1], 64):
            idx = torch.arange(c0, min(c0 + 64, ro[e + 1]), device=A.device)
            x = A[a_rows[idx].long() if a_rows is not None else idx].contiguous()
            want = ops.skinny_mxfp4(x, st.expert(e), swiglu=swiglu)
            bad = (_bits(out[idx]) != _bits(want)).nonzero()
            assert bad.numel() == 0, f"expert {e}, chunk at row {c0}: first mismatch {bad[0].tolist()}"


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("gather", [True, False], ids=["gather", "rows"])
@pytest.mark.parametrize("lens", [[0, 1, 17, 64, 0], [65, 0, 130, 16, 1]], ids=["short", "long"])
@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("N,K", [(64, 384), (128, 1152)])
def test_bitwise_the_dense_kernel_and_nothing_else_written(gpu, N, K, swiglu, lens, gather):
    """Empty, one-row, ragged, exactly-64 and longer-than-64 segments (65: a full chunk and one row; 130: two and two
    rows).  K = 384: 3 batches for 8 waves, K = 1152: 9.  The gather repeats source rows, as a token in k experts
    does.  ``out`` is a view into a sentinel-filled buffer, ``A`` a view into a NaN-filled one."""
    from llm_weighted_consensus_amd import ops

    st = _stack(gpu, 5, N, K, swiglu)
    rows = sum(lens)
    row_off = _row_off(gpu, lens)
    T = 23 if gather else rows
    A = _in_nan(gpu, T, K, N + K + rows)
    a_rows = ((torch.arange(rows, device=gpu) * 7 + 3) % T).to(torch.int32) if gather else None
    NC = N // 2 if swiglu else N
    buf = torch.full((rows + 3, NC + 16), 123.0, dtype=torch.bfloat16, device=gpu)
    out = ops.moe_skinny_mxfp4(A, st, row_off, a_rows=a_rows, rows=rows, out=buf[:rows, :NC], swiglu=swiglu)
    assert out.data_ptr() == buf.data_ptr() and out.shape == (rows, NC)
    assert bool(torch.isfinite(out.float()).all()), "a live lane read outside its rows"
    _check_chunks(st, A, a_rows, row_off, out, swiglu)
    assert bool((buf[rows:] == 123.0).all()) and bool((buf[:, NC:] == 123.0).all())


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
def test_wide_and_sparse_bounds_from_the_router(gpu, swiglu):
    """E = 128, 40 rows (T = 5, k = 8) with ``row_off`` and the gather as ``ops.route`` returns them: at least 88
    experts idle.  Then all 40 rows in one expert, the first and the last expert empty."""
    from llm_weighted_consensus_amd import ops

    E, N, K, T, k = 128, 64, 384, 5, 8
    st = _stack(gpu, E, N, K, swiglu)
    h = _in_nan(gpu, T, K, 11)
    router = torch.randn(E, K, generator=torch.Generator().manual_seed(12)).to(torch.bfloat16).to(gpu)
    _, _, row_off, src, _ = ops.route(h, router, k)
    assert row_off.dtype == torch.int32 and row_off.shape == (E + 1,) and int(row_off[-1]) == T * k
    one = torch.zeros(E + 1, dtype=torch.int32, device=gpu)
    one[78:] = T * k
    NC = N // 2 if swiglu else N
    for ro in (row_off, one):
        buf = torch.full((T * k + 3, NC + 16), 123.0, dtype=torch.bfloat16, device=gpu)
        out = ops.moe_skinny_mxfp4(h, st, ro, a_rows=src, rows=T * k, out=buf[:T * k, :NC], swiglu=swiglu)
        assert bool(torch.isfinite(out.float()).all())
        _check_chunks(st, h, src, ro, out, swiglu)
        assert bool((buf[T * k:] == 123.0).all()) and bool((buf[:, NC:] == 123.0).all())


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
def test_a_row_does_not_depend_on_its_neighbours(gpu, swiglu):
    """One row through expert 2: routed alone, as the last row of a 64-row chunk, and as row 65 of a 70-row segment
    (the first row of its second chunk, with other experts' rows around): the same bits each time."""
    from llm_weighted_consensus_amd import ops

    N, K = 128, 1152
    st = _stack(gpu, 5, N, K, swiglu)
    A = _in_nan(gpu, 90, K, 5)  # row 0 is the probe
    got = []
    for lens, pos in (([0, 0, 1, 0, 0], 0), ([3, 0, 64, 2, 0], 3 + 63), ([7, 1, 70, 0, 5], 8 + 64)):
        rows = sum(lens)
        a_rows = torch.arange(1, rows + 1, dtype=torch.int32, device=gpu)
        a_rows[pos] = 0
        out = ops.moe_skinny_mxfp4(A, st, _row_off(gpu, lens), a_rows=a_rows, rows=rows, swiglu=swiglu)
        got.append(_bits(out[pos]).clone())
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    assert torch.equal(got[0], _bits(ops.skinny_mxfp4(A[:1].contiguous(), st.expert(2), swiglu=swiglu)[0]))


def _fp32_all(st, A, a_rows, row_off, swiglu):
    ro = row_off.tolist()
    x = A[a_rows.long()] if a_rows is not None else A
    return torch.cat([_fp32(st, e, x[ro[e]:ro[e + 1]], swiglu) for e in range(st.shape[0])])


@pytest.mark.parametrize("swiglu", [False, True], ids=["plain", "swiglu"])
def test_matches_fp32_on_the_dequantised_weights(gpu, swiglu):
    """N(0, 1) rows, the bound of test_skinny_mxfp4_matches_fp32."""
    from llm_weighted_consensus_amd import ops

    st = _stack(gpu, 5, 128, 1152, swiglu)
    lens = [65, 0, 130, 16, 1]
    rows, row_off = sum(lens), _row_off(gpu, lens)
    A = _in_nan(gpu, 40, 1152, 3)
    a_rows = ((torch.arange(rows, device=gpu) * 11 + 1) % 40).to(torch.int32)
    out = ops.moe_skinny_mxfp4(A, st, row_off, a_rows=a_rows, rows=rows, swiglu=swiglu)
    _close(out, _fp32_all(st, A, a_rows, row_off, swiglu), 3e-2, 1e-2)


@pytest.mark.parametrize("path", ["stream", "dequant"])
def test_both_paths_of_both_wrappers(gpu, path):
    """700 rows over 5 experts through ``moe_swiglu_mxfp4`` (gathered) and ``moe_linear_mxfp4`` (expert-major), each
    path called directly: the same fp32 bound; after the dequantise path the scratch holds the exact stack."""
    from llm_weighted_consensus_amd import ops

    w13, w2 = _stack(gpu, 5, 128, 1152, True), _stack(gpu, 5, 64, 384)
    lens = [300, 0, 250, 149, 1]
    rows, row_off = sum(lens), _row_off(gpu, lens)
    scratch = torch.full((5 * 128 * 1152 + 64,), -7.0, dtype=torch.bfloat16, device=gpu)
    x = _in_nan(gpu, 350, 1152, 21)
    a_rows = ((torch.arange(rows, device=gpu) * 3 + 2) % 350).to(torch.int32)
    act = ops.moe_swiglu_mxfp4(x, w13, row_off, a_rows, rows, scratch, path=path)
    assert act.shape == (rows, 64)
    _close(act, _fp32_all(w13, x, a_rows, row_off, True), 3e-2, 1e-2)
    if path == "dequant":
        assert torch.equal(_bits(scratch[:5 * 128 * 1152]), _bits(w13.dequant().flatten()))
        assert bool((scratch[5 * 128 * 1152:] == -7.0).all())
    a2 = _in_nan(gpu, rows, 384, 22)
    y = ops.moe_linear_mxfp4(a2, w2, row_off, scratch, path=path)
    assert y.shape == (rows, 64)
    _close(y, _fp32_all(w2, a2, None, row_off, False), 3e-2, 1e-2)
    if path == "dequant":
        assert torch.equal(_bits(scratch[:5 * 64 * 384]), _bits(w2.dequant().flatten()))
    else:
        assert bool((scratch == -7.0).all())  # the stream path leaves the scratch alone


def test_bounds_are_read_on_the_device_under_a_graph(gpu):
    """The stream op captured once (a single chain); ``row_off`` and ``a_rows`` rewritten in place; the replay
    equals an eager call on the new values, bit for bit."""
    from llm_weighted_consensus_amd import ops

    st = _stack(gpu, 5, 128, 1152, True)
    rows = 40
    A = _in_nan(gpu, 16, 1152, 31)
    row_off = _row_off(gpu, [8, 8, 8, 8, 8])
    a_rows = (torch.arange(rows, device=gpu) % 16).to(torch.int32)
    out = torch.zeros(rows, 64, dtype=torch.bfloat16, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        ops.moe_skinny_mxfp4(A, st, row_off, a_rows=a_rows, rows=rows, out=out, swiglu=True)
    torch.cuda.current_stream(gpu).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.moe_skinny_mxfp4(A, st, row_off, a_rows=a_rows, rows=rows, out=out, swiglu=True)
    first = out.clone()
    row_off.copy_(_row_off(gpu, [0, 33, 0, 1, 6]))
    a_rows.copy_(((torch.arange(rows, device=gpu) * 5 + 2) % 16).to(torch.int32))
    out.zero_()
    g.replay()
    torch.cuda.synchronize(gpu)
    eager = ops.moe_skinny_mxfp4(A, st, row_off, a_rows=a_rows, rows=rows, swiglu=True)
    assert torch.equal(_bits(out), _bits(eager)) and not torch.equal(_bits(out), _bits(first))


def test_refusals_on_the_host(gpu):
    from llm_weighted_consensus_amd import ops

    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=gpu)  # noqa: E731
    ro = _row_off(gpu, [2, 2])
    with pytest.raises(RuntimeError, match="K % 128 == 0.*got K = 160"):
        ops.moe_skinny_mxfp4(z(4, 160), ops.Mxfp4Experts(z(2, 16, 160)), ro)
    with pytest.raises(RuntimeError, match="SwiGLU: N % 64 == 0.*got K = 128, N = 32"):
        ops.moe_skinny_mxfp4(z(4, 128), ops.Mxfp4Experts(z(2, 32, 128)), ro, swiglu=True)
    st = ops.Mxfp4Experts(z(2, 16, 128))
    with pytest.raises(RuntimeError, match="row_off has dtype"):
        ops.moe_skinny_mxfp4(z(4, 128), st, ro.long())
    with pytest.raises(RuntimeError, match="row_off has 4 elements, expected 3"):
        ops.moe_skinny_mxfp4(z(4, 128), st, _row_off(gpu, [2, 1, 1]))
    with pytest.raises(RuntimeError, match="a_rows has dtype"):
        ops.moe_skinny_mxfp4(z(4, 128), st, ro, a_rows=torch.zeros(4, dtype=torch.int64, device=gpu), rows=4)
    with pytest.raises(RuntimeError, match="without a_rows"):
        ops.moe_skinny_mxfp4(z(3, 128), st, ro, rows=4)
    # what the 32-bit offsets cannot index is the wrapper's to route around: the shape test says no
    assert ops.moe_skinny_mxfp4_ok(4, 128, 4, st) and not ops.moe_skinny_mxfp4_ok(1 << 23, 128, 4, st)
    with pytest.raises(ValueError, match="scratch"):
        ops.moe_linear_mxfp4(z(4, 128), st, ro, z(16), path="dequant")


# ------------------------------------------------------------------ model
ARCHS = ["qwen3-moe-tiny", "mixtral-tiny"]


def _model(gpu, arch, seed=2, **kw):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    cfg = decoder_config(arch)
    cls = Qwen3MoeModel if cfg.qk_norm else MixtralModel
    return cls(cfg, device=gpu, seed=seed, max_position=1024, expert_weights="mxfp4", **kw)


def _twin_layer(L):
    """The layer with its experts dequantised (the interleaved row order and ``gu_block`` kept): what the fp32
    oracles read."""
    return dataclasses.replace(L, w13=L.w13.dequant(), w2=L.w2.dequant())


def _twin(m):
    t = copy.copy(m)
    t.layers = [_twin_layer(L) for L in m.layers]
    return t


@pytest.fixture(scope="module", params=ARCHS)
def model(request, gpu):
    return _model(gpu, request.param)


@pytest.mark.parametrize("T", ["5", "64", "past"])
def test_one_moe_layer(model, gpu, T):
    """``model._mlp`` on N(0, 1) rows at 5 and 64 tokens and at a token count past the stream path's row limit,
    against the fp32 MLP of the dequantised experts for the experts and weights ``ops.route`` chose (no near-tie
    allowance needed); the bf16 bound of test_qwen_moe_gpu.test_one_moe_layer."""
    from llm_weighted_consensus_amd import ops

    m, L = model, model.layers[1]
    k, E = m.full_cfg.experts_per_token, m.full_cfg.num_experts
    if T == "past":
        T = ops.MOE_MXFP4_STREAM_AVG_ROWS * E // k + 9
        assert T * k > ops.MOE_MXFP4_STREAM_AVG_ROWS * E
    T = int(T)
    h = torch.randn(T, m.cfg.hidden, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16).to(gpu)
    ids, w, _, _, _ = ops.route(h, L.router, k)
    got = m._mlp(h, L).float()
    want = qwen_moe_ref.moe_mlp_given(_twin_layer(L), h, ids, w)
    err = (got - want).abs()
    print(f"\n[moe-mxfp4] {m.cfg.name} layer T={T}: max err {float(err.max()):.3g}, max |ref| "
          f"{float(want.abs().max()):.3g}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= 2e-2 * want.abs().max() + 2e-2 * want.abs()).all())


def _i(gpu, *v):
    return _i32(gpu, *v)


def _model_cosines(m, gpu):
    """Prefill of 37 tokens and 7 decode steps: the cosine of every compared logits row with the oracle's (the fp32
    forward of the dequantised twin)."""
    from llm_weighted_consensus_amd.models.llama import KVCache

    P, N = 37, 44
    toks = torch.randint(0, m.cfg.vocab_size, (N,), generator=torch.Generator().manual_seed(1)).to(gpu)
    oracle = qwen_moe_ref.qwen_moe_forward if m.cfg.qk_norm else ref.llama_forward
    want = oracle(_twin(m), toks)
    cache = KVCache(m.cfg, 16, 16, gpu)
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    lg = m.prefill(toks[:P].int(), ar, ar, _i(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    cos = [float(row_cosines(lg[:1], want[P - 1:P])[0])]
    bt = torch.arange(4, dtype=torch.int32, device=gpu).view(1, 4)
    for t in range(P, N):
        dl = m.decode(toks[t:t + 1].int(), _i(gpu, t), _i(gpu, t), bt, _i(gpu, t + 1), cache, num_splits=2)
        cos.append(float(row_cosines(dl[:1], want[t:t + 1])[0]))
    return cos


def test_whole_model_matches_reference_and_engine(model, gpu):
    """Prefill and 7 decode steps against the fp32 oracle, then greedy generation of 130 children through the
    engine (cascade tiles, captured graphs): all children agree and every block is freed."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    m = model
    cos = _model_cosines(m, gpu)
    print(f"\n[moe-mxfp4] {m.cfg.name} seed 2: prefill cos {cos[0]:.6f}, decode min {min(cos[1:]):.6f}, "
          f"largest 1 - cos {1 - min(cos):.3g}")
    assert min(cos) > COS_BOUND[m.cfg.name], cos
    assert m.graph_safe
    tok = ByteTokenizer(m.cfg.vocab_size)
    eng = LLMEngine(m, tok, num_blocks=1024, max_batch=160, max_model_len=512, cascade_min_batch=1)
    outs = eng.generate([tok.encode("a wide mixture of experts " * 3)],
                        SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True), n=130)
    assert len(outs[0]) == 130 and all(o == outs[0][0] for o in outs[0])
    assert eng.bm.num_free == 1024


def test_what_the_model_keeps_resident(model):
    """Each expert stack takes E * N * K * 17 / 32 bytes; no bf16 expert tensor remains, and the dequantisation
    scratch is the one bf16 buffer of E * 2F * d elements."""
    from llm_weighted_consensus_amd import ops

    m = model
    c = m.full_cfg
    E, F_, d = c.num_experts, c.ffn, c.hidden
    for L in m.layers:
        assert isinstance(L.w13, ops.Mxfp4Experts) and isinstance(L.w2, ops.Mxfp4Experts)
        assert L.w13.shape == (E, 2 * F_, d) and L.w2.shape == (E, d, F_) and L.gu_block == 32
        assert L.w13.nbytes == E * 2 * F_ * d * 17 // 32 and L.w2.nbytes == E * d * F_ * 17 // 32
        assert L.s13 is None and L.s2 is None
        big = [f.name for f in dataclasses.fields(L) if isinstance(getattr(L, f.name), torch.Tensor)
               and getattr(L, f.name).numel() >= E * d * F_]
        assert big == [], big
        assert L.wqkv.dtype == torch.bfloat16 and L.wo.dtype == torch.bfloat16 and L.router.dtype == torch.bfloat16
    assert m.moe_scratch.dtype == torch.bfloat16 and m.moe_scratch.numel() == E * 2 * F_ * d
    # (mixtral-tiny's embedding table and lm_head happen to have as many elements)
    held = [n for n, v in vars(m).items() if isinstance(v, torch.Tensor) and v.numel() == E * 2 * F_ * d
            and n not in ("embed", "lm_head")]
    assert held == ["moe_scratch"], held


@pytest.mark.parametrize("arch", ARCHS)
def test_served_through_the_worker_factory(gpu, arch):
    """``build_engine`` with the spec key builds the model with MXFP4 experts and completes one greedy chat request."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.chat.local import render_chat_prompt, template_for
    from llm_weighted_consensus_amd.engine.group import build_engine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.schema import chat as C

    msgs = [C.SystemMessage(content="You are one voter among several. Answer briefly."),
            C.UserMessage(content="Which of the candidate answers is the most complete one, and why?")]
    eng = build_engine({"arch": arch, "weights": "random:3", "max_model_len": 512, "max_batch": 16,
                        "kv_fraction": 0.02, "device": gpu.index or 0, "expert_weights": "mxfp4"}, 0)
    assert eng.model.expert_weights == "mxfp4" and isinstance(eng.model.layers[0].w13, ops.Mxfp4Experts)
    if arch == "qwen3-moe-tiny":
        assert template_for(arch) == "chatml"
    prompt = eng.tokenizer.encode(render_chat_prompt(msgs, None, template_for(eng.model.cfg.name)))
    free = eng.bm.num_free
    out = eng.generate([prompt], SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True), n=1)
    assert len(out[0][0]) == 8 and eng.bm.num_free == free
    del eng
    torch.cuda.empty_cache()
