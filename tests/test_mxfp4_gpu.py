"""MXFP4 weight-only projections on the GPU (csrc/kernels/mxfp4.hip): the dequantisation kernel bit for bit against
the host function, exact one-hot probes of the weight-stream GEMM (nibble order, scale-to-block mapping, the k
permutation, the wave split), the GEMM and its SwiGLU form against fp32, the scratch path above 64 rows, the
three tiny decoders against the fp32 forward of their dequantised twin, and the engine."""
import copy
from dataclasses import replace

import pytest
import torch

from tests import qwen_ref

pytestmark = pytest.mark.gpu

_W = {}  # (N, K, kind) -> (Mxfp4Weight, dequantised bf16 [N, K] by the host function): built once, never changed


def _close(a, b, atol, rtol=0.0):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    assert torch.isfinite(a).all(), "non-finite output"
    assert (err <= lim).all(), f"max err {err.max().item():.4g} (atol {atol}, rtol {rtol})"


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm())).item()


def _i32(gpu, *v):
    return torch.tensor(list(v), dtype=torch.int32, device=gpu)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _weight(gpu, N, K, kind):
    """``spread``: block b of row n times 2^((n + b) % 13 - 6), so the scales cover 13 exponents; ``plain``:
    randn / sqrt(K) (the operand scaling of test_skinny_gemm_matches_fp32) with one all-zero block and one
    all-zero row; ``swiglu``: plain, quantised after the 32-row gate|up interleave (dq stays [gate; up])."""
    from llm_weighted_consensus_amd import ops

    key = (N, K, kind)
    if key not in _W:
        g = torch.Generator(device="cpu").manual_seed(N * 31 + K + len(kind))
        w = torch.randn(N, K, generator=g).to(gpu) / K ** 0.5
        if kind == "spread":
            n, b = torch.arange(N, device=gpu).view(N, 1, 1), torch.arange(K // 32, device=gpu).view(1, K // 32, 1)
            w = (w.view(N, K // 32, 32) * torch.exp2(((n + b) % 13 - 6).float())).view(N, K)
        else:
            w[3] = 0
            w[5, K - 64:K - 32] = 0
        w = w.to(torch.bfloat16)
        q, s = ops.quant_mxfp4_weight(w)
        dq = ops.dequant_mxfp4(q, s)
        mw = ops.Mxfp4Weight(ops.swiglu_interleave(w)) if kind == "swiglu" else ops.Mxfp4Weight.from_packed(q, s)
        if kind == "spread":
            assert len(torch.unique(s)) >= 12
        _W[key] = (mw, dq)
    return _W[key]


# ------------------------------------------------------------------ dequant
@pytest.mark.parametrize("N,K", [(16, 128), (1040, 3584), (4096, 4096)])
def test_dequant_kernel_is_bitwise_the_host_function(gpu, N, K):
    """Pins the convert instruction's nibble order, byte select and scale semantics on the device."""
    from llm_weighted_consensus_amd import ops

    mw, dq = _weight(gpu, N, K, "spread")
    buf = torch.full((N * K + 64,), -7.0, dtype=torch.bfloat16, device=gpu)
    out = ops.mxfp4_dequant(mw, buf[:N * K].view(N, K))
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(_bits(out), _bits(dq))
    assert bool((buf[N * K:] == -7.0).all())  # nothing past the weight is written


# ------------------------------------------------------------------ exact one-hot probes
def _probe_columns(K, launch):
    """64 k per launch.  Launches 0 and 1: every k of the first 128-k batch (every k mod 128, both sides of the
    32-block boundaries 31|32, 63|64, 95|96).  Launch 2: the edges of the last batch and of its blocks, then k
    spread over all the batches (every wave of the K split)."""
    if launch < 2:
        return [64 * launch + m for m in range(64)]
    last = K - 128
    ks = [last + r for r in (0, 31, 32, 63, 64, 95, 96, 127)]
    ks += [(m * 1237 + 5 * m * m + 77) % K for m in range(8, 64)]
    return ks


@pytest.mark.parametrize("K", [128, 1152, 3584])
@pytest.mark.parametrize("N", [16, 1040, 6144])
def test_one_hot_rows_read_single_weights_exactly(gpu, N, K):
    """Row m of A is 1.0 at one k_m: out[m, n] is dq[n, k_m] bit for bit (the product and the sums with zeros are
    exact, the value is a bf16).  K = 128: one batch, seven idle waves; 1152: 9 batches over 8 waves; N = 6144:
    the 32-column workgroups."""
    from llm_weighted_consensus_amd import ops

    mw, dq = _weight(gpu, N, K, "spread")
    for launch in range(3):
        ks = torch.tensor(_probe_columns(K, launch), device=gpu)
        A = torch.zeros(64, K, dtype=torch.bfloat16, device=gpu)
        A[torch.arange(64, device=gpu), ks] = 1.0
        out = ops.skinny_mxfp4(A, mw)
        want = dq[:, ks].t().contiguous()
        bad = (_bits(out) != _bits(want)).nonzero()
        assert bad.numel() == 0, f"launch {launch}: first mismatch (m, n) = {bad[0].tolist()}, k = {int(ks[bad[0][0]])}"


# ------------------------------------------------------------------ against fp32
@pytest.mark.parametrize("M", [1, 7, 16, 17, 33, 64])
@pytest.mark.parametrize("N,K", [(16, 128), (1040, 384), (6144, 4096), (4096, 14336), (512, 18944)])
def test_skinny_mxfp4_matches_fp32(gpu, M, N, K):
    """Every m-tile count with ragged rows; one batch, fewer batches than waves, batch counts that do not divide by
    8 (3, 148), both tile widths (6144 columns: 32 per workgroup).  ``out`` is a view of a larger
    sentinel-filled buffer: rows past M and columns past N stay bitwise untouched."""
    from llm_weighted_consensus_amd import ops

    mw, dq = _weight(gpu, N, K, "plain")
    torch.manual_seed(M * 7 + N + K)
    A = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    buf = torch.full((M + 3, N + 16), 123.0, dtype=torch.bfloat16, device=gpu)
    out = ops.skinny_mxfp4(A, mw, out=buf[:M, :N])
    assert out.data_ptr() == buf.data_ptr()
    _close(out, A.float() @ dq.float().t(), 3e-2, 1e-2)
    assert bool((buf[M:] == 123.0).all()) and bool((buf[:, N:] == 123.0).all())
    assert bool((out[:, 3] == 0).all())  # the all-zero row of W
    if M == 33:  # a view of rows (lda > K) takes the same path
        big = torch.randn(M, K + 64, device=gpu).to(torch.bfloat16)
        _close(ops.skinny_mxfp4(big[:, :K], mw), big[:, :K].float() @ dq.float().t(), 3e-2, 1e-2)


@pytest.mark.parametrize("M", [1, 7, 16, 17, 33, 64])
@pytest.mark.parametrize("N,K", [(64, 512), (1024, 1152), (28672, 4096)])
def test_skinny_mxfp4_swiglu_matches_fp32(gpu, M, N, K):
    from llm_weighted_consensus_amd import ops

    mw, dq = _weight(gpu, N, K, "swiglu")
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    ref = A.float() @ dq.float().t()
    F = N // 2
    buf = torch.full((M + 3, F + 16), 123.0, dtype=torch.bfloat16, device=gpu)
    out = ops.skinny_mxfp4(A, mw, out=buf[:M, :F], swiglu=True)
    assert out.shape == (M, F)
    _close(out, torch.nn.functional.silu(ref[:, :F]) * ref[:, F:], 3e-2, 1e-2)
    assert bool((buf[M:] == 123.0).all()) and bool((buf[:, F:] == 123.0).all())
    assert bool((out[:, 3] == 0).all())  # silu(0) * up: the all-zero gate row


# ------------------------------------------------------------------ above 64 rows, refusals
@pytest.mark.parametrize("M", [65, 300])
def test_wrappers_take_the_scratch_path_above_64_rows(gpu, M):
    from llm_weighted_consensus_amd import ops

    scratch = torch.empty(6144 * 4096, dtype=torch.bfloat16, device=gpu)
    ptr = scratch.data_ptr()
    torch.manual_seed(M)
    for N, K in ((1040, 384), (6144, 4096)):
        mw, dq = _weight(gpu, N, K, "plain")
        A = torch.randn(M, K, device=gpu).to(torch.bfloat16)
        _close(ops.linear_mxfp4(A, mw, scratch), A.float() @ dq.float().t(), 3e-2, 1e-2)
        assert torch.equal(_bits(scratch[:N * K].view(N, K)), _bits(dq))  # the dequantised weight went through it
    mw, dq = _weight(gpu, 1024, 1152, "swiglu")
    A = torch.randn(M, 1152, device=gpu).to(torch.bfloat16)
    ref = A.float() @ dq.float().t()
    _close(ops.swiglu_mxfp4(A, mw, 32, scratch), torch.nn.functional.silu(ref[:, :512]) * ref[:, 512:], 3e-2, 1e-2)
    assert scratch.data_ptr() == ptr
    with pytest.raises(ValueError, match="scratch"):
        ops.linear_mxfp4(A, mw, scratch[:100])


def test_kernel_refuses_what_the_wrappers_route_to_scratch(gpu):
    from llm_weighted_consensus_amd import ops

    scratch = torch.empty(1040 * 384, dtype=torch.bfloat16, device=gpu)
    torch.manual_seed(0)

    def w(N, K):
        x = (torch.randn(N, K, device=gpu) / K ** 0.5).to(torch.bfloat16)
        mw = ops.Mxfp4Weight(x)
        return mw, mw.dequant()

    mw, dq = _weight(gpu, 1040, 384, "plain")
    A = torch.randn(65, 384, device=gpu).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="M <= 64"):
        ops.skinny_mxfp4(A, mw)
    for N, K, msg in ((32, 192, "K % 128 == 0"), (24, 128, "N % 16 == 0")):
        mw, dq = w(N, K)
        A = torch.randn(4, K, device=gpu).to(torch.bfloat16)
        with pytest.raises(RuntimeError, match=msg):
            ops.skinny_mxfp4(A, mw)
        _close(ops.linear_mxfp4(A, mw, scratch), A.float() @ dq.float().t(), 3e-2, 1e-2)
    mw, dq = w(96, 128)  # SwiGLU needs N % 64 == 0
    A = torch.randn(4, 128, device=gpu).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="N % 64 == 0"):
        ops.skinny_mxfp4(A, mw, swiglu=True)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.skinny_mxfp4(torch.zeros(4, 256, dtype=torch.bfloat16, device=gpu), mw)


# ------------------------------------------------------------------ model
_models = {}


def _model(gpu, arch):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    if arch not in _models:
        _models[arch] = LlamaModel(decoder_config(arch), device=gpu, seed=0, max_position=1024, mxfp4=True)
    return _models[arch]


def _twin(m):
    """The bf16 model computing the same function: every projection the host-dequantised tensor."""
    from llm_weighted_consensus_amd import ops

    t = copy.copy(m)
    t.layers = [replace(L, **{n: ops.dequant_mxfp4(getattr(L, n).q, getattr(L, n).s)
                              for n in ("wqkv", "wo", "w_gate_up", "w_down")}) for L in m.layers]
    return t


@pytest.mark.parametrize("arch", ["llama-tiny", "qwen2-tiny", "qwen3-tiny"])
def test_model_matches_the_fp32_forward_of_its_dequantised_twin(gpu, arch):
    """A 97-token prefill (scratch path), 7 decode steps at B = 1 (weight-stream kernel), one decode step of 80
    forked rows (scratch path): every logits row at the model tests' cosine > 0.995."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = _model(gpu, arch)
    cfg = m.cfg
    assert m.mxfp4 and not m._planned_gemms and not m._dense_residual and not m.norm_folded
    shapes = {"wqkv": (cfg.qkv_dim, cfg.hidden), "wo": (cfg.hidden, cfg.heads * cfg.head_dim),
              "w_gate_up": (2 * cfg.ffn, cfg.hidden), "w_down": (cfg.hidden, cfg.ffn)}
    for L in m.layers:
        assert L.gu_block == 32
        for n, (N, K) in shapes.items():
            w = getattr(L, n)
            assert isinstance(w, ops.Mxfp4Weight) and w.shape == (N, K)
            assert w.q.nbytes + w.s.nbytes == N * K // 2 + N * K // 32
    assert m.mx_scratch.nbytes == 2 * max(N * K for N, K in shapes.values())
    assert m.embed.dtype == torch.bfloat16 and m.lm_head.dtype == torch.bfloat16
    twin = _twin(m)

    P, T = 97, 104
    cache = KVCache(cfg, 16, 16, gpu)
    toks = torch.randint(0, cfg.vocab_size, (T,), generator=torch.Generator().manual_seed(0)).to(gpu)
    want = qwen_ref.qwen_forward(twin, toks)
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    scratch_ptr = m.mx_scratch.data_ptr()
    lg = m.prefill(toks[:P].int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    worst = _cos(lg[0], want[P - 1])
    assert worst > 0.995
    bt = torch.arange(8, dtype=torch.int32, device=gpu).view(1, 8)
    for t in range(P, T):
        dl = m.decode(toks[t:t + 1].int(), _i32(gpu, t), _i32(gpu, t), bt, _i32(gpu, t + 1), cache, num_splits=2)
        c = _cos(dl[0], want[t])
        worst = min(worst, c)
        assert c > 0.995, t

    # 80 rows forked from a 33-token prompt: two shared KV blocks, each row its own copy of the third
    P, B = 33, 80
    cache = KVCache(cfg, 4 + B, 16, gpu)
    g = torch.Generator().manual_seed(5)
    prompt = torch.randint(0, cfg.vocab_size, (P,), generator=g).to(gpu)
    nxt = torch.randint(0, cfg.vocab_size, (B,), generator=g).to(gpu)
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    m.prefill(prompt.int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    own = 3 + torch.arange(B, device=gpu)
    for li in range(cfg.layers):
        cache.k[li][own] = cache.k[li][2].clone()
        cache.v[li][own] = cache.v[li][2].clone()
    bt = torch.zeros(B, 4, dtype=torch.int32, device=gpu)
    bt[:, 1], bt[:, 2] = 1, own.int()
    full = lambda v: torch.full((B,), v, dtype=torch.int32, device=gpu)  # noqa: E731
    lg = m.decode(nxt.int(), full(P), (own * 16 + P % 16).int(), bt, full(P + 1), cache)
    for b in range(B):
        c = _cos(lg[b], qwen_ref.qwen_forward(twin, torch.cat([prompt, nxt[b:b + 1]]))[-1])
        worst = min(worst, c)
        assert c > 0.995, b
    assert m.mx_scratch.data_ptr() == scratch_ptr
    print(f"{arch} mxfp4: worst logit cosine {worst:.5f}")


# ------------------------------------------------------------------ engine
def test_engine_generates_and_graphs_match_eager(gpu, monkeypatch):
    """build_engine with "mxfp4": true generates; greedy decode through captured graphs == eager decode token for
    token at n = 4 (weight-stream kernel) and n = 72 (the scratch path inside a captured graph); every KV block
    is back in the pool afterwards."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.group import build_engine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams

    monkeypatch.setenv("LWC_STEP_AB", "0")
    eng = build_engine({"arch": "llama-tiny", "weights": "random:0", "mxfp4": True, "max_model_len": 256,
                        "max_batch": 128, "kv_fraction": 0.02, "device": gpu.index or 0}, 0)
    model, tok = eng.model, eng.tokenizer
    assert model.mxfp4 and isinstance(model.layers[0].wqkv, ops.Mxfp4Weight)
    free = eng.bm.num_free
    prompt = tok.encode("a prompt of more than one KV block, for a 4-bit voter")
    out = eng.generate([prompt], SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True), n=2)
    assert [len(c) for c in out[0]] == [8, 8] and out[0][0] == out[0][1] and eng.bm.num_free == free
    first = int(qwen_ref.qwen_forward(_twin(model), torch.tensor(prompt, device=gpu))[-1].argmax())
    assert out[0][0][0] == first

    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    for n in (4, 72):
        outs = []
        for graphs in (False, True):
            e = LLMEngine(model, tok, num_blocks=512, max_batch=128, max_model_len=256, use_graphs=graphs)
            outs.append(e.generate([prompt], sp, n=n))
            assert e.bm.num_free == 512
        assert outs[0] == outs[1], n
        assert len(outs[0][0]) == n and all(len(c) == 12 and c == outs[0][0][0] for c in outs[0][0])


# ------------------------------------------------------------------ server
def test_server_serves_an_mxfp4_model_like_any_other(gpu, monkeypatch):
    """An LWC_MODELS entry with "mxfp4": true answers /chat/completions and votes in /score/completions."""
    import asyncio

    import httpx

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.server.app import create_app
    from llm_weighted_consensus_amd.server.config import Config
    from llm_weighted_consensus_amd.server.main import build_state

    monkeypatch.delenv("LWC_FAULT", raising=False)
    models = {"tiny4": {"arch": "llama-tiny", "weights": "random:1", "max_model_len": 2048, "max_batch": 64,
                        "mxfp4": True}}
    state = build_state(Config(models=models, kv_fraction=0.05))
    assert isinstance(state.services["tiny4"].engine.model.layers[0].wo, ops.Mxfp4Weight)
    c = httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(state)), base_url="http://t", timeout=120)
    voter = {"model": "tiny4", "output_mode": "json_schema", "top_logprobs": 5}
    score = {"messages": [{"role": "user", "content": "Which city is the capital of France?"}],
             "model": {"llms": [voter, dict(voter, temperature=0.5)]}, "choices": ["Paris", "Madrid", "Rome"]}

    async def go():
        r = await c.post("/chat/completions", json={"model": "tiny4", "max_tokens": 8, "n": 2,
                                                    "messages": [{"role": "user", "content": "hi"}]})
        assert r.status_code == 200, r.text
        assert len(r.json()["choices"]) == 2 and r.json()["model"] == "tiny4"
        r = await c.post("/score/completions", json=score)
        assert r.status_code == 200, r.text
        body = r.json()
        voters = [ch for ch in body["choices"] if ch["index"] >= 3]
        assert len(voters) == 2 and all(v.get("error") is None for v in voters)
        assert sum(ch["confidence"] or 0 for ch in body["choices"] if ch["index"] < 3) == pytest.approx(1.0, abs=1e-6)

    try:
        asyncio.run(go())
    finally:
        for svc in state.services.values():
            svc.close()
