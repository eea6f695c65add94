"""W4A8 projections over MXFP4 weights on the GPU (csrc/kernels/mxfp4_a8.hip): exact one-hot probes of the mixed
e4m3 x e2m1 block-scaled MFMA (operand lane maps, nibble order, scale-to-block mapping, the K tiles), the GEMM and its
SwiGLU form against the exact product of the quantised operands, the wrappers, the refusals, the three tiny
decoders with ``mxfp4_act="e4m3"`` against the emulated and the unquantised forward of their dequantised twin, the
engine (captured graphs == eager) and the server."""
import copy
from dataclasses import replace

import pytest
import torch

from tests import mxfp4_a8_ref, qwen_ref

pytestmark = pytest.mark.gpu

_W = {}  # (N, K, kind) -> (Mxfp4Weight, dequantised bf16 [N, K] by the host function): built once, never changed


def _close(a, b, atol, rtol=0.0):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    assert torch.isfinite(a).all(), "non-finite output"
    assert (err <= lim).all(), f"max err {err.max().item():.4g} (atol {atol}, rtol {rtol})"


def _i32(gpu, *v):
    return torch.tensor(list(v), dtype=torch.int32, device=gpu)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _weight(gpu, N, K, kind):
    """``spread``: block b of row n times 2^((n + b) % 13 - 6), so the scales cover 13 exponents; ``plain``:
    randn / sqrt(K) with one all-zero block and one all-zero row; ``swiglu``: plain, quantised after the 32-row
    gate|up interleave (dq stays [gate; up])."""
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


def _acts(gpu, M, K, seed, lda=None):
    """Row-quantised randn activations -> (Aq e4m3 [M, K] (a view of [M, lda] with ``lda``), a_scale [M])."""
    from llm_weighted_consensus_amd import ops

    g = torch.Generator(device="cpu").manual_seed(seed)
    aq, s = ops.quant_fp8_rows(torch.randn(M, K, generator=g).to(gpu).to(torch.bfloat16))
    if lda is not None:
        big = torch.zeros(M, lda, device=gpu).to(torch.float8_e4m3fn)
        big[:, :K] = aq
        big[:, K:] = torch.full((M, lda - K), 3.0, device=gpu).to(torch.float8_e4m3fn)  # must not be read
        aq = big[:, :K]
    return aq, s


def _exact(aq, s, dq):
    """The exact product of the quantised operands, fp64."""
    return (aq.double() @ dq.double().t()) * s.double().view(-1, 1)


# ------------------------------------------------------------------ exact one-hot probes
M_PROBE = 80  # ragged against the MFMA's 16 rows and the 128-row tile


def _probe_columns(K, launch):
    """80 k per launch.  Launches 0 and 1: every k of the first 128 (every position of an e4m3 lane's two 16-byte
    chunks and of an e2m1 lane's block, both sides of 15|16, 31|32, 63|64, 95|96).  Launch 2: the edges of the last
    128 and of its 32-blocks, then k spread over all the K tiles."""
    if launch < 2:
        return [48 * launch + m for m in range(M_PROBE)]
    last = K - 128
    ks = [last + r for r in (0, 31, 32, 63, 64, 95, 96, 127)]
    ks += [(m * 1237 + 5 * m * m + 77) % K for m in range(8, M_PROBE)]
    return ks


@pytest.mark.parametrize("K", [128, 1152, 3584])
@pytest.mark.parametrize("N", [16, 1040, 6144])
def test_onehot_rows_read_single_weights_exactly(gpu, N, K):
    """Row m of Aq is e4m3 1.0 at one k_m: out[m, n] is dq[n, k_m] bit for bit (the product and the sums with zeros
    are exact, the value is a bf16) — which k of the e4m3 operand meets which code and which scale byte of the e2m1
    operand; then with row scales 2^((m % 5) - 2): dq * a_scale, still exact.  W is random with a different scale
    per (row, block): no symmetry hides a swapped map."""
    from llm_weighted_consensus_amd import ops

    mw, dq = _weight(gpu, N, K, "spread")
    M = M_PROBE
    rows = torch.arange(M, device=gpu)
    ones = torch.ones(M, device=gpu)
    pow2 = torch.exp2(((rows % 5) - 2).float())
    for launch in range(3):
        ks = torch.tensor(_probe_columns(K, launch), device=gpu)
        A = torch.zeros(M, K, device=gpu)
        A[rows, ks] = 1.0
        Aq = A.to(torch.float8_e4m3fn)
        for what, sc in (("unit row scales", ones), ("power-of-two row scales", pow2)):
            out = ops.gemm_mxfp4_a8(Aq, sc, mw)
            want = (dq[:, ks].t().float() * sc.view(-1, 1)).to(torch.bfloat16)
            assert torch.equal(want.float(), dq[:, ks].t().float() * sc.view(-1, 1))  # (the reference is exact)
            bad = (_bits(out) != _bits(want)).nonzero()
            assert bad.numel() == 0, (f"launch {launch}, {what}: {bad.shape[0]} mismatches, first (m, n, k) = "
                                      f"({bad[0][0].item()}, {bad[0][1].item()}, {int(ks[bad[0][0]])}): got "
                                      f"{out[tuple(bad[0])].item()}, want {want[tuple(bad[0])].item()}")


# ------------------------------------------------------------------ against the exact product
@pytest.mark.parametrize("M", [1, 64, 65, 129, 300])
@pytest.mark.parametrize("N,K", [(16, 128), (1040, 384), (6144, 4096), (512, 18944)])
def test_gemm_matches_the_exact_product(gpu, M, N, K):
    """Both operands are exact in fp32, so kernel and fp64 reference differ by the accumulation order and one bf16
    rounding: the bounds of the bf16 GEMM tests.  Ragged row tiles (1, 65, 129, 300), a ragged column tile (1040),
    one K tile and 148; ``out`` is a view of a larger sentinel-filled buffer: rows past M and columns past N stay
    bitwise untouched."""
    from llm_weighted_consensus_amd import ops

    mw, dq = _weight(gpu, N, K, "plain")
    aq, s = _acts(gpu, M, K, M * 7 + N + K)
    buf = torch.full((M + 3, N + 16), 123.0, dtype=torch.bfloat16, device=gpu)
    out = ops.gemm_mxfp4_a8(aq, s, mw, out=buf[:M, :N])
    assert out.data_ptr() == buf.data_ptr()
    _close(out, _exact(aq, s, dq), 3e-2, 1e-2)
    assert bool((buf[M:] == 123.0).all()) and bool((buf[:, N:] == 123.0).all())
    assert bool((out[:, 3] == 0).all())  # the all-zero row of W
    if M == 129:  # a view of rows (lda > K) computes the same
        av, sv = _acts(gpu, M, K, M * 7 + N + K, lda=K + 64)
        assert av.stride(0) == K + 64 and torch.equal(sv, s)
        assert torch.equal(_bits(ops.gemm_mxfp4_a8(av, sv, mw)), _bits(out))


@pytest.mark.parametrize("M", [65, 300])
@pytest.mark.parametrize("N,K", [(64, 512), (1024, 1152), (28672, 4096)])
def test_swiglu_matches_the_exact_product(gpu, M, N, K):
    from llm_weighted_consensus_amd import ops

    mw, dq = _weight(gpu, N, K, "swiglu")
    aq, s = _acts(gpu, M, K, M + N + K)
    ref = _exact(aq, s, dq)
    F = N // 2
    buf = torch.full((M + 3, F + 16), 123.0, dtype=torch.bfloat16, device=gpu)
    out = ops.gemm_mxfp4_a8(aq, s, mw, out=buf[:M, :F], swiglu=True)
    assert out.shape == (M, F) and out.data_ptr() == buf.data_ptr()
    _close(out, torch.nn.functional.silu(ref[:, :F]) * ref[:, F:], 3e-2, 1e-2)
    assert bool((buf[M:] == 123.0).all()) and bool((buf[:, F:] == 123.0).all())
    assert bool((out[:, 3] == 0).all())  # silu(0) * up: the all-zero gate row


def test_launches_carry_no_state(gpu):
    """Three launches in a row, a fresh Aq each, each compared: nothing is left behind for the next one."""
    from llm_weighted_consensus_amd import ops

    mw, dq = _weight(gpu, 1040, 384, "plain")
    mg, dg = _weight(gpu, 1024, 1152, "swiglu")
    for i in range(3):
        aq, s = _acts(gpu, 129, 384, 100 + i)
        _close(ops.gemm_mxfp4_a8(aq, s, mw), _exact(aq, s, dq), 3e-2, 1e-2)
        aq, s = _acts(gpu, 65, 1152, 200 + i)
        ref = _exact(aq, s, dg)
        _close(ops.gemm_mxfp4_a8(aq, s, mg, swiglu=True), torch.nn.functional.silu(ref[:, :512]) * ref[:, 512:],
               3e-2, 1e-2)


# ------------------------------------------------------------------ wrappers, refusals
def test_wrappers_quantise_rows_and_take_a_qact(gpu):
    from llm_weighted_consensus_amd import ops

    torch.manual_seed(3)
    mw, _ = _weight(gpu, 1040, 384, "plain")
    x = torch.randn(130, 384, device=gpu).to(torch.bfloat16)
    xq, xs = ops.quant_fp8_rows(x)
    want = ops.gemm_mxfp4_a8(xq, xs, mw)
    assert torch.equal(_bits(ops.linear_mxfp4_a8(x, mw)), _bits(want))
    assert torch.equal(_bits(ops.linear_mxfp4_a8(ops.QAct(None, xq, xs), mw)), _bits(want))
    mg, _ = _weight(gpu, 1024, 1152, "swiglu")
    x = torch.randn(70, 1152, device=gpu).to(torch.bfloat16)
    xq, xs = ops.quant_fp8_rows(x)
    want = ops.gemm_mxfp4_a8(xq, xs, mg, swiglu=True)
    assert want.shape == (70, 512)
    assert torch.equal(_bits(ops.swiglu_mxfp4_a8(x, mg, 32)), _bits(want))
    assert torch.equal(_bits(ops.swiglu_mxfp4_a8(ops.QAct(None, xq, xs), mg, 32)), _bits(want))
    # the old wrappers still go where they went (tests/test_mxfp4_gpu.py pins the scratch path itself)
    assert ops.MXFP4_A8_MIN_ROWS == 65


def test_kernel_refusals_name_the_condition(gpu):
    from llm_weighted_consensus_amd import ops

    torch.manual_seed(0)

    def w(N, K):
        return ops.Mxfp4Weight((torch.randn(N, K, device=gpu) / K ** 0.5).to(torch.bfloat16))

    def a(M, K, dtype=torch.float8_e4m3fn):
        return torch.zeros(M, K, device=gpu).to(dtype), torch.ones(M, device=gpu)

    for N, K, msg in ((32, 192, "K % 128 == 0"), (24, 128, "N % 16 == 0")):
        assert not ops.mxfp4_a8_ok(70, N, K)
        with pytest.raises(RuntimeError, match=msg):
            ops.gemm_mxfp4_a8(*a(70, K), w(N, K))
    assert not ops.mxfp4_a8_ok(70, 96, 128, swiglu=True)
    with pytest.raises(RuntimeError, match="N % 64 == 0"):
        ops.gemm_mxfp4_a8(*a(70, 128), w(96, 128), swiglu=True)
    mw = w(32, 128)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        ops.gemm_mxfp4_a8(*a(70, 128, torch.bfloat16), mw)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        ops.gemm_mxfp4_a8(*a(70, 128, torch.float8_e5m2), mw)
    aq, s = a(70, 128)
    with pytest.raises(RuntimeError, match="a_scale must hold one scale per row"):
        ops.gemm_mxfp4_a8(aq, s[:69], mw)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.gemm_mxfp4_a8(*a(70, 256), mw)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.gemm_mxfp4_a8(aq, s, mw, out=torch.empty(70, 16, dtype=torch.bfloat16, device=gpu))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.gemm_mxfp4_a8(torch.zeros(70, 136, device=gpu).to(torch.float8_e4m3fn)[:, :128], s, mw)


# ------------------------------------------------------------------ model
_models = {}


def _model(gpu, arch):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    if arch not in _models:
        _models[arch] = LlamaModel(decoder_config(arch), device=gpu, seed=0, max_position=1024, mxfp4=True,
                                   mxfp4_act="e4m3")
    return _models[arch]


def _twin(m):
    """The bf16 model computing the same function: every projection the host-dequantised tensor."""
    from llm_weighted_consensus_amd import ops

    t = copy.copy(m)
    t.layers = [replace(L, **{n: ops.dequant_mxfp4(getattr(L, n).q, getattr(L, n).s)
                              for n in ("wqkv", "wo", "w_gate_up", "w_down")}) for L in m.layers]
    return t


@pytest.mark.parametrize("arch", ["llama-tiny", "qwen2-tiny", "qwen3-tiny"])
def test_model_matches_its_emulated_and_its_unquantised_twin(gpu, arch, monkeypatch):
    """A 97-token prefill (W4A8: 97-row calls; the last layer's o / MLP run on the one kept row, weight-only), 7
    decode steps at B = 1 (weight-only), one decode step of 80 forked rows (W4A8 throughout).  Every logits row:
    cosine > 0.995 against the emulated forward (kernel against oracle), > 0.99 against the unquantised twin (the
    fp8 decoder's bound), and the B = 1 steps > 0.995 against the unquantised twin.  No scratch exists and the
    scratch wrappers are never called."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = _model(gpu, arch)
    cfg = m.cfg
    assert m.mxfp4 and m.weight_format == "mxfp4" and m.act_format == "e4m3"
    assert not m._planned_gemms and not m._dense_residual and not m.norm_folded
    assert m.mx_scratch is None
    for L in m.layers:
        assert L.gu_block == 32 and all(isinstance(getattr(L, n), ops.Mxfp4Weight)
                                        for n in ("wqkv", "wo", "w_gate_up", "w_down"))

    def never(*a, **k):
        raise AssertionError("the scratch wrappers were reached")

    monkeypatch.setattr(ops, "linear_mxfp4", never)
    monkeypatch.setattr(ops, "swiglu_mxfp4", never)
    calls = {"a8": 0, "skinny": 0}
    real_a8, real_sk = ops.gemm_mxfp4_a8, ops.skinny_mxfp4

    def count_a8(xq, *a, **k):
        assert xq.shape[0] >= ops.MXFP4_A8_MIN_ROWS
        calls["a8"] += 1
        return real_a8(xq, *a, **k)

    def count_sk(x, *a, **k):
        assert x.shape[0] < ops.MXFP4_A8_MIN_ROWS
        calls["skinny"] += 1
        return real_sk(x, *a, **k)

    monkeypatch.setattr(ops, "gemm_mxfp4_a8", count_a8)
    monkeypatch.setattr(ops, "skinny_mxfp4", count_sk)
    twin = _twin(m)
    nl = cfg.layers

    P, T = 97, 104
    cache = KVCache(cfg, 16, 16, gpu)
    toks = torch.randint(0, cfg.vocab_size, (T,), generator=torch.Generator().manual_seed(0)).to(gpu)
    plain = qwen_ref.qwen_forward(twin, toks)
    body = torch.arange(T, device=gpu) < P  # the prompt's rows ran in 97-row calls ...
    emu = mxfp4_a8_ref.a8_forward(twin, toks, body, torch.zeros(T, dtype=torch.bool, device=gpu))  # ... but the tail
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    lg = m.prefill(toks[:P].int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    assert calls == {"a8": 4 * nl - 3, "skinny": 3}
    worst_emu, worst_plain = [], []

    def check(row, e, p, where, plain_bound=0.99):
        ce = qwen_ref.row_cosines(row.view(1, -1), e.view(1, -1)).item()
        cp = qwen_ref.row_cosines(row.view(1, -1), p.view(1, -1)).item()
        worst_emu.append(ce)
        worst_plain.append(cp)
        assert ce > 0.995, (where, ce)
        assert cp > plain_bound, (where, cp)

    check(lg[0], emu[P - 1], plain[P - 1], "prefill")
    bt = torch.arange(8, dtype=torch.int32, device=gpu).view(1, 8)
    calls.update(a8=0, skinny=0)
    for t in range(P, T):
        dl = m.decode(toks[t:t + 1].int(), _i32(gpu, t), _i32(gpu, t), bt, _i32(gpu, t + 1), cache, num_splits=2)
        check(dl[0], emu[t], plain[t], f"decode {t}", plain_bound=0.995)
    assert calls == {"a8": 0, "skinny": 4 * nl * (T - P)}  # today's path

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
    calls.update(a8=0, skinny=0)
    lg = m.decode(nxt.int(), full(P), (own * 16 + P % 16).int(), bt, full(P + 1), cache)
    assert calls == {"a8": 4 * nl, "skinny": 0}
    new = torch.arange(P + 1, device=gpu) == P  # the 33-row prefill was weight-only; the new row ran in 80-row calls
    for b in range(B):
        seq = torch.cat([prompt, nxt[b:b + 1]])
        check(lg[b], mxfp4_a8_ref.a8_forward(twin, seq, new, new)[-1], qwen_ref.qwen_forward(twin, seq)[-1], f"row {b}")
    assert m.mx_scratch is None
    print(f"{arch} mxfp4 + e4m3: worst logit cosine {min(worst_emu):.5f} against the emulated forward, "
          f"{min(worst_plain):.5f} against the unquantised twin")


# ------------------------------------------------------------------ engine
def test_engine_generates_and_graphs_match_eager(gpu, monkeypatch):
    """build_engine with "mxfp4_act": "e4m3" generates; greedy decode through captured graphs == eager decode token
    for token at n = 4 (weight-only path), n = 72 (the W4A8 kernel inside a captured graph) and n = 300 (several
    row tiles); every KV block is back in the pool afterwards."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.group import build_engine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams

    monkeypatch.setenv("LWC_STEP_AB", "0")
    eng = build_engine({"arch": "llama-tiny", "weights": "random:0", "mxfp4": True, "mxfp4_act": "e4m3",
                        "max_model_len": 256, "max_batch": 128, "kv_fraction": 0.02, "device": gpu.index or 0}, 0)
    model, tok = eng.model, eng.tokenizer
    assert model.mxfp4 and model.act_format == "e4m3" and model.mx_scratch is None
    assert isinstance(model.layers[0].wqkv, ops.Mxfp4Weight)
    free = eng.bm.num_free
    prompt = tok.encode("a prompt of more than one KV block, for a 4-bit voter")
    out = eng.generate([prompt], SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True), n=2)
    assert [len(c) for c in out[0]] == [8, 8] and out[0][0] == out[0][1] and eng.bm.num_free == free

    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    for n in (4, 72, 300):
        outs = []
        for graphs in (False, True):
            e = LLMEngine(model, tok, num_blocks=1024, max_batch=320, max_model_len=256, use_graphs=graphs)
            outs.append(e.generate([prompt], sp, n=n))
            assert e.bm.num_free == 1024
        assert outs[0] == outs[1], n
        assert len(outs[0][0]) == n and all(len(c) == 12 and c == outs[0][0][0] for c in outs[0][0])


# ------------------------------------------------------------------ server
def test_server_serves_the_variant_like_any_other_model(gpu, monkeypatch):
    """An LWC_MODELS entry with "mxfp4_act": "e4m3" answers /chat/completions and votes in /score/completions."""
    import asyncio

    import httpx

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.server.app import create_app
    from llm_weighted_consensus_amd.server.config import Config
    from llm_weighted_consensus_amd.server.main import build_state

    monkeypatch.delenv("LWC_FAULT", raising=False)
    models = {"tiny48": {"arch": "llama-tiny", "weights": "random:1", "max_model_len": 2048, "max_batch": 64,
                         "mxfp4": True, "mxfp4_act": "e4m3"}}
    state = build_state(Config(models=models, kv_fraction=0.05))
    model = state.services["tiny48"].engine.model
    assert isinstance(model.layers[0].wo, ops.Mxfp4Weight) and model.act_format == "e4m3"
    c = httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(state)), base_url="http://t", timeout=120)
    voter = {"model": "tiny48", "output_mode": "json_schema", "top_logprobs": 5}
    score = {"messages": [{"role": "user", "content": "Which city is the capital of France?"}],
             "model": {"llms": [voter, dict(voter, temperature=0.5)]}, "choices": ["Paris", "Madrid", "Rome"]}

    async def go():
        r = await c.post("/chat/completions", json={"model": "tiny48", "max_tokens": 8, "n": 2,
                                                    "messages": [{"role": "user", "content": "hi"}]})
        assert r.status_code == 200, r.text
        assert len(r.json()["choices"]) == 2 and r.json()["model"] == "tiny48"
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
