"""Qwen2.5 / Qwen3 decoders on the GPU: the bias + per-head RMSNorm + RoPE + KV-write kernel against fp32, and the
models that call it (prefill, decode, encode, folded norms, fp8, engine, LoRA, server) against the fp32 forward
of tests/qwen_ref.py."""
import asyncio
import copy

import pytest
import torch

from tests import qwen_ref
from tests import torch_ref as ref

pytestmark = pytest.mark.gpu

D, BS, NB, EPS = 128, 16, 12, 1e-6
HEADS = [(3, 1), (8, 2), (40, 8)]  # units of 8 lanes: 32 (half a wave idle), 80 (one round), 384 (256 + 128)
FEATURES = ["norms", "bias", "both"]


def _close(a, b, atol, rtol=0.0):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    assert torch.isfinite(a).all(), "non-finite output"
    assert (err <= lim).all(), f"max err {err.max().item():.4g} (atol {atol}, rtol {rtol})"


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def tables(gpu):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import rope_tables

    return rope_tables(decoder_config("qwen3-tiny"), gpu, 256)


def _case(gpu, Hq, Hkv, T, features, seed=0):
    """Inputs of one kernel call: qkv rows, positions, a slot permutation, the optional operands."""
    g = torch.Generator(device="cpu").manual_seed(1000 * Hq + 10 * T + seed)
    bf = torch.bfloat16
    n = (Hq + 2 * Hkv) * D
    qkv = torch.randn(T, n, generator=g).to(bf).to(gpu)
    pos = torch.randint(0, 200, (T,), generator=g, dtype=torch.int32).to(gpu)
    slots = torch.randperm(NB * BS, generator=g)[:T].to(torch.int32).to(gpu)
    bias = (0.5 * torch.randn(n, generator=g)).to(bf).to(gpu) if features in ("bias", "both") else None
    qw = kw = None
    if features in ("norms", "both"):
        qw = (1 + 0.3 * torch.randn(D, generator=g)).to(bf).to(gpu)
        kw = (1 + 0.3 * torch.randn(D, generator=g)).to(bf).to(gpu)
    return qkv, pos, slots, bias, qw, kw


def _caches(gpu, Hkv):
    return (torch.zeros(NB, Hkv, BS, D, dtype=torch.bfloat16, device=gpu),
            torch.zeros(NB, Hkv, BS // 4, D, 4, dtype=torch.bfloat16, device=gpu))


def _reference(qkv0, pos, cos, sin, Hq, Hkv, bias, qw, kw):
    """fp32 from the bf16 inputs: (q rotated, q normalised but not rotated, k rotated, v)."""
    T = qkv0.shape[0]
    x = qkv0.float() + (bias.float() if bias is not None else 0.0)
    q = x[:, : Hq * D].view(T, Hq, D)
    k = x[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
    v = x[:, (Hq + Hkv) * D:].view(T, Hkv, D)
    if qw is not None:
        q = ref.rmsnorm(q, qw, EPS)
    if kw is not None:
        k = ref.rmsnorm(k, kw, EPS)
    return ref.rope(q, pos, cos, sin), q, ref.rope(k, pos, cos, sin), v


def _split(qkv, Hq, Hkv):
    T = qkv.shape[0]
    return (qkv[:, : Hq * D].view(T, Hq, D), qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D),
            qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D))


@pytest.mark.parametrize("features", FEATURES)
@pytest.mark.parametrize("T", [1, 21])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_kernel_matches_fp32(gpu, tables, Hq, Hkv, T, features):
    from llm_weighted_consensus_amd import ops

    cos, sin = tables
    qkv0, pos, slots, bias, qw, kw = _case(gpu, Hq, Hkv, T, features)
    q_rot, q_plain, k_ref, v_ref = _reference(qkv0, pos, cos, sin, Hq, Hkv, bias, qw, kw)
    blk, off = (slots // BS).long(), (slots % BS).long()
    kw_args = dict(slots=slots, bias=bias, q_weight=qw, k_weight=kw, eps=EPS)
    v_tol = (1e-2, 1e-2) if bias is not None else (0, 0)

    # rope_q=True (prefill, mixed steps): q, k rotated in place, v biased in place, k and v cached
    a = qkv0.clone()
    kc, vc = _caches(gpu, Hkv)
    ops.qknorm_rope_kv_write(a, pos, cos, sin, kc, vc, Hq, Hkv, D, rope_q=True, **kw_args)
    q, k, v = _split(a, Hq, Hkv)
    _close(q, q_rot, 3e-2, 2e-2)
    _close(k, k_ref, 3e-2, 2e-2)
    _close(v, v_ref, *v_tol)
    _close(kc[blk, :, off, :], k_ref, 3e-2, 2e-2)
    _close(ops.v_token(vc, blk, off), v_ref, *v_tol)
    assert torch.equal(_bits(kc[blk, :, off, :]), _bits(k))  # cached k == written-back k, bit for bit
    assert torch.equal(_bits(ops.v_token(vc, blk, off)), _bits(v))
    assert int((kc != 0).sum()) == int((kc[blk, :, off, :] != 0).sum())  # nothing outside the rows' lines
    assert int((vc != 0).sum()) == int((ops.v_token(vc, blk, off) != 0).sum())

    # rope_q=False (pure decode steps): q biased and normalised but NOT rotated; k, v only into the caches, which
    # end up bitwise as above
    b = qkv0.clone()
    kc2, vc2 = _caches(gpu, Hkv)
    ops.qknorm_rope_kv_write(b, pos, cos, sin, kc2, vc2, Hq, Hkv, D, rope_q=False, **kw_args)
    q2, k2, v2 = _split(b, Hq, Hkv)
    _close(q2, q_plain, 3e-2, 2e-2)
    assert torch.equal(_bits(kc2), _bits(kc)) and torch.equal(_bits(vc2), _bits(vc))
    q0, k0, v0 = _split(qkv0, Hq, Hkv)
    assert torch.equal(_bits(k2), _bits(k0)) and torch.equal(_bits(v2), _bits(v0))  # no write-back of k, v


@pytest.mark.parametrize("features", FEATURES)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_kernel_padding_rows(gpu, tables, Hq, Hkv, features):
    """Padding rows of a decode bucket (slot -1), k-only mode: no cache line is touched for them, their q / k / v
    are processed in place (as rope_kv_write does for k); the real rows are cached as without padding."""
    from llm_weighted_consensus_amd import ops

    cos, sin = tables
    T = 21
    qkv0, pos, slots, bias, qw, kw = _case(gpu, Hq, Hkv, T, features, seed=1)
    q_rot, q_plain, k_ref, v_ref = _reference(qkv0, pos, cos, sin, Hq, Hkv, bias, qw, kw)
    kw_args = dict(bias=bias, q_weight=qw, k_weight=kw, eps=EPS)
    full = qkv0.clone()
    kc, vc = _caches(gpu, Hkv)
    ops.qknorm_rope_kv_write(full, pos, cos, sin, kc, vc, Hq, Hkv, D, slots=slots, rope_q=False, **kw_args)
    sl = slots.clone()
    sl[::3] = -1
    pad, real = sl < 0, sl >= 0
    a = qkv0.clone()
    kc3, vc3 = _caches(gpu, Hkv)
    ops.qknorm_rope_kv_write(a, pos, cos, sin, kc3, vc3, Hq, Hkv, D, slots=sl, rope_q=False, **kw_args)
    b3, o3 = (sl[real] // BS).long(), (sl[real] % BS).long()
    assert torch.equal(_bits(kc3[b3, :, o3, :]), _bits(kc[b3, :, o3, :]))
    assert torch.equal(_bits(ops.v_token(vc3, b3, o3)), _bits(ops.v_token(vc, b3, o3)))
    assert int((kc3 != 0).sum()) == int((kc3[b3, :, o3, :] != 0).sum())
    assert int((vc3 != 0).sum()) == int((ops.v_token(vc3, b3, o3) != 0).sum())
    q, k, v = _split(a, Hq, Hkv)
    _close(q, q_plain, 3e-2, 2e-2)  # every row's q: normalised, un-rotated
    _close(k[pad], k_ref[pad], 3e-2, 2e-2)
    _close(v[pad], v_ref[pad], *((1e-2, 1e-2) if bias is not None else (0, 0)))
    assert torch.equal(_bits(a[real]), _bits(full[real]))
    # slots=None (encode): every row is such a row, with q rotated
    c = qkv0.clone()
    kc4, vc4 = _caches(gpu, Hkv)
    ops.qknorm_rope_kv_write(c, pos, cos, sin, kc4, vc4, Hq, Hkv, D, rope_q=True, **kw_args)
    q, k, v = _split(c, Hq, Hkv)
    _close(q, q_rot, 3e-2, 2e-2)
    _close(k, k_ref, 3e-2, 2e-2)
    _close(v, v_ref, *((1e-2, 1e-2) if bias is not None else (0, 0)))
    assert not bool(kc4.any()) and not bool(vc4.any())


@pytest.mark.parametrize("T", [1, 21])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_kernel_without_operands_is_rope_kv_write(gpu, tables, Hq, Hkv, T):
    """bias, q_weight and k_weight all None: qkv and both caches bitwise as ops.rope_kv_write leaves them, in both
    rope_q modes, with padding rows."""
    from llm_weighted_consensus_amd import ops

    cos, sin = tables
    qkv0, pos, slots, _, _, _ = _case(gpu, Hq, Hkv, T, "none", seed=2)
    if T > 1:
        slots[::3] = -1
    for rope_q in (True, False):
        a, b = qkv0.clone(), qkv0.clone()
        (kc, vc), (kc2, vc2) = _caches(gpu, Hkv), _caches(gpu, Hkv)
        ops.rope_kv_write(a, pos, cos, sin, kc, vc, Hq, Hkv, D, slots=slots, rope_q=rope_q)
        ops.qknorm_rope_kv_write(b, pos, cos, sin, kc2, vc2, Hq, Hkv, D, slots=slots, rope_q=rope_q, eps=EPS)
        assert torch.equal(_bits(a), _bits(b)), rope_q
        assert torch.equal(_bits(kc), _bits(kc2)) and torch.equal(_bits(vc), _bits(vc2)), rope_q
        assert bool(kc.any()) and bool(vc.any())


def test_kernel_in_a_captured_graph(gpu, tables):
    """The op as a graph node: no allocation, no synchronisation; two replays on changed inputs == eager."""
    from llm_weighted_consensus_amd import ops

    cos, sin = tables
    Hq, Hkv, T = 8, 2, 21
    qkv_s, pos_s, slots_s, bias, qw, kw = _case(gpu, Hq, Hkv, T, "both", seed=3)
    kc_s, vc_s = _caches(gpu, Hkv)

    def run(qkv, pos, slots, kc, vc):
        ops.qknorm_rope_kv_write(qkv, pos, cos, sin, kc, vc, Hq, Hkv, D, slots=slots, rope_q=False, bias=bias,
                                 q_weight=qw, k_weight=kw, eps=EPS)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(qkv_s, pos_s, slots_s, kc_s, vc_s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(qkv_s, pos_s, slots_s, kc_s, vc_s)
    for seed in (4, 5):
        qkv, pos, slots, _, _, _ = _case(gpu, Hq, Hkv, T, "both", seed=seed)
        want = qkv.clone()
        kc, vc = _caches(gpu, Hkv)
        run(want, pos, slots, kc, vc)
        qkv_s.copy_(qkv), pos_s.copy_(pos), slots_s.copy_(slots)
        kc_s.zero_(), vc_s.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(qkv_s), _bits(want)) and not torch.equal(_bits(want), _bits(qkv))
        assert torch.equal(_bits(kc_s), _bits(kc)) and torch.equal(_bits(vc_s), _bits(vc)) and bool(kc.any())


def test_kernel_refuses_what_it_does_not_take(gpu):
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import rope_tables

    bf = dict(dtype=torch.bfloat16, device=gpu)
    pos = torch.zeros(4, dtype=torch.int32, device=gpu)
    cos64, sin64 = rope_tables(decoder_config("qwen3-tiny", head_dim=64), gpu, 16)
    with pytest.raises(RuntimeError, match="128"):  # D = 64
        ops.qknorm_rope_kv_write(torch.zeros(4, 12 * 64, **bf), pos, cos64, sin64, torch.zeros(2, 2, 16, 64, **bf),
                                 torch.zeros(2, 2, 4, 64, 4, **bf), 8, 2, 64, q_weight=torch.ones(64, **bf))
    cos, sin = rope_tables(decoder_config("qwen3-tiny"), gpu, 16)
    qkv = torch.zeros(4, 12 * D, **bf)
    kc, vc = torch.zeros(2, 2, 16, D, **bf), torch.zeros(2, 2, 4, D, 4, **bf)
    with pytest.raises(RuntimeError, match="bias"):  # a bias of q's length only
        ops.qknorm_rope_kv_write(qkv, pos, cos, sin, kc, vc, 8, 2, D, bias=torch.zeros(8 * D, **bf))
    with pytest.raises(RuntimeError, match="k_weight"):
        ops.qknorm_rope_kv_write(qkv, pos, cos, sin, kc, vc, 8, 2, D, k_weight=torch.ones(64, **bf))
    assert not bool(qkv.any()) and not bool(kc.any())


# ------------------------------------------------------------------------------------------------ model


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm())).item()


def _model(gpu, arch, **kw):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    return LlamaModel(decoder_config(arch), device=gpu, max_position=1024, **{"seed": 0, **kw})


@pytest.fixture(scope="module")
def qwen3(gpu):
    return _model(gpu, "qwen3-tiny")


@pytest.fixture(scope="module")
def qwen2(gpu):
    return _model(gpu, "qwen2-tiny")


@pytest.fixture(params=["qwen3-tiny", "qwen2-tiny"])
def model(request, qwen3, qwen2):
    return qwen3 if request.param == "qwen3-tiny" else qwen2


def _i32(gpu, *v):
    return torch.tensor(list(v), dtype=torch.int32, device=gpu)


def test_prefill_and_decode_match_reference(model, gpu):
    """Prefill of a 48-token prompt, then 8 decode steps (k-only kernel mode, q rotated as the attention kernels
    load it): every logits row against the fp32 forward."""
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = model
    L = m.layers[0]
    assert (L.bqkv is not None) == m.cfg.qkv_bias and (L.q_norm is not None) == m.cfg.qk_norm
    cache = KVCache(m.cfg, 64, 16, gpu)
    P, N = 48, 56
    toks = torch.randint(0, m.cfg.vocab_size, (N,), generator=torch.Generator().manual_seed(3)).to(gpu)
    want = qwen_ref.qwen_forward(m, toks)
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    lg = m.prefill(toks[:P].int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    c = _cos(lg[0], want[P - 1])
    print(f"{m.cfg.name} prefill: cos {c:.5f}")
    assert c > 0.995
    bt = torch.arange(4, dtype=torch.int32, device=gpu).view(1, 4)
    for t in range(P, N):
        dl = m.decode(toks[t:t + 1].int(), _i32(gpu, t), _i32(gpu, t), bt, _i32(gpu, t + 1), cache, num_splits=2)
        c = _cos(dl[0], want[t])
        print(f"{m.cfg.name} decode {t}: cos {c:.5f}")
        assert c > 0.995, t


def test_encode_rows_match_reference_hidden_states(model, gpu):
    m = model
    g = torch.Generator().manual_seed(4)
    seqs = [torch.randint(0, m.cfg.vocab_size, (n,), generator=g).to(gpu) for n in (48, 13)]
    pos = torch.cat([torch.arange(len(s), dtype=torch.int32, device=gpu) for s in seqs])
    h = m.encode(torch.cat(seqs).int(), pos, _i32(gpu, 0, 48, 61), 48)
    want = torch.cat([qwen_ref.qwen_forward(m, s, hidden_only=True) for s in seqs])
    cs = qwen_ref.row_cosines(h, want)
    print(f"{m.cfg.name} encode: worst row cos {float(cs.min()):.5f}")
    assert h.shape == want.shape and float(cs.min()) > 0.995


def test_folded_norm_chain_matches_unfolded(model, gpu):
    """As tests/test_model_gpu.py test_folded_norm_chain_matches_unfolded, B = 300: the chain's qkv GEMM feeds
    the Qwen kernel."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = model
    assert m.norm_folded
    cache = KVCache(m.cfg, 64, 16, gpu)
    toks = torch.randint(0, m.cfg.vocab_size, (36,), generator=torch.Generator().manual_seed(3)).to(gpu)
    want = qwen_ref.qwen_forward(m, toks)
    P, B = 35, 300
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    m.prefill(toks[:P].int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    bt = torch.arange(4, dtype=torch.int32, device=gpu).view(1, 4).expand(B, 4).contiguous()
    full = lambda v: torch.full((B,), v, dtype=torch.int32, device=gpu)  # noqa: E731
    args = (toks[P:P + 1].int().expand(B).contiguous(), full(P), full(P), bt, full(P + 1), cache)
    if m.chain is None:
        m.chain = ops.NormChain(8192, m.cfg.hidden, m.cfg.rms_eps, gpu)
    saved = dict(m.chain_m)
    try:
        m.chain_m[B] = {"attn": False, "mlp": False, "final": False, "qkv_bn": 192, "o": "plain", "down": "plain"}
        assert not m.chain_ok(B)
        base = m.decode(*args, num_splits=1).float()
        m.chain_m[B] = {"attn": True, "mlp": True, "final": True, "qkv_bn": 192, "o": "own32", "down": "own64"}
        assert m.chain_ok(B)
        got = m.decode(*args, num_splits=1).float()
    finally:
        m.chain_m.clear()
        m.chain_m.update(saved)
    assert _cos(got, base) > 0.9995
    assert _cos(got[B - 1], want[P]) > 0.995 and _cos(got[0], want[P]) > 0.995


@pytest.mark.parametrize("arch", ["qwen3-tiny", "qwen2-tiny"])
def test_fp8_dense_prefill_matches_dequantised_reference(gpu, arch):
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = _model(gpu, arch, seed=3, fp8_dense=True)
    assert isinstance(m.layers[0].wqkv, ops.Fp8Weight)
    cache = KVCache(m.cfg, 64, 16, gpu)
    P = 48
    toks = torch.randint(0, m.cfg.vocab_size, (P,), generator=torch.Generator().manual_seed(6)).to(gpu)
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    lg = m.prefill(toks.int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    c = _cos(lg[0], qwen_ref.qwen_forward(m, toks)[P - 1])
    print(f"{arch} fp8 prefill: cos {c:.5f}")
    assert c > 0.99


# ------------------------------------------------------------------------------------------------ engine


def test_engine_greedy_graph_equivalence(qwen3, gpu, monkeypatch):
    """Captured decode graphs (the kernel as a graph node, k-only mode) == eager decode, greedy, token for token."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    monkeypatch.setenv("LWC_STEP_AB", "0")
    tok = ByteTokenizer(qwen3.cfg.vocab_size)
    prompts = [tok.encode("hello world, this is a prompt of some length " * 2), tok.encode("short")]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(qwen3, tok, num_blocks=256, max_batch=16, max_model_len=512, use_graphs=graphs)
        outs.append(eng.generate(prompts, sp, n=3))
        assert eng.bm.num_free == 256
    assert outs[0] == outs[1]
    for group in outs[0]:
        assert all(c == group[0] for c in group) and all(len(c) == 24 for c in group)
    first = int(qwen_ref.qwen_forward(qwen3, torch.tensor(prompts[0], device=gpu))[-1].argmax())
    assert outs[0][0][0][0] == first


def test_engine_chunked_prefill_matches_whole_prompt(qwen3):
    """Mixed chunked-prefill steps (decode rows and prompt-chunk rows through one kernel call, rope_q on) give the
    whole-prompt run's greedy continuations, by the comparison of tests/test_chunked_prefill_gpu.py."""
    from tests.test_chunked_prefill_gpu import _assert_same_greedy, _run

    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, 4000, (n,), generator=g).tolist() for n in (150, 17, 64)]
    want, _ = _run(qwen3, prompts, 0)
    got, eng = _run(qwen3, prompts, 48)
    assert eng.stats["mixed_steps"] == eng.stats["prefill_chunks"] >= sum(len(p) for p in prompts) // 48
    _assert_same_greedy(got, want)


# ------------------------------------------------------------------------------------------------ LoRA


def test_lora_on_qkv_matches_merged_reference(gpu):
    """One adapter on q, k, v of qwen2-tiny: the adapter adds to the projection output BEFORE the bias and the
    rotation.  Adapted prefill and decode against the fp32 forward of the merged weights (same bias)."""
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache, LayerWeights, LlamaModel
    from llm_weighted_consensus_amd.models.lora import merged_weights, random_adapter

    cfg = decoder_config("qwen2-tiny")
    ad = random_adapter("a", cfg, seed=11, rank=8, alpha=16, targets=("q", "k", "v"), std=0.1)
    m = LlamaModel(cfg, device=gpu, seed=0, max_position=1024, lora=[ad])
    assert m.lora is not None and not m.norm_folded and m.layers[0].bqkv is not None
    merged = copy.copy(m)
    merged.layers = []
    for li, L in enumerate(m.layers):
        w = merged_weights(L, m.lora.adapters[0], li)
        merged.layers.append(LayerWeights(L.attn_norm, w["wqkv"], w["wo"], L.mlp_norm, w["w_gate_up"], w["w_down"],
                                          L.gu_block, bqkv=L.bqkv))
    cache = KVCache(m.cfg, 64, 16, gpu)
    g = torch.Generator().manual_seed(5)
    lens, steps = [33, 20], 4
    toks = [torch.randint(0, cfg.vocab_size, (n + steps,), generator=g).to(gpu) for n in lens]
    refs = [qwen_ref.qwen_forward(merged, toks[0]), qwen_ref.qwen_forward(m, toks[1])]
    assert _cos(refs[0][lens[0] - 1], qwen_ref.qwen_forward(m, toks[0])[lens[0] - 1]) < 0.9  # the adapter matters

    def run(row_ids):
        cache.pool.zero_()
        i32 = dict(dtype=torch.int32, device=gpu)
        pos = torch.cat([torch.arange(n, **i32) for n in lens])
        slots = torch.cat([64 * r + torch.arange(n, **i32) for r, n in enumerate(lens)])
        cu = _i32(gpu, 0, lens[0], sum(lens))
        out = [m.prefill(torch.cat([t[:n] for t, n in zip(toks, lens)]).int(), pos, slots, cu, max(lens),
                         (cu[1:] - 1).long(), cache,
                         lora_ids=row_ids.repeat_interleave(torch.tensor(lens, device=gpu)))]
        bt = torch.arange(8, **i32).view(2, 4)
        for s in range(steps):
            p = torch.tensor([n + s for n in lens], **i32)
            tk = torch.stack([t[n + s] for t, n in zip(toks, lens)]).int()
            sl = torch.tensor([64 * r + n + s for r, n in enumerate(lens)], **i32)
            out.append(m.decode(tk, p, sl, bt, p + 1, cache, num_splits=2, lora_ids=row_ids))
        return out

    outs = run(_i32(gpu, 0, -1))
    for s, lg in enumerate(outs):
        for r in range(2):
            c = _cos(lg[r], refs[r][lens[r] - 1 + s])
            print(f"step {s} row {r}: cos {c:.5f}")
            assert c > 0.995, (s, r, c)
    none = run(_i32(gpu, -1, -1))
    for a, b in zip(outs, none):  # the row without an adapter is the base model's row, bit for bit
        assert torch.equal(_bits(a[1]), _bits(b[1]))


# ------------------------------------------------------------------------------------------------ server


def test_server_serves_a_qwen_voter(gpu, monkeypatch):
    import httpx

    from llm_weighted_consensus_amd.server.app import create_app
    from llm_weighted_consensus_amd.server.config import Config
    from llm_weighted_consensus_amd.server.main import build_state

    monkeypatch.delenv("LWC_FAULT", raising=False)
    models = {"q": {"arch": "qwen3-tiny", "weights": "random:0", "chat_template": "chatml", "max_model_len": 1024,
                    "max_batch": 16}}
    state = build_state(Config(models=models, kv_fraction=0.05))
    c = httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(state)), base_url="http://t", timeout=120)

    async def go():
        r = await c.post("/chat/completions", json={"model": "q", "max_tokens": 8, "n": 2, "seed": 1,
                                                    "messages": [{"role": "user", "content": "hi"}]})
        assert r.status_code == 200, r.text
        ch = r.json()["choices"]
        assert sorted(x["index"] for x in ch) == [0, 1] and all(x["message"] is not None for x in ch)

    try:
        assert state.services["q"].engine.cfg.qk_norm
        asyncio.run(go())
    finally:
        for svc in state.services.values():
            svc.close()
