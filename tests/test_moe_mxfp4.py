"""MoE decoders with MXFP4 experts, without a GPU: the spec key and its refusals, the expert-stack container, the CPU
model against its dequantised twin, and the two safetensors loaders."""
import pytest
import torch

from tests import qwen_moe_ref
from tests import torch_ref as ref

ADS = {"a": {"weights": "random:7"}}


def _cfg(name, **kw):
    from llm_weighted_consensus_amd.models.config import decoder_config

    return decoder_config(name, **kw)


# ------------------------------------------------------------------ spec key and refusals
@pytest.mark.parametrize("spec,embedder,msg", [
    ({"expert_weights": "fp4"}, False, "expert_weights 'fp4': must be one of 'bf16', 'mxfp4'"),
    ({"expert_weights": "mxfp4", "arch": "llama-tiny"}, False, r"expert_weights applies to MoE decoders only \(llama-tiny"),
    ({"expert_weights": "bf16", "arch": "llama-tiny"}, False, "expert_weights applies to MoE decoders only"),
    ({"expert_weights": "mxfp4", "fp8": True}, False, "mxfp4 expert weights do not combine with fp8 weights"),
    ({"expert_weights": "mxfp4", "tp": 2}, False, "mxfp4 expert weights do not combine with tp > 1"),
    ({"expert_weights": "mxfp4", "adapters": ADS}, False, "mxfp4 expert weights do not combine with LoRA adapters"),
    ({"expert_weights": "mxfp4"}, True, "mxfp4 expert weights are served on generation models only"),
    # the dense flag on a MoE arch stays refused in the words it always had, with or without the new key
    ({"mxfp4": True}, False, r"mxfp4 weights are not supported on MoE decoders \(mixtral-tiny\)"),
    ({"mxfp4": True, "expert_weights": "mxfp4"}, False, r"mxfp4 weights are not supported on MoE decoders \(mixtral-tiny\)"),
])
def test_spec_refusals(spec, embedder, msg):
    from llm_weighted_consensus_amd.models.lora import check_model_spec

    spec = {"arch": "mixtral-tiny", "weights": "random:0", **spec}
    with pytest.raises(ValueError, match=msg):
        check_model_spec("m", spec, embedder=embedder)
    # the factories refuse before they touch a device or a weight
    if embedder:
        from llm_weighted_consensus_amd.embeddings.service import build_embedding_service

        with pytest.raises(ValueError, match=msg):
            build_embedding_service("m", spec, "cpu")
    else:
        from llm_weighted_consensus_amd.engine.group import build_engine

        with pytest.raises(ValueError, match="^model mixtral-tiny: |^model llama-tiny: "):
            build_engine(spec, 0)


def test_spec_accepts_the_key_on_moe_archs():
    from llm_weighted_consensus_amd.models.lora import check_model_spec

    assert check_model_spec("v", {"arch": "qwen3-moe-tiny", "expert_weights": "mxfp4"}) == ()
    for arch in ("qwen3-moe-tiny", "mixtral-tiny", "qwen3-30b-a3b", "mixtral-8x7b"):
        for fmt in ("bf16", "mxfp4"):
            assert check_model_spec("v", {"arch": arch, "weights": "random:0", "expert_weights": fmt}) == ()
    assert check_model_spec("v", {"arch": "mixtral-tiny", "expert_weights": "bf16", "fp8": True, "tp": 2}) == ()


def test_model_constructor_refusals():
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    cfg = _cfg("mixtral-tiny")
    for kw, msg in (({"expert_weights": "int4"}, "expert_weights 'int4': must be one of"),
                    ({"expert_weights": "mxfp4", "fp8": True}, "mxfp4 expert weights do not combine with fp8"),
                    ({"expert_weights": "mxfp4", "tp_size": 2}, "mxfp4 expert weights do not combine with tensor par"),
                    ({"expert_weights": "mxfp4", "ep_size": 2}, "mxfp4 expert weights do not combine with expert par"),
                    ({"expert_weights": "mxfp4", "mxfp4": True}, "mxfp4 weights are not supported on MoE")):
        with pytest.raises(ValueError, match=msg):
            MixtralModel(cfg, device="cpu", **kw)
    with pytest.raises(ValueError, match="expert_weights 'int4'"):
        Qwen3MoeModel(_cfg("qwen3-moe-tiny"), device="cpu", expert_weights="int4")


# ------------------------------------------------------------------ the container
def test_expert_stack_holds_the_documented_format():
    from llm_weighted_consensus_amd import ops

    E, N, K = 3, 64, 256
    w = (torch.randn(E, N, K, generator=torch.Generator().manual_seed(3)) * 0.05).to(torch.bfloat16)
    w[1, 7] = 0
    st = ops.Mxfp4Experts(w)
    assert st.shape == (E, N, K)
    assert st.q.shape == (E, N, K // 2) and st.s.shape == (E, N, K // 32)
    assert st.q.dtype == torch.uint8 and st.s.dtype == torch.uint8 and st.q.is_contiguous() and st.s.is_contiguous()
    assert st.nbytes == E * N * K * 17 // 32
    dq = st.dequant()
    assert dq.shape == (E, N, K) and dq.dtype == torch.bfloat16
    for e in range(E):
        q, s = ops.quant_mxfp4_weight(w[e])
        assert torch.equal(st.q[e], q) and torch.equal(st.s[e], s)
        assert torch.equal(dq[e], ops.dequant_mxfp4(q, s))
        one = st.expert(e)
        assert isinstance(one, ops.Mxfp4Weight) and one.shape == (N, K) and one.nbytes == N * K * 17 // 32
        assert one.q.data_ptr() == st.q[e].data_ptr() and one.s.data_ptr() == st.s[e].data_ptr()  # a view, no copy
        assert torch.equal(one.dequant(), dq[e])
    # per row, so it commutes with the gate|up interleave of an expert
    wi = ops.Mxfp4Experts(torch.stack([ops.swiglu_interleave(w[e], 32) for e in range(E)]))
    assert all(torch.equal(wi.q[e], ops.swiglu_interleave(st.q[e], 32)) for e in range(E))
    with pytest.raises(ValueError, match="K % 32"):
        ops.Mxfp4Experts(torch.zeros(2, 4, 48, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r"\[E, N, K\]"):
        ops.Mxfp4Experts(torch.zeros(4, 64, dtype=torch.bfloat16))


# ------------------------------------------------------------------ the CPU model
def _dq(w):
    from llm_weighted_consensus_amd import ops

    return torch.stack([ops.dequant_mxfp4(*ops.quant_mxfp4_weight(w[e])) for e in range(w.shape[0])])


def _build(arch, **kw):
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    cfg = _cfg(arch)
    return (Qwen3MoeModel if cfg.qk_norm else MixtralModel)(cfg, device="cpu", max_position=128, **kw)


@pytest.mark.parametrize("arch", ["qwen3-moe-tiny", "mixtral-tiny"])
def test_cpu_model_equals_the_dequantised_twin(arch):
    """On a CPU device the model holds the dequantised bf16 experts in the plain row order: its logits (the fp32
    oracle reads the model's own tensors) are those of a bf16 twin of the same seed whose experts were replaced by
    dequant(quant(w)), and nothing but the experts differs from the bf16 model."""
    m, twin, plain = _build(arch, seed=4, expert_weights="mxfp4"), _build(arch, seed=4), _build(arch, seed=4)
    assert m.expert_weights == "mxfp4" and twin.expert_weights == "bf16" and m.moe_scratch is None
    for L, T, P in zip(m.layers, twin.layers, plain.layers):
        T.w13, T.w2 = _dq(T.w13), _dq(T.w2)
        assert L.gu_block == T.gu_block == 0 and L.s13 is None and L.s2 is None
        for a, b in ((L.w13, T.w13), (L.w2, T.w2)):
            assert a.dtype == torch.bfloat16 and torch.equal(a, b)
        for n in ("wqkv", "wo", "router", "attn_norm", "mlp_norm"):
            assert torch.equal(getattr(L, n), getattr(P, n))
        assert not torch.equal(L.w13, P.w13) and not torch.equal(L.w2, P.w2)  # the quantisation is not a no-op
    assert torch.equal(m.embed, plain.embed) and torch.equal(m.lm_head, plain.lm_head)
    toks = torch.randint(0, m.cfg.vocab_size, (9,), generator=torch.Generator().manual_seed(1))
    oracle = qwen_moe_ref.qwen_moe_forward if m.cfg.qk_norm else ref.llama_forward
    assert torch.equal(oracle(m, toks), oracle(twin, toks))


def test_default_is_the_bf16_model():
    a, b = _build("mixtral-tiny", seed=1), _build("mixtral-tiny", seed=1, expert_weights="bf16")
    for L, M in zip(a.layers, b.layers):
        assert torch.equal(L.w13, M.w13) and torch.equal(L.w2, M.w2) and L.gu_block == M.gu_block == 0


# ------------------------------------------------------------------ loaders
def _mixtral_state(cfg, seed=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.05).to(torch.bfloat16)  # noqa: E731
    d, D, F_ = cfg.hidden, cfg.head_dim, cfg.ffn
    sd = {"model.embed_tokens.weight": r(cfg.vocab_size, d), "model.norm.weight": r(d),
          "lm_head.weight": r(cfg.vocab_size, d)}
    for i in range(cfg.layers):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = r(d), r(d)
        sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.o_proj.weight"] = r(cfg.heads * D, d), r(d, cfg.heads * D)
        sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.v_proj.weight"] = r(cfg.kv_heads * D, d), r(cfg.kv_heads * D, d)
        sd[p + "block_sparse_moe.gate.weight"] = r(cfg.num_experts, d)
        for e in range(cfg.num_experts):
            m = f"{p}block_sparse_moe.experts.{e}."
            sd[m + "w1.weight"], sd[m + "w3.weight"], sd[m + "w2.weight"] = r(F_, d), r(F_, d), r(d, F_)
    return sd


@pytest.mark.parametrize("family", ["qwen3-moe", "mixtral"])
def test_loaders_quantise_what_random_init_quantises(tmp_path, family):
    """Both safetensors loaders hand their expert tensors to the same ``_shard_layer``: the loaded model holds
    dequant(quant(.)) of the checkpoint's gate / up / down per expert, and everything else as stored."""
    from safetensors.torch import save_file

    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel
    from tests.test_qwen_moe import _hf_state

    small = dict(vocab_size=64, hidden=64, layers=1, heads=2, kv_heads=1, ffn=32)
    if family == "qwen3-moe":
        cfg = _cfg("qwen3-moe-tiny", num_experts=20, **small)
        sd, cls = _hf_state(cfg), Qwen3MoeModel
        names = lambda e: tuple(f"model.layers.0.mlp.experts.{e}.{n}_proj.weight" for n in ("gate", "up", "down"))  # noqa
    else:
        cfg = _cfg("mixtral-tiny", **small)
        sd, cls = _mixtral_state(cfg), MixtralModel
        names = lambda e: tuple(f"model.layers.0.block_sparse_moe.experts.{e}.{n}.weight" for n in ("w1", "w3", "w2"))  # noqa
    f = tmp_path / "model.safetensors"
    save_file(sd, str(f))
    m = cls(cfg, device="cpu", weights_path=str(f), expert_weights="mxfp4")
    plain = cls(cfg, device="cpu", weights_path=str(f))
    L, P = m.layers[0], plain.layers[0]
    one = lambda w: _dq(w.unsqueeze(0))[0]  # noqa: E731
    for e in range(cfg.num_experts):
        g, u, dn = (sd[n] for n in names(e))
        assert torch.equal(L.w13[e], torch.cat([one(g), one(u)])) and torch.equal(L.w2[e], one(dn))
    assert torch.equal(L.wqkv, P.wqkv) and torch.equal(L.wo, P.wo) and torch.equal(L.router, P.router)
    assert torch.equal(m.embed, plain.embed) and torch.equal(m.lm_head, plain.lm_head)
    assert not torch.equal(L.w13, P.w13)
