"""Qwen3-MoE decoders on the CPU: the registered shapes, the probe families at 128 experts, construction, the
safetensors loader and what is refused (models/qwen_moe.py, models/config.py)."""
import pytest
import torch

from tests import select_probes as sp
from tests.test_qwen import _sha

WIDE_PROBE_SHAPES = [(300, 128, 8), (77, 96, 8), (1, 128, 8), (1025, 128, 8)]


def _cfg(name, **kw):
    from llm_weighted_consensus_amd.models.config import decoder_config
    return decoder_config(name, **kw)


def test_registered_shapes():
    from llm_weighted_consensus_amd.chat.local import template_for
    from llm_weighted_consensus_amd.models.config import check_decoder

    big, tiny = _cfg("qwen3-30b-a3b"), _cfg("qwen3-moe-tiny")
    assert (big.vocab_size, big.hidden, big.layers, big.heads, big.kv_heads, big.head_dim, big.ffn, big.num_experts,
            big.experts_per_token) == (151936, 2048, 48, 32, 4, 128, 768, 128, 8)
    assert big.qk_norm and not big.qkv_bias and not big.tie_embeddings and big.rope_theta == 1e6
    assert big.rms_eps == 1e-6 and big.bos_token_id is None and big.eos_token_id == 151645
    assert big.max_position == 40960
    assert (tiny.vocab_size, tiny.hidden, tiny.layers, tiny.heads, tiny.kv_heads, tiny.head_dim, tiny.ffn,
            tiny.num_experts, tiny.experts_per_token) == (4096, 512, 2, 8, 2, 128, 384, 128, 8)
    assert tiny.qk_norm and not tiny.tie_embeddings and tiny.max_position == 2048 and tiny.eos_token_id == 2
    for c in (big, tiny):
        check_decoder(c)
        assert template_for(c.name) == "chatml"
    assert 30.0e9 < big.params() < 31.0e9


@pytest.mark.parametrize("T,E,k", WIDE_PROBE_SHAPES)
def test_probe_families_are_sound_at_128_experts(T, E, k):
    """The honest emulations pass route_violations at the wide shapes and the two route mutants are rejected, so
    the GPU comparisons of tests/test_moe_wide_gpu.py can tell a wrong tie or a short read."""
    gen = torch.Generator().manual_seed(T + 3 * E + k)
    lg = sp.route_logits(T, E, k, gen)
    ids, w, ro = sp.route_emul(lg, k)
    assert not sp.route_violations(ids, w, ro, lg, k, 2.0)
    assert sp.route_violations(*sp.route_emul(lg, k, tie_high=True), lg, k, 2.0)
    assert sp.route_violations(*sp.route_emul(lg, k, e_read=64), lg, k, 2.0)
    h, r = sp.router_sign(T, E, 64, gen, scaled=True)
    ids, w, ro, lg2 = sp.router_emul(h, r, k)
    assert not bool(sp.bitwise(lg2, sp.router_want(h, r)).any())
    assert not sp.route_violations(ids, w, ro, lg2, k, float(lg2.float().abs().max()))
    if T in (1, 1025):   # the GPU test's own logits: an expert with more rows than a 128-row tile / idle experts
        cnt = torch.bincount(sp.route_emul(sp.route_logits(T, E, k, torch.Generator().manual_seed(
            sum((i + 1) * v for i, v in enumerate((T, E, k))) + 43)), k)[0].flatten().long(), minlength=E)
        assert int(cnt.max()) >= 130 if T == 1025 else int(cnt.min()) == 0, (int(cnt.max()), int(cnt.min()))


def _checksums():
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel

    a = LlamaModel(_cfg("llama-tiny"), device="cpu", seed=0)
    b = MixtralModel(_cfg("mixtral-tiny"), device="cpu", seed=0)
    out = [_sha(a.embed), _sha(a.lm_head)] + [_sha(t) for L in a.layers for t in (L.wqkv, L.wo, L.w_gate_up, L.w_down)]
    out += [_sha(b.embed), _sha(b.lm_head)] + [_sha(t) for L in b.layers for t in (L.wqkv, L.wo, L.router, L.w13, L.w2)]
    return out


def test_construction_on_cpu_moves_no_other_arch():
    before = _checksums()
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    m = Qwen3MoeModel(_cfg("qwen3-moe-tiny"), device="cpu", seed=0)
    assert len(m.layers) == 2
    for L in m.layers:
        assert L.q_norm.shape == (128,) and L.k_norm.shape == (128,) and L.router.shape == (128, 512)
        assert L.w13.shape == (128, 768, 512) and L.w2.shape == (128, 512, 384)
        assert L.q_norm.dtype == torch.bfloat16 and 0.5 < float(L.q_norm.float().std() / 0.3) < 1.5
    assert not torch.equal(m.layers[0].q_norm, m.layers[0].k_norm)
    assert _checksums() == before
    # the norm weights are drawn after everything MixtralModel draws: the same shapes without the flag give the
    # same matrices
    class Plain(MixtralModel):
        pass

    p = Plain(_cfg("qwen3-moe-tiny", qk_norm=False), device="cpu", seed=0)
    assert _sha(p.embed) == _sha(m.embed) and _sha(p.lm_head) == _sha(m.lm_head)
    for a, b in zip(p.layers, m.layers):
        assert a.q_norm is None and all(_sha(getattr(a, n)) == _sha(getattr(b, n)) for n in ("wqkv", "wo", "router",
                                                                                             "w13", "w2"))
    with pytest.raises(NotImplementedError):                   # MixtralModel itself keeps refusing the flag
        MixtralModel(_cfg("qwen3-moe-tiny"), device="cpu")


def _hf_state(cfg, seed=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.05).to(torch.bfloat16)  # noqa: E731
    d, D, F_ = cfg.hidden, cfg.head_dim, cfg.ffn
    sd = {"model.embed_tokens.weight": r(cfg.vocab_size, d), "model.norm.weight": r(d),
          "lm_head.weight": r(cfg.vocab_size, d)}
    for i in range(cfg.layers):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = r(d), r(d)
        sd[p + "self_attn.q_proj.weight"] = r(cfg.heads * D, d)
        sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.v_proj.weight"] = r(cfg.kv_heads * D, d), r(cfg.kv_heads * D, d)
        sd[p + "self_attn.o_proj.weight"] = r(d, cfg.heads * D)
        sd[p + "self_attn.q_norm.weight"], sd[p + "self_attn.k_norm.weight"] = r(D), r(D)
        sd[p + "mlp.gate.weight"] = r(cfg.num_experts, d)
        for e in range(cfg.num_experts):
            m = f"{p}mlp.experts.{e}."
            sd[m + "gate_proj.weight"], sd[m + "up_proj.weight"], sd[m + "down_proj.weight"] = r(F_, d), r(F_, d), r(d, F_)
    return sd


def test_loader_reads_hf_names_and_refuses_by_tensor_name(tmp_path):
    from safetensors.torch import save_file

    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    # the loader's names and shapes at a small size: 20 experts of width 32, one layer
    cfg = _cfg("qwen3-moe-tiny", vocab_size=64, hidden=64, layers=1, heads=2, kv_heads=1, ffn=32, num_experts=20)
    sd = _hf_state(cfg)
    f = tmp_path / "model.safetensors"
    save_file(sd, str(f))
    m = Qwen3MoeModel(cfg, device="cpu", weights_path=str(f))
    L, p = m.layers[0], "model.layers.0."
    eq = lambda a, b: torch.equal(a.view(torch.int16), b.contiguous().view(torch.int16))  # noqa: E731
    assert eq(m.embed, sd["model.embed_tokens.weight"]) and eq(m.lm_head, sd["lm_head.weight"])
    assert eq(m.final_norm, sd["model.norm.weight"])
    assert eq(L.wqkv, torch.cat([sd[p + f"self_attn.{x}_proj.weight"] for x in "qkv"]))
    assert eq(L.wo, sd[p + "self_attn.o_proj.weight"]) and eq(L.router, sd[p + "mlp.gate.weight"])
    assert eq(L.q_norm, sd[p + "self_attn.q_norm.weight"]) and eq(L.k_norm, sd[p + "self_attn.k_norm.weight"])
    assert eq(L.attn_norm, sd[p + "input_layernorm.weight"]) and eq(L.mlp_norm, sd[p + "post_attention_layernorm.weight"])
    for e in range(cfg.num_experts):
        x = f"{p}mlp.experts.{e}."
        assert eq(L.w13[e], torch.cat([sd[x + "gate_proj.weight"], sd[x + "up_proj.weight"]]))
        assert eq(L.w2[e], sd[x + "down_proj.weight"])
    # without lm_head.weight the embedding table is the head
    tied = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    save_file(tied, str(tmp_path / "tied.safetensors"))
    mt = Qwen3MoeModel(cfg, device="cpu", weights_path=str(tmp_path / "tied.safetensors"))
    assert mt.lm_head is mt.embed

    missing = p + "mlp.experts.5.up_proj.weight"
    save_file({k: v for k, v in sd.items() if k != missing}, str(tmp_path / "missing.safetensors"))
    with pytest.raises(ValueError, match="mlp.experts.5.up_proj.weight"):
        Qwen3MoeModel(cfg, device="cpu", weights_path=str(tmp_path / "missing.safetensors"))
    bad = dict(sd)
    bad[p + "self_attn.q_norm.weight"] = torch.ones(64, dtype=torch.bfloat16)
    save_file(bad, str(tmp_path / "bad.safetensors"))
    with pytest.raises(ValueError, match="self_attn.q_norm.weight"):
        Qwen3MoeModel(cfg, device="cpu", weights_path=str(tmp_path / "bad.safetensors"))


def test_refusals():
    from llm_weighted_consensus_amd.models.lora import check_model_spec
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    cfg = _cfg("qwen3-moe-tiny")
    for kw in ({"tp_size": 2}, {"ep_size": 2}):
        with pytest.raises(ValueError, match="qwen3-moe-tiny"):
            Qwen3MoeModel(cfg, device="cpu", **kw)
    with pytest.raises(ValueError):
        Qwen3MoeModel(_cfg("mixtral-tiny"), device="cpu")
    base = {"arch": "qwen3-moe-tiny", "weights": "random:0"}
    assert check_model_spec("v", base) == ()
    for extra in ({"tp": 2}, {"adapters": {"a": {"weights": "random:1"}}}, {"mxfp4": True}):
        with pytest.raises(ValueError, match="qwen3-moe-tiny"):
            check_model_spec("v", {**base, **extra})
    with pytest.raises(ValueError, match="qwen3-moe-tiny"):      # the arch in LWC_EMBED_MODELS
        check_model_spec("v", base, embedder=True)
    with pytest.raises(ValueError, match="qwen3-30b-a3b"):
        check_model_spec("v", {"arch": "qwen3-30b-a3b"}, embedder=True)
