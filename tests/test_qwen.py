"""Qwen2.5 / Qwen3 decoders without a GPU: what the two attention-block steps are worth (fp32 reference), the
loader's reading of the bias and norm tensors, their tensor-parallel sharding, and the registered shapes."""
import hashlib
from dataclasses import replace

import pytest
import torch

from tests import qwen_ref

QWEN = ["qwen3-0.6b", "qwen3-4b", "qwen3-8b", "qwen3-32b", "qwen2.5-3b", "qwen2.5-72b", "qwen3-tiny", "qwen2-tiny"]


def _cpu_model(arch, seed=3, **kw):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    return LlamaModel(decoder_config(arch), device="cpu", seed=seed, max_position=256, **kw)


@pytest.mark.parametrize("arch,ablate", [("qwen3-tiny", {"use_qk_norm": False}), ("qwen2-tiny", {"use_bias": False})])
def test_dropping_the_step_ruins_the_logits(arch, ablate):
    """The model tests ask for a logit cosine > 0.995 against the reference: that bound only means something if
    a forward without the bias / the q-k norm lands far below it.  Worst row of a 48-token prompt < 0.9."""
    m = _cpu_model(arch)
    L = m.layers[0]
    assert (L.bqkv is not None) == m.cfg.qkv_bias and (L.q_norm is not None) == (L.k_norm is not None) == m.cfg.qk_norm
    toks = torch.randint(0, m.cfg.vocab_size, (48,), generator=torch.Generator().manual_seed(3))
    full = qwen_ref.qwen_forward(m, toks)
    worst = float(qwen_ref.row_cosines(full, qwen_ref.qwen_forward(m, toks, **ablate)).min())
    print(f"{arch}: worst-row logit cosine without the step {worst:.4f}")
    assert worst < 0.9


def _hf_state(m):
    """The model's tensors under their HF checkpoint names."""
    cfg = m.cfg
    Q, K = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    sd = {"model.embed_tokens.weight": m.embed, "model.norm.weight": m.final_norm}
    if not cfg.tie_embeddings:
        sd["lm_head.weight"] = m.lm_head
    for i, L in enumerate(m.layers):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = L.attn_norm, L.mlp_norm
        for name, lo, hi in (("q", 0, Q), ("k", Q, Q + K), ("v", Q + K, Q + 2 * K)):
            sd[p + f"self_attn.{name}_proj.weight"] = L.wqkv[lo:hi]
            if L.bqkv is not None:
                sd[p + f"self_attn.{name}_proj.bias"] = L.bqkv[lo:hi]
        if L.q_norm is not None:
            sd[p + "self_attn.q_norm.weight"], sd[p + "self_attn.k_norm.weight"] = L.q_norm, L.k_norm
        sd[p + "self_attn.o_proj.weight"] = L.wo
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = L.w_gate_up.chunk(2)
        sd[p + "mlp.down_proj.weight"] = L.w_down
    return {k: v.clone().contiguous() for k, v in sd.items()}


def _save(sd, path):
    from safetensors.torch import save_file

    save_file(sd, str(path))
    return str(path)


def test_loader_reads_bias_and_norm_weights(tmp_path):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    # a config with both flags: one checkpoint exercises both readers
    cfg = replace(decoder_config("qwen3-tiny"), qkv_bias=True)
    src = LlamaModel(cfg, device="cpu", seed=5, max_position=64)
    sd = _hf_state(src)
    m = LlamaModel(cfg, device="cpu", weights_path=_save(sd, tmp_path / "model.safetensors"), max_position=64)
    for i, (L, S) in enumerate(zip(m.layers, src.layers)):
        p = f"model.layers.{i}.self_attn."
        assert torch.equal(L.bqkv, torch.cat([sd[p + "q_proj.bias"], sd[p + "k_proj.bias"], sd[p + "v_proj.bias"]]))
        assert torch.equal(L.bqkv, S.bqkv) and L.bqkv.shape == (cfg.qkv_dim,)
        assert torch.equal(L.q_norm, S.q_norm) and torch.equal(L.k_norm, S.k_norm)
        assert torch.equal(L.wqkv, S.wqkv)
    assert m.lm_head is m.embed  # tied
    # a required tensor that is absent, and one of the wrong shape: refused by name
    missing = dict(sd)
    del missing["model.layers.1.self_attn.k_norm.weight"]
    with pytest.raises(ValueError, match=r"model\.layers\.1\.self_attn\.k_norm\.weight"):
        LlamaModel(cfg, device="cpu", weights_path=_save(missing, tmp_path / "missing.safetensors"), max_position=64)
    bad = dict(sd)
    bad["model.layers.0.self_attn.k_proj.bias"] = torch.zeros(cfg.heads * cfg.head_dim, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"model\.layers\.0\.self_attn\.k_proj\.bias"):
        LlamaModel(cfg, device="cpu", weights_path=_save(bad, tmp_path / "bad.safetensors"), max_position=64)
    # an unflagged config reads none of them
    plain = LlamaModel(replace(cfg, qkv_bias=False, qk_norm=False), device="cpu",
                       weights_path=str(tmp_path / "model.safetensors"), max_position=64)
    assert plain.layers[0].bqkv is None and plain.layers[0].q_norm is None and plain.layers[0].k_norm is None


def test_tp_shards_cut_the_bias_by_heads_and_replicate_the_norms():
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from llm_weighted_consensus_amd.models.tp import shard_dense_layer

    cfg = replace(decoder_config("qwen2-tiny"), qk_norm=True)
    m = LlamaModel(cfg, device="cpu", seed=1, max_position=64)
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    for L in m.layers:
        shards = [shard_dense_layer(L, cfg, r, 2) for r in range(2)]
        hq, hk = Hq // 2, Hkv // 2
        parts = [(s.bqkv[: hq * D], s.bqkv[hq * D:(hq + hk) * D], s.bqkv[(hq + hk) * D:]) for s in shards]
        assert all(s.bqkv.shape == ((hq + 2 * hk) * D,) for s in shards)
        full = torch.cat([torch.cat([p[j] for p in parts]) for j in range(3)])  # q heads, k heads, v heads
        assert torch.equal(full, L.bqkv)
        for r, s in enumerate(shards):  # head by head: the bias element rides with its weight row
            rows = torch.cat([torch.arange(r * hq * D, (r + 1) * hq * D),
                              Hq * D + torch.arange(r * hk * D, (r + 1) * hk * D),
                              (Hq + Hkv) * D + torch.arange(r * hk * D, (r + 1) * hk * D)])
            assert torch.equal(s.bqkv, L.bqkv[rows]) and torch.equal(s.wqkv, L.wqkv[rows])
            assert torch.equal(s.q_norm, L.q_norm) and torch.equal(s.k_norm, L.k_norm)


@pytest.mark.parametrize("arch", QWEN)
def test_registered_shapes_fit_the_decode_kernels(arch):
    from llm_weighted_consensus_amd.models.config import decoder_config

    cfg = decoder_config(arch)
    assert cfg.head_dim == 128 and cfg.heads % cfg.kv_heads == 0 and 16 % (cfg.heads // cfg.kv_heads) == 0
    assert cfg.qkv_bias != cfg.qk_norm and cfg.qk_norm == arch.startswith("qwen3")
    assert cfg.bos_token_id is None and cfg.rope_theta == 1e6 and cfg.rms_eps == 1e-6 and cfg.rope_scaling is None
    assert cfg.eos_token_id == (2 if arch.endswith("tiny") else 151645)


def test_flagged_moe_config_is_refused():
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel

    for flag in ("qkv_bias", "qk_norm"):
        with pytest.raises(NotImplementedError):
            MixtralModel(decoder_config("mixtral-tiny", **{flag: True}), device="cpu")


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.int16).numpy().tobytes()).hexdigest()


def test_unflagged_random_init_draws_what_it_always_drew():
    """llama-tiny, seed 0, CPU generator: checksums recorded before the Qwen fields existed (the benchmark pins
    sampled tokens to this sequence)."""
    m = _cpu_model("llama-tiny", seed=0)
    assert _sha(m.embed) == "795a6e8904931eb89bb26853019cbbdb4826a0e83d39599c1dd8047f6cb39e69"
    assert _sha(m.layers[1].w_down) == "32efe586e3063a7e99b1312e609d713ed733811c855640a2e95c130a656c16ae"
    assert m.layers[0].bqkv is None and m.layers[0].q_norm is None and m.layers[0].k_norm is None
