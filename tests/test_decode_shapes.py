"""head_dim-64 and any-GQA-group decoders without a GPU: the registered shapes, what is refused at configuration
time, the cascade tile planner at super-tile sizes that are no power of two, the weight shapes of models whose
heads * head_dim differs from hidden, their tensor-parallel shards, and the GEMM planner's shape predicates at
the new (N, K) pairs."""
from dataclasses import replace

import numpy as np
import pytest
import torch

# arch -> nominal parameter count (billions): a guard against a mistyped shape
NOMINAL = {"llama-3.2-1b": 1.24, "llama-3.2-3b": 3.21, "qwen2.5-1.5b": 1.54, "qwen2.5-7b": 7.6, "qwen2.5-14b": 14.8,
           "qwen2.5-32b": 32.8, "qwen3-14b": 14.8}
TINIES = ["llama-hd64-tiny", "llama-g3-tiny", "qwen2-g7-tiny", "qwen3-g5-tiny"]
# (heads, kv_heads, head_dim) the issue sets for the tinies
TINY_SHAPES = {"llama-hd64-tiny": (8, 2, 64), "llama-g3-tiny": (6, 2, 128), "qwen2-g7-tiny": (14, 2, 128),
               "qwen3-g5-tiny": (10, 2, 128)}


@pytest.mark.parametrize("arch", list(NOMINAL) + TINIES)
def test_new_archs_resolve_to_shapes_the_decode_kernels_take(arch):
    from llm_weighted_consensus_amd.models.config import check_decoder, decoder_config

    cfg = decoder_config(arch)
    assert cfg.name == arch
    assert cfg.heads % cfg.kv_heads == 0 and cfg.heads // cfg.kv_heads <= 16
    assert cfg.head_dim in (64, 128)
    check_decoder(cfg)
    if arch in NOMINAL:
        got = cfg.params() / 1e9
        print(f"{arch}: {got:.3f} B parameters (nominal {NOMINAL[arch]})")
        assert abs(got / NOMINAL[arch] - 1) < 0.05
    else:
        assert (cfg.heads, cfg.kv_heads, cfg.head_dim) == TINY_SHAPES[arch]
        assert (cfg.hidden, cfg.layers, cfg.vocab_size, cfg.max_position) == (512, 2, 4096, 2048)


def test_groups_and_head_dims_of_the_new_archs():
    """The shapes the old rule (head_dim 128, group dividing 16) kept out are all present."""
    from llm_weighted_consensus_amd.models.config import decoder_config

    group = lambda a: decoder_config(a).heads // decoder_config(a).kv_heads  # noqa: E731
    assert decoder_config("llama-3.2-1b").head_dim == 64 and group("llama-3.2-1b") == 4
    assert [group(a) for a in ("llama-3.2-3b", "qwen2.5-1.5b", "qwen2.5-7b", "qwen2.5-14b", "qwen2.5-32b",
                               "qwen3-14b")] == [3, 6, 7, 5, 5, 5]
    for a in ("llama-3.2-1b", "llama-3.2-3b"):
        c = decoder_config(a)
        assert c.tie_embeddings and c.rope_scaling == (32.0, 1.0, 4.0, 8192) and c.max_position == 131072
        assert (c.bos_token_id, c.eos_token_id, c.rope_theta) == (128000, 128001, 500000.0)
    assert decoder_config("qwen2.5-7b").qkv_bias and decoder_config("qwen3-14b").qk_norm


@pytest.mark.parametrize("flags", [{"qkv_bias": True}, {"qk_norm": True}, {"qkv_bias": True, "qk_norm": True}])
def test_head_dim_64_with_bias_or_qk_norm_is_refused_by_name(flags):
    from llm_weighted_consensus_amd.models.config import check_decoder, decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    cfg = replace(decoder_config("llama-hd64-tiny"), name="qwen-hd64-probe", **flags)
    with pytest.raises(ValueError, match="qwen-hd64-probe.*head_dim 64"):
        check_decoder(cfg)
    with pytest.raises(ValueError, match="qwen-hd64-probe"):
        LlamaModel(cfg, device="cpu", max_position=64)


def test_unserved_head_dim_and_group_are_refused_by_name():
    from llm_weighted_consensus_amd.models.config import check_decoder, decoder_config

    with pytest.raises(ValueError, match="llama-tiny: head_dim 96"):
        check_decoder(decoder_config("llama-tiny", head_dim=96))
    with pytest.raises(ValueError, match="llama-tiny: 64 heads / 2 kv heads"):
        check_decoder(decoder_config("llama-tiny", heads=64))
    with pytest.raises(ValueError, match="llama-tiny: 7 heads / 2 kv heads"):
        check_decoder(decoder_config("llama-tiny", heads=7))


@pytest.mark.parametrize("per", [16, 24, 40])
def test_cascade_tiles_cover_every_row_once(per):
    """Super-tiles of 16, 24 and 40 sequences (GQA groups 6 / 7, 5 and 3) over runs that straddle them: shared
    runs longer and shorter than a tile, singletons and prompts without a full block (packed into plain tiles)."""
    from llm_weighted_consensus_amd.engine.engine import cascade_tiles

    counts = [(per + 9, 2), (1, 4), (2 * per, 5), (3, 0), (per - 1, 3), (1, 0), (per + 1, 19), (2, 1)]
    runs, row = [], 0
    for n, pblk in counts:
        runs.append((row, n, pblk))
        row += n
    B = row
    tiles = np.zeros((-(-B // per) + len(runs) + 2, 3), dtype=np.int32)
    nt = cascade_tiles(runs, per, tiles)
    seen = np.zeros(B, dtype=np.int64)
    pblk_of = np.concatenate([np.full(n, p if n >= 2 else 0) for n, p in counts])
    for r0, nseq, pblk in tiles[:nt].tolist():
        assert 0 < nseq <= per and r0 + nseq <= B
        seen[r0:r0 + nseq] += 1
        if pblk:  # a shared tile lies inside one run and carries that run's prefix
            assert (pblk_of[r0:r0 + nseq] == pblk).all()
            assert any(s <= r0 and r0 + nseq <= s + n for s, n, _ in runs)
    assert (seen == 1).all()
    assert (tiles[nt:] == 0).all()
    assert sum(1 for _, _, p in tiles[:nt].tolist() if p) >= 2 + 2 + 1 + 2  # the long runs were split


@pytest.mark.parametrize("arch", TINIES)
def test_cpu_model_weight_shapes_follow_heads_times_head_dim(arch):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache, LlamaModel, rope_tables

    cfg = decoder_config(arch)
    m = LlamaModel(cfg, device="cpu", seed=1, max_position=64)
    Q, KV = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    assert cfg.qkv_dim == Q + 2 * KV
    for L in m.layers:
        assert L.wqkv.shape == (Q + 2 * KV, cfg.hidden) and L.wo.shape == (cfg.hidden, Q)
        assert (L.bqkv is not None) == cfg.qkv_bias and (L.q_norm is not None) == cfg.qk_norm
        if cfg.qkv_bias:
            assert L.bqkv.shape == (Q + 2 * KV,)
        if cfg.qk_norm:
            assert L.q_norm.shape == (cfg.head_dim,) and L.k_norm.shape == (cfg.head_dim,)
    cos, sin = rope_tables(cfg, "cpu", 64)
    assert cos.shape == (64, cfg.head_dim // 2) and sin.shape == cos.shape and m.cos.shape == cos.shape
    cache = KVCache(cfg, 3, 16, "cpu")
    assert cache.k[0].shape == (3, cfg.kv_heads, 16, cfg.head_dim)
    assert cache.v[0].shape == (3, cfg.kv_heads, 4, cfg.head_dim, 4)


@pytest.mark.parametrize("arch", TINIES)
def test_reference_forward_runs_at_the_new_shapes(arch):
    """tests/torch_ref.llama_forward / tests/qwen_ref.qwen_forward (the GPU tests' oracle) at head_dim 64 and at
    heads * head_dim != hidden: finite logits of the right shape, and causal (a later token changes no earlier
    row)."""
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from tests import qwen_ref

    m = LlamaModel(decoder_config(arch), device="cpu", seed=2, max_position=64)
    toks = torch.randint(0, m.cfg.vocab_size, (9,), generator=torch.Generator().manual_seed(1))
    lg = qwen_ref.qwen_forward(m, toks)
    assert lg.shape == (9, m.cfg.vocab_size) and torch.isfinite(lg).all()
    toks2 = toks.clone()
    toks2[-1] = (toks2[-1] + 1) % m.cfg.vocab_size
    assert torch.equal(qwen_ref.qwen_forward(m, toks2)[:-1], lg[:-1])


def test_tp_shards_of_a_group_7_layer_reassemble():
    """As tests/test_qwen.py checks for qwen2-tiny: 14 / 2 heads over 2 ranks, 7 query heads and one KV head each."""
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from llm_weighted_consensus_amd.models.tp import shard_dense_layer

    cfg = decoder_config("qwen2-g7-tiny")
    m = LlamaModel(cfg, device="cpu", seed=1, max_position=64)
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    hq, hk = Hq // 2, Hkv // 2
    assert (hq, hk) == (7, 1)
    for L in m.layers:
        shards = [shard_dense_layer(L, cfg, r, 2) for r in range(2)]
        for r, s in enumerate(shards):
            rows = torch.cat([torch.arange(r * hq * D, (r + 1) * hq * D),
                              Hq * D + torch.arange(r * hk * D, (r + 1) * hk * D),
                              (Hq + Hkv) * D + torch.arange(r * hk * D, (r + 1) * hk * D)])
            assert s.wqkv.shape == ((hq + 2 * hk) * D, cfg.hidden) and s.bqkv.shape == ((hq + 2 * hk) * D,)
            assert torch.equal(s.wqkv, L.wqkv[rows]) and torch.equal(s.bqkv, L.bqkv[rows])
            assert s.wo.shape == (cfg.hidden, hq * D)
        assert torch.equal(torch.cat([s.wo for s in shards], dim=1), L.wo)
        parts = [(s.bqkv[: hq * D], s.bqkv[hq * D:(hq + hk) * D], s.bqkv[(hq + hk) * D:]) for s in shards]
        assert torch.equal(torch.cat([torch.cat([p[j] for p in parts]) for j in range(3)]), L.bqkv)


@pytest.mark.parametrize("arch", list(NOMINAL) + TINIES)
def test_gemm_planner_predicates_take_the_new_shapes(arch):
    """Shapes the hand-written GEMM cores do not take (hidden 1536 / 3584 miss the skinny core's K % 2048) must
    come back as False from the planner's predicates, so the call falls to the library backend; none may raise."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.ops import gemm_plan

    cfg = decoder_config(arch)
    shapes = {"qkv": (cfg.qkv_dim, cfg.hidden, "plain"), "o": (cfg.hidden, cfg.heads * cfg.head_dim, "residual"),
              "gu": (2 * cfg.ffn, cfg.hidden, "swiglu"), "down": (cfg.hidden, cfg.ffn, "residual"),
              "lm": (cfg.vocab_size, cfg.hidden, "plain")}
    for name, (N, K, epi) in shapes.items():
        for M in (1, 16, 64, 300):
            x = torch.empty(M, K, dtype=torch.bfloat16)
            assert isinstance(ops.skinny_ok(M, N, K, swiglu=epi == "swiglu"), bool)
            assert isinstance(gemm_plan._g8_ok(N, K, epi), bool)
            for b in ("gv", "g8", "g4", "g4n192", "blas"):
                assert gemm_plan._own_ok(b, x, N, K, epi) in (True, False), (name, b)
            assert gemm_plan._own_ok("blas", x, N, K, epi) is False
    if cfg.hidden in (1536, 3584):
        assert not ops.skinny_ok(16, cfg.qkv_dim, cfg.hidden)
