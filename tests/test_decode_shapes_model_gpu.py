"""Decoders at head_dim 64 and at GQA groups that do not divide 16, on the GPU: the four tiny configs
(llama-hd64-tiny 8 / 2 heads at head_dim 64, llama-g3-tiny 6 / 2, qwen2-g7-tiny 14 / 2 with a q|k|v bias,
qwen3-g5-tiny 10 / 2 with the per-head QK RMSNorm) against the fp32 forward of tests/qwen_ref.py (which is
tests/torch_ref.llama_forward where a config has neither a bias nor the norms), and through the engine: captured
graphs against eager decode, the cascade attention path against plain decode, and what head_dim 64 does not take."""
import pytest
import torch

from tests import qwen_ref

pytestmark = pytest.mark.gpu

ARCHS = ["llama-hd64-tiny", "llama-g3-tiny", "qwen2-g7-tiny", "qwen3-g5-tiny"]
_models = {}


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm())).item()


def _i32(gpu, *v):
    return torch.tensor(list(v), dtype=torch.int32, device=gpu)


@pytest.fixture(params=ARCHS)
def model(request, gpu):
    """One model per arch for the whole module."""
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    if request.param not in _models:
        _models[request.param] = LlamaModel(decoder_config(request.param), device=gpu, seed=0, max_position=1024)
    return _models[request.param]


def test_prefill_and_decode_match_reference(model, gpu):
    """A 33-token prefill into blocks 0..2, then 7 decode steps with 2 splits (q rotated as the attention kernel
    loads it): every logits row against the fp32 forward."""
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = model
    L = m.layers[0]
    assert (L.bqkv is not None) == m.cfg.qkv_bias and (L.q_norm is not None) == m.cfg.qk_norm
    assert L.wo.shape[1] == m.cfg.heads * m.cfg.head_dim
    cache = KVCache(m.cfg, 64, 16, gpu)
    P, N = 33, 40
    toks = torch.randint(0, m.cfg.vocab_size, (N,), generator=torch.Generator().manual_seed(0)).to(gpu)
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


def test_cascade_decode_step_matches_reference(model, gpu):
    """One decode step of B rows forked from a 33-token prompt (two shared KV blocks, each row its own copy of
    the third) through the cascade kernel, every row with a different token: each logits row against the fp32
    forward of the prompt plus that token.  B = one super-tile and one row, so the second tile is the short one."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.engine.engine import cascade_tiles
    from llm_weighted_consensus_amd.models.llama import KVCache
    import numpy as np

    m = model
    P = 33
    B = ops.cascade_rows_per_tile(m.cfg.heads // m.cfg.kv_heads) + 1
    cache = KVCache(m.cfg, 4 + B, 16, gpu)
    g = torch.Generator().manual_seed(5)
    prompt = torch.randint(0, m.cfg.vocab_size, (P,), generator=g).to(gpu)
    nxt = torch.randint(0, m.cfg.vocab_size, (B,), generator=g).to(gpu)
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    m.prefill(prompt.int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    own = 3 + torch.arange(B, device=gpu)
    for li in range(m.cfg.layers):  # fork: every row gets its own copy of the prompt's partial block
        cache.k[li][own] = cache.k[li][2].clone()
        cache.v[li][own] = cache.v[li][2].clone()
    bt = torch.zeros(B, 4, dtype=torch.int32, device=gpu)
    bt[:, 1], bt[:, 2] = 1, own.int()
    tiles_np = np.zeros((4, 3), dtype=np.int32)
    per = B - 1
    assert cascade_tiles([(0, B, 2)], per, tiles_np) == 2 and tiles_np[1].tolist() == [per, 1, 2]
    full = lambda v: torch.full((B,), v, dtype=torch.int32, device=gpu)  # noqa: E731
    lg = m.decode(nxt.int(), full(P), (own * 16 + P % 16).int(), bt, full(P + 1), cache,
                  cascade_tiles=torch.from_numpy(tiles_np).to(gpu))
    worst = 1.0
    for b in sorted({0, 1, per - 1, per, B // 2}):
        want = qwen_ref.qwen_forward(m, torch.cat([prompt, nxt[b:b + 1]]))[-1]
        worst = min(worst, _cos(lg[b], want))
        assert _cos(lg[b], want) > 0.995, b
    print(f"{m.cfg.name} cascade decode step, B = {B}: worst cos {worst:.5f}")


def _spied_generate(eng, model, monkeypatch, prompts, sp, n):
    """eng.generate, counting the model.decode calls (eager steps, or graph captures) that got cascade tiles."""
    seen, decode = [], model.decode

    def spy(*a, **kw):
        seen.append(kw.get("cascade_tiles") is not None)
        return decode(*a, **kw)

    monkeypatch.setattr(model, "decode", spy)
    try:
        return eng.generate(prompts, sp, n=n), sum(seen)
    finally:
        monkeypatch.setattr(model, "decode", decode)


def test_engine_graphs_match_eager_and_prefix_sharing_matches_plain(model, gpu, monkeypatch):
    """Greedy, as tests/test_model_gpu.py runs llama-tiny: captured decode graphs == eager decode token for token;
    prefix_sharing on and off agree on >= 95 % of the tokens; every KV block is back in the pool afterwards."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    monkeypatch.setenv("LWC_STEP_AB", "0")
    tok = ByteTokenizer(model.cfg.vocab_size)
    prompts = [tok.encode("hello world, this is a prompt of some length " * 2), tok.encode("short")]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(model, tok, num_blocks=256, max_batch=16, max_model_len=512, use_graphs=graphs)
        outs.append(eng.generate(prompts, sp, n=3))
        assert eng.bm.num_free == 256
    assert outs[0] == outs[1]
    for group in outs[0]:
        assert all(c == group[0] for c in group) and all(len(c) == 24 for c in group)
    first = int(qwen_ref.qwen_forward(model, torch.tensor(prompts[0], device=gpu))[-1].argmax())
    assert outs[0][0][0][0] == first

    prompts = [tok.encode("x" * 70 + " a shared prompt longer than a few KV blocks"), tok.encode("y" * 33)]
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    outs = []
    for share in (False, True):
        eng = LLMEngine(model, tok, num_blocks=256, max_batch=16, max_model_len=512, prefix_sharing=share)
        outs.append(eng.generate(prompts, sp, n=5))
        assert eng.bm.num_free == 256
    same = sum(a == b for ga, gb in zip(*outs) for ca, cb in zip(ga, gb) for a, b in zip(ca, cb))
    total = sum(len(c) for g in outs[0] for c in g)
    print(f"{model.cfg.name}: prefix sharing on vs off {same}/{total} tokens")
    assert same >= 0.95 * total, (same, total)


def test_engine_cascade_path_graphs_match_eager(model, gpu, monkeypatch):
    """cascade_min_batch = 1: the 10-row batch (two runs of 5 forked sequences) decodes through the cascade
    kernel, with tiles planned for super-tiles of 32 / 40 / 16 / 24 sequences and padded with nseq = 0 entries
    in the graph buckets.  Captured graphs == eager token for token, and the pool is whole afterwards.

    Token agreement of this path with plain decode is not asserted: on these random-weight models the two
    attention kernels (different summation orders) flip greedy near-ties.  Measured for llama-g3-tiny: 109 of
    120 tokens, the two partings at fp32 logit margins of 0.0099 and 0.0075 where one bf16 step of the logits is
    0.0078, the cascade engine taking the fp32 argmax at the first.  The numbers of the cascade path are held by
    test_cascade_decode_step_matches_reference."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    monkeypatch.setenv("LWC_STEP_AB", "0")
    tok = ByteTokenizer(model.cfg.vocab_size)
    prompts = [tok.encode("x" * 70 + " a shared prompt longer than a few KV blocks"), tok.encode("y" * 33)]
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(model, tok, num_blocks=256, max_batch=16, max_model_len=512, use_graphs=graphs,
                        cascade_min_batch=1)
        out, cascade_calls = _spied_generate(eng, model, monkeypatch, prompts, sp, 5)
        assert cascade_calls > 0 and eng.bm.num_free == 256
        assert all(len(c) == 12 for g in out for c in g)
        outs.append(out)
    assert outs[0] == outs[1]


def test_fp8_dense_at_head_dim_64_keeps_attention_in_bf16(gpu):
    """fp8 projections at head_dim 64: the MX attention output needs head_dim 128, so the model selects bf16
    attention plus the row quantisation of the o projection's input by itself.  Prefill and decode steps through
    the split-K and the cascade kernel against the fp32 forward on the dequantised weights, at the bound
    tests/test_qwen_gpu.py holds fp8 prefill to (cosine > 0.99)."""
    import numpy as np

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.engine.engine import cascade_tiles
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache, LlamaModel

    m = LlamaModel(decoder_config("llama-hd64-tiny"), device=gpu, seed=3, max_position=1024, fp8_dense=True)
    assert isinstance(m.layers[0].wo, ops.Fp8Weight) and not m._attn_mx()
    cache = KVCache(m.cfg, 8, 16, gpu)
    P, N = 33, 37
    toks = torch.randint(0, m.cfg.vocab_size, (N,), generator=torch.Generator().manual_seed(6)).to(gpu)
    want = qwen_ref.qwen_forward(m, toks)
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    lg = m.prefill(toks[:P].int(), ar, ar, _i32(gpu, 0, P), P, torch.tensor([P - 1], device=gpu), cache)
    assert _cos(lg[0], want[P - 1]) > 0.99
    bt = torch.arange(4, dtype=torch.int32, device=gpu).view(1, 4)
    tiles_np = np.zeros((2, 3), dtype=np.int32)
    assert cascade_tiles([(0, 1, 0)], ops.cascade_rows_per_tile(4), tiles_np) == 1
    tiles = torch.from_numpy(tiles_np).to(gpu)
    for t in range(P, N):
        kw = {"num_splits": 2} if t % 2 else {"cascade_tiles": tiles}
        dl = m.decode(toks[t:t + 1].int(), _i32(gpu, t), _i32(gpu, t), bt, _i32(gpu, t + 1), cache, **kw)
        c = _cos(dl[0], want[t])
        print(f"fp8 llama-hd64-tiny decode {t} {list(kw)[0]}: cos {c:.5f}")
        assert c > 0.99, t


def test_head_dim_64_refuses_chunked_prefill_and_build_engine_turns_it_off(gpu):
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.group import build_engine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    arch = "llama-hd64-tiny"
    if arch not in _models:
        _models[arch] = LlamaModel(decoder_config(arch), device=gpu, seed=0, max_position=1024)
    m = _models[arch]
    tok = ByteTokenizer(m.cfg.vocab_size)
    with pytest.raises(ValueError, match="chunked prefill.*head_dim 128"):
        LLMEngine(m, tok, num_blocks=64, max_batch=8, max_model_len=256, chunked_prefill=256)
    eng = build_engine({"arch": arch, "weights": "random:0", "max_model_len": 256, "max_batch": 8,
                        "kv_fraction": 0.02, "chunked_prefill": 256, "device": gpu.index or 0}, 0)
    assert eng.chunked_prefill == 0 and eng.cfg.head_dim == 64
    free = eng.bm.num_free
    out = eng.generate([eng.tokenizer.encode("a prompt of more than one KV block, head_dim 64")],
                       SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True), n=2)
    assert [len(c) for c in out[0]] == [8, 8] and out[0][0] == out[0][1]
    assert eng.bm.num_free == free
