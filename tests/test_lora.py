"""LoRA adapters off the GPU: the stacked LoraSet layout against plain torch (PEFT directories, fused q|k|v and
interleaved gate|up, mixed ranks and partial targets), the prefix cache's salt, "<model>:<adapter>" routing
through LocalChatClient onto a fake engine, and the refused spec combinations."""
import asyncio
import json

import pytest
import torch

from llm_weighted_consensus_amd.models.config import decoder_config
from llm_weighted_consensus_amd.models.llama import LayerWeights
from llm_weighted_consensus_amd.models import lora as L

CFG = decoder_config("llama-tiny")


def _write_peft(path, rank, alpha, targets, seed):
    from safetensors.torch import save_file

    g = torch.Generator().manual_seed(seed)
    dims = L.target_dims(CFG)
    hf = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
          "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
    sd = {}
    for i in range(CFG.layers):
        for t in targets:
            n, k = dims[t]
            p = f"base_model.model.model.layers.{i}.{hf[t]}."
            sd[p + "lora_A.weight"] = torch.randn(rank, k, generator=g) * 0.05
            sd[p + "lora_B.weight"] = torch.randn(n, rank, generator=g) * 0.05
    path.mkdir()
    save_file(sd, str(path / "adapter_model.safetensors"))
    (path / "adapter_config.json").write_text(json.dumps(
        {"r": rank, "lora_alpha": alpha, "target_modules": [hf[t].split(".")[1] for t in targets], "peft_type": "LORA"}))
    return sd


def _base_layer(gu_block, seed=0):
    from llm_weighted_consensus_amd.ops import swiglu_interleave

    g = torch.Generator().manual_seed(seed)
    d, qkv, f, hq = CFG.hidden, CFG.qkv_dim, CFG.ffn, CFG.heads * CFG.head_dim
    wgu = torch.randn(2 * f, d, generator=g) * 0.02
    if gu_block:
        wgu = swiglu_interleave(wgu, gu_block)
    return LayerWeights(torch.ones(d), torch.randn(qkv, d, generator=g) * 0.02, torch.randn(d, hq, generator=g) * 0.02,
                        torch.ones(d), wgu, torch.randn(d, f, generator=g) * 0.02, gu_block)


@pytest.mark.parametrize("gu_block", [0, 32])
def test_loraset_layout_equals_merged_weights(tmp_path, gu_block):
    _write_peft(tmp_path / "a", 8, 16, ["q", "v", "gate", "down"], 1)
    sd_b = _write_peft(tmp_path / "b", 24, 12, ["k", "o", "gate", "up"], 2)
    spec = {"a": {"weights": str(tmp_path / "a")}, "b": {"weights": str(tmp_path / "b")}}
    ls = L.LoraSet.from_spec(CFG, spec, gu_block=gu_block, device="cpu")
    # (fp32 stacks for the identity below; the model keeps them in bf16)
    ls = L.LoraSet(CFG, ls.adapters, gu_block, "cpu", dtype=torch.float32)
    assert ls.names == ["a", "b"] and ls.index("b") == 1 and ls.rank == 32
    assert ls.slots == {"qkv": ("q", "k", "v"), "o": ("o",), "gate_up": ("gate", "up"), "down": ("down",)}
    assert ls.adapters[1].rank == 24 and ls.adapters[1].scale == 0.5
    assert torch.equal(ls.adapters[1].layers[1]["k"][0],
                       sd_b["base_model.model.model.layers.1.self_attn.k_proj.lora_A.weight"])
    with pytest.raises(ValueError):
        ls.index("zzz")
    base = _base_layer(gu_block)
    g = torch.Generator().manual_seed(9)
    for li in range(CFG.layers):
        for ai, ad in enumerate(ls.adapters):
            merged = L.merged_weights(base, ad, li)
            for proj, attr in (("qkv", "wqkv"), ("o", "wo"), ("gate_up", "w_gate_up"), ("down", "w_down")):
                w = getattr(base, attr)
                A, B = ls.A[li][proj][ai], ls.B[li][proj][ai]
                assert A.shape == (len(ls.slots[proj]) * 32, w.shape[1]) and B.shape == (w.shape[0], A.shape[0])
                x = torch.randn(5, w.shape[1], generator=g)
                got = x @ w.t() + (x @ A.t()) @ B.t()
                want = x @ merged[attr].t()
                assert torch.allclose(got, want, atol=1e-5, rtol=0), (li, ad.name, proj)
                carried = any(t in ad.layers[li] for t in L.PROJ_TARGETS[proj])
                assert carried == bool((merged[attr] != w).any())  # a delta exactly where the adapter has targets
    # the merged q|k|v delta sits in the target's own rows only (adapter a: q and v, not k)
    d = L.merged_weights(base, ls.adapters[0], 0)["wqkv"] - base.wqkv
    nq, nkv = CFG.heads * CFG.head_dim, CFG.kv_heads * CFG.head_dim
    assert bool(d[:nq].any()) and not bool(d[nq:nq + nkv].any()) and bool(d[nq + nkv:].any())


def test_loraset_refuses_bad_targets_and_ranks():
    with pytest.raises(ValueError):
        L.load_adapter("a", {"weights": "random:1", "targets": ["q", "lm_head"]}, CFG)
    with pytest.raises(ValueError):
        L.random_adapter("a", CFG, 0, targets=["embed"])
    with pytest.raises(ValueError):
        L.load_adapter("a:b", {"weights": "random:1"}, CFG)
    with pytest.raises(ValueError):  # 3 fused targets x rank 80 (padded) > the kernels' 192
        L.LoraSet(CFG, [L.random_adapter("a", CFG, 0, rank=72)])
    ok = L.LoraSet(CFG, [L.random_adapter("a", CFG, 0, rank=72, targets=["q", "o"])])  # one slot of 80
    assert ok.A[0]["qkv"].shape == (1, 80, CFG.hidden) and ok.A[0]["gate_up"] is None and not ok.adapts_gate_up
    with pytest.raises(ValueError):
        L.LoraSet(CFG, [L.random_adapter("a", CFG, 0), L.random_adapter("a", CFG, 1)])


def test_block_manager_salt_separates_equal_tokens():
    from llm_weighted_consensus_amd._runtime import BlockManager

    bm = BlockManager(64, 16)
    bm.set_prefix_caching(True)
    toks = list(range(100, 140))  # 40 tokens: two full blocks + a tail
    assert bm.add_sequence_cached(1, toks, 5) == 0
    bm.cache_prefix(1, toks, 5)
    assert bm.match_prefix(toks, 5) == 32          # same tokens, same salt
    assert bm.match_prefix(toks, salt=6) == 0      # another salt
    assert bm.match_prefix(toks) == 0 and bm.match_prefix(toks, 0) == 0
    assert bm.add_sequence_cached(2, toks, 6) == 0
    bm.cache_prefix(2, toks, 6)                    # both salts now hold their own copies
    assert bm.match_prefix(toks, 6) == 32 and bm.num_cached_blocks == 4
    assert set(bm.block_table(1)[:2]).isdisjoint(bm.block_table(2)[:2])
    assert bm.add_sequence_cached(3, toks, 5) == 32 and bm.block_table(3)[:2] == bm.block_table(1)[:2]
    # salt 0 is the unsalted chain: blocks cached by a call that passed no salt
    assert bm.add_sequence_cached(4, toks) == 0
    bm.cache_prefix(4, toks)
    assert bm.match_prefix(toks, 0) == 32 and bm.match_prefix(toks) == 32
    assert bm.add_sequence_cached(5, toks, salt=0) == 32 and bm.block_table(5)[:2] == bm.block_table(4)[:2]


def _req(model, models=None):
    from llm_weighted_consensus_amd.schema import chat as C

    return C.ChatCompletionCreateParams.model_validate(
        {"model": model, "models": models, "stream": True, "max_tokens": 3,
         "messages": [{"role": "user", "content": "hi"}]})


def test_adapter_names_route_to_the_base_models_service():
    from llm_weighted_consensus_amd.chat.local import LocalChatClient
    from llm_weighted_consensus_amd.engine.service import EngineService
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer
    from llm_weighted_consensus_amd.errors import ChatError
    from tests.fake_engine import FakeEngine

    eng = FakeEngine(0.0)
    eng.tokenizer, eng.cfg, eng.max_model_len = ByteTokenizer(CFG.vocab_size), CFG, 2048
    seen = []
    add = eng.add_request
    eng.add_request = lambda prompt, params, n=1, callback=None: (seen.append(params), add(prompt, params, n, callback))[1]
    svc = EngineService(eng, "m")
    svc.adapters = L.check_model_spec("m", {"arch": "llama-tiny", "adapters": {"a": {"weights": "random:7"}}})
    assert svc.adapters == ("a",)
    cl = LocalChatClient({"m": svc})
    assert cl.serves("m") and cl.serves("m:a") and not cl.serves("m:zzz") and not cl.serves("x:a")

    async def go(model, models=None):
        return [c async for c in await cl.create_streaming(None, _req(model, models))]

    try:
        chunks = asyncio.run(go("m:a"))
        assert chunks and all(c.model == "m:a" for c in chunks)
        assert chunks[-1].choices[0].finish_reason == "length"
        assert len(seen) == 1 and seen[0].adapter == "a"
        chunks = asyncio.run(go("m"))
        assert all(c.model == "m" for c in chunks) and seen[1].adapter is None
        with pytest.raises(ChatError) as ei:
            asyncio.run(go("m:zzz"))
        assert ei.value.code == 404 and ei.value.detail["kind"] == "model_not_found"
        chunks = asyncio.run(go("m:zzz", ["m:a"]))  # an unknown adapter falls over like an unknown model
        assert all(c.model == "m:a" for c in chunks) and seen[-1].adapter == "a" and len(seen) == 3
    finally:
        svc.close()


def test_specs_refuse_adapters_where_they_do_not_run():
    ads = {"a": {"weights": "random:7", "rank": 16}}
    assert L.check_model_spec("m", {"arch": "llama-tiny"}) == ()
    assert L.check_model_spec("m", {"arch": "llama-tiny", "adapters": ads}) == ("a",)
    for bad in ({"tp": 2}, {"fp8": True}, {"arch": "mixtral-tiny"}):
        with pytest.raises(ValueError):
            L.check_model_spec("m", dict({"arch": "llama-tiny", "adapters": ads}, **bad))
    with pytest.raises(ValueError):
        L.check_model_spec("e", {"arch": "llama-tiny", "adapters": ads}, embedder=True)
    with pytest.raises(ValueError):
        L.check_model_spec("m", {"arch": "llama-tiny", "adapters": {"a": {"targets": ["lm_head"]}}})
    with pytest.raises(ValueError):
        L.check_model_spec("m", {"arch": "llama-tiny", "adapters": {"a:b": {}}})
    # the worker factory and the server refuse them before touching a device
    from llm_weighted_consensus_amd.engine.group import build_engine
    from llm_weighted_consensus_amd.server.config import Config
    from llm_weighted_consensus_amd.server.main import build_state

    for bad in ({"tp": 2}, {"fp8": True}):
        spec = dict({"arch": "llama-tiny", "adapters": ads}, **bad)
        with pytest.raises(ValueError, match="LoRA"):
            build_engine(spec, 0)
        with pytest.raises(ValueError, match="LoRA"):
            build_state(Config(models={"m": spec}))


def test_loraset_refuses_dimensions_outside_the_kernel_contract():
    ok = L.random_adapter("a", CFG, 0, targets=["o"])  # o reads heads * head_dim = 1024 features: fits
    L.LoraSet(CFG, [ok])
    odd = decoder_config("llama-tiny", hidden=544)  # 544 % 64 == 32: q / k / v / gate / up read it
    with pytest.raises(ValueError, match="multiple of 64"):
        L.LoraSet(odd, [L.random_adapter("a", odd, 0, targets=["q"])])
    odd_out = decoder_config("llama-tiny", ffn=1028)  # gate|up writes 2056 columns: 2056 % 8 == 0, down reads 1028
    with pytest.raises(ValueError, match="multiple of 64"):
        L.LoraSet(odd_out, [L.random_adapter("a", odd_out, 0, targets=["down"])])
    L.LoraSet(odd_out, [L.random_adapter("a", odd_out, 0, targets=["gate"])])  # K = 512, N = 2056


def test_gate_up_rows_follow_the_models_own_interleave():
    """The set permutes B's gate|up rows with the function the model permutes its weight with: a 2F x r matrix
    whose entries name their row shows the permutation itself."""
    from llm_weighted_consensus_amd.ops import swiglu_interleave

    f, r = 64, 3
    b = torch.arange(2 * f, dtype=torch.float32).view(-1, 1).repeat(1, r)
    got = L._interleave_rows(b, 32)
    assert torch.equal(got, swiglu_interleave(b, 32))
    want_rows = list(range(0, 32)) + list(range(64, 96)) + list(range(32, 64)) + list(range(96, 128))
    assert got[:, 0].tolist() == [float(x) for x in want_rows]
    ad = L.random_adapter("a", CFG, 3, rank=16, targets=["gate", "up"])
    plain, inter = L.LoraSet(CFG, [ad], 0, dtype=torch.float32), L.LoraSet(CFG, [ad], 32, dtype=torch.float32)
    assert torch.equal(inter.B[0]["gate_up"][0], swiglu_interleave(plain.B[0]["gate_up"][0], 32))
    assert inter.laid_out_for(32, "cpu") and not inter.laid_out_for(0, "cpu") and not inter.laid_out_for(32, "cuda:0")


def test_engine_add_request_refuses_unknown_and_prefilled_adapters():
    """LLMEngine.add_request's adapter branches, on a stand-in engine state (no device): a name the LoraSet
    lacks, any adapter on a model without a LoraSet, and an adapter combined with an imported prefill."""
    import threading
    import types
    from collections import deque

    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    def state(lora):
        return types.SimpleNamespace(cfg=CFG, tokenizer=ByteTokenizer(CFG.vocab_size), max_model_len=256, lora=lora,
                                     lock=threading.Lock(), waiting=deque(), _deadlines=0)

    ls = L.LoraSet(CFG, [L.random_adapter("a", CFG, 0, targets=["q"]), L.random_adapter("b", CFG, 1, targets=["o"])])

    def sp(adapter):
        return SamplingParams(max_tokens=4, adapter=adapter)

    assert SamplingParams().adapter is None
    eng = state(ls)
    assert LLMEngine.add_request(eng, [1, 2, 3], sp("b")).adapter_id == 1
    assert LLMEngine.add_request(eng, [1, 2, 3], sp(None)).adapter_id == -1
    assert len(eng.waiting) == 2
    with pytest.raises(ValueError, match="unknown adapter 'zzz'"):
        LLMEngine.add_request(eng, [1, 2, 3], sp("zzz"))
    with pytest.raises(ValueError, match="prefilled"):
        LLMEngine.add_request(eng, [1, 2, 3], sp("a"), prefilled=(torch.zeros(1), torch.zeros(1)))
    with pytest.raises(ValueError, match="no adapters"):
        LLMEngine.add_request(state(None), [1, 2, 3], sp("a"))
    assert len(eng.waiting) == 2  # nothing refused was queued
    LLMEngine.add_request(state(None), [1, 2, 3], sp(None), prefilled=(torch.zeros(1), torch.zeros(1)))


def test_health_lists_adapter_model_names():
    import httpx

    from llm_weighted_consensus_amd.chat.fake import FakeChatClient
    from llm_weighted_consensus_amd.server.app import create_app
    from llm_weighted_consensus_amd.server.config import Config
    from llm_weighted_consensus_amd.server.main import build_state
    import types

    state = build_state(Config(), chat_client=FakeChatClient(lambda req: []))
    state.services = {"m": types.SimpleNamespace(adapters=("a", "b")), "plain": types.SimpleNamespace()}

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(state)), base_url="http://t") as c:
            return (await c.get("/health")).json()

    assert asyncio.run(go())["models"] == ["m", "m:a", "m:b", "plain"]
