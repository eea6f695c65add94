"""LoRA adapters on the GPU: the batched shrink / expand-add kernels against fp32, the adapted Llama forward
against an fp32 forward of the merged weights, mixed-adapter batches through the engine (graphs on / off) and
the prefix cache's isolation between adapters."""
import copy

import pytest
import torch

from tests import torch_ref as ref

pytestmark = pytest.mark.gpu

N_ADAPTERS = 3


def _ids(pattern: str, M: int) -> torch.Tensor:
    if pattern == "one":
        return torch.full((M,), 1, dtype=torch.int32)
    if pattern == "none":
        return torch.full((M,), -1, dtype=torch.int32)
    if pattern == "runs":  # runs of 5 rows: 16-row tiles mix adapters and rows without one
        return torch.tensor([(0, -1, 2, 1)[(m // 5) % 4] for m in range(M)], dtype=torch.int32)
    g = torch.Generator().manual_seed(M)
    return torch.randint(-1, N_ADAPTERS, (M,), generator=g, dtype=torch.int32)


def _inputs(M, K, N, R, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * M + K + N + R)
    bf = torch.bfloat16
    X = torch.randn(M, K, generator=g).to(bf).to(dev)
    A = (torch.randn(N_ADAPTERS, R, K, generator=g) / K ** 0.5).to(bf).to(dev)
    B = torch.randn(N_ADAPTERS, N, R, generator=g).to(bf).to(dev)
    Y0 = torch.randn(M, N, generator=g).to(bf).to(dev)
    return X, A, B, Y0


def _reference(X, A, B, Y0, ids):
    """fp32 from the bf16 inputs: want [M, N] and the per-element magnitude the bound scales with."""
    safe = ids.clamp(min=0).long()
    T = torch.einsum("mk,mrk->mr", X.float(), A.float()[safe])  # [M, R]
    Bm = B.float()[safe]  # [M, N, R]
    prod = T.unsqueeze(1) * Bm
    has = (ids >= 0).view(-1, 1).float()
    want = Y0.float() + prod.sum(-1) * has
    mag = Y0.float().abs() + prod.abs().sum(-1) * has
    return want, mag


def _check(out, Y0, want, mag, ids):
    # one bf16 rounding of T (<= 2^-9 per term) + one of the output (<= 2^-9 |want|) <= 2^-8 mag; twice that
    # for the fp32 summation order
    err = (out.float() - want).abs()
    bound = 2.0 ** -7 * mag + 1e-6
    worst = (err / bound).max().item()
    print(f"max |err| / bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst
    none = ids < 0
    if bool(none.any()):  # rows without an adapter: bitwise untouched
        assert torch.equal(out[none].view(torch.int16), Y0[none].view(torch.int16))


# lora_shrink / lora_expand_add: exact probes (every rank 16..192, 64 adapters, every k and r walked, bitwise) in
# tests/test_lora_probes_gpu.py; tests/test_lora_probes.py shows what those comparisons reject.
@pytest.mark.parametrize("R", [16, 48, 64])
@pytest.mark.parametrize("K,N", [(512, 1536), (4096, 520)])
@pytest.mark.parametrize("M", [1, 17, 300])
def test_lora_kernels_match_fp32(gpu, M, K, N, R):
    from llm_weighted_consensus_amd import ops

    X, A, B, Y0 = _inputs(M, K, N, R, gpu)
    for pattern in ("one", "none", "runs", "random"):
        ids = _ids(pattern, M).to(gpu)
        want, mag = _reference(X, A, B, Y0, ids)
        outs = []
        for _ in range(2):  # twice into fresh copies: no state carried between launches
            Y = Y0.clone()
            T = ops.lora_shrink(X, A, ids)
            assert T.shape == (M, R) and T.dtype == torch.bfloat16
            assert ops.lora_expand_add_(Y, T, B, ids) is Y
            outs.append(Y)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), pattern
        _check(outs[0], Y0, want, mag, ids)
        if pattern != "none":
            assert not torch.equal(outs[0], Y0)  # the delta is large: an ignored adapter cannot pass


@pytest.mark.parametrize("M,K,N,R", [
    # expand-add past 31 row groups: 4 column tiles per wave, several trips of the column loop on the same T
    # fragments (33 column tiles, the last one half: N % 16 == 8), M % 64 != 0
    (2100, 128, 520, 16), (2100, 128, 520, 48),
    # shrink past 8192 rows: 4 waves on 4 / 2 / 1 row tiles per workgroup (R <= 48 / 96 / 192), M % 64 != 0
    (8200, 128, 64, 16), (8200, 128, 64, 64), (8200, 128, 64, 128),
    # and the last row count of the one-tile form
    (8192, 128, 64, 48)])
def test_lora_kernels_large_batch_configurations(gpu, M, K, N, R):
    """The launchers choose other kernel configurations by M (lora.hip launch_shrink / launch_expand): the same
    reference and bound as above on the shapes that take them, K and N small."""
    from llm_weighted_consensus_amd import ops

    X, A, B, Y0 = _inputs(M, K, N, R, gpu)
    for pattern in ("runs", "random", "one"):
        ids = _ids(pattern, M).to(gpu)
        want, mag = _reference(X, A, B, Y0, ids)
        outs = []
        for _ in range(2):
            Y = Y0.clone()
            ops.lora_expand_add_(Y, ops.lora_shrink(X, A, ids), B, ids)
            outs.append(Y)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), pattern
        _check(outs[0], Y0, want, mag, ids)
        assert not torch.equal(outs[0], Y0)


@pytest.mark.parametrize("M,R", [(17, 16), (300, 48)])
def test_lora_kernels_strided_views(gpu, M, R):
    """Y a column slice of a wider buffer (the columns around it stay bitwise unchanged), X a row view with
    ldx > K."""
    from llm_weighted_consensus_amd import ops

    K, N = 512, 520
    X, A, B, Y0 = _inputs(M, K, N, R, gpu, seed=7)
    ids = _ids("runs", M).to(gpu)
    want, mag = _reference(X, A, B, Y0, ids)
    g = torch.Generator(device="cpu").manual_seed(3)
    wide0 = torch.randn(M, N + 24, generator=g).to(torch.bfloat16).to(gpu)
    wide0[:, 8:8 + N] = Y0
    xwide = torch.randn(M, K + 64, generator=g).to(torch.bfloat16).to(gpu)
    xwide[:, :K] = X
    outs = []
    for _ in range(2):
        wide = wide0.clone()
        T = ops.lora_shrink(xwide[:, :K], A, ids)
        ops.lora_expand_add_(wide[:, 8:8 + N], T, B, ids)
        outs.append(wide)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    wide = outs[0]
    _check(wide[:, 8:8 + N], Y0, want, mag, ids)
    assert torch.equal(wide[:, :8].view(torch.int16), wide0[:, :8].view(torch.int16))
    assert torch.equal(wide[:, 8 + N:].view(torch.int16), wide0[:, 8 + N:].view(torch.int16))


def test_lora_kernels_refuse_shapes_outside_the_contract(gpu):
    from llm_weighted_consensus_amd import ops

    bf = torch.bfloat16
    ids = torch.zeros(4, dtype=torch.int32, device=gpu)
    x = torch.zeros(4, 512, dtype=bf, device=gpu)
    with pytest.raises(RuntimeError):  # K % 64
        ops.lora_shrink(x[:, :480].contiguous(), torch.zeros(1, 16, 480, dtype=bf, device=gpu), ids)
    with pytest.raises(RuntimeError):  # R % 16
        ops.lora_shrink(x, torch.zeros(1, 24, 512, dtype=bf, device=gpu), ids)
    with pytest.raises(RuntimeError):  # R > 192
        ops.lora_shrink(x, torch.zeros(1, 208, 512, dtype=bf, device=gpu), ids)
    with pytest.raises(RuntimeError):  # more than 64 adapters
        ops.lora_shrink(x, torch.zeros(65, 16, 512, dtype=bf, device=gpu), ids)
    t = torch.zeros(4, 16, dtype=bf, device=gpu)
    with pytest.raises(RuntimeError):  # N % 8
        ops.lora_expand_add_(torch.zeros(4, 516, dtype=bf, device=gpu), t, torch.zeros(1, 516, 16, dtype=bf, device=gpu),
                             ids)


# ------------------------------------------------------------------------------------------------ model


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm())).item()


ADAPTER_STD = 0.1  # base weights are N(0, 0.02): the adapters' (alpha / r) B A then outweighs them


@pytest.fixture(scope="module")
def adapted(gpu):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from llm_weighted_consensus_amd.models.lora import random_adapter

    cfg = decoder_config("llama-tiny")
    ads = [random_adapter("a", cfg, seed=11, rank=8, alpha=16, std=ADAPTER_STD),
           random_adapter("b", cfg, seed=12, rank=16, alpha=32, std=ADAPTER_STD)]
    return LlamaModel(cfg, device=gpu, seed=0, max_position=1024, lora=ads)  # (laid out once, by the model)


def _merged_model(model, adapter):
    """A copy of ``model`` for the fp32 reference forward with ``adapter`` baked into its weights."""
    from llm_weighted_consensus_amd.models.llama import LayerWeights
    from llm_weighted_consensus_amd.models.lora import merged_weights

    if adapter is None:
        return model
    m = copy.copy(model)
    m.layers = []
    for li, L in enumerate(model.layers):
        w = merged_weights(L, adapter, li)
        m.layers.append(LayerWeights(L.attn_norm, w["wqkv"], w["wo"], L.mlp_norm, w["w_gate_up"], w["w_down"],
                                     L.gu_block))
    return m


def test_adapted_prefill_and_decode_match_merged_reference(adapted, gpu):
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = adapted
    assert m.lora is not None and not m.norm_folded and m.lora.rank == 16
    cache = KVCache(m.cfg, 64, 16, gpu)
    g = torch.Generator(device="cpu").manual_seed(5)
    lens, steps = [33, 20, 27], 4
    toks = [torch.randint(0, m.cfg.vocab_size, (n + steps,), generator=g).to(gpu) for n in lens]
    row_adapter = [m.lora.adapters[0], m.lora.adapters[1], None]
    ids = torch.tensor([0, 1, -1], dtype=torch.int32, device=gpu)
    refs = [ref.llama_forward(_merged_model(m, ad), t) for ad, t in zip(row_adapter, toks)]  # [n + steps, V]
    base = [ref.llama_forward(m, t) for t in toks[:2]]
    # the references themselves tell the adapters apart: ignoring or swapping one cannot pass the bound below
    for r in range(2):
        assert _cos(refs[r][lens[r] - 1], base[r][lens[r] - 1]) < 0.9
    swapped = ref.llama_forward(_merged_model(m, row_adapter[1]), toks[0])
    assert _cos(refs[0][lens[0] - 1], swapped[lens[0] - 1]) < 0.9

    # sequence r lives in blocks 4 r .. 4 r + 3 (64 token slots each)
    def run(row_ids):
        cache.pool.zero_()
        i32 = dict(dtype=torch.int32, device=gpu)
        pos = torch.cat([torch.arange(n, **i32) for n in lens])
        slots = torch.cat([64 * r + torch.arange(n, **i32) for r, n in enumerate(lens)])
        cu = torch.tensor([0, lens[0], lens[0] + lens[1], sum(lens)], **i32)
        last = (cu[1:] - 1).long()
        out = [m.prefill(torch.cat([t[:n] for t, n in zip(toks, lens)]).int(), pos, slots, cu, max(lens), last,
                         cache, lora_ids=row_ids.repeat_interleave(torch.tensor(lens, device=gpu)))]
        bt = torch.arange(12, **i32).view(3, 4)
        for s in range(steps):
            p = torch.tensor([n + s for n in lens], **i32)
            tk = torch.stack([t[n + s] for t, n in zip(toks, lens)]).int()
            sl = torch.tensor([64 * r + n + s for r, n in enumerate(lens)], **i32)
            out.append(m.decode(tk, p, sl, bt, p + 1, cache, num_splits=2, lora_ids=row_ids))
        return out

    outs = run(ids)
    for s, lg in enumerate(outs):  # s = 0: the prompts' last tokens; then the decode steps
        for r in range(3):
            c = _cos(lg[r], refs[r][lens[r] - 1 + s])
            print(f"step {s} row {r}: cos {c:.5f}")
            assert c > 0.995, (s, r, c)
    # the row without an adapter is the base model's row, bit for bit
    none = run(torch.full((3,), -1, dtype=torch.int32, device=gpu))
    for a, b in zip(outs, none):
        assert torch.equal(a[2].view(torch.int16), b[2].view(torch.int16))


# ------------------------------------------------------------------------------------------------ engine


def _run_requests(eng, reqs, n):
    """reqs: [(prompt ids, SamplingParams)] submitted together -> tokens[request][choice]."""
    groups = [eng.add_request(p, sp, n) for p, sp in reqs]
    while eng.has_work():
        eng.step()
    return [[list(s.tokens) for s in g.seqs] for g in groups]


def test_engine_mixed_adapters_graph_equivalence(adapted, gpu):
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    tok = ByteTokenizer(adapted.cfg.vocab_size)
    prompt = tok.encode("select the response among the choices below: ")

    def sp(adapter):
        return SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True, adapter=adapter)

    reqs = [(prompt, sp("a")), (prompt, sp("b")), (prompt, sp(None))]
    outs = []
    for graphs in (True, False):
        eng = LLMEngine(adapted, tok, num_blocks=256, max_batch=16, max_model_len=512, use_graphs=graphs)
        outs.append(_run_requests(eng, reqs, n=2))
        assert eng.bm.num_free == 256
    assert outs[0] == outs[1]
    for group in outs[0]:
        assert len(group) == 2 and group[0] == group[1] and len(group[0]) == 12  # forked rows share the adapter
    # same prompt, three different voters
    assert outs[0][0][0] != outs[0][1][0] and outs[0][0][0] != outs[0][2][0] and outs[0][1][0] != outs[0][2][0]
    # the first token of each is among the fp32 merged reference's top 3 of 4096 (bf16 against fp32: the
    # exact argmax of a random model's flat logits can flip between near-ties)
    p = torch.tensor(prompt, device=gpu)
    for r, ad in enumerate([adapted.lora.adapters[0], adapted.lora.adapters[1], None]):
        top = ref.llama_forward(_merged_model(adapted, ad), p)[-1].topk(3).indices.tolist()
        assert outs[0][r][0][0] in top, (r, outs[0][r][0][0], top)
    eng = LLMEngine(adapted, tok, num_blocks=64, max_batch=4, max_model_len=256)
    with pytest.raises(ValueError):
        eng.add_request(prompt, sp("zzz"))


def test_engine_chunked_prefill_carries_adapters(adapted, gpu):
    """Mixed steps (decode rows + prompt chunks in one forward) build per-row ids for both kinds of rows: the
    same requests give the same greedy tokens as whole-prompt prefill, with the prefix cache on (salted)."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    tok = ByteTokenizer(adapted.cfg.vocab_size)
    head = "system: select the response among the choices below. "
    prompts = [tok.encode(head + t) for t in ("voter one", "voter two, longer tail", "three")]

    def sp(adapter):
        return SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True, logprobs=True, top_logprobs=3,
                              adapter=adapter)

    reqs = [(prompts[0], sp("a")), (prompts[1], sp("b")), (prompts[2], sp(None)), (prompts[1], sp("a"))]
    traces = []
    for chunk in (0, 32):
        eng = LLMEngine(adapted, tok, num_blocks=512, max_batch=32, max_model_len=768, chunked_prefill=chunk,
                        prefix_caching=True)
        eng.collect_events = True
        groups = [eng.add_request(p, q, 2) for p, q in reqs]
        trace = {}
        while eng.has_work():
            for ev in eng.step():
                trace.setdefault((ev.seq.group.id, ev.seq.index), []).append(
                    (ev.token_id, ev.logprob, dict(ev.top_logprobs)))
        traces.append([[trace[(g.id, s.index)] for s in g.seqs] for g in groups])
        if chunk:
            assert eng.stats["mixed_steps"] > 0
    # token for token, or up to a near tie of the random model's logits (mixed steps run other GEMM shapes):
    # at the first differing step each run's token is in the other's top 3 within 2e-2 of its log-probability
    tol = 2e-2
    for tg, tw in zip(*traces):
        for a, b in zip(tg, tw):
            assert len(a) == len(b) == 10
            for step, ((ta, la, topa), (tb, lb, topb)) in enumerate(zip(a, b)):
                assert abs(la - lb) < tol, (step, la, lb)
                if ta != tb:
                    assert tb in topa and abs(topa[tb] - la) < tol, (step, ta, tb, topa)
                    assert ta in topb and abs(topb[ta] - lb) < tol, (step, ta, tb, topb)
                    break
    first = [[c[0][0] for c in g] for g in traces[0]]
    assert first[1] != first[3] or traces[0][1][0][0][1] != traces[0][3][0][0][1]  # one prompt, two adapters


def test_prefix_cache_does_not_cross_adapters(adapted, gpu):
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    tok = ByteTokenizer(adapted.cfg.vocab_size)
    prompt = tok.encode("system: select the response among the choices below. ")[:40]
    assert len(prompt) == 40

    def sp(adapter):
        return SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True, adapter=adapter)

    def engine():
        return LLMEngine(adapted, tok, num_blocks=256, max_batch=16, max_model_len=512, prefix_caching=True)

    eng = engine()
    first_a = _run_requests(eng, [(prompt, sp("a"))], 1)
    assert eng.stats["prefix_cache_tokens"] == 0
    under_b = _run_requests(eng, [(prompt, sp("b"))], 1)
    assert eng.stats["prefix_cache_tokens"] == 0  # equal tokens under another adapter: no block reused
    assert under_b == _run_requests(engine(), [(prompt, sp("b"))], 1)
    again_a = _run_requests(eng, [(prompt, sp("a"))], 1)
    assert eng.stats["prefix_cache_tokens"] == 32  # the prompt's two full blocks, cached by the first request
    assert again_a == first_a and first_a != under_b
