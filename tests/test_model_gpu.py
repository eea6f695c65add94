"""Llama decoder + engine on the GPU: kernel-path forward vs an fp32 PyTorch forward, paged decode
consistency with prefill, prefix-sharing fork/COW, hipGraph replay equivalence."""
import math

import pytest
import torch

from tests import torch_ref as ref

pytestmark = pytest.mark.gpu


def _cos(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return (a @ b / (a.norm() * b.norm())).item()


@pytest.fixture(scope="module")
def tiny(gpu):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    return LlamaModel(decoder_config("llama-tiny"), device=gpu, seed=0, max_position=1024)


def test_prefill_and_decode_match_reference(tiny, gpu):
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = tiny
    cache = KVCache(m.cfg, 64, 16, gpu)
    g = torch.Generator(device="cpu").manual_seed(0)
    toks = torch.randint(0, m.cfg.vocab_size, (40,), generator=g).to(gpu)
    ref_logits = ref.llama_forward(m, toks)  # [40, V]
    # prefill the first 33 tokens into blocks 0..2, then decode 7 tokens one by one
    P = 33
    slots = torch.arange(P, dtype=torch.int32, device=gpu)
    cu = torch.tensor([0, P], dtype=torch.int32, device=gpu)
    lg = m.prefill(toks[:P].int(), torch.arange(P, dtype=torch.int32, device=gpu), slots, cu, P,
                   torch.tensor([P - 1], device=gpu), cache)
    assert _cos(lg[0], ref_logits[P - 1]) > 0.995
    bt = torch.arange(4, dtype=torch.int32, device=gpu).view(1, 4)
    for t in range(P, 40):
        dl = m.decode(toks[t:t + 1].int(), torch.tensor([t], dtype=torch.int32, device=gpu),
                      torch.tensor([t], dtype=torch.int32, device=gpu), bt,
                      torch.tensor([t + 1], dtype=torch.int32, device=gpu), cache, num_splits=2)
        assert _cos(dl[0], ref_logits[t]) > 0.995, t


@pytest.mark.parametrize("step_ab", ["0", "1"])
def test_engine_greedy_graph_equivalence_and_fork(tiny, gpu, step_ab, monkeypatch):
    """Graph replay == eager decode, greedy.  With the in-step A/B on (engine._step_ab), the graph engine runs
    first: its A/B installs the winning plan in the model, which the eager engine then runs too."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    monkeypatch.setenv("LWC_STEP_AB", step_ab)
    monkeypatch.setenv("LWC_STEP_AB_MIN", "1")  # the tiny model's buckets are small
    tok = ByteTokenizer(tiny.cfg.vocab_size)
    prompts = [tok.encode("hello world, this is a prompt of some length " * 2), tok.encode("short")]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    outs = []
    for graphs in ((True, False) if step_ab == "1" else (False, True)):
        eng = LLMEngine(tiny, tok, num_blocks=256, max_batch=16, max_model_len=512, use_graphs=graphs)
        outs.append(eng.generate(prompts, sp, n=3))
        assert eng.bm.num_free == 256  # everything released
    assert outs[0] == outs[1]
    for group in outs[0]:
        assert all(c == group[0] for c in group)  # greedy children of one prompt agree
        assert all(len(c) == 24 for c in group)
    # greedy engine output == greedy over the fp32 reference forward (first tokens; bf16 drift later)
    p = torch.tensor(prompts[0], device=gpu)
    first = int(ref.llama_forward(tiny, p)[-1].argmax())
    assert outs[0][0][0][0] == first


def test_engine_prefix_sharing_equivalence(tiny, gpu):
    """The cascade (prefix-shared) attention path gives the same greedy continuations."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    tok = ByteTokenizer(tiny.cfg.vocab_size)
    prompts = [tok.encode("x" * 70 + " a shared prompt longer than a few KV blocks"), tok.encode("y" * 33)]
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    outs = []
    for share in (False, True):
        eng = LLMEngine(tiny, tok, num_blocks=256, max_batch=16, max_model_len=512, prefix_sharing=share)
        outs.append(eng.generate(prompts, sp, n=5))
    same = sum(a == b for ga, gb in zip(*outs) for ca, cb in zip(ga, gb) for a, b in zip(ca, cb))
    total = sum(len(c) for g in outs[0] for c in g)
    assert same >= 0.95 * total, (same, total)


def test_engine_sampling_seeded(tiny, gpu):
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    tok = ByteTokenizer(tiny.cfg.vocab_size)
    eng = LLMEngine(tiny, tok, num_blocks=256, max_batch=32, max_model_len=512)
    sp = SamplingParams(temperature=1.0, top_p=0.9, max_tokens=16, ignore_eos=True, seed=1234, top_logprobs=5,
                        logprobs=True)
    a = eng.generate([tok.encode("abc")], sp, n=4)
    b = eng.generate([tok.encode("abc")], sp, n=4)
    assert a == b
    assert len({tuple(x) for x in a[0]}) > 1  # different children sample differently


def test_engine_export_import_prefill_equivalence(tiny, gpu):
    """Candidate-parallel path: a prompt prefilled by export_prefill and started via add_request(prefilled=)
    samples exactly what the engine's own prefill path samples (same seeds)."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer
    from llm_weighted_consensus_amd.parallel.prefill_share import all_gather_prefills

    tok = ByteTokenizer(tiny.cfg.vocab_size)
    prompts = [tok.encode("z" * 40 + " exported prompt"), tok.encode("q" * 16)]  # partial + exact block
    sp = SamplingParams(temperature=0.9, top_p=0.9, max_tokens=10, ignore_eos=True, seed=77)
    a = LLMEngine(tiny, tok, num_blocks=256, max_batch=16, max_model_len=512)
    want = a.generate(prompts, sp, n=3)
    b = LLMEngine(tiny, tok, num_blocks=256, max_batch=16, max_model_len=512)
    kv, lg, nbl = b.export_prefill(prompts)
    assert b.bm.num_free == 256 and kv.shape[2] == sum(nbl) and len(nbl) == 2
    shared = all_gather_prefills(kv, lg, nbl)  # single process: plain split
    groups = [b.add_request(p, sp, n=3, prefilled=shared[i]) for i, p in enumerate(prompts)]
    while b.has_work():
        b.step()
    got = [[list(s.tokens) for s in g.seqs] for g in groups]
    assert got == want
    assert b.bm.num_free == 256


def _mixed_rows_traces(tiny, use_graphs=True, async_first=True, chunked=0):
    """One engine, one batch whose rows differ in every sampler column (penalties, bias, top_logprobs, seeds,
    filters), then the bias and penalty requests again on the same engine (recycled count / bias rows).
    Returns per request [(top_logprobs asked, per child [(token, logprob, top list)])] of both rounds."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    tok = ByteTokenizer(tiny.cfg.vocab_size)
    eng = LLMEngine(tiny, tok, num_blocks=256, max_batch=16, max_model_len=512, use_graphs=use_graphs,
                    chunked_prefill=chunked)
    eng.async_first_tokens = async_first
    eng.collect_events = True
    sp = lambda **kw: SamplingParams(max_tokens=12, ignore_eos=True, **kw)  # noqa: E731
    r0 = (tok.encode("rows of one batch that differ"), sp(temperature=0.0), 1)
    r1 = (tok.encode("a biased row"), sp(temperature=0.0, logit_bias={65: 100}, top_logprobs=2, logprobs=True), 1)
    r2 = (tok.encode("two penalised children of one prompt"), sp(temperature=0.0, presence_penalty=100), 2)
    r3 = (tok.encode("three sampled children"), sp(temperature=0.8, top_k=20, top_p=0.9, min_p=0.01, seed=5,
                                                   top_logprobs=5, logprobs=True), 3)

    def run(reqs):
        groups = [eng.add_request(p, params, n) for p, params, n in reqs]
        traces = {}
        while eng.has_work():
            for ev in eng.step():
                traces.setdefault(ev.seq.id, []).append((ev.token_id, ev.logprob, list(ev.top_logprobs)))
        return [(g.params.top_logprobs, [traces[s.id] for s in g.seqs]) for g in groups]

    first = run([r0, r0, r1, r2, r3])
    again = run([r1, r2])
    assert eng.bm.num_free == 256 and len(eng.free_count_rows) == 16 and len(eng.free_bias_rows) == 16
    return first, again


def _check_mixed_rows(first, again, exact):
    """What every path must give, whatever its logits' last bits; ``exact``: the batch is the same in every step
    (whole-prompt prefill), so equal requests have equal logprobs too, not only equal tokens."""
    tokens = lambda req: [[t for t, _, _ in c] for c in req[1]]  # noqa: E731
    same = (lambda req: req) if exact else tokens  # what two equal requests of one batch must share
    r0, r0b, r1, r2, r3 = first
    for k, children in first + again:
        for trace in children:
            assert len(trace) == 12
            for _, lp, top in trace:
                assert len(top) == k  # each row reports its own request's count, not the batch's
                assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)
                assert not k or (math.isfinite(lp) and all(math.isfinite(v) for _, v in top))
    assert [t for t, _, _ in r1[1][0]] == [65] * 12  # the bias reaches its own row
    for child in r2[1]:
        assert len({t for t, _, _ in child}) == 12  # generated tokens are penalised before the greedy pick
    assert same(r0b) == same(r0)
    assert len({tuple(t for t, _, _ in c) for c in r3[1]}) > 1  # every child has its own seed
    # recycled count / bias rows start clean.  Tokens only: the second round's smaller batch runs in another
    # bucket, whose GEMM backends are timed and chosen on their own, so its logprobs may differ in the last bits
    assert [tokens(r) for r in again] == [tokens(r1), tokens(r2)]


def test_engine_batch_of_rows_that_differ_on_every_sampler_path(tiny, gpu):
    """Rows that differ in penalties, bias, logprob counts and seeds share one batch: every column reaches its
    own row on the decode path (graph and eager), on both first-token paths and in mixed chunked-prefill steps,
    and the three whole-prompt paths give identical (token, logprob, top list) traces."""
    base = _mixed_rows_traces(tiny)
    _check_mixed_rows(*base, exact=True)
    for graphs, async_first in ((True, False), (False, True)):
        assert _mixed_rows_traces(tiny, use_graphs=graphs, async_first=async_first) == base, (graphs, async_first)
    # mixed steps: other kernels compute the logits, and prompts complete (rows join the batch) at different steps
    _check_mixed_rows(*_mixed_rows_traces(tiny, chunked=16), exact=False)


@pytest.mark.parametrize("fused", ["ffn2", "all", "0"])
@pytest.mark.parametrize("arch", ["bge-small-en-v1.5", "bert-tiny"])
def test_bert_encoder_matches_reference(gpu, arch, fused):
    """HIP encoder (LN, varlen bidirectional attention incl. head_dim 32, bias+GELU, pooling) vs the
    fp32 PyTorch reference forward of the same weights; ``fused``: which of o / FFN2 add into the residual stream
    in their GEMM epilogue, the LayerNorm then taking their bias (default "ffn2"), else projection + LN(x + r)."""
    from llm_weighted_consensus_amd.models.bert import BertEncoder
    from llm_weighted_consensus_amd.models.config import encoder_config

    m = BertEncoder(encoder_config(arch), device=gpu, seed=5)
    m.fused_residual = fused
    lists = [[101] + list(range(1000, 1000 + n)) + [102] for n in (3, 40, 77, 130)]
    ids, pos, cu, max_len = m.pack(lists)
    h = m.forward_packed(ids, pos, cu, max_len)
    ref = m.forward_reference(ids, pos, cu)
    for i in range(len(lists)):
        s0, s1 = int(cu[i]), int(cu[i + 1])
        assert _cos(h[s0:s1], ref[s0:s1]) > 0.995, (arch, i)
    e, _ = m.embed_packed(ids, pos, cu, max_len)
    er = BertEncoder.pool_reference(ref, cu, m.cfg.pooling)
    assert (e - er).abs().max().item() < 2e-2


@pytest.mark.parametrize("fp8", [False, True])
def test_mixtral_moe_matches_reference_and_engine(gpu, fp8):
    """Mixtral MoE decoder (router top-2, grouped MFMA expert GEMMs, combine; fp8 experts) vs the fp32
    reference, then greedy generation through the engine (cascade + graphs) with prefill/decode agreeing."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel

    m = MixtralModel(decoder_config("mixtral-tiny"), device=gpu, seed=2, max_position=1024, fp8=fp8)
    g = torch.Generator(device="cpu").manual_seed(1)
    toks = torch.randint(0, m.cfg.vocab_size, (37,), generator=g).to(gpu)
    ref_logits = ref.llama_forward(m, toks)
    cache = KVCache(m.cfg, 16, 16, gpu)
    P = 37
    lg = m.prefill(toks.int(), torch.arange(P, dtype=torch.int32, device=gpu), torch.arange(P, dtype=torch.int32,
                   device=gpu), torch.tensor([0, P], dtype=torch.int32, device=gpu), P,
                   torch.tensor([P - 1], device=gpu), cache)
    # measured 0.99999 (bf16) / 0.9990 (fp8) over seeds 2-4 (scripts/mixtral_cos_probe.py); the bounds leave room
    # for a near-tie router flip.  (They were 0.99 / 0.985 while the router's softmax was wrong — README.)
    assert _cos(lg[0], ref_logits[P - 1]) > (0.998 if fp8 else 0.999)
    tok = ByteTokenizer(m.cfg.vocab_size)
    eng = LLMEngine(m, tok, num_blocks=1024, max_batch=160, max_model_len=512, cascade_min_batch=1)
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    outs = eng.generate([tok.encode("mixture of experts " * 3)], sp, n=130)
    assert all(o == outs[0][0] for o in outs[0])  # greedy children agree (cascade tiles > 1 per group)
    assert eng.bm.num_free == 1024


def test_decoder_embedder_last_token(tiny, gpu):
    """e5-mistral-style embedder: cache-less encode == the fp32 reference forward's final normed state of the
    last token (pooled, unit norm), independent of batch packing."""
    from llm_weighted_consensus_amd.models.embedder import DecoderEmbedder

    emb = DecoderEmbedder(tiny)
    lists = [[5, 6, 7, 8, 9] * 7, [11, 12, 13], list(range(100, 190))]
    e, _ = emb.embed(lists)
    assert torch.allclose(e.norm(dim=-1), torch.ones(3, device=gpu), atol=1e-3)
    for i, tl in enumerate(lists):
        t = torch.tensor(tl, device=gpu)
        cfg = tiny.cfg
        # reference: hidden state before lm_head = rmsnorm(x) at the last position
        x = ref.llama_hidden(tiny, t)[-1]
        r = torch.nn.functional.normalize(x, dim=0)
        assert _cos(e[i], r) > 0.995
        solo, _ = emb.embed([tl])
        assert _cos(solo[0], e[i]) > 0.999


def test_prefill_with_cached_prefix_matches_full_prefill(tiny, gpu):
    """Cross-request prefix cache at the model level: prefilling only a prompt's tail on top of its cached
    head blocks (key ranges gathered from the paged cache) gives the full prefill's last-token logits."""
    import numpy as np

    from llm_weighted_consensus_amd.models.llama import KVCache

    m = tiny
    cache = KVCache(m.cfg, 64, 16, gpu)
    g = torch.Generator(device="cpu").manual_seed(3)
    P, C = 53, 32  # 2 cached blocks, 21 new tokens
    toks = torch.randint(0, m.cfg.vocab_size, (P,), generator=g).to(gpu).int()
    ar = torch.arange(P, dtype=torch.int32, device=gpu)
    full = m.prefill(toks, ar, ar, torch.tensor([0, P], dtype=torch.int32, device=gpu), P,
                     torch.tensor([P - 1], device=gpu), cache)
    # second sequence: blocks 0,1 shared with the first, tail in blocks 8.. (slots 128..)
    slots_tail = torch.arange(128, 128 + P - C, dtype=torch.int32, device=gpu)
    k_slots = torch.cat([torch.arange(C, device=gpu), slots_tail.long()])
    ctx = {"k_slots": k_slots, "cu_k": torch.tensor([0, P], dtype=torch.int32, device=gpu),
           "q_lens": [P - C], "k_lens": [P]}
    part = m.prefill(toks[C:], ar[C:], slots_tail, torch.tensor([0, P - C], dtype=torch.int32, device=gpu), P - C,
                     torch.tensor([P - C - 1], device=gpu), cache, ctx=ctx)
    assert _cos(part[0], full[0]) > 0.999


def test_engine_prefix_cache_reuses_blocks_across_requests(tiny, gpu):
    """Two requests sharing a long prompt head: with the prefix cache the second prefills only its tail,
    yet greedy continuations equal the uncached engine's."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    tok = ByteTokenizer(tiny.cfg.vocab_size)
    head = "system: select the response among the choices below. " * 3
    p1, p2 = tok.encode(head + "voter one keys A B"), tok.encode(head + "voter two keys Q R T")
    sp = SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True)
    outs = []
    for cache_on in (False, True):
        eng = LLMEngine(tiny, tok, num_blocks=256, max_batch=16, max_model_len=512, prefix_caching=cache_on)
        a = eng.generate([p1], sp, n=2)
        b = eng.generate([p2], sp, n=2)
        outs.append((a, b))
        if cache_on:
            assert eng.stats["prefix_cache_tokens"] >= (len(tok.encode(head)) // 16 - 1) * 16
            assert eng.bm.num_free == 256  # cached blocks are evictable capacity
            assert eng.bm.num_cached_blocks > 0
        else:
            assert eng.stats["prefix_cache_tokens"] == 0
    assert outs[0] == outs[1]


def test_engine_prefix_cache_shares_heads_within_one_batch(tiny, gpu):
    """Voters of one score request arrive together: the shared head is computed once (wave 1) and the
    other prompts take it from the cache (wave 2), with unchanged greedy output."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer

    tok = ByteTokenizer(tiny.cfg.vocab_size)
    head = "user: which answer is right? " * 4
    prompts = [tok.encode(head + f"system: keys {k}") for k in ("A B", "C D E", "F G", "H")]
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    outs, stats = [], []
    for cache_on in (False, True):
        eng = LLMEngine(tiny, tok, num_blocks=256, max_batch=16, max_model_len=512, prefix_caching=cache_on)
        outs.append(eng.generate(prompts, sp, n=1))
        stats.append(dict(eng.stats))
    assert outs[0] == outs[1]
    saved = stats[0]["prefill_tokens"] - stats[1]["prefill_tokens"]
    assert saved == stats[1]["prefix_cache_tokens"] >= 3 * 96


def test_fp8_dense_decoder_embedder_and_prefill(gpu):
    """fp8 dense projections (config 5's e5-mistral embedder; e4m3 weights with per-channel scales, row-
    quantised activations into the fp8 library GEMM): embeddings and prefill logits track the fp32
    reference of the dequantised weights; the engine decodes with them (graphs on)."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.embedder import DecoderEmbedder
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    m = LlamaModel(decoder_config("llama-tiny"), device=gpu, seed=3, max_position=1024, fp8_dense=True)
    assert isinstance(m.layers[0].wqkv, ops.Fp8Weight) and not m._dense_residual
    lists = [list(range(40, 100)), [7, 8, 9, 10]]
    e, _ = DecoderEmbedder(m).embed(lists)
    for i, tl in enumerate(lists):
        r = torch.nn.functional.normalize(ref.llama_hidden(m, torch.tensor(tl, device=gpu))[-1], dim=0)
        assert _cos(e[i], r) > 0.99
    tok = ByteTokenizer(m.cfg.vocab_size)
    eng = LLMEngine(m, tok, num_blocks=256, max_batch=16, max_model_len=512)
    out = eng.generate([tok.encode("fp8 projections " * 4)], SamplingParams(temperature=0.0, max_tokens=6,
                                                                          ignore_eos=True), n=2)
    assert len(out[0]) == 2 and out[0][0] == out[0][1] and len(out[0][0]) == 6


@pytest.mark.parametrize("qkv_bn", [192, 256])
def test_folded_norm_chain_matches_unfolded(tiny, gpu, qkv_bn):
    """Folded RMSNorm decode chain (models/llama.py, gemm4w RS modes): the norm weights live in the projection
    weights (the model's norms are ones), the o / down residual epilogues emit the row scales the next
    projection applies — the decode logits equal the unfolded path's (norm kernels + projections) and the fp32
    reference forward.  qkv_bn 192: both producers gemm4w RS 2 (schedules 32 / 64); 256: the down
    producer by rms_rowsumsq after the planner's residual GEMM."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.llama import KVCache

    m = tiny
    assert m.norm_folded and bool((m.layers[0].attn_norm == 1).all())
    cache = KVCache(m.cfg, 64, 16, gpu)
    g = torch.Generator(device="cpu").manual_seed(3)
    toks = torch.randint(0, m.cfg.vocab_size, (36,), generator=g).to(gpu)
    ref_logits = ref.llama_forward(m, toks)
    P = 35
    slots = torch.arange(P, dtype=torch.int32, device=gpu)
    cu = torch.tensor([0, P], dtype=torch.int32, device=gpu)
    m.prefill(toks[:P].int(), torch.arange(P, dtype=torch.int32, device=gpu), slots, cu, P,
              torch.tensor([P - 1], device=gpu), cache)
    B = 300  # rows: one sequence repeated (ragged last m-tile of the chain's 256-row tiles)
    bt = torch.arange(4, dtype=torch.int32, device=gpu).view(1, 4).expand(B, 4).contiguous()
    args = (toks[P:P + 1].int().expand(B).contiguous(), torch.full((B,), P, dtype=torch.int32, device=gpu),
            torch.full((B,), P, dtype=torch.int32, device=gpu), bt, torch.full((B,), P + 1, dtype=torch.int32,
                                                                                 device=gpu), cache)
    if m.chain is None:
        m.chain = ops.NormChain(8192, m.cfg.hidden, m.cfg.rms_eps, gpu)
    saved = dict(m.chain_m)
    try:
        m.chain_m[B] = {"attn": False, "mlp": False, "final": False, "qkv_bn": qkv_bn, "o": "plain", "down": "plain"}
        assert not m.chain_ok(B)
        base = m.decode(*args, num_splits=1).float()
        m.chain_m[B] = {"attn": True, "mlp": True, "final": True, "qkv_bn": qkv_bn,
                        "o": "own64" if qkv_bn == 256 else "own32", "down": "sumsq" if qkv_bn == 256 else "own64"}
        assert m.chain_ok(B)
        got = m.decode(*args, num_splits=1).float()
    finally:
        m.chain_m.clear()
        m.chain_m.update(saved)
    assert _cos(got, base) > 0.9995
    assert (got - base).abs().max() < 0.05 * base.abs().max()
    assert _cos(got[B - 1], ref_logits[P]) > 0.995 and _cos(got[0], ref_logits[P]) > 0.995


def test_fold_moves_from_library_plan_bring_their_producer(tiny, gpu):
    """The engine's single-decision moves from the all-library plan (nothing folded, o / down "plain"): folding
    one norm point must also make its producer leave the partial row sums of squares, or the row-scaled GEMM
    reads whatever the chain's buffer held.  The buffer is poisoned (1e30: row scales near 0) before every
    decode; each folded step must equal the unfolded one, B = 300 as in the test above."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.llama import KVCache
    from llm_weighted_consensus_amd.ops import gemm_plan

    m = tiny
    cache = KVCache(m.cfg, 64, 16, gpu)
    g = torch.Generator(device="cpu").manual_seed(3)
    toks = torch.randint(0, m.cfg.vocab_size, (36,), generator=g).to(gpu)
    P = 35
    pos = torch.arange(P, dtype=torch.int32, device=gpu)
    m.prefill(toks[:P].int(), pos, pos.clone(), torch.tensor([0, P], dtype=torch.int32, device=gpu), P,
              torch.tensor([P - 1], device=gpu), cache)
    B = 300

    def full(v):
        return torch.full((B,), v, dtype=torch.int32, device=gpu)

    bt = torch.arange(4, dtype=torch.int32, device=gpu).view(1, 4).expand(B, 4).contiguous()
    args = (toks[P:P + 1].int().expand(B).contiguous(), full(P), full(P), bt, full(P + 1), cache)
    if m.chain is None:
        m.chain = ops.NormChain(8192, m.cfg.hidden, m.cfg.rms_eps, gpu)
    saved, choices = dict(m.chain_m), dict(gemm_plan._CHOICE)
    try:
        for k in m._plan_keys(B).values():  # the planner's state at B, as recorded without timing anything
            gemm_plan._CHOICE[k] = "blas"
        m.chain_m[B] = {"attn": False, "mlp": False, "final": False, "qkv_bn": 192, "o": "plain", "down": "plain"}
        lib = m.step_plans(B)["library"]
        moves = {lb: dl for lb, dl in m.step_moves(B, lib) if lb.endswith("_fold=True")}
        assert sorted(moves) == ["attn_fold=True", "final_fold=True", "mlp_fold=True"]
        outs = {}
        for lb, plan in [("library", lib)] + [(lb, m.with_move(lib, dl)) for lb, dl in moves.items()]:
            m.apply_step_plan(B, plan)
            assert m.chain_ok(B) == (lb != "library")
            m.chain.ss.fill_(1e30)
            outs[lb] = m.decode(*args, num_splits=1).float()
    finally:
        m.chain_m.clear()
        m.chain_m.update(saved)
        gemm_plan._CHOICE.clear()
        gemm_plan._CHOICE.update(choices)
    base = outs.pop("library")
    for lb, got in outs.items():
        assert _cos(got, base) > 0.9995, lb
        assert (got - base).abs().max() < 0.05 * base.abs().max(), lb


def test_pinned_step_plan_runs_untimed_and_repeats(gpu, monkeypatch):
    """LlamaModel.pin_step_plan: at the pinned batch neither tune_gemms nor the engine's in-step A/B times
    anything, the decode step runs exactly the pinned kernels (here the whole folded norm chain), and two fresh
    models + engines sample the same tokens from the same seeds."""
    from llm_weighted_consensus_amd.engine.engine import LLMEngine
    from llm_weighted_consensus_amd.engine.sampling import SamplingParams
    from llm_weighted_consensus_amd.engine.tokenizer import ByteTokenizer
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from llm_weighted_consensus_amd.ops import gemm_plan

    monkeypatch.setenv("LWC_STEP_AB_MIN", "1")  # without the pin, the A/B would race this small bucket
    B = 256  # 2 prompts x 100 candidates decode in the 256-row bucket (one 256-row tile, 56 rows of it empty)
    plan = {"choices": {n: "blas" for n in ("qkv", "o", "gu", "down", "lm")},
            "chain": {"attn": True, "mlp": True, "final": True, "qkv_bn": 192, "qkv_var": 32, "gu_var": 64,
                      "lm_var": 32, "lm_split": False, "o": "own32", "down": "sumsq"}}
    saved, timed = dict(gemm_plan._CHOICE), set(gemm_plan.TIMINGS)
    outs = []
    try:
        for _ in range(2):
            m = LlamaModel(decoder_config("llama-tiny"), device=gpu, seed=0, max_position=1024)
            m.pin_step_plan(B, plan)
            tok = ByteTokenizer(m.cfg.vocab_size)
            eng = LLMEngine(m, tok, num_blocks=2048, max_batch=B, max_model_len=256)
            sp = SamplingParams(temperature=0.8, top_p=0.95, max_tokens=12, ignore_eos=True, seed=7)
            outs.append(eng.generate([tok.encode("a prompt of some length " * 3), tok.encode("another one")], sp, n=100))
            assert eng.step_ab[B] == {"choice": "pinned"}
            assert not any(k[0] == B for k in set(gemm_plan.TIMINGS) - timed)  # nothing timed at the pinned batch
            assert m.chain_m[B] == plan["chain"] and m.chain_ok(B)
            assert m.plan_summary(B) == {"qkv": "g4 rs192 v32", "o": "g4 rs2 v32", "gu": "g4 rs v64",
                                         "down": "blas+sumsq", "lm": "g4 rs v32"}
    finally:
        gemm_plan._CHOICE.clear()  # (module-wide, keyed by shape: later tests tune their own)
        gemm_plan._CHOICE.update(saved)
    assert outs[0] == outs[1]
    assert len(outs[0]) == 2 and all(len(g) == 100 and all(len(c) == 12 for c in g) for g in outs[0])


def test_folded_norms_keep_encode_and_logits_with_real_norm_weights(gpu):
    """Norm folding with NON-unit norm weights (random init has unit ones, which hide a dropped weight): the
    folded model's prefill logits and its encode() hidden states (the decoder-as-embedder output, which has
    no lm_head to carry the final norm weight) equal the unfolded model's."""
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache, LlamaModel

    cfg = decoder_config("llama-tiny")
    gen = torch.Generator(device="cpu").manual_seed(11)

    def norm():
        return (0.5 + torch.rand(cfg.hidden, generator=gen)).to(gpu, torch.bfloat16)

    norms = [(norm(), norm()) for _ in range(cfg.layers)]
    final = norm()
    models = []
    for fold in (False, True):
        m = LlamaModel(cfg, device=gpu, seed=5, max_position=512, fold_norms=False)
        for L, (na, nm) in zip(m.layers, norms):
            L.attn_norm, L.mlp_norm = na.clone(), nm.clone()
        m.final_norm = final.clone()
        if fold:
            m._fold_norms()
            assert m.norm_folded and bool((m.final_norm == 1).all())
        models.append(m)
    a, b = models
    P = 29
    toks = torch.randint(0, cfg.vocab_size, (P,), generator=gen).to(gpu).int()
    pos = torch.arange(P, dtype=torch.int32, device=gpu)
    cu = torch.tensor([0, P], dtype=torch.int32, device=gpu)
    ea = a.encode(toks, pos, cu, P).float()
    eb = b.encode(toks, pos, cu, P).float()
    assert _cos(ea, eb) > 0.9995 and (ea - eb).abs().max() < 0.05 * ea.abs().max()
    last = torch.tensor([P - 1], device=gpu)
    la = a.prefill(toks, pos, pos, cu, P, last, KVCache(cfg, 16, 16, gpu)).float()
    lb = b.prefill(toks, pos, pos, cu, P, last, KVCache(cfg, 16, 16, gpu)).float()
    assert _cos(la, lb) > 0.9995
