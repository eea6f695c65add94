"""The fused sampler under structured inputs (tests/sampler_probes.py) against float64 references.

The random rows and 4096-draw histograms of tests/test_kernels_gpu.py cannot see a kept set wrong by one token,
an index rebuilt wrongly at a row edge, or the paths only an unusual row takes.  Here the vocabularies are
32000 (SLOTS=4), 65504 (SLOTS=8), 128256 (SLOTS=16) and the two Qwen sizes 151936 and 152064 (SLOTS=20: two
dwords per lane in the owner walk, a ragged slot and a whole padding slot), and six groups of checks:

1. one-hot rows on every edge position: the token, exactly, sampled, greedy and filtered;
2. rows whose kept set is known exactly: the set of drawn tokens equals it over 1024 seeds, frequencies over
   65536 seeds are within five binomial standard deviations + the fp16 mass rounding (top_p = 0.5 sends a third
   of the rows through the reject path and its second uniform);
3. two equal tokens that share a dword, a thread, a wave edge or the row's ends: one half each;
4. top-logprobs: ids exactly and logprobs at 2e-3 / 1e-3 on random rows, on a row that overflows the 64
   collection slots with distinct values, on ties inside the top K, on a row where 200 tokens tie at the K-th
   value and are visited before the values above them, and on grammar-constrained rows;
5. bias, grammar mask and penalties together on full-size random rows;
6. contract checks: batch independence, all 64 bits of seed and offset, a strided logits view, host refusals.

tests/test_sampler_probes.py shows on the CPU that the preconditions of every exact comparison hold and that
the comparison functions reject the wrong references.  Inputs are built on the device; rows that differ only in
their seed share one row through expand (row stride 0)."""
import math

import pytest
import torch

from tests import sampler_probes as sp
from tests.test_kernels_gpu import _penalised_ref

pytestmark = pytest.mark.gpu

R_SUPPORT, R_FREQ, R_PAIR = 1024, 65536, 16384
TOPK_VOCABS = (32000, 128256, 151936)
PAIR_VOCABS = (65504, 128256, 151936)
PROC_VOCABS = (65504, 128256, 152064)
MAX_LOGITS_BYTES = 256 << 20


def _sample(logits, **kw):
    """ops.sample with per-row parameters given as scalars (one value for every row) or tensors."""
    from llm_weighted_consensus_amd import ops

    B, dev = logits.shape[0], logits.device

    def per_row(name, default, dtype):
        v = kw.pop(name, default)
        return v if torch.is_tensor(v) else torch.full((B,), v, dtype=dtype, device=dev)

    args = dict(temperature=per_row("temperature", 1.0, torch.float32), top_p=per_row("top_p", 1.0, torch.float32),
                top_k=per_row("top_k", 0, torch.int32), min_p=per_row("min_p", 0.0, torch.float32),
                top_a=per_row("top_a", 0.0, torch.float32))
    args["seeds"] = kw.pop("seeds", None)
    if args["seeds"] is None:
        args["seeds"] = torch.arange(B, device=dev, dtype=torch.int64) * 7919 + 1
    args["offsets"] = kw.pop("offsets", None)
    if args["offsets"] is None:
        args["offsets"] = torch.zeros(B, device=dev, dtype=torch.int64)
    args.update(kw)
    return ops.sample(logits, **args)


def _rand_rows(B, V, gpu, seed, scale):
    g = torch.Generator(device=gpu).manual_seed(seed)
    return (torch.randn(B, V, device=gpu, generator=g) * scale).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------
# 1. one-hot sweep


@pytest.mark.parametrize("background", [-math.inf, -40.0], ids=["rest_-inf", "rest_-40"])
@pytest.mark.parametrize("V", sp.VOCABS)
def test_one_hot_sweep(gpu, V, background):
    """One row per edge position, that token at 0.0, the rest at -inf or at -40 (u underflows to 0): the token
    comes back exactly from a sampled, a greedy and a filtered call, as the drawn token and as top-1."""
    hot_all = sp.edge_positions(V)
    step = MAX_LOGITS_BYTES // (2 * V)
    for r0 in range(0, len(hot_all), step):
        hot = hot_all[r0:r0 + step]
        rows = sp.one_hot_rows(V, hot, background, gpu)
        seeds = torch.arange(len(hot), device=gpu, dtype=torch.int64) * 104729 + 12345
        for kw in ({"seeds": seeds}, {"temperature": 0.0}, {"top_p": 0.5, "top_k": 5}):
            tok, lp, ids, lps = _sample(rows, num_logprobs=1, **kw)
            sp.check_one_hot(tok, hot)
            sp.check_one_hot(ids[:, 0], hot)
            assert lp.abs().max().item() <= 1e-3 and lps.abs().max().item() <= 1e-3, kw
        if background == -math.inf:
            tok, lp, ids, lps = _sample(rows, num_logprobs=20, seeds=seeds)
            sp.check_one_hot(tok, hot)
            sp.check_one_hot(ids[:, 0], hot)
            assert lps[:, 0].abs().max().item() <= 1e-3
            assert bool((ids[:, 1:] == -1).all()) and bool((lps[:, 1:] == -math.inf).all())


# ---------------------------------------------------------------------------------------------------------
# 2. exact support and frequencies

_refs = {}


def _support_case(V, name, gpu):
    if (V, name) not in _refs:
        kind, kw, _ = sp.SUPPORT_CASES[name]
        row = sp.support_row(V, kind, gpu)
        _refs[V, name] = (row, sp.kept_reference(row, **kw), kw)
    return _refs[V, name]


@pytest.mark.parametrize("name", list(sp.SUPPORT_CASES))
@pytest.mark.parametrize("V", sp.VOCABS)
def test_exact_support(gpu, V, name):
    """The tokens drawn over 1024 seeds are the kept set of the float64 reference, exactly."""
    row, ref, kw = _support_case(V, name, gpu)
    assert ref.ids.numel() == sp.SUPPORT_CASES[name][2]
    sp.assert_preconditions(ref, R_SUPPORT)
    tok, *_ = _sample(row.expand(R_SUPPORT, V), **kw)
    sp.check_support(tok, ref)


@pytest.mark.parametrize("name", sp.FREQUENCY_CASES)
@pytest.mark.parametrize("V", sp.VOCABS)
def test_frequencies(gpu, V, name):
    """65536 seeds: per kept token |count / R - q| <= 5 sqrt(q (1 - q) / R) + 2e-3."""
    row, ref, kw = _support_case(V, name, gpu)
    sp.assert_preconditions(ref, R_FREQ)
    tok, *_ = _sample(row.expand(R_FREQ, V), **kw)
    sp.check_frequencies(tok, ref)


@pytest.mark.parametrize("V", sp.VOCABS)
def test_reject_path_returns_argmax(gpu, V):
    """top_p = 0.3 keeps the argmax alone; 59 % of the first draws are rejected and drawn again."""
    row, ref, kw = _support_case(V, "top_p_0.3", gpu)
    sp.assert_preconditions(ref, R_PAIR)
    assert ref.ids.tolist() == [sp.live_positions(V)[sp.LIVE_ORDER[0]]]
    first_draw_kept = float(sp.kept_reference(row).q.max())
    assert 0.40 < first_draw_kept < 0.42
    tok, *_ = _sample(row.expand(R_PAIR, V), **kw)
    assert bool((tok == int(ref.ids[0])).all()), torch.unique(tok).tolist()


# ---------------------------------------------------------------------------------------------------------
# 3. two-hot pairs


@pytest.mark.parametrize("pair", list(sp.edge_pairs(sp.VOCABS[0])))
@pytest.mark.parametrize("V", PAIR_VOCABS)
def test_two_hot_pair(gpu, V, pair):
    p = sp.edge_pairs(V)[pair]
    tok, *_ = _sample(sp.two_hot_row(V, p, gpu).expand(R_PAIR, V))
    sp.check_two_hot(tok, p)


# ---------------------------------------------------------------------------------------------------------
# 4. top-logprobs paths


@pytest.mark.parametrize("V", TOPK_VOCABS)
def test_topk_random_rows(gpu, V):
    """Random rows (scale 3), K in {1, 5, 20}: ids and logprobs match the float64 log-softmax ordered value
    descending, index ascending.  In bf16 the best 21 values of such a row almost always hold equal ones (about
    21 values on a grid of 1/16 between 11 and 14), so a tie-free row cannot be had by redrawing; the rows are
    kept as drawn and the tied ids must come out in the reference's index order, which is the kernel's
    documented order as long as the candidates fit the collection buffer (asserted from the reference)."""
    B = 6
    rows = _rand_rows(B, V, gpu, 20 + V % 7, 3.0)
    refs = [sp.topk_reference(rows[r], 20) for r in range(B)]
    ties = sum(int(ref.lps.unique().numel() < 20) for ref in refs)
    for K in (1, 5, 20):
        for r in range(B):
            assert sp.thread_max_candidates(rows[r], K) <= sp.COLLECT
        for kw in ({"temperature": 0.0}, {}):
            tok, lp, ids, lps = _sample(rows, num_logprobs=K, **kw)
            for r in range(B):
                sp.check_topk(ids[r], lps[r], sp.TopK(refs[r].ids[:K], refs[r].lps[:K]), f"row {r} K {K} {kw}")
    assert ties > 0   # the index order of equal values was exercised


@pytest.mark.parametrize("V", TOPK_VOCABS)
def test_topk_forced_overflow_distinct(gpu, V):
    """100 distinct values in [8, 16) in 10 threads: for K = 5 and 20 more than 64 elements reach the K-th largest
    thread maximum, so the exact search and the second collection run.  (K = 1 cannot overflow without ties:
    its bound is the row maximum itself; it runs the same row on the first path.)"""
    row = sp.overflow_row(V, torch.Generator().manual_seed(9), gpu)
    assert sp.thread_max_candidates(row, 1) == 1
    for K in (1, 5, 20):
        if K > 1:
            assert sp.thread_max_candidates(row, K) > sp.COLLECT
        ref = sp.topk_reference(row, K)
        assert ref.lps.unique().numel() == K
        tok, lp, ids, lps = _sample(row[None], num_logprobs=K, temperature=0.0)
        sp.check_topk(ids[0], lps[0], ref, f"K {K}")
        assert tok.item() == int(ref.ids[0])


@pytest.mark.parametrize("V", TOPK_VOCABS)
def test_topk_ties_in_index_order(gpu, V):
    row, ties = sp.tied_three_row(V, torch.Generator().manual_seed(10), gpu)
    ref = sp.topk_reference(row, 5)
    assert sp.thread_max_candidates(row, 5) <= sp.COLLECT and ref.ids[1:4].tolist() == ties
    _, _, ids, lps = _sample(row[None], num_logprobs=5)
    sp.check_topk(ids[0], lps[0], ref)


@pytest.mark.parametrize("n_above", [1, 3])
@pytest.mark.parametrize("V", TOPK_VOCABS)
def test_topk_tie_overflow_keeps_values_above_the_tie(gpu, V, n_above):
    """200 tokens tie at the K-th value (K = 5) on the elements every thread visits first; the values above the
    tie sit on the last element of threads of wave 15.  A collection that appends everything >= the threshold
    in arrival order fills its 64 slots with tied tokens and loses the row maximum.  The best ``n_above``
    outputs must be those values, exactly; the rest carry the tie's logprob with ids among the 200."""
    K = 5
    row, above, ties = sp.tie_overflow_row(V, n_above, gpu)
    assert sp.thread_max_candidates(row, K) == 200 + n_above
    ref = sp.topk_reference(row, K)
    assert ref.ids[:n_above].tolist() == above
    for kw in ({"temperature": 0.0}, {}):
        _, _, ids, lps = _sample(row.expand(8, V), num_logprobs=K, **kw)
        for r in range(8):
            sp.check_topk_tied_tail(ids[r], lps[r], ref, n_above, ties, f"row {r} {kw}")


@pytest.mark.parametrize("n_ties", [45, 60])
@pytest.mark.parametrize("V", TOPK_VOCABS)
def test_topk_tie_window(gpu, V, n_ties):
    """A row that overflows the first collection (three threads hold everything above the background) and whose
    1 + n_ties candidates fit the buffer after the exact search (K = 5: up to 60 ties): every tie is held, so
    the reported ones are those of lowest index, on every row and every run."""
    K = 5
    row, above, ties = sp.tie_window_row(V, n_ties, gpu)
    assert sp.thread_max_candidates(row, K) > sp.COLLECT and n_ties <= sp.COLLECT - (K - 1)
    ref = sp.topk_reference(row, K)
    assert ref.ids.tolist() == above + ties[:K - 1]
    _, _, ids, lps = _sample(row.expand(8, V), num_logprobs=K)
    for r in range(8):
        sp.check_topk(ids[r], lps[r], ref, f"row {r}")


def test_topk_constrained_rows(gpu):
    """mask_logprobs at V = 151936: three allowed tokens at 0, in the ragged slot and at V - 1, K = 20.  The
    masked row reports exactly those three with the restricted log-softmax and 17 empty slots; its unmasked
    neighbour reports raw logprobs."""
    V, K = 151936, 20
    allowed = [0, sp.element_index(sp.valid_slots(V) - 1, 100, 0), V - 1]
    rows = _rand_rows(2, V, gpu, 31, 3.0)
    mask = torch.zeros(1, V // 32, dtype=torch.int32, device=gpu)
    for a in allowed:
        mask[0, a // 32] |= -(1 << 31) if a % 32 == 31 else 1 << (a % 32)   # int32 words: bit 31 is the sign
    mask_rows = torch.tensor([0, -1], dtype=torch.int32, device=gpu)
    ref0, ref1 = sp.topk_reference(rows[0], K, allowed), sp.topk_reference(rows[1], K)
    assert sorted(ref0.ids[:3].tolist()) == allowed and sp.thread_max_candidates(rows[1], K) <= sp.COLLECT
    tok, lp, ids, lps = _sample(rows, num_logprobs=K, mask=mask, mask_rows=mask_rows, mask_logprobs=True)
    sp.check_topk(ids[0], lps[0], ref0, "masked row")
    assert abs(torch.logsumexp(lps[0, :3].double(), 0).item()) <= 2e-3
    assert bool((ids[0, 3:] == -1).all()) and bool((lps[0, 3:] == -math.inf).all())
    assert tok[0].item() in allowed
    sp.check_topk(ids[1], lps[1], ref1, "unmasked neighbour")


# ---------------------------------------------------------------------------------------------------------
# 5. processing at full vocabulary


def _processing_inputs(V, gpu):
    """16 random rows; a dense bias row whose non-zeros (integers in -2..6) sit on edge positions only, next to a
    decoy row that must not be read; a mask with about half its bits set (the words of the ragged slot included;
    the last token and the first of the ragged slot allowed); random counts on 5 % of the tokens and on half of
    the edge positions, so that biased tokens are penalised too.  Every fourth row takes no bias.  Row 0 also
    holds a pair that tells the two possible orders of bias and repetition penalty apart: token 8191 (thread
    1023) at 12.0 with bias 6 and count 1 is worth (12 + 6) / 1.3 - 0.5 = 13.35 when the penalty scales raw +
    bias and 12 / 1.3 - 0.5 + 6 = 14.73 when the bias is added last; token 20000 at 14.0, plain, lies between."""
    g = torch.Generator(device=gpu).manual_seed(40 + V % 11)
    B = 16
    rows = _rand_rows(B, V, gpu, 41 + V % 11, 2.0)
    edges = torch.tensor(sp.edge_positions(V), device=gpu)
    bias = torch.zeros(2, V, device=gpu)
    bias[0, 1000:1064] = 9.0                                      # the decoy
    bias[1, edges] = (torch.rand(edges.numel(), device=gpu, generator=g) * 8 - 2).round()
    S = sp.valid_slots(V)
    bias[1, V - 1], bias[1, sp.element_index(S - 1, 0, 0)] = 6.0, 6.0
    bias_rows = torch.tensor([-1 if r % 4 == 3 else 1 for r in range(B)], dtype=torch.int32, device=gpu)
    words = torch.randint(-2 ** 31, 2 ** 31, (1, V // 32), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    words[0, (V - 1) // 32] |= -(2 ** 31)                         # bit 31: token V - 1
    words[0, sp.element_index(S - 1, 0, 0) // 32] |= 1
    bits = (words[0].long()[:, None] >> torch.arange(32, device=gpu)) & 1
    allowed = bits.reshape(-1).bool()
    ragged = allowed[(S - 1) * 8192:]
    assert 0.45 < allowed.float().mean().item() < 0.55 and 0.4 < ragged.float().mean().item() < 0.6
    seen = torch.rand(B, V, device=gpu, generator=g) < 0.05
    seen[:, edges] = torch.rand(B, edges.numel(), device=gpu, generator=g) < 0.5
    counts = (seen * torch.randint(1, 4, (B, V), device=gpu, generator=g)).to(torch.int16)
    rows[0, 8191], rows[0, 20000] = 12.0, 14.0
    bias[1, 8191], bias[1, 20000] = 6.0, 0.0
    counts[0, 8191], counts[0, 20000] = 1, 0
    words[0, 8191 // 32] |= -(2 ** 31)
    words[0, 20000 // 32] |= 1
    allowed[8191] = allowed[20000] = True
    return rows, bias, bias_rows, words, allowed, counts


def _processed_ref(rows, bias, counts, fpen, ppen, rpen, allowed):
    """fp32 reference of the processed row in the kernel's documented order (the header of sampler.hip: y = raw
    + bias - penalties, masked -> -inf): the bias is added first, the repetition penalty then scales raw + bias,
    and the row is rounded to bf16 once.  NOT ``_penalised_ref(raw) + bias``: the two differ on every token that
    carries both a bias and a count."""
    y = rows.float() + bias
    c = counts.float()
    seen = c > 0
    y = torch.where(seen & (y > 0), y / rpen, torch.where(seen, y * rpen, y))
    y = torch.where(seen, y - fpen * c - ppen, y).to(torch.bfloat16).float()
    return torch.where(allowed[None], y, torch.full_like(y, -math.inf))


@pytest.mark.parametrize("V", PROC_VOCABS)
def test_processing_full_vocab(gpu, V):
    """Bias, grammar mask and all three penalties together on full-size rows, the count rows reached through a
    permutation and the bias row through ``bias_rows``.  The reference follows the kernel's documented order
    (``_processed_ref``).  Conditions read off the reference before the kernel runs: maximisers on and off the
    edge positions; rows whose unpenalised maximiser is a counted token that the penalties dethrone, on an edge
    position among them; and counts read from the wrong row, or the bias after the penalties, would move some
    row's maximiser."""
    fpen, ppen, rpen = 0.3, 0.2, 1.3
    rows, bias, bias_rows, words, allowed, counts = _processing_inputs(V, gpu)
    B = rows.shape[0]
    f = lambda v, n=B: torch.full((n,), float(v), device=gpu)
    zeros = lambda n: torch.zeros(n, dtype=torch.int32, device=gpu)
    row_bias = torch.where((bias_rows >= 0)[:, None], bias[1][None], torch.zeros_like(bias[:1]))
    ref = _processed_ref(rows, row_bias, counts, fpen, ppen, rpen, allowed)
    best = ref.argmax(-1)
    edges = torch.tensor(sp.edge_positions(V), device=gpu)
    on_edge = torch.isin(best, edges)
    assert on_edge.any() and (~on_edge).any() and best[0].item() == 20000
    assert bool((row_bias.gather(1, best[:, None])[:, 0][on_edge] > 0).all())
    unpen = _processed_ref(rows, row_bias, torch.zeros_like(counts), fpen, ppen, rpen, allowed).argmax(-1)
    dethroned = (counts.gather(1, unpen[:, None])[:, 0] > 0) & (unpen != best)
    assert dethroned.any() and (dethroned & torch.isin(unpen, edges)).any()
    is_max = lambda r: r.gather(1, best[:, None])[:, 0] == r.max(-1).values
    assert not is_max(_processed_ref(rows, row_bias, counts.flip(0), fpen, ppen, rpen, allowed)).all()
    issue_order = (_penalised_ref(rows, counts, fpen, ppen, rpen) + row_bias).to(torch.bfloat16).float()
    assert not is_max(torch.where(allowed[None], issue_order, torch.full_like(ref, -math.inf))).all()
    lsm = torch.log_softmax(rows.double(), -1)
    perm = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=gpu)   # row r counts in row B - 1 - r
    proc = dict(bias=bias, bias_rows=bias_rows, mask=words, mask_rows=zeros(B), count_rows=perm, freq_pen=f(fpen),
                pres_pen=f(ppen), rep_pen=f(rpen))
    held = counts.flip(0).contiguous()
    tok, lp, *_ = _sample(rows, temperature=0.0, counts=held, **proc)
    got = ref.gather(1, tok.long()[:, None])[:, 0]
    assert torch.equal(got, ref.max(-1).values)   # the chosen token is a maximiser (ties allowed)
    want_lp = lsm.gather(1, tok.long()[:, None])[:, 0]
    assert bool(((lp.double() - want_lp).abs() <= sp.LP_ATOL + sp.LP_RTOL * want_lp.abs()).all())   # RAW logprob
    bumped = counts.clone()   # every row counted its own token, in its own count row
    bumped[torch.arange(B, device=gpu), tok.long()] += 1
    assert torch.equal(held.flip(0), bumped)
    # sampled: 1024 seeds of row 0 in two calls (a private count row each), never a masked token
    half = R_SUPPORT // 2
    for h in range(2):
        seeds = (torch.arange(half, device=gpu, dtype=torch.int64) + h * half) * 7919 + 1
        p1 = dict(bias=bias, bias_rows=zeros(half) + 1, mask=words, mask_rows=zeros(half),
                  count_rows=torch.arange(half, dtype=torch.int32, device=gpu), freq_pen=f(fpen, half),
                  pres_pen=f(ppen, half), rep_pen=f(rpen, half))
        tok, *_ = _sample(rows[0].expand(half, V), seeds=seeds, counts=counts[0].expand(half, V).contiguous(), **p1)
        assert bool(((tok >= 0) & (tok < V)).all()) and bool(allowed[tok.long()].all())
    # every token masked: token 0, greedy and sampled
    none = torch.zeros(1, V // 32, dtype=torch.int32, device=gpu)
    for T in (0.0, 1.0):
        tok, *_ = _sample(rows, temperature=T, mask=none, mask_rows=zeros(B))
        assert bool((tok == 0).all()), (T, tok.tolist())


# ---------------------------------------------------------------------------------------------------------
# 6. contract checks


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_batch_independence(gpu):
    """Row i's outputs are bit-equal alone and inside a batch of 64 rows with different parameters."""
    V, B, K = 151936, 64, 20
    rows = _rand_rows(B, V, gpu, 50, 2.0)
    i = torch.arange(B, device=gpu)
    kw = dict(temperature=torch.where(i % 4 == 0, 0.0, 0.5 + 0.02 * i).float(),
              top_p=torch.where(i % 3 == 0, 1.0, 0.3 + 0.01 * i).float(),
              top_k=torch.where(i % 5 == 0, 0, 1 + i).to(torch.int32),
              min_p=torch.where(i % 7 == 1, 0.05, 0.0).float(), top_a=torch.where(i % 11 == 2, 0.2, 0.0).float(),
              seeds=i.long() * 7919 + 1 + (i.long() << 33), offsets=i.long() * 3)
    batch = _sample(rows, num_logprobs=K, **kw)
    for r in (0, 1, 2, 3, 13, 22, 40, 63):
        alone = _sample(rows[r:r + 1], num_logprobs=K, **{k: v[r:r + 1] for k, v in kw.items()})
        for a, b in zip(alone, batch):
            assert torch.equal(_bits(a[0]), _bits(b[r])), f"row {r}"


@pytest.mark.parametrize("which", ["seeds", "offsets"])
def test_high_bits_of_seed_and_offset(gpu, which):
    """s and s + 2^32 are different streams: on a two-hot row over 1024 seeds they disagree on 35..65 % of the
    rows (independent fair draws: 0.5 +- about 10 sigma)."""
    V, R = 151936, 1024
    row = sp.two_hot_row(V, sp.edge_pairs(V)["first_last"], gpu).expand(R, V)
    s = torch.arange(R, device=gpu, dtype=torch.int64) * 7919 + 1
    a, *_ = _sample(row, **{which: s})
    b, *_ = _sample(row, **{which: s + 2 ** 32})
    assert 0.35 <= (a != b).float().mean().item() <= 0.65


def test_strided_logits_view(gpu):
    V, B, K = 151936, 8, 20
    rows = _rand_rows(B, V, gpu, 60, 2.0)
    wide = torch.full((B, V + 64), float("nan"), dtype=torch.bfloat16, device=gpu)
    wide[:, :V] = rows
    view = wide[:, :V]
    assert view.stride(0) == V + 64
    for kw in ({"top_p": 0.9}, {"temperature": 0.0}):
        for a, b in zip(_sample(view, num_logprobs=K, **kw), _sample(rows, num_logprobs=K, **kw)):
            assert torch.equal(_bits(a), _bits(b)), kw


def test_host_refusals(gpu):
    """Shapes no instance serves are refused by the host check, which runs before any launch."""
    for V, K in ((163872, 0), (4104, 0), (4096, 21)):
        rows = torch.zeros(2, V, dtype=torch.bfloat16, device=gpu)
        with pytest.raises(RuntimeError):
            _sample(rows, num_logprobs=K)
    tok, *_ = _sample(torch.zeros(2, 4096, dtype=torch.bfloat16, device=gpu), num_logprobs=20, temperature=0.0)
    assert tok.tolist() == [0, 0]
