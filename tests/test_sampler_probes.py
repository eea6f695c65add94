"""The sampler probes (tests/sampler_probes.py) checked on the CPU: at every vocabulary and case that
tests/test_sampler_probes_gpu.py runs, the preconditions of an exact comparison hold from the reference alone,
data synthesised from the honest reference passes the comparison functions, and data from each wrong reference
— a kept set one token short or long, a nucleus that splits ties, an index map with slot and thread or the dword
halves swapped or without the ragged slot, a top-K that keeps the first 64 candidates it visits — is rejected by
the same functions."""
import math

import pytest
import torch

from tests import sampler_probes as sp

R_SUPPORT, R_FREQ, R_PAIR = 1024, 65536, 16384
TOPK_VOCABS = (32000, 128256, 151936)
PAIR_VOCABS = (65504, 128256, 151936)

# the worst margins of the live-logit cases that depend on rounded masses, worked out by hand
MARGINS = {"top_p_0.8": 0.0176, "top_p_0.5": 0.086, "top_p_0.3": 0.114, "top_k_4_top_p_0.8": 0.069,
           "tie_top_p_0.6": 0.125}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_vocabularies_and_instances():
    shape = {V: (sp.valid_slots(V), sp.last_slot_vectors(V), sp.instance_slots(V)) for V in sp.VOCABS}
    assert shape == {32000: (4, 928, 4), 65504: (8, 1020, 8), 128256: (16, 672, 16), 151936: (19, 560, 20),
                     152064: (19, 576, 20)}
    assert all(V % 32 == 0 for V in sp.VOCABS)
    assert sp.instance_slots(20 * 8192) == 20
    with pytest.raises(ValueError):
        sp.instance_slots(20 * 8192 + 32)


@pytest.mark.parametrize("V", [152064, 65504])
def test_edge_positions_against_enumeration(V):
    """Brute force over every token of the row: the map and its inverse agree, and the edge positions are valid,
    distinct and cover every (slot, dword, half) of every valid slot."""
    S, nl = sp.valid_slots(V), sp.last_slot_vectors(V)
    where = {}
    for j in range(S):
        for t in range(sp.THREADS if j < S - 1 else nl):
            for e in range(sp.VEC):
                where[sp.element_index(j, t, e)] = (j, t, e)
    assert sorted(where) == list(range(V))           # a bijection onto the row, padding excluded
    pos = sp.edge_positions(V)
    assert len(set(pos)) == len(pos) and all(p in where for p in pos)
    assert all(sp.element_coords(p) == where[p] for p in pos)
    assert {(where[p][0], where[p][2] >> 1, where[p][2] & 1) for p in pos} == \
        {(j, d, h) for j in range(S) for d in range(4) for h in range(2)}
    for t in (0, 63, 64):
        assert {(j, e) for p in pos for j, tt, e in [where[p]] if tt == t} == {(j, e) for j in range(S) for e in range(8)}
    named = {0, 7, 8, 8191, 8192, V - 1, sp.element_index(S - 1, 0, 0), sp.element_index(S - 2, 1023, 7)}
    assert named <= set(pos)
    assert where[8191] == (0, 1023, 7) and where[V - 1] == (S - 1, nl - 1, 7)
    pairs = sp.edge_pairs(V)
    a, b = (where[p] for p in pairs["same_dword"])
    assert a[:2] == b[:2] and a[2] >> 1 == b[2] >> 1 and a[2] != b[2]
    a, b = (where[p] for p in pairs["same_thread_first_last_slot"])
    assert a[1] == b[1] and (a[0], b[0]) == (0, S - 1)
    assert [where[p][1] for p in pairs["threads_63_64"]] == [63, 64]
    assert [where[p][1] for p in pairs["threads_0_1023"]] == [0, 1023]
    assert set(pairs["same_dword"]) | set(pairs["same_thread_first_last_slot"]) <= set(pos)
    live = sp.live_positions(V)
    assert set(live) <= set(pos) and len(set(live)) == 6
    assert len({where[p][1] // 64 for p in live}) >= 4 and where[live[3]][0] == S - 1 and live[4] == V - 1
    assert where[live[0]][:2] == where[live[1]][:2] and where[live[0]][2] >> 1 == where[live[1]][2] >> 1


def _case(V, name, background=-math.inf):
    kind, kw, n = sp.SUPPORT_CASES[name]
    row = sp.support_row(V, kind, background=background)
    return row, sp.kept_reference(row, **kw), n


@pytest.mark.parametrize("name", list(sp.SUPPORT_CASES))
@pytest.mark.parametrize("V", sp.VOCABS)
def test_support_preconditions_and_honest_data(V, name):
    row, ref, n = _case(V, name)
    assert ref.ids.numel() == n
    pos = sp.live_positions(V)
    kind = sp.SUPPORT_CASES[name][0]
    order = sp.LIVE_ORDER if kind == "live" else sp.TIE_ORDER
    assert ref.ids.tolist() == sorted(pos[o] for o in order[:n])   # the n largest logits (ties included)
    sp.assert_preconditions(ref, R_SUPPORT)
    if name in MARGINS:
        assert abs(ref.margin - MARGINS[name]) < 1e-3
    assert sp.miss_probability(ref, R_SUPPORT) < (1e-14 if name == "none" else sp.MISS_MAX)
    sp.check_support(sp.draw_tokens(ref, R_SUPPORT, _gen(1)), ref)
    # a background that underflows to u = 0 changes nothing
    ref40 = sp.kept_reference(sp.support_row(V, kind, background=-40.0), **sp.SUPPORT_CASES[name][1])
    assert torch.equal(ref40.ids, ref.ids) and torch.allclose(ref40.q, ref.q, rtol=0, atol=1e-12)
    if name in sp.FREQUENCY_CASES:
        sp.assert_preconditions(ref, R_FREQ)
        sp.check_frequencies(sp.draw_tokens(ref, R_FREQ, _gen(2)), ref)


def test_preconditions_reject_close_calls():
    """The preconditions are not vacuous: a nucleus cut 0.002 from a token's mass, a live token in the fp16
    subnormal range and a kept token too rare for R rows are each refused."""
    V = 32000
    row = sp.support_row(V, "live")
    full = sp.kept_reference(row)
    above_third = float(full.q.sort(descending=True).values[:2].sum())
    with pytest.raises(AssertionError, match="threshold"):
        sp.assert_preconditions(sp.kept_reference(row, top_p=above_third + 0.002), R_SUPPORT)
    faint = row.clone()
    faint[100] = -9.0   # u = 1.7e-5: live, fp16 subnormal
    with pytest.raises(AssertionError, match="2\\^-10"):
        sp.assert_preconditions(sp.kept_reference(faint), R_SUPPORT)
    rare = row.clone()
    rare[100] = -4.5    # u = 1.5e-3, q = 6.2e-4: missed by 1024 rows with p = 0.53
    with pytest.raises(AssertionError, match="missed"):
        sp.assert_preconditions(sp.kept_reference(rare), R_SUPPORT)


@pytest.mark.parametrize("name", list(sp.SUPPORT_CASES))
@pytest.mark.parametrize("V", sp.VOCABS)
def test_wrong_kept_sets_are_rejected(V, name):
    row, ref, _ = _case(V, name)
    wrong = [w for w in (sp.kept_one_short(ref), sp.kept_one_long(ref)) if w is not None]
    assert wrong   # every case has at least one neighbour set
    assert (sp.kept_one_long(ref) is None) == (ref.ids.numel() == ref.live_ids.numel())
    for w in wrong:
        assert abs(w.ids.numel() - ref.ids.numel()) == 1
        assert sp.miss_probability(w, R_SUPPORT) < sp.MISS_MAX   # the surplus token does get drawn
        with pytest.raises(AssertionError):
            sp.check_support(sp.draw_tokens(w, R_SUPPORT, _gen(3)), ref)
        if name in sp.FREQUENCY_CASES:
            with pytest.raises(AssertionError):
                sp.check_frequencies(sp.draw_tokens(w, R_FREQ, _gen(4)), ref)
    top_p = sp.SUPPORT_CASES[name][1].get("top_p")
    if top_p is not None and "top_k" not in sp.SUPPORT_CASES[name][1]:
        cut = sp.kept_sort_and_cut(row, top_p)
        if name.startswith("tie"):   # the cut falls inside the tie: two of four kept
            assert cut.ids.numel() == 2
            with pytest.raises(AssertionError):
                sp.check_support(sp.draw_tokens(cut, R_SUPPORT, _gen(5)), ref)
        else:                        # without ties both rules agree: only the tie rows tell them apart
            assert torch.equal(cut.ids, ref.ids)


def test_frequency_bound_notices_a_shifted_nucleus():
    """The derived bound is tight enough: at R = 65536 a two-token nucleus drawn at 0.60 / 0.40 instead of
    0.622 / 0.378 is rejected (the bound there is 0.0115)."""
    ref = _case(151936, "top_p_0.5")[1]
    assert float(sp.frequency_bound(ref.q, R_FREQ).max()) < 0.0115
    shifted = ref._replace(q=torch.tensor([0.60, 0.40], dtype=torch.float64)[ref.q.argsort(descending=True).argsort()])
    with pytest.raises(AssertionError):
        sp.check_frequencies(sp.draw_tokens(shifted, R_FREQ, _gen(6)), ref)


@pytest.mark.parametrize("V", sp.VOCABS)
def test_wrong_index_maps_are_rejected(V):
    hot = sp.edge_positions(V)
    assert len(hot) * V * 2 < 256 << 20   # one bf16 logits tensor per sweep
    sp.check_one_hot(sp.one_hot_answers(V, hot), hot)
    for name, f in sp.WRONG_MAPS.items():
        with pytest.raises(AssertionError):
            sp.check_one_hot(sp.one_hot_answers(V, hot, f), hot)
    # each single family of positions catches its own fault: thread 0 alone the swapped halves, V - 1 alone the
    # dropped slot, thread 1023 of slot 0 alone the swapped slot and thread
    for name, p in (("halves_swapped", 0), ("ragged_slot_dropped", V - 1), ("slot_thread_swapped", 8191)):
        with pytest.raises(AssertionError):
            sp.check_one_hot(sp.one_hot_answers(V, [p], sp.WRONG_MAPS[name]), [p])
    for r in range(2):   # one-hot rows: the hot token is the whole kept set under every filter
        ref = sp.kept_reference(sp.one_hot_rows(V, hot[-2:], -40.0)[r], top_p=0.5, top_k=5)
        assert ref.ids.tolist() == [hot[-2:][r]] and ref.margin > sp.MARGIN


@pytest.mark.parametrize("V", PAIR_VOCABS)
def test_two_hot_pairs(V):
    for name, pair in sp.edge_pairs(V).items():
        ref = sp.kept_reference(sp.two_hot_row(V, pair))
        assert ref.ids.tolist() == sorted(pair) and ref.q.tolist() == [0.5, 0.5]
        sp.assert_preconditions(ref, R_PAIR)
        sp.check_two_hot(sp.draw_tokens(ref, R_PAIR, _gen(7)), pair)
        skew = ref._replace(q=torch.tensor([0.53, 0.47], dtype=torch.float64))   # bound: 0.0195
        with pytest.raises(AssertionError):
            sp.check_two_hot(sp.draw_tokens(skew, R_PAIR, _gen(8)), pair)
        with pytest.raises(AssertionError):   # a walk that lands on the neighbour of the second token
            sp.check_two_hot(torch.tensor([pair[0], pair[1] ^ 1] * 512), pair)


def _as_outputs(ref):
    """A TopK as the kernel would return it: int32 ids, fp32 logprobs."""
    return ref.ids.to(torch.int32), ref.lps.float()


@pytest.mark.parametrize("V", TOPK_VOCABS)
def test_topk_rows_and_first_collected(V):
    row = sp.overflow_row(V, _gen(9))
    vals = row.double()
    assert int((vals >= 8).sum()) == 100 and vals[vals >= 8].unique().numel() == 100
    assert len({sp.element_coords(int(i))[1] for i in (vals >= 8).nonzero()[:, 0]}) == 10
    assert sp.thread_max_candidates(row, 1) == 1          # K = 1: the bound IS the maximum, nothing overflows
    for K in (5, 20):
        assert sp.thread_max_candidates(row, K) > sp.COLLECT
        ref = sp.topk_reference(row, K)
        assert ref.lps.unique().numel() == K              # distinct values: the order is unambiguous
        sp.check_topk(*_as_outputs(ref), ref)
        sp.check_topk(*_as_outputs(sp.topk_first_collected(row, K)), ref)   # distinct values: K candidates
        with pytest.raises(AssertionError):               # without the exact search the best, visited last, are lost
            sp.check_topk(*_as_outputs(sp.topk_first_collected(row, K, exact=False)), ref)
    # three equal values among the best five, few candidates: index order decides
    row, ties = sp.tied_three_row(V, _gen(10))
    ref = sp.topk_reference(row, 5)
    assert sp.thread_max_candidates(row, 5) <= sp.COLLECT and ref.ids[1:4].tolist() == ties
    sp.check_topk(*_as_outputs(ref), ref)
    swapped = ref.ids.clone()
    swapped[1:4] = ref.ids[1:4].flip(0)
    with pytest.raises(AssertionError):
        sp.check_topk(swapped, ref.lps, ref)
    # a logprob off by 0.01 is outside the bound
    with pytest.raises(AssertionError):
        sp.check_topk(ref.ids, ref.lps + 0.01, ref)


@pytest.mark.parametrize("n_above", [1, 3])
@pytest.mark.parametrize("V", TOPK_VOCABS)
def test_tie_overflow_row_rejects_first_collected(V, n_above):
    """200 tokens tie at the K-th value and are visited first; the values above them are visited last.  The
    honest top-5 passes; the first-64-collected top-K has lost every value above the tie."""
    K = 5
    row, above, ties = sp.tie_overflow_row(V, n_above)
    assert all(sp.element_coords(a)[1] >= 960 and sp.element_coords(a)[2] == 7 for a in above)   # wave 15
    assert all(a + 8192 >= V or sp.element_coords(a)[0] == sp.valid_slots(V) - 1 for a in above)  # last valid element
    assert sp.thread_max_candidates(row, K) == 200 + n_above > sp.COLLECT
    ref = sp.topk_reference(row, K)
    assert ref.ids[:n_above].tolist() == above and set(ref.ids[n_above:].tolist()) <= set(ties)
    assert ref.lps[n_above:].unique().numel() == 1
    sp.check_topk_tied_tail(*_as_outputs(ref), ref, n_above, ties)
    other = ref._replace(ids=torch.cat([ref.ids[:n_above], torch.tensor(ties[-(K - n_above):])]))
    sp.check_topk_tied_tail(*_as_outputs(other), ref, n_above, ties)   # which of the tied tokens: left open
    lost = sp.topk_first_collected(row, K)
    assert not set(above) & set(lost.ids.tolist())
    with pytest.raises(AssertionError):
        sp.check_topk_tied_tail(*_as_outputs(lost), ref, n_above, ties)


@pytest.mark.parametrize("n_ties", [45, 60])
@pytest.mark.parametrize("V", TOPK_VOCABS)
def test_tie_window_row(V, n_ties):
    """An overflowing row whose candidates fit the buffer again after the exact search (1 above + n_ties <= 64 -
    (K - 1) + 1 at K = 5): the reference's ties are the four of lowest index, and a top-K that holds only some
    of the ties, by arrival, is rejected by the exact comparison."""
    K = 5
    row, above, ties = sp.tie_window_row(V, n_ties)
    assert len(set(ties)) == n_ties <= sp.COLLECT - (K - 1)
    assert {sp.element_coords(i)[1] for i in ties} == {10, 11}
    assert sp.thread_max_candidates(row, K) == V > sp.COLLECT      # the bound is the background: overflow
    ref = sp.topk_reference(row, K)
    assert ref.ids.tolist() == above + ties[:K - 1]
    sp.check_topk(*_as_outputs(ref), ref)
    late = ref._replace(ids=torch.tensor(above + ties[-(K - 1):]))   # the ties that arrived last
    with pytest.raises(AssertionError):
        sp.check_topk(*_as_outputs(late), ref)


def test_constrained_reference():
    V = 151936
    S = sp.valid_slots(V)
    allowed = [0, sp.element_index(S - 1, 100, 0), V - 1]
    row = (torch.randn(V, generator=_gen(11)) * 3).to(torch.bfloat16)
    ref = sp.topk_reference(row, 20, allowed)
    assert sorted(ref.ids[:3].tolist()) == allowed and ref.ids[3:].tolist() == [-1] * 17
    assert abs(float(torch.logsumexp(ref.lps[:3], 0))) < 1e-12 and bool((ref.lps[3:] == -math.inf).all())
