"""Structured inputs and float64 references for the fused sampler (csrc/kernels/sampler.hip), and
deliberately wrong references.

The kernel holds a logits row in registers: thread ``t`` of 1024, slot ``j`` and element ``e`` of a 16-byte
vector own token ``(j * 1024 + t) * 8 + e``; ``e >> 1`` is the dword and ``e & 1`` the half the packed searches
and the owner walk address.  A vocabulary of V tokens has ``ceil(V / 8 / 1024)`` valid slots, the last one
ragged, and runs the template instance with 4, 8, 16 or 20 slots.  ``VOCABS`` in valid slots x vectors of the
last slot: 4 x 928 (SLOTS=4), 8 x 1020 (SLOTS=8), 16 x 672 (SLOTS=16), 19 x 560 and 19 x 576 (SLOTS=20, slot 19
all padding).

Three references, all float64 from the bf16 logits:

* ``kept_reference``: the exact set of tokens a filtered draw may return and their probabilities, by the
  conventions at the top of sampler.hip — ties at a threshold are kept; top-p keeps a token iff the mass
  strictly above it is < top_p * mass(top-k set); the argmax is never filtered; zero-mass tokens never kept.
  Its ``assert_preconditions`` states, from the reference alone, when a kernel working on fp16 masses must
  agree exactly: every decision clears its threshold by more than ``MARGIN`` (the kernel's u is fp16 rounded
  toward zero, relative error < 2^-10; the factor 4 covers the sum and the fp16 conversion of min_p and
  top_a / Z), every live u is >= 2^-10 (no fp16 subnormals) and every kept token is drawn in R rows except
  with probability < 1e-9.
* ``topk_reference``: log-softmax ordered value descending, then index ascending (a stable sort).
* the index map itself (``element_index``), with ``edge_positions`` naming the tokens where a wrong map shows.

The wrong references at the end are what tests/test_sampler_probes.py feeds to the same comparison functions
to show that they would notice: a kept set one token short or long, a sort-and-cut nucleus that splits ties,
index maps with slot and thread or the dword halves swapped or the ragged slot dropped, and a top-K that keeps
the first 64 candidates in visit order.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

THREADS = 1024
VEC = 8
COLLECT = 64         # kCollect: candidate slots of the top-logprob collection
VOCABS = (32000, 65504, 128256, 151936, 152064)

U_REL = 2.0 ** -10           # relative error bound of one fp16 u (round toward zero)
MARGIN = 4 * U_REL           # every decision must clear its threshold by more than this
U_LIVE_MIN = 2.0 ** -10      # live tokens: fp16 normal, far from the subnormal range
U_DEAD_MAX = 2.0 ** -25      # below half the smallest fp16 subnormal: u is exactly 0 in the kernel
MISS_MAX = 1e-9
LP_ATOL, LP_RTOL = 2e-3, 1e-3        # logprob bound of test_sample_greedy_and_logprobs
FREQ_SIGMAS, FREQ_ROUND = 5.0, 2e-3  # binomial standard deviations + the fp16 mass rounding bound


# ---------------------------------------------------------------------------------------------------------
# the index map


def element_index(j: int, t: int, e: int) -> int:
    return (j * THREADS + t) * VEC + e


def element_coords(i: int) -> Tuple[int, int, int]:
    """(slot, thread, element) of token i: the inverse of ``element_index``."""
    return i // (THREADS * VEC), (i // VEC) % THREADS, i % VEC


def valid_slots(V: int) -> int:
    return -(-(V // VEC) // THREADS)


def last_slot_vectors(V: int) -> int:
    """Threads that hold a vector in the last valid slot."""
    return V // VEC - (valid_slots(V) - 1) * THREADS


def instance_slots(V: int) -> int:
    """SLOTS of the template instance lwc_sample launches for V."""
    for s in (4, 8, 16, 20):
        if valid_slots(V) <= s:
            return s
    raise ValueError(f"V = {V} exceeds the largest instance")


def last_valid_slot(V: int, t: int) -> int:
    """Highest slot in which thread t holds tokens."""
    return valid_slots(V) - (1 if t < last_slot_vectors(V) else 2)


def edge_pairs(V: int) -> Dict[str, Tuple[int, int]]:
    """Token pairs that a walk over the owner's dwords, or a scan over threads, can confuse."""
    S = valid_slots(V)
    return {
        "same_dword": (element_index(1, 200, 2), element_index(1, 200, 3)),
        "same_thread_first_last_slot": (element_index(0, 100, 5), element_index(S - 1, 100, 5)),
        "threads_63_64": (element_index(0, 63, 7), element_index(0, 64, 0)),
        "threads_0_1023": (element_index(1, 0, 3), element_index(1, 1023, 4)),
        "first_last": (0, V - 1),
    }


def edge_positions(V: int) -> List[int]:
    """Tokens where an index map goes wrong first: 0, 7, 8, thread 1023 of slot 0 and its successor, V - 1, both
    ends of the last valid slot, the end of the last full slot, every (slot, element) of threads 0, 63 and 64
    (both halves of all four dwords of every valid slot) and the dword-sharing and thread-sharing pairs."""
    S, nl = valid_slots(V), last_slot_vectors(V)
    pos = {0, 7, 8, 8191, 8192, V - 1, element_index(S - 1, 0, 0), element_index(S - 1, nl - 1, 7),
           element_index(S - 2, THREADS - 1, 7)}
    for t in (0, 63, 64):
        pos |= {element_index(j, t, e) for j in range(S) for e in range(VEC)}
    pairs = edge_pairs(V)
    pos |= set(pairs["same_dword"]) | set(pairs["same_thread_first_last_slot"])
    return sorted(pos)


def live_positions(V: int) -> List[int]:
    """Six of the edge positions for the support rows, in four or more waves: the pair in one dword (thread 200,
    wave 3), one of thread 0 (slot 2), one in the ragged slot (thread 100, wave 1), V - 1 (the ragged slot's last
    thread, wave 8..15) and the end of the last full slot (thread 1023, wave 15)."""
    S = valid_slots(V)
    pairs = edge_pairs(V)
    return [*pairs["same_dword"], element_index(2, 0, 4), pairs["same_thread_first_last_slot"][1], V - 1,
            element_index(S - 2, THREADS - 1, 7)]


# ---------------------------------------------------------------------------------------------------------
# support rows and their cases

LIVE_LOGITS = (2.0, 1.5, 1.0, 0.5, 0.0, -0.5)
# which live position takes which logit: 2.0 in the ragged slot, 1.5 at V - 1, 1.0 and 0.5 share a dword (the
# boundary of top_p 0.8, top_k 3 and min_p 0.3 runs between the halves of that dword), 0.0 on thread 0, -0.5 at
# the end of the last full slot
LIVE_ORDER = (3, 4, 0, 1, 2, 5)
TIE_LOGITS = (1.0, 0.0, 0.0, 0.0)
TIE_ORDER = (3, 0, 1, 4)   # the maximum in the ragged slot; ties in one dword and at V - 1

# name -> (row kind, sampling parameters, size of the kept set)
SUPPORT_CASES: Dict[str, Tuple[str, dict, int]] = {
    "none": ("live", {}, 6),
    "top_p_0.8": ("live", {"top_p": 0.8}, 3),
    "top_p_0.5": ("live", {"top_p": 0.5}, 2),
    "top_p_0.3": ("live", {"top_p": 0.3}, 1),
    "top_k_3": ("live", {"top_k": 3}, 3),
    "top_k_4_top_p_0.8": ("live", {"top_k": 4, "top_p": 0.8}, 3),
    "min_p_0.3": ("live", {"min_p": 0.3}, 3),
    "top_a_0.5": ("live", {"top_a": 0.5}, 4),
    "tie_top_p_0.6": ("tie", {"top_p": 0.6}, 4),
    "tie_top_k_2": ("tie", {"top_k": 2}, 4),
}
FREQUENCY_CASES = ("none", "top_p_0.5")   # the second: a third of the rows reject and draw again from ctr[1]


def support_row(V: int, kind: str, device="cpu", background: float = -math.inf) -> torch.Tensor:
    """bf16 [V]: the live (or tie) logits on ``live_positions`` and ``background`` everywhere else."""
    pos = live_positions(V)
    vals, order = (LIVE_LOGITS, LIVE_ORDER) if kind == "live" else (TIE_LOGITS, TIE_ORDER)
    row = torch.full((V,), background, dtype=torch.float32, device=device)
    row[torch.tensor([pos[o] for o in order], device=device)] = torch.tensor(vals, device=device)
    return row.to(torch.bfloat16)


def two_hot_row(V: int, pair: Tuple[int, int], device="cpu") -> torch.Tensor:
    row = torch.full((V,), -math.inf, dtype=torch.float32, device=device)
    row[torch.tensor(pair, device=device)] = 0.0
    return row.to(torch.bfloat16)


def one_hot_rows(V: int, hot: Sequence[int], background: float, device="cpu") -> torch.Tensor:
    """bf16 [len(hot), V]: row r has token hot[r] at 0.0 and ``background`` elsewhere."""
    rows = torch.full((len(hot), V), background, dtype=torch.bfloat16, device=device)
    rows[torch.arange(len(hot), device=device), torch.tensor(list(hot), device=device)] = 0.0
    return rows


# ---------------------------------------------------------------------------------------------------------
# kept-set reference


class Kept(NamedTuple):
    ids: torch.Tensor       # int64, ascending: the tokens a draw may return
    q: torch.Tensor         # float64, their probabilities (sum 1)
    live_ids: torch.Tensor  # int64, ascending: every token with mass
    live_u: torch.Tensor    # float64: exp((y - ymax) / T) of the live tokens
    margin: float           # smallest distance of a decision from its threshold (inf: no filter decides)
    min_live_u: float       # smallest u that is not exactly 0 in the kernel


def _renormalised(ref: Kept, keep: torch.Tensor) -> Kept:
    u = ref.live_u[keep]
    return ref._replace(ids=ref.live_ids[keep], q=u / u.sum())


def kept_reference(row: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                   min_p: float = 0.0, top_a: float = 0.0) -> Kept:
    """The exact kept set of a bf16 logits row [V] and its probabilities, in float64."""
    y = row.detach().to("cpu").double()
    u = torch.exp((y - y.max()) / temperature)
    nz = u >= U_DEAD_MAX          # below: exactly 0 in the kernel's fp16 form, "zero mass"
    live_ids = nz.nonzero()[:, 0]
    ul = u[live_ids]
    Z = ul.sum()
    top = ul == 1.0               # the argmax (and its exact ties): never filtered, compared exactly
    keep = torch.ones_like(top)
    margins: List[float] = []
    mass_k = Z
    if 0 < top_k <= ul.numel():
        tau = torch.sort(ul, descending=True).values[top_k - 1]
        keep &= ul >= tau         # ties at the k-th value are kept
        mass_k = ul[ul >= tau].sum()
        if (ul < tau).any():
            margins.append(float(1 - ul[ul < tau].max() / tau))
    if top_p < 1.0:
        s, order = torch.sort(ul, descending=True, stable=True)
        c = torch.cumsum(s, 0)
        _, inv, counts = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
        starts = torch.cumsum(counts, 0) - counts
        above = torch.empty_like(ul)
        above[order] = (c[starts] - s[starts])[inv]   # mass strictly above each token (ties share it)
        keep &= above < top_p * mass_k
        margins.append(float((above / mass_k - top_p).abs().min()))
    for thr in ([min_p] if min_p > 0 else []) + ([min(float(top_a / Z), 1.0)] if top_a > 0 else []):
        keep &= ul >= thr
        if (~top).any():
            margins.append(float((ul[~top] / thr - 1).abs().min()))
    keep |= top
    ref = Kept(live_ids, ul, live_ids, ul, min(margins) if margins else math.inf, float(ul.min()))
    return _renormalised(ref, keep)


def miss_probability(ref: Kept, R: int) -> float:
    """Upper bound on the chance that R independent draws leave some kept token undrawn."""
    return float(((1 - ref.q) ** R).sum())


def assert_preconditions(ref: Kept, R: int) -> None:
    assert ref.margin > MARGIN, f"a decision sits {ref.margin:.3g} from its threshold (need > {MARGIN:.3g})"
    assert ref.min_live_u >= U_LIVE_MIN, f"live u {ref.min_live_u:.3g} below 2^-10"
    assert miss_probability(ref, R) < MISS_MAX, f"a kept token is missed with p = {miss_probability(ref, R):.3g}"


def draw_tokens(ref: Kept, R: int, gen: torch.Generator) -> torch.Tensor:
    """R independent draws from the reference distribution (CPU stand-in for the kernel's output)."""
    return ref.ids[torch.multinomial(ref.q, R, replacement=True, generator=gen)]


# ---------------------------------------------------------------------------------------------------------
# comparisons (the GPU tests and the CPU tests call the same ones)


def check_one_hot(tok: torch.Tensor, hot: Sequence[int]) -> None:
    tok = tok.detach().to("cpu").long()
    want = torch.as_tensor(list(hot), dtype=torch.long)
    bad = (tok != want).nonzero()[:, 0]
    assert bad.numel() == 0, (f"{bad.numel()} of {want.numel()} one-hot rows returned another token; first: hot "
                              f"{int(want[bad[0]])} {element_coords(int(want[bad[0]]))} -> {int(tok[bad[0]])}")


def check_support(tok: torch.Tensor, ref: Kept) -> None:
    """The set of drawn tokens is the kept set, exactly."""
    got = torch.unique(tok.detach().to("cpu").long())
    assert torch.equal(got, ref.ids), (f"drawn {got.tolist()[:12]} ({got.numel()} tokens), "
                                       f"kept {ref.ids.tolist()} ({ref.ids.numel()})")


def frequency_bound(q: torch.Tensor, R: int) -> torch.Tensor:
    return FREQ_SIGMAS * torch.sqrt(q * (1 - q) / R) + FREQ_ROUND


def check_frequencies(tok: torch.Tensor, ref: Kept) -> None:
    """Per kept token |count / R - q| <= 5 sqrt(q (1 - q) / R) + 2e-3, and nothing else drawn."""
    tok = tok.detach().to("cpu").long()
    R = tok.numel()
    got, cnt = torch.unique(tok, return_counts=True)
    stray = got[~torch.isin(got, ref.ids)]
    assert stray.numel() == 0, f"tokens outside the kept set: {stray[:8].tolist()}"
    f = torch.zeros_like(ref.q)
    f[torch.searchsorted(ref.ids, got)] = cnt.double() / R
    err, lim = (f - ref.q).abs(), frequency_bound(ref.q, R)
    assert bool((err <= lim).all()), f"frequencies {f.tolist()} vs q {ref.q.tolist()} (bounds {lim.tolist()})"


def check_two_hot(tok: torch.Tensor, pair: Tuple[int, int]) -> None:
    """Two equal tokens: nothing else drawn, each within five binomial standard deviations of one half."""
    tok = tok.detach().to("cpu").long()
    R = tok.numel()
    n0, n1 = int((tok == pair[0]).sum()), int((tok == pair[1]).sum())
    stray = tok[(tok != pair[0]) & (tok != pair[1])]
    assert stray.numel() == 0, f"{stray.numel()} draws outside the pair {pair}: {stray[:8].tolist()}"
    assert abs(n0 / R - 0.5) <= FREQ_SIGMAS * math.sqrt(0.25 / R), f"pair {pair}: {n0 / R:.4f} / {n1 / R:.4f}"


class TopK(NamedTuple):
    ids: torch.Tensor   # int64 [K], -1 where fewer than K tokens are finite
    lps: torch.Tensor   # float64 [K], -inf there


def _ranked(y: torch.Tensor, idx: torch.Tensor, K: int, lse: torch.Tensor) -> TopK:
    """Best K of tokens ``idx`` by (value descending, index ascending), padded with -1 / -inf."""
    idx = idx.sort().values
    vals, o = torch.sort(-y[idx], stable=True)
    ids = torch.full((K,), -1, dtype=torch.long)
    lps = torch.full((K,), -math.inf, dtype=torch.float64)
    n = min(K, int((vals < math.inf).sum()))
    ids[:n], lps[:n] = idx[o[:n]], -vals[:n] - lse
    return TopK(ids, lps)


def _raw(row: torch.Tensor, allowed: Optional[Sequence[int]] = None) -> torch.Tensor:
    y = row.detach().to("cpu").double()
    if allowed is not None:   # constrained logprobs: everything else is -inf from the start
        a = torch.as_tensor(list(allowed), dtype=torch.long)
        y = torch.full_like(y, -math.inf).index_put_((a,), y[a])
    return y


def topk_reference(row: torch.Tensor, K: int, allowed: Optional[Sequence[int]] = None) -> TopK:
    """Float64 log-softmax of a bf16 row, best K ordered value descending then index ascending."""
    y = _raw(row, allowed)
    return _ranked(y, torch.arange(y.numel()), K, torch.logsumexp(y, 0))


def thread_max_candidates(row: torch.Tensor, K: int, allowed: Optional[Sequence[int]] = None) -> int:
    """Finite elements >= the K-th largest per-thread maximum: what the kernel's first collection pass appends.
    More than COLLECT of them send it to the exact search and a second collection."""
    y = _raw(row, allowed)
    S = valid_slots(y.numel())
    pad = torch.full((S * THREADS * VEC,), -math.inf, dtype=torch.float64)
    pad[:y.numel()] = y
    tmax = pad.view(S, THREADS, VEC).amax((0, 2))
    lb = torch.sort(tmax, descending=True).values[K - 1]
    return int(((y >= lb) & (y > -math.inf)).sum())


def check_topk(ids: torch.Tensor, lps: torch.Tensor, ref: TopK, what: str = "") -> None:
    """ids exactly; logprobs within atol 2e-3 + rtol 1e-3 where finite, -inf exactly where not."""
    ids, lps = ids.detach().to("cpu").long(), lps.detach().to("cpu").double()
    assert torch.equal(ids, ref.ids), f"{what}: ids {ids.tolist()} want {ref.ids.tolist()}"
    fin = ref.lps > -math.inf
    assert torch.equal(lps[~fin], ref.lps[~fin]), f"{what}: empty slots hold {lps[~fin].tolist()}"
    err, lim = (lps[fin] - ref.lps[fin]).abs(), LP_ATOL + LP_RTOL * ref.lps[fin].abs()
    assert bool((err <= lim).all()), f"{what}: logprobs {lps.tolist()} want {ref.lps.tolist()}"


def check_topk_tied_tail(ids: torch.Tensor, lps: torch.Tensor, ref: TopK, n_above: int, ties: Sequence[int],
                         what: str = "") -> None:
    """A row whose K-th value is shared by more tokens than fit: the ``n_above`` tokens strictly above the tie
    come first, exactly; the rest carry the tie's logprob, with distinct ids among the tied tokens."""
    K = ref.ids.numel()
    ids_c, lps_c = ids.detach().to("cpu").long(), lps.detach().to("cpu").double()
    check_topk(ids_c[:n_above], lps_c[:n_above], TopK(ref.ids[:n_above], ref.lps[:n_above]), what + " (above the tie)")
    tail = ids_c[n_above:]
    assert tail.unique().numel() == K - n_above and bool(torch.isin(tail, torch.as_tensor(list(ties))).all()), \
        f"{what}: tail ids {tail.tolist()} are not {K - n_above} distinct tied tokens"
    err = (lps_c[n_above:] - ref.lps[n_above:]).abs()
    assert bool((err <= LP_ATOL + LP_RTOL * ref.lps[n_above:].abs()).all()), \
        f"{what}: tail logprobs {lps_c[n_above:].tolist()} want {ref.lps[n_above:].tolist()}"


# ---------------------------------------------------------------------------------------------------------
# top-logprob rows


def overflow_row(V: int, gen: torch.Generator, device="cpu") -> torch.Tensor:
    """bf16 [V]: N(0, 1) background and 100 distinct bf16 values in [8, 16) packed into 10 threads, spread over
    all slots of each: 28 values in each of three threads (descending: the best 28 in the first) and 16 over
    the other seven.  The fifth-largest thread maximum is then about the 87th value, and from the eleventh on
    the thread maxima are background: for K >= 5 the first collection pass meets more than 64 candidates."""
    S = valid_slots(V)
    row = torch.randn(V, generator=gen)
    vals = (8.0 + torch.randperm(128, generator=gen)[:100].double() / 16).sort(descending=True).values
    threads = [0, 63, 64, 100, 200, 300, 400, 500, 511, 555]
    per = [28, 28, 28, 3, 3, 2, 2, 2, 2, 2]
    k = 0
    for t, n in zip(threads, per):
        for i in range(n):
            row[element_index(S - 1 - i % S, t, VEC - 1 - (i // S) % VEC)] = vals[k]   # the best are visited last
            k += 1
    return row.to(torch.bfloat16).to(device)


def tied_three_row(V: int, gen: torch.Generator, device="cpu") -> Tuple[torch.Tensor, List[int]]:
    """bf16 [V]: N(0, 1) background, 9.0 once, then 8.0 three times at tokens the collection visits in DESCENDING
    index order (one wave, the ragged slot: element 0 of thread 302, then element 3 of 301, then element 7 of
    300), then 7.0: the three must come out in ascending index order."""
    S = valid_slots(V)
    row = torch.randn(V, generator=gen)
    ties = [element_index(S - 1, 302, 0), element_index(S - 1, 301, 3), element_index(S - 1, 300, 7)]
    row[element_index(2, 17, 4)] = 9.0
    row[torch.tensor(ties)] = 8.0
    row[element_index(0, 900, 3)] = 7.0
    return row.to(torch.bfloat16).to(device), sorted(ties)


def tie_overflow_row(V: int, n_above: int, device="cpu") -> Tuple[torch.Tensor, List[int], List[int]]:
    """bf16 [V]: 200 tokens at 1.0 on slot 0, element 0 of threads 0..199 (visited first), ``n_above`` distinct
    values 5.0, 4.0, ... on the LAST valid element of threads 1000, 990, ... (wave 15, visited last) and -20
    elsewhere.  Returns (row, the tokens above the tie best first, the tied tokens)."""
    ties = [element_index(0, t, 0) for t in range(200)]
    above = [element_index(last_valid_slot(V, 1000 - 10 * i), 1000 - 10 * i, 7) for i in range(n_above)]
    row = torch.full((V,), -20.0, device=device)
    row[torch.tensor(ties, device=device)] = 1.0
    row[torch.tensor(above, device=device)] = torch.tensor([5.0 - i for i in range(n_above)], device=device)
    return row.to(torch.bfloat16), above, ties


def tie_window_row(V: int, n_ties: int, device="cpu") -> Tuple[torch.Tensor, List[int], List[int]]:
    """bf16 [V]: like ``tie_overflow_row`` with one value above the tie, but the ``n_ties`` tokens at 1.0 fill the
    first elements of threads 10 and 11 only.  Three threads hold everything above the background, so for K > 3
    the bound from the thread maxima is the background and the first collection overflows; after the exact search
    1 + n_ties candidates remain.  While they fit the buffer (n_ties <= 64 - (K - 1)) every tie is held and
    the reported ones are those of lowest index, exactly."""
    S = valid_slots(V)
    half = -(-n_ties // 2)
    assert half <= S * VEC
    ties = sorted(element_index(i % S, t, i // S) for t in (10, 11) for i in range(half))[:n_ties]
    above = [element_index(last_valid_slot(V, 1000), 1000, 7)]
    row = torch.full((V,), -20.0, device=device)
    row[torch.tensor(ties, device=device)] = 1.0
    row[above[0]] = 5.0
    return row.to(torch.bfloat16), above, ties


# ---------------------------------------------------------------------------------------------------------
# wrong references (CPU tests only)


def kept_one_short(ref: Kept) -> Optional[Kept]:
    """The kept set without its least likely token (None: a single token cannot lose one)."""
    if ref.ids.numel() < 2:
        return None
    keep = torch.isin(ref.live_ids, ref.ids)
    keep[ref.live_ids == ref.ids[ref.q.argmin()]] = False
    return _renormalised(ref, keep)


def kept_one_long(ref: Kept) -> Optional[Kept]:
    """The kept set plus the most likely filtered token (None: nothing with mass was filtered)."""
    keep = torch.isin(ref.live_ids, ref.ids)
    if bool(keep.all()):
        return None
    keep[torch.where(keep, torch.zeros_like(ref.live_u), ref.live_u).argmax()] = True
    return _renormalised(ref, keep)


def kept_sort_and_cut(row: torch.Tensor, top_p: float, temperature: float = 1.0) -> Kept:
    """The textbook nucleus: sort, cumulate, cut after the first token that reaches top_p — which splits a tie
    that straddles the cut."""
    ref = kept_reference(row, temperature)
    s, order = torch.sort(ref.live_u, descending=True, stable=True)
    before = torch.cumsum(s, 0) - s
    keep = torch.zeros_like(ref.live_u, dtype=torch.bool)
    keep[order[before < top_p * s.sum()]] = True
    return _renormalised(ref, keep)


def map_slot_thread_swapped(j: int, t: int, e: int, V: int) -> int:
    return (t * instance_slots(V) + j) * VEC + e


def map_halves_swapped(j: int, t: int, e: int, V: int) -> int:
    return element_index(j, t, e ^ 1)


def map_ragged_slot_dropped(j: int, t: int, e: int, V: int) -> int:
    """A sampler that never looks at the ragged slot finds no mass there and answers 0."""
    return 0 if j == valid_slots(V) - 1 else element_index(j, t, e)


WRONG_MAPS: Dict[str, Callable[[int, int, int, int], int]] = {
    "slot_thread_swapped": map_slot_thread_swapped,
    "halves_swapped": map_halves_swapped,
    "ragged_slot_dropped": map_ragged_slot_dropped,
}


def one_hot_answers(V: int, hot: Sequence[int], index_map: Optional[Callable] = None) -> torch.Tensor:
    """What a sampler whose walk rebuilds indices with ``index_map`` returns for one-hot rows."""
    f = index_map or (lambda j, t, e, V: element_index(j, t, e))
    return torch.tensor([f(*element_coords(h), V) for h in hot], dtype=torch.long)


def topk_first_collected(row: torch.Tensor, K: int, exact: bool = True) -> TopK:
    """A top-K that appends every element >= its threshold in visit order (slot, then element, then thread) into
    COLLECT slots, drops what arrives later and ranks what it holds.  The threshold is the K-th largest value
    (``exact``: only ties at it can overflow) or the K-th largest thread maximum (a kernel without the exact
    search)."""
    y = _raw(row)
    if exact:
        thr = torch.sort(y, descending=True).values[K - 1]
    else:
        S = valid_slots(y.numel())
        pad = torch.cat([y, torch.full((S * THREADS * VEC - y.numel(),), -math.inf, dtype=torch.float64)])
        thr = torch.sort(pad.view(S, THREADS, VEC).amax((0, 2)), descending=True).values[K - 1]
    cand = ((y >= thr) & (y > -math.inf)).nonzero()[:, 0]
    j, t, e = cand // (THREADS * VEC), (cand // VEC) % THREADS, cand % VEC
    first = cand[torch.argsort((j * VEC + e) * THREADS + t)[:COLLECT]]
    return _ranked(y, first, K, torch.logsumexp(y, 0))
