"""Structured inputs ("score programmes") for the attention kernels, and deliberately wrong references.

The oracle of every attention test stays ``torch_ref.attention`` on the bf16 tensors the kernel gets; only
the inputs change.  A query row is ONE-HOT (amplitude ``AMP`` in one dimension ``c``), so its score against
key ``t`` is ``AMP * K[t, kvh, c] * scale`` and column ``c`` of K is a programme of scores for that row alone.
Rows that share a KV head (heads of a GQA group, query tokens of a prefill tile, sequences of a cascade
super-tile) take different columns and therefore different programmes; the remaining K columns stay random
(loaded and multiplied by zeros).

Programmes (``Prog.kind``):
  stair  score = 0.25 * AMP * scale nats per key (0.354 at head_dim 128, 0.5 at 64), rising with t: every
         32-key tile beats the running max by > 8 log2 units, so every tile takes the lazy-rescale branch
         with a live accumulator, the last visible key weighs most and a leaked later key outweighs all.
         (slope -1: falling, for kernels that do not walk the keys front to back.)
         The K values 0.25 * (t - anchor) are bf16-exact for |t - anchor| <= 256.
  spike  key ``at`` is SPIKE_NATS above an N(0, 1) background: the output is V[at].
  flat   column of zeros: every score is exactly 0, P = 1, l = count, output = mean(V).  With small integer
         V the kernel's sums are exact and its only rounding is the bf16 store.
  bg     N(0, 1) scores: the control row that must not move when a neighbour rescales.

The second half holds what the CPU tests need to show that these inputs would notice a broken kernel:
``softmax_out`` with a key dropped or counted twice, and ``emulate``, the kernels' tiled log2-domain
recurrence (32-key tiles, lazy rescale, bf16 P, bf16 output) with switches that break it.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

AMP = 16.0          # one-hot amplitude (bf16-exact)
SPIKE_NATS = 30.0
LOG2E = 1.4426950408889634
LAZY_LOG2 = 8.0     # kLazyRescale of both kernels
TILE = 32           # keys per softmax step: a block pair (decode) or a key tile (prefill)
ATOL, RTOL = 2e-2, 2e-2      # the suite's attention bound (V ~ N(0, 1))
FLAT_RTOL = 2.0 ** -8        # flat rows, integer V: one bf16 rounding (2^-9) with a factor of 2; atol 0


class Prog(NamedTuple):
    kind: str            # "stair" | "spike" | "flat" | "bg"
    at: int = -1         # spike: key position
    anchor: int = 0      # stair: key position whose score is 0
    slope: int = 1       # stair: +1 rises with the key position, -1 falls


def probe_dims(D: int) -> List[int]:
    """All D dimensions, ordered so that consecutive entries walk the MFMA k-steps first, then the lane
    groups, then the element: dimension 32 s + 8 g + j lives in k-step s, lane group g, element j."""
    S = D // 32
    return [32 * (i % S) + 8 * ((i // S) % 4) + i // (4 * S) for i in range(D)]


def one_hot(cols: Sequence[int], D: int) -> torch.Tensor:
    """bf16 [len(cols), D] query rows: AMP in the row's column, zero elsewhere."""
    q = torch.zeros(len(cols), D)
    q[torch.arange(len(cols)), torch.tensor(list(cols))] = AMP
    return q.to(torch.bfloat16)


def k_column(prog: Prog, t: torch.Tensor, scale: float, gen: torch.Generator) -> torch.Tensor:
    """fp32 values of a K column at key positions ``t`` (int64) that give a one-hot row this programme."""
    nat = 1.0 / (AMP * scale)  # K value worth one nat of score
    if prog.kind == "flat":
        return torch.zeros(t.numel())
    if prog.kind == "stair":
        return 0.25 * prog.slope * (t - prog.anchor).float()
    vals = torch.randn(t.numel(), generator=gen) * nat
    if prog.kind == "spike":
        vals[t == prog.at] = SPIKE_NATS * nat
    else:
        assert prog.kind == "bg", prog.kind
    return vals


def int_values(shape, gen: torch.Generator) -> torch.Tensor:
    """bf16 tensor of non-zero integers in +-1..8 (sums of a few thousand are exact in fp32)."""
    mag = torch.randint(1, 9, tuple(shape), generator=gen).float()
    sign = torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 - 1
    return (mag * sign).to(torch.bfloat16)


def nonzero_prefix_sums(v: torch.Tensor, carry: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``v`` [L, ...] of int_values with the sign of a key flipped wherever the running sum over keys (started
    from ``carry``, the sum of the keys before) would reach 0.  An exact mean of 0 cannot be compared at
    atol = 0: the fp32 reference itself, and any path that combines partial results in floating point
    (split-K), return ~1e-8 there.  Every prefix of the keys then has a mean of at least 1/L in magnitude, far
    above either error (~1e-7 absolute), and still cancels to about |v| / sqrt(L), where one key shows."""
    v = v.clone().float()
    run = torch.zeros(v.shape[1:]) if carry is None else carry.clone().float()
    for t in range(v.shape[0]):
        v[t] = torch.where(run + v[t] == 0, -v[t], v[t])
        run = run + v[t]
        assert (run != 0).all()
    return v.to(torch.bfloat16)


def decode_programmes(L: int, splits: int) -> List[Prog]:
    """Programmes of a plain-decode context of L keys: staircase, flat, background and a spike at every edge
    key — block, pair and context edges, and the first and last key of every split range."""
    at = sorted(p for p in {0, 15, 16, 31, 32, L - 2, L - 1, *split_edges(L, splits)} if 0 <= p < L)
    return [Prog("stair", anchor=L // 2), Prog("flat"), Prog("bg")] + [Prog("spike", at=p) for p in at]


def cascade_programmes(pblk: int) -> List[Prog]:
    """Programmes of the rows of a cascade group with ``pblk`` shared blocks, as functions of the row's own
    context length: entries are ``Prog`` or callables L -> Prog.  Spikes sit on both sides of the prefix /
    suffix boundary, on the first and the last key, and (prefix longer than one 256-key LDS chunk) on both
    sides of the chunk edge.  The staircase is anchored at the boundary, so it rises through it.  A prefix of
    one chunk is attended BETWEEN the suffix pairs (suffix pair, prefix pair, suffix pair, ...), where a rising
    staircase never beats the first suffix pair by a whole tile; there a falling staircase is added, whose
    first prefix pair towers over the suffix pair already accumulated.  The count is odd for every prefix, so
    with 16/G sequences of G consecutive programmes per wave no two sequences of a wave get the same ones."""
    pctx = 16 * pblk
    progs = [Prog("stair", anchor=pctx), Prog("spike", at=pctx), Prog("spike", at=0), Prog("flat"), Prog("bg"),
             Prog("spike", at=max(pctx - 1, 0)), lambda L: Prog("spike", at=L - 1)]
    if pctx > 256:
        progs += [Prog("spike", at=255), Prog("spike", at=256)]
    elif pctx:
        progs += [Prog("spike", at=16), Prog("stair", anchor=pctx, slope=-1)]
    return progs


def prefill_programmes(kl: int, qoff: int) -> List[Prog]:
    """Programmes of the K columns of a prefill sequence with kl keys whose first query sits at key qoff:
    staircase, flat, background, and spikes at the first and last key, at the first query's own key and on
    both sides of the 32-key tile edge and of the 64-query workgroup edge."""
    at = sorted(p for p in {0, qoff, 31, 32, 63, 64, qoff + 31, qoff + 32, qoff + 63, qoff + 64, kl - 1}
                if 0 <= p < kl)
    return [Prog("stair", anchor=kl // 2), Prog("flat"), Prog("bg")] + [Prog("spike", at=p) for p in at]


def build_wave(progs: Sequence[Prog], n_keys: int, D: int, scale: float, gen: torch.Generator):
    """One-hot rows q [R, D] and keys k [n_keys, D] (bf16, one KV head) with programme r in column
    probe_dims(D)[r]; the other columns of k are N(0, 1)."""
    cols = probe_dims(D)[:len(progs)]
    k = torch.randn(n_keys, D, generator=gen)
    t = torch.arange(n_keys)
    for c, prog in zip(cols, progs):
        k[:, c] = k_column(prog, t, scale, gen)
    return one_hot(cols, D), k.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------
# conditions read off the reference's own scores


def scores_nats(q: torch.Tensor, k: torch.Tensor, scale: float) -> torch.Tensor:
    """fp64 scores [R, L] of query rows q [R, D] against keys k [L, D] (the bf16 tensors, exactly)."""
    return q.double() @ k.double().t() * scale


def key_weight(s: torch.Tensor, p: int) -> float:
    """Softmax weight of key p under the visible scores s [L] (nats, -inf = masked)."""
    return float(torch.softmax(s.double(), 0)[p])


def tiles_of(L: int, start: int = 0) -> List[Tuple[int, int]]:
    return [(a, min(a + TILE, L)) for a in range(start, L, TILE)]


def forced_rescales(s: torch.Tensor, tiles: Sequence[Tuple[int, int]]) -> int:
    """Number of tiles, in processing order, whose largest visible score exceeds EVERY earlier visible score
    by more than LAZY_LOG2 log2 units while earlier visible keys exist.  The kernels' running max never
    exceeds the true one, so each such tile takes the rescale branch with a non-empty accumulator whatever
    the other rows of its wave do."""
    s2 = s.double() * LOG2E
    seen, n = -math.inf, 0
    for a, b in tiles:
        if b <= a:
            continue
        mx = float(s2[a:b].max())
        if mx == -math.inf:
            continue
        if seen > -math.inf and mx > seen + LAZY_LOG2:
            n += 1
        seen = max(seen, mx)
    return n


def stair_rises(tiles: Sequence[Tuple[int, int]], scale: float, slope: int = 1) -> int:
    """What a staircase promises for ``tiles`` of VISIBLE keys in processing order: the number of tiles whose
    top step clears every earlier tile's by more than LAZY_LOG2 (a rise of 16 keys at head_dim 128, 12 at 64).
    ``forced_rescales`` of the reference's scores must confirm it."""
    step = 0.25 * AMP * scale * LOG2E
    n, top = 0, None
    for a, b in tiles:
        if b <= a:
            continue
        t = (b - 1) if slope > 0 else -a
        if top is not None and (t - top) * step > LAZY_LOG2:
            n += 1
        top = t if top is None else max(top, t)
    return n


def decode_tiles(L: int, splits: int, path: str) -> List[List[Tuple[int, int]]]:
    """Key ranges of the block pairs each softmax state of a plain decode walks, in order: one state per
    (split, wave) in the 4-wave kernel ("wg4": wave w takes every fourth pair), one per split in the
    wave-per-item kernel ("wave").  Empty lists are states that see no key."""
    nblk = -(-L // 16)
    per = -(-nblk // splits)
    out = []
    for sp in range(splits):
        b0, b1 = sp * per, min(nblk, sp * per + per)
        pairs = [(16 * b, min(16 * min(b + 2, b1), L)) for b in range(b0, b1, 2)]
        if path == "wg4":
            out += [pairs[w::4] for w in range(4)]
        else:
            out.append(pairs)
    return out


def split_edges(L: int, splits: int) -> List[int]:
    """First and last key of every non-empty split range of a context of L keys."""
    nblk = -(-L // 16)
    per = -(-nblk // splits)
    edges = []
    for sp in range(splits):
        b0, b1 = sp * per, min(nblk, sp * per + per)
        if b0 < b1:
            edges += [16 * b0, min(16 * b1, L) - 1]
    return edges


def cascade_row_tiles(pblk: int, ctxs: Sequence[int], j: int, chunk_blocks: int = 16) -> List[Tuple[int, int]]:
    """Key ranges, in processing order, that reach the rows of sequence ``j`` of a cascade wave whose
    sequences have contexts ``ctxs`` and share ``pblk`` prefix blocks.  A prefix of more than one LDS chunk
    is attended first, pair by pair; a shorter one is interleaved: after every suffix pair of ANY of the
    wave's sequences comes the next prefix pair, and what is left follows the last suffix pair."""
    pctx = 16 * pblk
    prefix = [(16 * b, min(16 * (b + 2), pctx)) for b in range(0, pblk, 2)]
    walk = []  # (sequence, key range) of every suffix pair the wave walks
    for i, L in enumerate(ctxs):
        end = -(-L // 16)
        walk += [(i, (16 * b, min(16 * min(b + 2, end), L))) for b in range(pblk, end, 2)]
    own = [r for i, r in walk if i == j]
    if pblk > chunk_blocks:
        return prefix + own
    out, pre = [], 0
    for i, r in walk:
        if i == j:
            out.append(r)
        if pre < len(prefix):
            out.append(prefix[pre])
            pre += 1
    return out + prefix[pre:]


# ---------------------------------------------------------------------------------------------------------
# comparisons


def violations(got: torch.Tensor, want: torch.Tensor, atol: float, rtol: float) -> torch.Tensor:
    """Elements outside |got - want| <= atol + rtol |want| (non-finite elements included)."""
    got, want = got.double(), want.double()
    return ~((got - want).abs() <= atol + rtol * want.abs())


def accepted(got: torch.Tensor, want: torch.Tensor, atol: float = ATOL, rtol: float = RTOL) -> bool:
    return not bool(violations(got, want, atol, rtol).any())


def assert_close(got: torch.Tensor, want: torch.Tensor, atol: float, rtol: float, what: str = "") -> None:
    bad = violations(got, want, atol, rtol)
    if bad.any():
        err = (got.double() - want.double()).abs()
        idx = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound (atol {atol}, rtol {rtol:.3g}); "
                             f"max err {float(err[bad].max()):.4g}; first at {idx}: "
                             f"got {float(got[tuple(idx)]):.6g} want {float(want[tuple(idx)]):.6g}")


# ---------------------------------------------------------------------------------------------------------
# wrong references (CPU tests only)


def softmax_out(s: torch.Tensor, v: torch.Tensor, drop: Optional[int] = None, double: Optional[int] = None):
    """fp64 attention output [R, D] from scores s [R, L] (nats, -inf = masked) and values v [L, D]; ``drop``
    removes a key, ``double`` counts one twice.  A leaked key is a score the caller leaves unmasked."""
    s = s.double().clone()
    if drop is not None:
        s[:, drop] = -math.inf
    w = torch.exp(s - s.max(1, keepdim=True).values)
    if double is not None:
        w[:, double] *= 2
    return (w @ v.double()) / w.sum(1, keepdim=True)


def emulate(s: torch.Tensor, v: torch.Tensor, tiles: Optional[Sequence[Tuple[int, int]]] = None, *,
            skip_o_rescale: bool = False, alpha_shift: int = 0, state: bool = False) -> torch.Tensor:
    """The kernels' recurrence for the rows of one wave: s [R, L] scores (nats, -inf = masked), v [L, D] bf16
    values, ``tiles`` = key ranges in processing order (default: 32-key tiles from 0).  fp32 state in the log2
    domain; the running max m moves, and O and l are rescaled, only when some row's tile max exceeds its m by
    more than LAZY_LOG2 (one decision for the whole wave); P is rounded to bf16 for P V but summed unrounded
    into l; the output is rounded to bf16.  ``skip_o_rescale`` leaves O unscaled in that branch;
    ``alpha_shift`` = n scales row r of O by the alpha of row r - n.  ``state``: return the fp32 (o / l, l) before
    the bf16 store (what the cascade kernel's MX epilogue quantises)."""
    R, L = s.shape
    s2 = (s.double() * LOG2E).float()
    vf = v.float()
    m = torch.full((R,), -1e30)
    l = torch.zeros(R)
    o = torch.zeros(R, v.shape[1])
    for a, b in (tiles if tiles is not None else tiles_of(L)):
        st = s2[:, a:b]
        mx = st.max(1).values.clamp_min(-1e30)
        if bool((mx > m + LAZY_LOG2).any()):
            m_new = torch.maximum(m, mx)
            alpha = torch.exp2(m - m_new)
            l = l * alpha
            m = m_new
            if not skip_o_rescale:
                o = o * torch.roll(alpha, alpha_shift)[:, None]
        p = torch.exp2(st - m[:, None])
        l = l + p.sum(1)
        o = o + p.to(torch.bfloat16).float() @ vf[a:b]
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    if state:
        return o * inv[:, None], l
    return (o * inv[:, None]).to(torch.bfloat16).float()
