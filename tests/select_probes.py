"""Exact inputs, fp64 / integer oracles, sentinel cages and deliberately wrong references for the scoring kernels
(csrc/kernels/consensus.hip: pool_l2norm, cosine_consensus, knn_topk, vote_tally) and the MoE selection and
dispatch kernels (csrc/kernels/moe.hip: moe_route, moe_router, moe_combine).  All seven select or reduce: what
goes wrong is a tie broken the wrong way, one element left out of a sum, an index off by one at a block boundary.

``rne``, ``bitwise``, ``one_step``, ``steps``, ``SENTINEL`` and ``poison_a`` are those of tests/gemm_probes.py,
``RowCage``, ``SENT32``, ``one_step_cond`` and the spike constants those of tests/rowwise_probes.py.

Rules
-----
bitwise (``same32`` for fp32 / int32 outputs, ``bitwise`` for bf16) wherever the result is determined:

  * exact families: small integers or +-2^e chosen so that every product and every partial sum is exact in fp32 in
    ANY order; the bound max|term| * count < 2^24 (in units of the smallest term) stands next to each family
    below and tests/test_select_probes.py evaluates it for every shape used;
  * values the kernel computes in a fixed serial order, reproduced on the CPU in fp32 in that order from the
    kernel's own earlier output: the centrality (sum over j ascending of S_ij, the diagonal replaced by +0, then
    one division by n - 1).  The build passes no fast-math flag and hipcc's default fp32 division is correctly
    rounded, so ``s / (n - 1)`` is the IEEE quotient, which torch computes on the CPU when both operands are
    tensors (a Python-scalar divisor may be turned into a reciprocal multiply: ``_div`` avoids it);
  * every index output (``best``, kNN rows, expert ids, ``row_off``): a STABLE descending sort of the exact scores,
    so ties go to the lower index; ``first_max`` for an arg-max.

derived bounds, counting one rounding (2^-24 relative) per fp32 operation, one ulp (2^-23) for v_rsq_f32 and
v_exp_f32, and |x| 2^-24 for a rounded exponent argument; no tolerance is taken from what a kernel returns.

  W_ERR(X)   relative error of a softmax weight w_i = e_i / sum_j e_j with e_i = __expf(a_i), a_i = x_i - max,
             X >= every |x_i| (cosine_consensus: |cen_i * inv_tau|; the routers: |logit|, so |a_i| <= 2 X).
             The rounding of ``max`` is common to every term and cancels in the quotient.  Per term:
               x_i = cen_i * inv_tau rounded            X 2^-24         (absolute, in the exponent)
               a_i = x_i - max rounded                  2 X 2^-24
               a_i * log2(e) rounded (__expf = exp2)    2 X 2^-24
               log2(e) held in fp32 (2^-26 relative)    2 X 2^-26 < X 2^-24
               v_exp_f32                                2^-23 = 2 * 2^-24  (relative)
             so e_i = exp(a_i)(1 + t), |t| <= (6 X + 2) 2^-24.  The denominator adds at most 4 serial adds per
             thread and 6 + 4 levels of shuffles (n <= 1024 over 256 threads; the routers: k <= 8 serial adds) of
             positive terms: 14 * 2^-24; the division one more.  w_i is off by at most
             (2 (6 X + 2) + 14 + 1) 2^-24 < (12 X + 20) 2^-24 = W_ERR(X).  A term below the normal range may be
             flushed: the absolute floor W_FLOOR = 2^-126 is added.  tau = 0.001, |cen| <= 1.01: X = 1010,
             W_ERR = 7.2e-4; routing logits within +-2: W_ERR(2) = 2.6e-6.
             Sum of the weights: the e_i of numerator and denominator are the same numbers; summing n of them
             takes at most n - 1 inexact additions in any tree ((n - 1) 2^-24) and the n quotients round by at
             most 2^-24 of their sum: |sum_i w_i - 1| <= n 2^-24 < n 2^-23, the bound used.
  POOL_ERR   relative error of out[c] = pooled[c] * rsqrtf(ss), ss = sum_c pooled[c]^2 over d <= 4096 columns:
               pooled[c] = acc / len                    1     (exact for CLS / LAST)
               ss: the same rounding, squared           2
                   each square                          1
                   <= 16 serial adds per thread         16    (4096 / 256)
                   6 + 4 levels of shuffles / LDS       10
               rsqrt halves the 29 above                14.5
               v_rsq_f32                                2
               the product                              1
             in units of 2^-24: 1 + 14.5 + 2 + 1 = 18.5, below POOL_ERR = 2^-19 (32 units, 1.9e-6).  An exactly
             zero reference must come out as zero.  The bf16 output is RNE of that fp32 value: 2^-19 << 2^-9, so
             ``one_step`` of the fp64 reference.
  S bound    |S_ij - <E_i, E_j>| <= d 2^-24 || |E_i| || || |E_j| ||: d accumulations, each rounding a partial sum
             that is at most sum_k |E_ik E_jk| <= || |E_i| || || |E_j| || (Cauchy-Schwarz); the products of two bf16
             numbers are exact in fp32.  No tighter bound is claimed: the MFMA's internal order is not documented.
  combine    out = RNE_bf16(sum_j w_j y_j) over k <= 8 terms: k products and k adds, each relative to at most
             mag = sum_j |w_j y_j|: error <= (k + 1) 2^-24 mag < COMBINE_ERR mag, COMBINE_ERR = 2^-20.  The terms
             of the random family cancel (y ~ N(0, 1)), so the rule is ``one_step_cond``: plain one_step wherever
             |want| >= 2^10 COMBINE_ERR mag = 2^-10 mag (the error is then below 2^-10 |want|, under the half step
             of the store), the absolute bound COMBINE_ERR mag + one bf16 step on the few outputs that cancel
             harder (about 1 in 1000; asserted to be under 5 %).  Plain one_step of the fp64 sum is not a rule an
             fp32 kernel can keep there: the unfused fp32 emulation of tests/test_select_probes.py is 22 codes off
             at one cancelling output of the (300, 8, 2056) case and within a code everywhere else; the GPU test
             prints how plain one_step fared for the kernel.

Input families
--------------
pool_l2norm
  spike walk   one sequence per row (cu = arange, the form DecoderEmbedder.embed uses): zero except SPIKE at
               FIXED_COL and +-SPIKE at a column that walks EVERY column of the row (the kernel is a thread per
               column).  v / |v| is +-2^-1/2 at the two spikes and exactly 0 elsewhere; a column left out of
               the pooling or of ss gives 1 or 0 there.
  integer seqs rows of integers within +-8, lengths POOL_LENS = 3, 1, 0, 30, 2, 1 (the last row all zero):
               column sums <= 8 * 30 = 240 < 2^24 are exact, so the pooled numerator is.  A range off by one at
               either end, LAST reading t1, a lost row stride move the unit vector by tens of percent.
  framed       any of these as the [:T, :d] view of a buffer with ld = d + 8 whose padding columns and two
               trailing rows hold the NaN sentinel.
cosine_consensus
  sign         E = +-1; ``scaled``: row i times 2^(i % 5 - 2).  Terms are multiples of 2^-4 of magnitude <= 16,
               so S (d terms) needs 256 d < 2^24 and the centrality sum (n d terms) 256 n d < 2^24, i.e.
               n d < 65536: the largest cases are 33 x 1024 and 1024 x 32.  ``plant_tie`` copies the best row
               (scale included) over other rows until the maximum centrality is attained at least twice.
  unit rows    normalize(randn) rounded to bf16; ``clustered`` adds a common direction (cosines around 0.5, as
               answers to one question have): cen / tau reaches 500 at tau = 0.001, where exp overflows unless
               the maximum is subtracted.  Plain random rows at d >= 384 have |cen| / tau < 88 too often to show it.
knn_topk
  integers     E, q integers within +-8 as fp32, |dot| <= 64 d <= 24576 < 2^24; ``wide``: +-64 at d = 64,
               |dot| <= 4096 * 64 = 2^18.  Row n - 1 is made the unique best row 8 sign(q) (it lives in the last,
               partial slab and in the last merge group).
  equal        all rows equal: rows 0 .. k - 1 in order.
  negative     q >= 1, E <= -1: a missing row scored 0 instead of -inf would win.
  slab tie     rows 250 .. 250 + 2k (clamped to n) all equal to the best possible row: the winners straddle
               the slab boundary at 256.
  group tie    the same block from row (4096 // k) * 256 - k, the boundary of the first merging workgroup, at
               the shapes where that boundary is below n.
moe_route      logits multiples of 0.5 within +-2 (bf16-exact); every row is built so that its k-th and
               (k + 1)-th largest are equal; one row of equal logits; one row with -inf in its lowest experts
               while k stay finite; one row whose last expert is the only maximum.
moe_router
  sign         h, router = +-1; ``scaled``: row t of h times 2^(t % 5 - 2), router row e times 2^(e % 3 - 1):
               terms multiples of 2^-3 of magnitude <= 8, d <= 4096 of them: 64 * 4096 = 2^18 < 2^24.
  one-hot      row t of h holds one N(0, 1) bf16 value at column 8 c + c % 8 of chunk c; the logit is the
               16-bit product h * r, exact in fp32: bitwise RNE(h r), a full-mantissa value at the store.
moe_combine
  exact        Y integers within +-16, w from {1, 0.5, 0.25, 0}: terms multiples of 0.25 of magnitude <= 16, k <= 8
               of them: 64 * 8 < 2^24, exact fused or not.  ``fine``: w from {W_FINE, 0.25, 0} with
               W_FINE = 0.5 (1 + 3 * 2^-9), an fp32 number that bf16 cannot hold: terms multiples of 2^-10,
               2^14 * 8 < 2^24.  Shows weights that went through bf16, which {1, 0.5, 0.25, 0} cannot.
  one-hot      a single weight 1 per token: a bitwise row copy of distinct bf16 codes.
  random       Y ~ N(0, 1), w a softmax: ``one_step_cond`` as derived above.

The last part holds plain torch emulations of each kernel's contract with switches that break them in one way
each; tests/test_select_probes.py shows that the honest emulation passes and every mutant is rejected.
"""
from __future__ import annotations

import itertools
from typing import List, Optional, Sequence, Tuple

import torch

from tests.gemm_probes import SENTINEL, _signs, bits, bitwise, one_step, poison_a, rne, steps  # noqa: F401
from tests.rowwise_probes import (BF, FIXED_COL, SENT32, SPIKE, RowCage, distinct, one_step_cond,  # noqa: F401
                                  walk_cols)

POOL_ERR = 2.0 ** -19
W_FLOOR = 2.0 ** -126
COMBINE_ERR = 2.0 ** -20
W_FINE = 0.5 * (1 + 3 * 2.0 ** -9)
POOL_LENS = [3, 1, 0, 30, 2, 1]
POOL_WALK_DS = [8, 256, 264, 1000, 4096]
CONS_DS, CONS_NS, CONS_RS = [32, 96, 1024], [1, 2, 15, 16, 17, 33], [1, 3]
CONS_BIG = (1, 1024, 32)                       # (R, n, d)
KNN_SHAPES = [(1, 1), (64, 64), (255, 7), (256, 64), (257, 64), (300, 33), (513, 3), (16385, 64), (1048577, 64),
              (70000, 1)]
ROUTE_SHAPES = [(1, 1, 1), (1, 2, 2), (255, 6, 2), (256, 8, 2), (257, 8, 3), (300, 9, 8), (300, 16, 4), (300, 17, 1),
                (77, 33, 8), (300, 64, 8), (4096, 8, 2), (4097, 8, 2), (8193, 8, 1), (1025, 64, 8)]
ROUTER_DS = [8, 256, 2048, 2056, 4096]
ROUTER_TS = [1, 3, 4, 5, 130]
ROUTER_EK = [(6, 2), (8, 2), (8, 3), (9, 4), (16, 4)]
COMBINE_TS, COMBINE_KS, COMBINE_DS = [1, 5, 300], [1, 2, 8], [8, 2048, 2056]


def W_ERR(x_max: float) -> float:
    return (12.0 * x_max + 20.0) * 2.0 ** -24


def same32(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Mask of 4-byte outputs (fp32 / int32) whose bits differ."""
    return got.contiguous().view(torch.int32) != want.to(got.device).to(got.dtype).contiguous().view(torch.int32)


def _div(a: torch.Tensor, b: float) -> torch.Tensor:
    """IEEE fp32 division of every element by ``b`` (tensor / tensor)."""
    return a.float() / torch.full_like(a, float(b), dtype=torch.float32)


def first_max(c: torch.Tensor) -> torch.Tensor:
    """Index of the first maximum along the last dimension."""
    n = c.shape[-1]
    idx = torch.arange(n).expand(c.shape)
    return torch.where(c == c.max(-1, keepdim=True).values, idx, n).min(-1).values


def stable_topk(scores: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values, indices) of the k largest along the last dimension, ties to the lower index, best first."""
    v, i = torch.sort(scores, dim=-1, descending=True, stable=True)
    return v[..., :k], i[..., :k]


def framed(x: torch.Tensor, pad_cols: int = 0, pad_rows: int = 2, device=None) -> torch.Tensor:
    """x [T, d] bf16 as the [:T, :d] view of a sentinel-filled [T + pad_rows, d + pad_cols] buffer."""
    T, d = x.shape
    buf = torch.empty(T + pad_rows, d + pad_cols, dtype=BF, device=device if device is not None else x.device)
    bits(buf).fill_(SENTINEL)
    buf[:T, :d] = x.to(buf.device)
    return buf[:T, :d]


def tail_cage(n: int, dtype, device="cpu", extra: int = 24) -> RowCage:
    """A flat output of n + extra elements in a RowCage: a kernel that is told n must leave the tail alone."""
    return RowCage((n + extra,), device=device, dtype=dtype)


def tail_touched(cage: RowCage, n: int) -> int:
    return int((cage.view[n:].view(cage.raw_dtype) != cage.code).sum()) + cage.outside_touched()


# ---------------------------------------------------------------------------------------------------------
# pool_l2norm


def pool_cols(d: int) -> List[int]:
    return [c for c in range(d) if c != FIXED_COL]


def pool_walk(d: int, cols: Sequence[int]) -> torch.Tensor:
    """[len(cols), d] bf16: SPIKE at FIXED_COL, +-SPIKE (odd rows negative) at cols[i], zero elsewhere."""
    assert FIXED_COL not in cols and max(cols) < d
    x = torch.zeros(len(cols), d)
    x[:, FIXED_COL] = SPIKE
    r = torch.arange(len(cols))
    x[r, torch.tensor(list(cols))] = torch.where(r % 2 == 1, -SPIKE, SPIKE)
    return x.to(BF)


def pool_seqs(d: int, gen: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """(hidden [36 + 1, d] bf16 integers within +-8 with an all-zero last row, cu [7] int32) for POOL_LENS."""
    T = sum(POOL_LENS)
    h = torch.randint(-8, 9, (T, d), generator=gen).float()
    h[-1] = 0
    cu = torch.tensor([0] + list(itertools.accumulate(POOL_LENS)), dtype=torch.int32)
    assert 8 * max(POOL_LENS) < (1 << 24)
    return h.to(BF), cu


def pool_want(h: torch.Tensor, cu: torch.Tensor, mode: int) -> torch.Tensor:
    """fp64 v / |v| per sequence (0 = CLS, 1 = mean, 2 = last); zero-length sequences and zero vectors give 0."""
    h, out = h.double().cpu(), []
    for s in range(cu.numel() - 1):
        t0, t1 = int(cu[s]), int(cu[s + 1])
        if t1 <= t0:
            v = torch.zeros(h.shape[1], dtype=torch.float64)
        else:
            v = h[t0] if mode == 0 else (h[t1 - 1] if mode == 2 else h[t0:t1].sum(0) / (t1 - t0))
        nrm = v.norm()
        out.append(v / nrm if nrm > 0 else v * 0)
    return torch.stack(out)


def pool_violations(of: torch.Tensor, ob: Optional[torch.Tensor], want: torch.Tensor) -> List[str]:
    out, w = [], want.double().to(of.device)
    g = of.double()
    bad = ~torch.isfinite(g) | ((g - w).abs() > POOL_ERR * w.abs())
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        out.append(f"{int(bad.sum())} of {bad.numel()} fp32 outputs off POOL_ERR; first at {list(i)}: got "
                   f"{float(g[i]):.9g} want {float(w[i]):.9g}")
    if ob is not None:
        bad = one_step(ob, w)
        if bool(bad.any()):
            out.append(f"{int(bad.sum())} of {bad.numel()} bf16 outputs fail one_step")
    return out


# ---------------------------------------------------------------------------------------------------------
# cosine_consensus


def sign_rows(R: int, n: int, d: int, gen: torch.Generator, scaled: bool = False) -> torch.Tensor:
    """E [R, n, d] bf16 of +-1 (``scaled``: row i times 2^(i % 5 - 2)), other signs in every request."""
    assert 256 * n * d < (1 << 24)
    E = _signs((R, n, d), gen)
    if scaled:
        E = E * torch.exp2((torch.arange(n) % 5 - 2).float())[None, :, None]
    return E.to(BF)


def gram(E: torch.Tensor) -> torch.Tensor:
    """The exact Gram matrix of a sign family as fp64, through int64 (entries of 4 E are integers)."""
    Ei = (E.double() * 4).long()
    assert bool((Ei.double() == E.double() * 4).all())
    return (Ei @ Ei.transpose(1, 2)).double() / 16


def cen_exact(S: torch.Tensor) -> torch.Tensor:
    """fp32(exact off-diagonal row sum) / fp32(n - 1): one correctly rounded division; 1 for a sole candidate."""
    n = S.shape[-1]
    if n == 1:
        return torch.ones(S.shape[0], 1)
    s = S.double().sum(-1) - S.double().diagonal(dim1=1, dim2=2)
    assert bool((s.float().double() == s).all())
    return _div(s.float(), n - 1)


def cen_serial(S: torch.Tensor) -> torch.Tensor:
    """The kernel's order in fp32: j ascending, +0 on the diagonal, then the division."""
    S = S.float().cpu()
    R, n, _ = S.shape
    if n == 1:
        return torch.ones(R, 1)
    s = torch.zeros(R, n)
    for j in range(n):
        col = S[:, :, j].clone()
        col[:, j] = 0.0
        s = s + col
    return _div(s, n - 1)


def plant_tie(E: torch.Tensor) -> torch.Tensor:
    """Copy the best row of every request over further rows until the best centrality is attained twice."""
    E = E.clone()
    R, n, _ = E.shape
    if n < 2:
        return E
    for r in range(R):
        b = int(first_max(cen_exact(gram(E[r:r + 1])))[0])
        for m in dict.fromkeys([n // 2] + list(range(1, n))):
            E[r, (b + m) % n] = E[r, b]
            c = cen_exact(gram(E[r:r + 1]))[0]
            if int((c == c.max()).sum()) >= 2 and bool(c[b] == c.max()):
                break
    return E


def unit_rows(R: int, n: int, d: int, gen: torch.Generator, clustered: bool = False) -> torch.Tensor:
    x = torch.randn(R, n, d, generator=gen)
    if clustered:
        x = x + torch.randn(R, 1, d, generator=gen)
    return torch.nn.functional.normalize(x, dim=-1).to(BF)


def s_bound(E: torch.Tensor) -> torch.Tensor:
    nrm = E.double().abs().norm(dim=-1)
    return E.shape[-1] * 2.0 ** -24 * nrm[:, :, None] * nrm[:, None, :]


def softmax_violations(w: torch.Tensor, x: torch.Tensor, x_max: float, what: str = "weights") -> List[str]:
    """w against the fp64 softmax of x (last dimension) under W_ERR(x_max), and their sum against 1."""
    out, w64 = [], w.double().cpu()
    want = torch.softmax(x.double().cpu(), -1)
    bad = ~torch.isfinite(w64) | ((w64 - want).abs() > W_ERR(x_max) * want + W_FLOOR)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        out.append(f"{int(bad.sum())} of {bad.numel()} {what} off W_ERR({x_max:g}); first at {list(i)}: got "
                   f"{float(w64[i]):.9g} want {float(want[i]):.9g}")
    n = w.shape[-1]
    off = (w64.sum(-1) - 1).abs()
    if not bool((off <= n * 2.0 ** -23).all()):
        out.append(f"{what} sum to 1 +- {float(off.max()):.3g}, allowed {n * 2.0 ** -23:.3g}")
    return out


def inv_tau32(tau: float) -> float:
    return float(torch.tensor(1.0 / float(tau), dtype=torch.float32))


def consensus_exact_violations(S, cen, best, E) -> List[str]:
    """Sign families: S, centrality and best are all determined."""
    out, G = [], gram(E.cpu())
    S, cen, best = S.float().cpu(), cen.float().cpu(), best.cpu().long()
    if bool(same32(S, G.float()).any()):
        out.append(f"{int(same32(S, G.float()).sum())} entries of S differ from the integer Gram matrix")
    want = cen_exact(G)
    if bool(same32(cen, want).any()):
        out.append(f"{int(same32(cen, want).sum())} centralities differ from fp32(sum) / (n - 1)")
    if not torch.equal(best, first_max(want)):
        out.append(f"best {best.tolist()} is not the first maximum {first_max(want).tolist()}")
    return out


def consensus_random_violations(S, cen, w, best, E, tau: float) -> List[str]:
    out = []
    S, cen, w, best, E = S.float().cpu(), cen.float().cpu(), w.float().cpu(), best.cpu().long(), E.cpu()
    ref = E.double() @ E.double().transpose(1, 2)
    bad = ~torch.isfinite(S) | ((S.double() - ref).abs() > s_bound(E))
    if bool(bad.any()):
        out.append(f"{int(bad.sum())} entries of S off the sum bound; worst {float((S.double() - ref).abs().max()):.3g}")
    want = cen_serial(S)
    if bool(same32(cen, want).any()):
        out.append(f"{int(same32(cen, want).sum())} centralities differ from the serial fp32 sum of the kernel's S")
    if not torch.equal(best, first_max(cen)):
        out.append(f"best {best.tolist()} is not the first maximum of the centrality {first_max(cen).tolist()}")
    it = inv_tau32(tau)
    return out + softmax_violations(w, cen.double() * it, 1.01 * it)


# ---------------------------------------------------------------------------------------------------------
# knn_topk


def knn_case(family: str, n: int, d: int, k: int, gen: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """(E [n, d] fp32, q [d] fp32) of integers; see the module docstring."""
    top = 64 if family == "wide" else 8
    assert top * top * d < (1 << 24)
    E = torch.randint(-top, top + 1, (n, d), generator=gen).float()
    q = torch.randint(-top, top + 1, (d,), generator=gen).float()
    q[q == 0] = 1.0
    best_row = top * torch.sign(q)
    if family in ("integers", "wide"):
        E[n - 1] = best_row
    elif family == "equal":
        E[:] = E[0].clone()
    elif family == "negative":
        q = q.abs()
        E = -E.abs() - 1
        E.clamp_(min=-top)
    elif family == "slab_tie":
        E[250:min(n, 250 + 2 * k)] = best_row
    elif family == "group_tie":
        b = group_boundary(k)
        assert b < n
        E[b - k:min(n, b + k)] = best_row
    else:
        raise ValueError(family)
    return E.contiguous(), q


def group_boundary(k: int) -> int:
    """First row of the second merging workgroup (4096 // k lists of 256 rows each)."""
    return (4096 // k) * 256


def knn_families(n: int, k: int) -> List[str]:
    fam = ["integers", "equal", "negative"]
    if n > 250:
        fam.append("slab_tie")
    if n > group_boundary(k):
        fam.append("group_tie")
    return fam


def knn_d(n: int) -> List[int]:
    """Widths per table size: the 16 MB table is the (1048577, 4) one."""
    return [4, 64, 384] if n <= 513 else ([4, 64] if n <= 16385 else [4])


def knn_scores(E: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    return E.cpu().long() @ q.cpu().long()


def knn_oracle(E: torch.Tensor, q: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    v, i = stable_topk(knn_scores(E, q), k)
    return v.float(), i


def knn_violations(vals, rows, E, q, k: int) -> List[str]:
    out, n = [], E.shape[0]
    vals, rows = vals.float().cpu(), rows.cpu().long()
    wv, wr = knn_oracle(E, q, k)
    if bool(((rows < 0) | (rows >= n)).any()):
        out.append(f"rows outside [0, {n}): {rows[(rows < 0) | (rows >= n)].tolist()[:4]}")
    if bool(same32(vals, wv).any()):
        j = int(same32(vals, wv).nonzero()[0])
        out.append(f"value {j}: got {float(vals[j])} want {float(wv[j])}")
    if not torch.equal(rows, wr):
        j = int((rows != wr).nonzero()[0])
        out.append(f"row {j}: got {int(rows[j])} want {int(wr[j])}")
    return out


# ---------------------------------------------------------------------------------------------------------
# moe_route / moe_router


def route_logits(T: int, E: int, k: int, gen: torch.Generator) -> torch.Tensor:
    """[T, E] bf16 multiples of 0.5 within +-2 whose k-th and (k + 1)-th largest are equal in every row; one row of
    equal logits, one with -inf in its lowest experts (k stay finite) and, from T = 4, row 1 with the LAST expert as
    its only maximum (under forced ties the highest id is otherwise never the k-th choice)."""
    x = torch.randint(-4, 5, (T, E), generator=gen).float() * 0.5
    s, _ = torch.sort(x, dim=1, descending=True)
    if k < E:
        s[:, k] = s[:, k - 1]
    perm = torch.rand(T, E, generator=gen).argsort(1)
    x = torch.gather(s, 1, perm)
    x[(T - 1) // 2] = 0.5                                  # equal logits
    if T >= 4:                                             # the last expert as the only maximum
        x[1] = x[1].clamp(max=1.5)
        x[1, E - 1] = 2.0
    ninf = min(E - k, max(1, E // 2))
    if ninf > 0 and T > 1:
        x[T - 1, :ninf] = -float("inf")
    elif ninf > 0 and E % 2 == 0:
        x[0, :ninf] = -float("inf")
    return x.to(BF)


def route_oracle(logits: torch.Tensor, k: int):
    """(ids [T, k] int64, fp64 weights, row_off [E + 1] int64) of the contract."""
    lf = logits.float().cpu()
    v, ids = stable_topk(lf, k)
    cnt = torch.bincount(ids.flatten(), minlength=lf.shape[1])
    return ids, torch.softmax(v.double(), -1), torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)]), v


def route_violations(ids, w, row_off, logits, k: int, x_max: float) -> List[str]:
    out = []
    wi, _, wro, v = route_oracle(logits, k)
    ids, row_off = ids.cpu().long().view(-1, k), row_off.cpu().long()
    if not torch.equal(ids, wi):
        t = int((ids != wi).any(1).nonzero()[0])
        out.append(f"{int((ids != wi).any(1).sum())} rows of ids differ from the stable sort; row {t}: got "
                   f"{ids[t].tolist()} want {wi[t].tolist()}")
    if not torch.equal(row_off, wro):
        out.append("row_off differs from the prefix sum of the expert counts")
    return out + softmax_violations(w.view(-1, k), v, x_max, "routing weights")


def permute_ref(ids: torch.Tensor, E: int):
    """(row_off, src_row, inv) of an expert-sorted dispatch (rows of one expert in token order)."""
    T, k = ids.shape
    flat = ids.flatten().long()
    order = torch.sort(flat, stable=True).indices
    inv = torch.empty(T * k, dtype=torch.long)
    inv[order] = torch.arange(T * k)
    cnt = torch.bincount(flat, minlength=E)
    return torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)]), order // k, inv


def router_sign(T: int, E: int, d: int, gen: torch.Generator, scaled: bool = False):
    """(h [T, d], router [E, d]) bf16 of +-1 (``scaled``: rows times 2^(t % 5 - 2) / 2^(e % 3 - 1))."""
    assert 64 * d < (1 << 24)
    h, r = _signs((T, d), gen), _signs((E, d), gen)
    if scaled:
        h = h * torch.exp2((torch.arange(T) % 5 - 2).float())[:, None]
        r = r * torch.exp2((torch.arange(E) % 3 - 1).float())[:, None]
    return h.to(BF), r.to(BF)


def router_chunks(d: int, T: Optional[int] = None) -> List[int]:
    """The 8-wide chunks a one-hot walk of T rows visits: all of them (T = None), else the first, the last
    (the tail chunk of 2056), both sides of the 256-chunk trip, then a stride."""
    nc = d // 8
    if T is None:
        return list(range(nc))
    pick = [nc - 1, 0] + [c for c in (255, 256) if c < nc] + list(range(1, nc, max(1, nc // max(T, 1))))
    pick = list(dict.fromkeys(pick))
    return [pick[i % len(pick)] for i in range(T)]


def router_onehot(d: int, chunks: Sequence[int], E: int, gen: torch.Generator):
    T = len(chunks)
    cols = walk_cols(chunks)
    v = torch.randn(T, generator=gen)
    v = torch.where(v.abs() < 0.05, torch.full_like(v, 0.75), v)
    h = torch.zeros(T, d)
    h[torch.arange(T), cols] = v
    return h.to(BF), torch.randn(E, d, generator=gen).to(BF)


def router_want(h: torch.Tensor, router: torch.Tensor) -> torch.Tensor:
    """bf16 logits: RNE of the fp64 product, which is exact for both families."""
    return rne(h.double().cpu() @ router.double().cpu().t())


# ---------------------------------------------------------------------------------------------------------
# moe_combine


def combine_inputs(kind: str, T: int, k: int, d: int, gen: torch.Generator, rows: Optional[int] = None):
    """(Y [rows, d] bf16, w [T, k] fp32); rows defaults to T k."""
    rows = T * k if rows is None else rows
    if kind in ("exact", "fine"):
        Y = torch.randint(-16, 17, (rows, d), generator=gen).float().to(BF)
        vals = torch.tensor([1.0, 0.5, 0.25, 0.0] if kind == "exact" else [W_FINE, 0.25, 0.0, W_FINE])
        w = vals[torch.randint(0, 4, (T, k), generator=gen)]
    elif kind == "onehot":
        Y = distinct((rows, d), start=rows + d)
        w = torch.zeros(T, k)
        w[torch.arange(T), torch.randint(0, k, (T,), generator=gen)] = 1.0
    elif kind == "random":
        Y = torch.randn(rows, d, generator=gen).to(BF)
        w = torch.softmax(torch.randn(T, k, generator=gen), -1)
    else:
        raise ValueError(kind)
    return Y, w.float().contiguous()


def combine_want(Y, inv, w, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp64 sum, magnitude sum |w y|)."""
    T = w.shape[0]
    y = Y.double().cpu()[inv.cpu().long()[:T * k]].view(T, k, -1)
    t = w.double().cpu()[:, :, None] * y
    return t.sum(1), t.abs().sum(1)


def combine_violations(cage: RowCage, want, mag, kind: str) -> List[str]:
    out, got = [], cage.view
    want, mag = want.to(got.device), mag.to(got.device)
    if kind == "random":
        bad, share = one_step_cond(got, want, mag, COMBINE_ERR)
        if share < 0.95:
            out.append(f"only {share:.4f} of the outputs are well conditioned")
    else:
        bad = bitwise(got, want)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        out.append(f"{int(bad.sum())} of {bad.numel()} outputs fail; first at {list(i)}: got {float(got[i]):.8g} "
                   f"want {float(rne(want)[i]):.8g}")
    if cage.outside_touched():
        out.append(f"{cage.outside_touched()} sentinels outside the output overwritten")
    return out


# ---------------------------------------------------------------------------------------------------------
# emulations of the contracts in plain torch (CPU, fp32 where the kernels are), each with switches that break it


def _tree_sum(x: torch.Tensor) -> torch.Tensor:
    """fp32 pairwise sum of a vector: an order no kernel here uses."""
    x = x.float()
    while x.numel() > 1:
        if x.numel() % 2:
            x = torch.cat([x, torch.zeros(1)])
        x = x[0::2] + x[1::2]
    return x[0]


def pool_emul(view: torch.Tensor, cu: torch.Tensor, mode: int, *, lo: int = 0, hi: int = 0, last: int = -1,
              ignore_stride: bool = False, drop_chunk: bool = False, zero_nan: bool = False):
    """(fp32, bf16) outputs from ``view``, a [:T, :d] window of a ``framed`` buffer (reads outside the window land
    in its sentinels).  Mutants: mean over [t0 + lo, t1 + hi), LAST reading t1 + last, rows read at stride d,
    the last 256-column trip left out of ss, rsqrt taken of a zero sum."""
    T, d = view.shape
    ld = d if ignore_stride else view.stride(0)
    flat = torch.as_strided(view, (view.untyped_storage().nbytes() // 2 - view.storage_offset(),), (1,)).float()
    out = []
    for s in range(cu.numel() - 1):
        t0, t1 = int(cu[s]), int(cu[s + 1])
        row = lambda t: flat[t * ld:t * ld + d]  # noqa: E731
        if t1 <= t0:
            v = torch.zeros(d)
        elif mode == 0:
            v = row(t0)
        elif mode == 2:
            v = row(t1 + last)
        else:
            v = torch.zeros(d)
            for t in range(t0 + lo, t1 + hi):
                v = v + row(t)
            v = _div(v, t1 - t0)
        sq = v * v
        ss = _tree_sum(sq[:(d - 1) // 256 * 256] if drop_chunk else sq) if sq.numel() else torch.zeros(())
        inv = torch.rsqrt(ss) if (zero_nan or bool(ss > 0)) else torch.zeros(())
        out.append(v * inv)
    of = torch.stack(out)
    return of, of.to(BF)


def consensus_emul(E: torch.Tensor, tau: float, *, keep_diag: bool = False, div_n: bool = False,
                   tie_high: bool = False, no_max: bool = False, transpose_tile: bool = False,
                   skip_cols: int = 0):
    """(S, centrality, weights, best) in fp32."""
    Ef = E.float()[..., :E.shape[-1] - skip_cols]
    S = Ef @ Ef.transpose(1, 2)
    R, n, _ = S.shape
    if transpose_tile:
        S = S.clone()
        S[:, 0:16, 16:32] = S[:, 0:16, 16:32].transpose(1, 2).clone()
    if n == 1:
        cen = torch.ones(R, 1)
    else:
        s = torch.zeros(R, n)
        for j in range(n):
            col = S[:, :, j].clone()
            if not keep_diag:
                col[:, j] = 0.0
            s = s + col
        cen = _div(s, n if div_n else n - 1)
    x = cen * torch.tensor(inv_tau32(tau))
    e = torch.exp(x if no_max else x - x.max(-1, keepdim=True).values)
    w = e / e.sum(-1, keepdim=True)
    best = (n - 1 - first_max(cen.flip(-1))) if tie_high else first_max(cen)
    return S, cen, w, best.to(torch.int32)


def knn_emul(E: torch.Tensor, q: torch.Tensor, k: int, *, tie_high: bool = False, missing_zero: bool = False,
             drop_partial_group: bool = False, lose_offset: bool = False):
    """The slab / merge structure of knn_topk: per 256-row slab the k best, then groups of 4096 // k lists merged
    level by level.  Mutants: ties to the higher row, rows past n scored 0, a merge that drops a trailing partial
    group, the slab offset not added to the winners' positions."""
    n = E.shape[0]
    NEG = -float("inf")
    sims = knn_scores(E, q).double()
    slabs = (n + 255) // 256
    pad = torch.full((slabs * 256 - n,), 0.0 if missing_zero else NEG, dtype=torch.float64)
    v = torch.cat([sims, pad]).view(slabs, 256)
    idx = torch.arange(slabs * 256).view(slabs, 256)
    if lose_offset:
        idx = idx % 256

    def best_k(v, idx):
        if tie_high:   # by row descending first, then a stable sort by value
            o = torch.sort(idx, dim=1, descending=True, stable=True).indices
            v, idx = v.gather(1, o), idx.gather(1, o)
        sv, si = torch.sort(v, dim=1, descending=True, stable=True)
        return sv[:, :k], idx.gather(1, si)[:, :k]

    v, idx = best_k(v, idx)
    idx = torch.where(v == NEG, -1, idx)
    group = 4096 // k
    while True:
        lists = v.shape[0]
        blocks = max(1, lists // group) if drop_partial_group else (lists + group - 1) // group
        fill = blocks * group - lists
        if fill > 0:
            v = torch.cat([v, torch.full((fill, k), NEG, dtype=torch.float64)])
            idx = torch.cat([idx, torch.full((fill, k), -1, dtype=torch.long)])
        v, idx = best_k(v[:blocks * group].reshape(blocks, group * k), idx[:blocks * group].reshape(blocks, group * k))
        if blocks == 1:
            return v[0].float(), idx[0]


def route_emul(logits: torch.Tensor, k: int, *, tie_high: bool = False, e_read: Optional[int] = None):
    """(ids int32 [T, k], fp32 weights, row_off).  Mutants: ties to the higher expert, only the first ``e_read``
    experts read."""
    lf = logits.float()
    E = lf.shape[1]
    if e_read is not None:
        lf = lf[:, :e_read]
    if tie_high:
        v, i = stable_topk(lf.flip(1), k)
        i = lf.shape[1] - 1 - i
    else:
        v, i = stable_topk(lf, k)
    e = torch.exp(v - v[:, :1])
    cnt = torch.bincount(i.flatten(), minlength=E)
    return i.to(torch.int32), e / e.sum(-1, keepdim=True), torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])


def router_emul(h: torch.Tensor, router: torch.Tensor, k: int, *, round_first: bool = True):
    """(ids, weights, row_off, bf16 logits).  Mutant: the selection made on the fp32 sums."""
    acc = (h.double() @ router.double().t()).float()
    lg = acc.to(BF)
    ids, w, ro = route_emul(lg if round_first else acc, k)
    return ids, w, ro, lg


def combine_emul(Y, inv, w, k: int, *, w_bf16: bool = False, transposed: bool = False) -> torch.Tensor:
    """bf16 [T, d] from an unfused fp32 sum.  Mutants: weights through bf16, inv read as [k, T]."""
    T = w.shape[0]
    acc = torch.zeros(T, Y.shape[1])
    t = torch.arange(T)
    for j in range(k):
        pos = inv.long()[t + j * T] if transposed else inv.long()[t * k + j]
        wj = w[:, j].to(BF).float() if w_bf16 else w[:, j].float()
        acc = acc + wj[:, None] * Y[pos].float()
    return acc.to(BF)
