"""Host quantiser, plane layouts, edge blocks, byte cages and deliberately wrong references for the kernels that
exchange activations in MX form: e4m3 rows plus one e8m0 scale byte per 32 values, value = q * 2^(byte - 127).

Writers: prefill_attention_mx and the cascade decode kernel (plane [Hq, rows, 4], head_dim 128) and gemm8g's SwiGLU
epilogue with MX output (plane [F / 128, rows, 4]).  Reader: gemm8g with ``a_mx`` (plane [K / 128, rows, 4]).  Block b
of a 128-slice is its columns [32 b, 32 b + 32); with head_dim 128 a head is a slice, so both planes are one layout.

The quantiser (``mx_exp`` of csrc/kernels/common.h followed by the hardware's e4m3 conversion):

    e    = clamp(frexp_exp(amax) - 9 + (frexp_mant(amax) > 0.875), -127, 127)     amax over the 32 values
    q    = RNE_e4m3(v * 2^-e)
    byte = e + 127

frexp_mant is in [0.5, 1), so the largest |q| of a live block is in (224, 448]: 0.875 * 2^9 = 448 is e4m3's largest
value, and a mantissa above it takes the next binade (> 0.875 * 2^8 = 224).  A zero block has frexp_exp 0: byte 118.
fp32 has no amax with frexp_exp above 128, so e <= 120 (byte 247) and the upper clamp is never taken; the lower
one is taken from amax < 2^-118 down.

Every writer quantises one value per element, so its bytes are determined: the bf16-rounded tile for prefill and
SwiGLU (the tile their bf16 twins store), the fp32 ``o * inv`` for cascade decode.  The reader's block-scaled MFMA
applies 2^(byte - 127) to the 32 products of a block; with e4m3 operands in {+-1, +-2}, one scale per live block and
a spread of at most 2^10 between the 128-slices of a row every partial sum is exact in fp32, and the bf16 output is
the RNE code of the exact product.

The last part holds what tests/test_mx_probes.py needs to show that these checks reject a broken kernel.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from tests import gemm_probes as gp

E4M3 = torch.float8_e4m3fn
SENTINEL8 = gp.SENTINEL8   # e4m3fn NaN: no quantiser output
PLANE_SENTINEL = 0xA5      # 2^38: no probe family has a block maximum near 2^47
ZERO_BYTE = 118
PAD_ROWS, PAD_BYTES, PAD_PLANE_ROWS = 8, 16, 7


# ---------------------------------------------------------------------------------------------------------
# the quantiser


def e4m3_rne(x: torch.Tensor, trunc: bool = False) -> torch.Tensor:
    """fp64 |x| <= 448 -> the nearest e4m3 value, ties to the even mantissa (``trunc``: towards zero), written
    from the format: 3 mantissa bits, normal from 2^-6, subnormal step 2^-9."""
    x = x.double()
    a = x.abs().clamp(max=448.0)
    _, ex = torch.frexp(a)                       # a = m * 2^ex, m in [0.5, 1): leading bit at 2^(ex - 1)
    step = torch.exp2((ex - 4).clamp(min=-9).double())
    n = a / step
    n = torch.floor(n) if trunc else torch.round(n)   # torch.round: half to even
    return torch.copysign(n * step, x)


def mx_exp_ref(amax: torch.Tensor, threshold: str = "gt", bump: bool = True) -> torch.Tensor:
    m, ea = torch.frexp(amax.float())
    up = (m > 0.875) if threshold == "gt" else (m >= 0.875)
    e = ea.to(torch.int32) - 9 + (up.to(torch.int32) if bump else 0)
    return e.clamp(-127, 127)


def mx_quant_ref(x: torch.Tensor, *, threshold: str = "gt", bump: bool = True, trunc: bool = False,
                 span: int = 32) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 [..., 32 k] -> (e4m3 bytes uint8 [..., 32 k], scale bytes uint8 [..., k]).  The keywords are the wrong
    references: ``threshold="ge"``, ``bump=False`` (the block maximum saturates), ``trunc`` (conversion towards
    zero), ``span`` = 8 / 16 (amax over the first 8 / 16 values of the block only)."""
    x = x.float()
    lead, n = x.shape[:-1], x.shape[-1]
    assert n % 32 == 0
    blocks = x.reshape(*lead, n // 32, 32)
    amax = blocks[..., :span].abs().amax(-1)
    e = mx_exp_ref(amax, threshold, bump)
    scaled = torch.ldexp(blocks.double(), -e[..., None]).clamp(-448.0, 448.0)
    if trunc:
        q = e4m3_rne(scaled, trunc=True).float().to(E4M3)
    else:
        q = scaled.float().to(E4M3)
    return q.view(torch.uint8).reshape(*lead, n), (e + 127).to(torch.uint8)


def q_values(qb: torch.Tensor) -> torch.Tensor:
    return qb.contiguous().view(E4M3).float()


def dequant(qb: torch.Tensor, sc: torch.Tensor) -> torch.Tensor:
    """fp64 [..., 32 k] values of e4m3 bytes [..., 32 k] under scale bytes [..., k]."""
    s = torch.exp2(sc.double() - 127.0).repeat_interleave(32, dim=-1)
    return q_values(qb).double() * s


def element_bound(x: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """|dequant - x| <= max(|x| * 2^-4, 2^(e - 10)) for x [..., 32 k] and block exponents e [..., k]: half an e4m3
    step is 2^-4 of the value's binade in the normal range and half the subnormal step 2^-9 below 2^-6 (both
    times 2^e)."""
    sub = torch.exp2(e.double() - 10.0).repeat_interleave(32, dim=-1)
    return torch.maximum(x.double().abs() * 2.0 ** -4, sub)


# ---------------------------------------------------------------------------------------------------------
# planes: scale bytes [rows, 4 P] <-> [P, rows, 4]  (P = heads of 128 dims, or 128-slices of K)


def to_plane(sc: torch.Tensor, s_rows: Optional[int] = None, fill: int = PLANE_SENTINEL) -> torch.Tensor:
    rows = sc.shape[0]
    assert sc.shape[1] % 4 == 0
    pl = sc.reshape(rows, -1, 4).permute(1, 0, 2)
    if s_rows is None or s_rows == rows:
        return pl.contiguous()
    out = torch.full((pl.shape[0], s_rows, 4), fill, dtype=torch.uint8, device=sc.device)
    out[:, :rows] = pl
    return out


def from_plane(pl: torch.Tensor, rows: Optional[int] = None) -> torch.Tensor:
    rows = pl.shape[1] if rows is None else rows
    return pl[:, :rows].permute(1, 0, 2).reshape(rows, -1)


def head_plane(sc: torch.Tensor, Hq: int, s_rows: Optional[int] = None, fill: int = PLANE_SENTINEL) -> torch.Tensor:
    """Scale bytes [rows, Hq * 4] of rows of Hq heads of 128 dims -> [Hq, s_rows, 4]."""
    assert sc.shape[1] == 4 * Hq
    return to_plane(sc, s_rows, fill)


def slice_plane(sc: torch.Tensor, K: int, s_rows: Optional[int] = None, fill: int = PLANE_SENTINEL) -> torch.Tensor:
    """Scale bytes [rows, K / 32] -> [K / 128, s_rows, 4]."""
    assert sc.shape[1] * 32 == K and K % 128 == 0
    return to_plane(sc, s_rows, fill)


# ---------------------------------------------------------------------------------------------------------
# edge blocks

POSITIONS = (0, 31, 3, 12, 20, 27)   # lane 0, lane 31, and one lane in each 8-element quarter
# (name, block maximum); its scaled maximum S = max * 2^-e and e follow from the quantiser
CLASSES = (("zero", 0.0), ("m7", 7.0), ("m7.5", 7.5), ("m8", 8.0), ("m448", 448.0), ("m480", 480.0),
           ("tiny", 2.0 ** -126), ("clamp", 2.0 ** -120), ("large", 2.0 ** 100))
# other elements, in the scaled domain (what the e4m3 conversion sees), each with at most 8 significant bits:
# ties of the normal range (432 -> 448, 400 -> 384, 8.5 -> 8, 9.5 -> 10, 1.0625 -> 1), plain roundings (101 -> 104,
# 99 -> 96), and the subnormal range below 2^-6 (step 2^-9): its smallest value, exact values, ties (3 * 2^-10 ->
# 2^-8, 5 * 2^-10 -> 2^-8, 2^-10 -> 0, 7.5 * 2^-9 -> 2^-6, the smallest normal) and 2^-11 -> 0
SCALED = (432.0, 400.0, 8.5, 9.5, 1.0625, 101.0, 99.0, 2.0, 3.0, 2.0 ** -9, 7 * 2.0 ** -9, 3 * 2.0 ** -10,
          5 * 2.0 ** -10, 2.0 ** -10, 7.5 * 2.0 ** -9, 2.0 ** -11, 0.0)


def class_exp(mx: float) -> int:
    return int(mx_exp_ref(torch.tensor(mx)))


def edge_block(mx: float, pos: int, rot: int = 0, min_value: float = 2.0 ** -126) -> torch.Tensor:
    """fp32 [32]: the maximum ``mx`` in lane ``pos`` (sign by ``rot``), the other lanes walking SCALED times 2^e
    from entry ``rot`` with alternating signs; entries above the maximum, and entries below ``min_value`` (which
    would be subnormal where they are computed), are 0."""
    out = torch.zeros(32, dtype=torch.float64)
    if mx == 0:
        return out.float()
    e = class_exp(mx)
    S = mx * 2.0 ** -e
    cand = [t for t in SCALED if t < S and (t == 0 or t * 2.0 ** e >= min_value)]
    j = rot
    for lane in range(32):
        if lane == pos:
            out[lane] = mx * (-1.0 if rot % 2 else 1.0)
            continue
        t = cand[j % len(cand)] if cand else 0.0
        out[lane] = t * 2.0 ** e * (-1.0 if (lane + rot) % 2 else 1.0)
        j += 1
    f = (out + 0.0).float()   # no negative zeros: a kernel's sum of +0 and -0 products is +0
    assert torch.equal(f.double(), out) and torch.equal(f.to(torch.bfloat16).float(), f), (mx, pos)
    return f


def edge_table(min_value: float = 2.0 ** -126) -> Tuple[List[Tuple[str, int]], torch.Tensor]:
    """Names [(class, position)] and fp32 [n, 32] blocks, all bf16-exact; classes whose maximum is below
    ``min_value`` are left out."""
    names, rows = [], []
    for ci, (name, mx) in enumerate(CLASSES):
        if mx != 0 and mx < min_value:
            continue
        for pi, pos in enumerate(POSITIONS if mx != 0 else POSITIONS[:1]):
            names.append((name, pos))
            rows.append(edge_block(mx, pos, rot=pi + 2 * ci, min_value=min_value))
    return names, torch.stack(rows)


def edge_classes(min_value: float = 2.0 ** -126) -> List[int]:
    return [i for i, (_, mx) in enumerate(CLASSES) if mx == 0 or mx >= min_value]


def edge_grid(min_value: float = 2.0 ** -126) -> torch.Tensor:
    """fp32 [classes, 6, 32]: the table by (class, position); the zero class repeats its block."""
    return torch.stack([torch.stack([edge_block(CLASSES[ci][1], pos, rot=pi + 2 * ci, min_value=min_value)
                                     for pi, pos in enumerate(POSITIONS)]) for ci in edge_classes(min_value)])


def edge_rows(rows: int, nblocks: int, min_value: float = 2.0 ** -126, shift: int = 0) -> torch.Tensor:
    """fp32 [rows, 32 nblocks] of table blocks: column block cb holds class (cb + shift) mod the number of
    classes — one magnitude per column, as a per-channel weight scale needs — and row r position r % 6."""
    cls = edge_classes(min_value)
    x = torch.zeros(rows, nblocks, 32)
    for cb in range(nblocks):
        ci = cls[(cb + shift) % len(cls)]
        for pi, pos in enumerate(POSITIONS):
            x[pi::6, cb] = edge_block(CLASSES[ci][1], pos, rot=pi + 2 * ci, min_value=min_value)
    return x.reshape(rows, nblocks * 32)


SATURATED_MIN = 2.0 ** -120   # activations of the saturated-gate family: up = act / 64 stays a normal fp32 number


def saturated_gate_operands(rows: int, F: int, K: int, shift: int = 0):
    """Operands of a SwiGLU GEMM whose activations are ``edge_rows(rows, F / 32, SATURATED_MIN, shift)`` exactly:
    e4m3 A [rows, K], W [2 F, K] (gate rows, then up rows; fp32 holding e4m3 values), channel scales w_s [2 F]
    (powers of two), row scales 1, and the activations.  gate = 64 exactly (A[:, 0] = 1 against a gate weight of 1
    under a channel scale of 64), where silu(gate) = 64 / (1 + exp(-64)) is 64 in fp32.  A row of position p adds
    column 1 + p (1) and column 7 + p (2^-4) of the up weights: the value's e4m3 rounding and 16 times the
    remainder, both e4m3 numbers, so up = act / 64 with two exact products.  The clamp class (maximum 2^-120)
    keeps only its maximum: any smaller element would need a subnormal ``up``; the 2^-126 class is left to the
    attention writers for the same reason."""
    assert K >= 13 and F % 32 == 0
    x = edge_rows(rows, F // 32, SATURATED_MIN, shift)
    A = torch.zeros(rows, K)
    p = torch.arange(rows) % 6
    A[:, 0] = 1.0
    A[torch.arange(rows), 1 + p] = 1.0
    A[torch.arange(rows), 7 + p] = 2.0 ** -4
    W = torch.zeros(2 * F, K, dtype=torch.float64)
    w_s = torch.ones(2 * F, dtype=torch.float64)
    W[:F, 0] = 1.0
    w_s[:F] = 64.0
    cls = edge_classes(SATURATED_MIN)
    for cb in range(F // 32):
        ci = cls[(cb + shift) % len(cls)]
        name, mx = CLASSES[ci]
        e = class_exp(mx) if mx else 0
        down = 7 if name == "clamp" else 0     # keeps the channel scale a normal number
        ch = slice(F + 32 * cb, F + 32 * cb + 32)
        w_s[ch] = 2.0 ** (e - 6 + down)
        for pi, pos in enumerate(POSITIONS):
            t = edge_block(mx, pos, rot=pi + 2 * ci, min_value=SATURATED_MIN).double() * 2.0 ** (-e - down)
            hi = e4m3_rne(t)
            lo = (t - hi) * 16.0
            assert torch.equal(e4m3_rne(lo), lo) and float(lo.abs().max()) <= 448
            W[ch, 1 + pi], W[ch, 7 + pi] = hi, lo
    assert torch.equal(W.float().to(E4M3).float().double(), W) and torch.equal(A.to(E4M3).float(), A)
    return A.to(E4M3), W.float(), w_s.float(), x


def block_keys(qb: torch.Tensor, sc: torch.Tensor) -> set:
    """The set of (32 e4m3 bytes + scale byte) of every block of qb [..., 32 k], sc [..., k]."""
    q = qb.reshape(-1, 32).cpu()
    q = torch.where(q == 0x80, torch.zeros_like(q), q)   # -0 is 0: a zero lane of V[at] takes the sign of the leak
    s = sc.reshape(-1, 1).cpu()
    both = torch.unique(torch.cat([q, s], 1), dim=0)
    return {bytes(r.tolist()) for r in both}


def missing_edge_blocks(qb: torch.Tensor, sc: torch.Tensor, names, table: torch.Tensor) -> list:
    """Names of the table's blocks whose quantised bytes appear nowhere in (qb, sc)."""
    have = block_keys(qb, sc)
    tq, ts = mx_quant_ref(table)
    tq = torch.where(tq == 0x80, torch.zeros_like(tq), tq)
    return [n for n, q, s in zip(names, tq, ts) if bytes(q.tolist() + s.tolist()) not in have]


# ---------------------------------------------------------------------------------------------------------
# rows whose quantiser input is fp32 (cascade decode): bounded against the kernel's own bf16 output

TALL_K = 192.0   # K value of a one-hot row's spike key: 16 * 192 / sqrt(128) = 271 nats, every other weight is 0 in fp32
NEAR = 2.0 ** -8


def bounded_violations(qb: torch.Tensor, sc: torch.Tensor, out: torch.Tensor, where: Optional[torch.Tensor] = None):
    """e4m3 bytes qb [R, 32 k] and scale bytes sc [R, k] of a writer that quantises the fp32 value whose bf16
    rounding is ``out`` [R, 32 k].  With x the fp32 value, |out - x| <= 2^-9 |x| and |deq - x| <= max(|x| 2^-4,
    2^(e - 10)), so |deq - out| <= max(|out| 2^-4, 2^(e - 10)) (1 + 2^-8) + 2^-8 |out|.  The scale byte is that of
    mx_quant_ref(out), unless the block maximum of ``out`` has a mantissa within 2^-8 relative of 0.875 or of a
    power of two, where the rounding to bf16 may have crossed the threshold: there the byte may differ by one and
    the bound is taken with the kernel's own e.  -> (violations, share of exempt blocks among those compared);
    ``where`` [R, k] restricts the blocks."""
    R, n = out.shape
    o = out.double()
    _, ref_sc = mx_quant_ref(out.float())
    m, _ = torch.frexp(out.float().view(R, n // 32, 32).abs().amax(-1))
    near = ((m - 0.875).abs() <= 0.875 * NEAR) | ((m - 0.5).abs() <= 0.5 * NEAR) | ((1.0 - m) <= NEAR)
    near &= m > 0
    use = torch.ones_like(near) if where is None else where.to(near.device)
    diff = (sc.int() - ref_sc.int()).abs()
    bad_sc = use & torch.where(near, diff > 1, diff > 0)
    e = sc.double() - 127.0
    bound = element_bound(o, e) * (1 + NEAR) + NEAR * o.abs()
    err = (dequant(qb, sc) - o).abs()
    bad_q = (~(err <= bound)) & use.repeat_interleave(32, dim=1)
    v = []
    if bool(bad_sc.any()):
        r, b = (int(i) for i in bad_sc.nonzero()[0])
        v.append(f"{int(bad_sc.sum())} scale bytes off; first at row {r} block {b}: got {int(sc[r, b])} want "
                 f"{int(ref_sc[r, b])}")
    if bool(bad_q.any()):
        r, c = (int(i) for i in bad_q.nonzero()[0])
        v.append(f"{int(bad_q.sum())} elements out of bound; first at row {r} column {c}: got "
                 f"{float(dequant(qb, sc)[r, c]):.8g} bf16 {float(o[r, c]):.8g} bound {float(bound[r, c]):.3g}")
    share = float((near & use).sum()) / max(1, int(use.sum()))
    return v, share


# ---------------------------------------------------------------------------------------------------------
# byte cages


class ByteCage:
    """An e4m3 matrix [rows, cols] as the [:rows, :cols] view of a [rows + 8, cols + pad] buffer of SENTINEL8
    (pad a multiple of 16 bytes: the row stride stays 16-byte aligned; pad 0: rows below only)."""

    def __init__(self, rows: int, cols: int, device="cpu", pad: int = PAD_BYTES):
        assert pad % 16 == 0
        self.rows, self.cols = rows, cols
        self.buf = torch.empty(rows + PAD_ROWS, cols + pad, dtype=torch.uint8, device=device)
        self.view = self.buf[:rows, :cols]
        self.poison()

    def poison(self) -> "ByteCage":
        self.buf.fill_(SENTINEL8)
        return self

    @property
    def f8(self) -> torch.Tensor:
        return self.buf.view(E4M3)[:self.rows, :self.cols]

    def outside(self) -> List[Tuple[int, int]]:
        m = self.buf != SENTINEL8
        m[:self.rows, :self.cols] = False
        return [tuple(int(v) for v in i) for i in m.nonzero()[:4]] if bool(m.any()) else []


class PlaneCage:
    """A scale plane [P, rows, 4] as the [:, :rows] part of a [P, rows + 7, 4] buffer of PLANE_SENTINEL."""

    def __init__(self, P: int, rows: int, device="cpu", extra: int = PAD_PLANE_ROWS):
        self.P, self.rows = P, rows
        self.buf = torch.empty(P, rows + extra, 4, dtype=torch.uint8, device=device)
        self.poison()

    def poison(self) -> "PlaneCage":
        self.buf.fill_(PLANE_SENTINEL)
        return self

    @property
    def s_rows(self) -> int:
        return self.buf.shape[1]

    def outside(self) -> List[Tuple[int, int, int]]:
        m = self.buf[:, self.rows:] != PLANE_SENTINEL
        return [(int(i[0]), self.rows + int(i[1]), int(i[2])) for i in m.nonzero()[:4]] if bool(m.any()) else []


def violations(qc: Optional[ByteCage], pc: Optional[PlaneCage], want_q: Optional[torch.Tensor],
               want_sc: Optional[torch.Tensor], where: Optional[torch.Tensor] = None) -> List[str]:
    """What a writer left wrong: the first differing (row, column) of the e4m3 bytes and (row, block) of the
    scale bytes (``where``: a bool mask [rows, P] of the 128-value slices that are compared), and every kind of
    overwritten sentinel.  ``want_sc`` is [rows, 4 P].  Empty = accepted."""
    out = []
    if qc is not None and want_q is not None:
        bad = qc.view != want_q.to(qc.view.device)
        if where is not None:
            bad &= where.to(bad.device).repeat_interleave(128, dim=1)
        if bool(bad.any()):
            r, c = (int(v) for v in bad.nonzero()[0])
            out.append(f"{int(bad.sum())} e4m3 bytes differ; first at row {r} column {c}: got "
                       f"0x{int(qc.view[r, c]):02x} want 0x{int(want_q[r, c]):02x}")
    if pc is not None and want_sc is not None:
        got = from_plane(pc.buf, pc.rows)
        bad = got != want_sc.to(got.device)
        if where is not None:
            bad &= where.to(bad.device).repeat_interleave(4, dim=1)
        if bool(bad.any()):
            r, b = (int(v) for v in bad.nonzero()[0])
            out.append(f"{int(bad.sum())} scale bytes differ; first at row {r} block {b} (plane {b // 4}): got "
                       f"{int(got[r, b])} want {int(want_sc[r, b])}")
    if qc is not None and qc.outside():
        out.append(f"e4m3 sentinels outside [:{qc.rows}, :{qc.cols}] overwritten, first at {qc.outside()}")
    if pc is not None and pc.outside():
        out.append(f"plane sentinels past row {pc.rows} overwritten, first (plane, row, block) {pc.outside()}")
    return out


def check(qc, pc, want_q, want_sc, what: str = "", where: Optional[torch.Tensor] = None) -> None:
    v = violations(qc, pc, want_q, want_sc, where)
    assert not v, f"{what}: " + "; ".join(v)


# ---------------------------------------------------------------------------------------------------------
# consumer families: A in {+-1, +-2} (0 in dead blocks) with scale bytes that tell rows, slices and blocks apart

LIVE_LO, LIVE_SPAN = 122, 11      # live scales 2^-5 .. 2^5: spread 2^10 across a row
DEAD_LO, DEAD_SPAN = 110, 35      # dead blocks (q = 0): any byte of 110..144


def _live_byte(r: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return LIVE_LO + (5 * (r % 32) + 3 * s + r // 32) % LIVE_SPAN


def scale_walk(rows: int, K: int, gen: torch.Generator, all_live: bool = False):
    """e4m3 A [rows, K] and scale bytes [rows, K / 32].  ``all_live``: every value is +-1 / +-2 and the four
    blocks of a 128-slice share one byte that differs between slices and rows.  Otherwise one block per (row,
    slice) is live, chosen by a hash of both, and carries that byte; the three dead blocks hold zeros under bytes
    of 110..144 that differ from the live one and between (row % 32, slice, block)."""
    S = K // 128
    r = torch.arange(rows)[:, None, None]
    s = torch.arange(S)[None, :, None]
    b = torch.arange(4)[None, None, :]
    live = _live_byte(r, s).expand(rows, S, 4)
    vals = (gp._signs((rows, K), gen) * torch.randint(1, 3, (rows, K), generator=gen).float()).view(rows, S, 4, 32)
    if all_live:
        sc = live
    else:
        pick = ((3 * r + 5 * s + r // 32) % 4) == b
        dead = DEAD_LO + (7 * (r % 32) + 13 * s + 3 * b) % DEAD_SPAN
        dead = torch.where(dead == live, DEAD_LO + (dead - DEAD_LO + 17) % DEAD_SPAN, dead)
        sc = torch.where(pick, live, dead)
        vals = vals * pick[..., None]
    assert int(sc.max()) < 255
    return vals.reshape(rows, K).to(E4M3), sc.reshape(rows, S * 4).to(torch.uint8).contiguous()


def mx_product(A: torch.Tensor, sc: torch.Tensor, W: torch.Tensor, w_s: torch.Tensor, *,
               block_xor: int = 0, row_xor: int = 0) -> torch.Tensor:
    """fp64 (A * 2^(sc - 127)) . W^T * w_s for e4m3 A [rows, K], scale bytes [rows, K / 32], W [N, K].  Wrong
    references: ``block_xor`` = 1 reads the scale of block b ^ 1, ``row_xor`` = 16 that of row r ^ 16."""
    rows = A.shape[0]
    if block_xor:
        sc = sc.reshape(rows, -1, 4)[:, :, torch.arange(4) ^ block_xor].reshape(rows, -1)
    if row_xor:
        idx = (torch.arange(rows, device=sc.device) ^ row_xor).clamp(max=rows - 1)
        sc = sc[idx]
    a = A.float().double() * torch.exp2(sc.double() - 127.0).repeat_interleave(32, dim=1)
    return (a @ W.float().double().t()) * w_s.double()[None, :]


def exact_in_fp32(A: torch.Tensor, sc: torch.Tensor) -> bool:
    """Premise of the bitwise consumer claim: per row, 4 * 32 * (K / 128) products of magnitude <= 4 * 2^(byte -
    127) on a grid of 2^(min byte - 127) fit 24 bits, dead blocks aside."""
    rows, K = A.shape
    live = A.float().view(rows, -1, 32).abs().amax(-1) > 0
    hi = torch.where(live, sc.int(), torch.zeros_like(sc, dtype=torch.int32)).amax(1)
    lo = torch.where(live, sc.int(), torch.full_like(sc, 255, dtype=torch.int32)).amin(1)
    return bool(((hi - lo) + 2 + (32 * live.sum(1)).float().log2().ceil().int() <= 24).all())


# ---------------------------------------------------------------------------------------------------------
# wrong writers (CPU tests only): what a kernel leaves in the cages


def write(qc: ByteCage, pc: PlaneCage, x: torch.Tensor, *, row0: int = 0, plane_row0: Optional[int] = None,
          flip_blocks: bool = False, transposed: bool = False, neighbour_row: bool = False,
          past_rows: int = 0, **quant) -> None:
    """A writer storing rows ``x`` [n, 32 k] at rows row0.. of the cages.  Mutants: ``plane_row0`` = the plane row
    of x's first row (a sequence-local ``qr`` where ``s0 + qr`` is meant), ``flip_blocks`` = block 3 - b,
    ``transposed`` = the plane laid out [rows, P, 4], ``neighbour_row`` = row r takes the scale of row r + 1,
    ``past_rows`` = that many rows past the end are stored as well; ``quant`` goes to mx_quant_ref."""
    q, sc = mx_quant_ref(x, **quant)
    n = x.shape[0]
    if neighbour_row:
        sc = torch.cat([sc[1:], sc[-1:]])
    if flip_blocks:
        sc = sc.reshape(n, -1, 4).flip(2).reshape(n, -1)
    pr0 = row0 if plane_row0 is None else plane_row0
    if transposed:
        flat = pc.buf.view(-1)
        flat[pr0 * sc.shape[1]:(pr0 + n) * sc.shape[1]] = sc.reshape(-1)
    else:
        pc.buf[:, pr0:pr0 + n] = to_plane(sc)
    qc.buf[row0:row0 + n, :qc.cols] = q
    for i in range(past_rows):
        qc.buf[row0 + n + i, :qc.cols] = q[-1]
        pc.buf[:, pr0 + n + i] = to_plane(sc[-1:])[:, 0]
