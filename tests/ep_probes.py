"""Exact inputs, a byte-for-byte oracle, row cages and deliberately wrong emulations for the expert-parallel exchange
kernels of csrc/kernels/ep.hip (ep_pack, ep_unpack, ep_back, ep_combine).  All four move rows between layouts: what
goes wrong is an offset (a chunk base, a slot, an expert segment), a count read from the wrong place, a slot left
unwritten, and none of it is visible in a comparison of a final output between two processes.  Here one process
plays all W ranks on one device and the all-to-all is tensor indexing (``recv_r[s] = send_s[r]``).

``RowCage``, ``SENTINEL``, ``SENT32``, ``distinct``, ``rne``, ``bitwise``, ``same32``, ``one_step_cond``,
``combine_inputs``, ``combine_want`` and ``COMBINE_ERR`` are those of tests/gemm_probes.py, tests/rowwise_probes.py and
tests/select_probes.py.

Contract tested (the header comment of ep.hip)
----------------------------------------------
Rank r owns experts [r El, (r + 1) El).  A rank's routed rows are expert-sorted: ``row_off`` [E + 1], sorted row p reads
token ``src[p]``, (t, j) sits at sorted row ``inv[t k + j]``.  Exchange buffer [W][C + 1 slots][RB bytes],
RB = round16(max(row_bytes + 4 has_scale, 4 El)):

  send      chunk r, slot 0: El int32 counts (the experts of rank r), the rest of the slot zero; slot 1 + j, j < n_r:
            the row_bytes of token src[row_off[r El] + j], then (fp8) its f32 scale at byte row_bytes; slots past n_r
            all zero.
  x_local   received (source s, slot i) of local expert e lands after every row of experts < e (all sources) and after
            expert e's rows from sources < s; ``s_local`` the same for the scales; ``map[s C + i]`` that position, -1
            for an unused slot; ``row_off_local`` [El + 1] the local segments.  A source whose counts cannot be real
            (one negative, or a sum above C, in whatever width the sum needs) counts as sending nothing.
  back      back[s C + i] = y_local[map[s C + i]], all zero where map is -1.
  out       out[t] = sum_j w[t, j] ret[owner(p) C + p - row_off[owner(p) El]], p = inv[t k + j], ret the returned
            chunks [W C, d_out], accumulated in fp32 and stored as RNE bf16.

Two regions are NOT specified and are treated so: the tail of a used slot past row_bytes + 4 has_scale, and the rows
of x_local / s_local at or past row_off_local[El].  They are masked out of the ``send`` comparison, and filled with
the NaN sentinel (bf16 SENTINEL, fp32 SENT32, all-ones bytes for e4m3 rows) before the next kernel reads the buffer:
every later stage must still match the oracle bit for bit, so nothing of them reaches a result.

Families and bounds
-------------------
  rows      bf16: ``distinct`` codes numbered through all ranks' tokens (``tame`` folds the 16 highest and lowest
            exponents to the middle so that the expert function neither overflows nor leaves the normal range);
            e4m3: counting bytes (every value 0..255, never decoded), scales (2 i + 1) 2^(i % 7 - 3), i the global
            token number.  Pure copies: bitwise, no bound needed.
  experts   row i of local expert e of rank r times 2^((r El + e) % 5 - 2), columns tiled or truncated to d_out;
            e4m3 rows: RNE_bf16(byte * scale * factor), one rounding of an exact fp32 product (8 + 8 bits).  A power
            of two times a tamed bf16 value is exact.  A row grouped under the wrong expert has the wrong factor.
  combine   in the chain the weights are one-hot, so ``out`` is a bitwise row copy (0 * finite = +0, every value is
            positive).  On a ``ret`` built by the oracle, the four moe_combine families of tests/select_probes.py under
            their rules: exact (terms multiples of 0.25 within 16, k <= 8: 64 * 8 < 2^24), fine (multiples of 2^-10:
            2^14 * 8 < 2^24), one-hot (a copy) bitwise; random under ``one_step_cond`` with COMBINE_ERR, at least
            95 % of the outputs well conditioned (asserted on the fp64 reference for every shape used).

Shapes and what they reach
--------------------------
``copy_bytes`` / ``zero_bytes`` move 16 bytes per thread, 4096 per trip of a 256-thread block: row_bytes 16 (one
thread), 528 (33 threads), 4112 (a second trip of one thread).  The combine loop covers 2048 columns per trip:
d_out = 2056 is the second trip, 8 one thread, 264 a partial block.  (1, 64) at bf16 d = 8 is the slot sized by its
header (RB = 256 > 16); e4m3 d = 4112 has RB = 4128: the scale at byte 4112 and 12 bytes of tail; e4m3 d = 16 has
RB = 32.  W El = 64 is ``kEpMaxCounts``; k = 8 fills ``s_row``.  CASES lists the combinations.

The last part holds emulations of the four kernels, written after their code (not after the oracle) with switches that
break them in one way each; tests/test_ep_probes.py shows that the honest emulation passes every case and names the
case that rejects each mutant.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from tests.gemm_probes import SENTINEL, bits, bitwise, rne  # noqa: F401
from tests.rowwise_probes import BF, SENT32, RowCage, distinct, one_step_cond  # noqa: F401
from tests.select_probes import COMBINE_ERR, combine_inputs, combine_want, same32  # noqa: F401

U8, I32, F32 = torch.uint8, torch.int32, torch.float32


# ---------------------------------------------------------------------------------------------------------
# cases


@dataclass(frozen=True)
class Case:
    name: str
    W: int
    El: int
    k: int
    d: int
    fp8: bool
    d_out: int
    cap: str                      # "full": C = max R, one chunk exactly full; "plus3"; "one": C = 1, a single row
    routing: str                  # random | single | starved | holes | idle | one
    T: Tuple[int, ...]            # tokens per rank

    @property
    def E(self) -> int:
        return self.W * self.El

    @property
    def row_bytes(self) -> int:
        return self.d * (1 if self.fp8 else 2)

    @property
    def RB(self) -> int:
        return -(-max(self.row_bytes + (4 if self.fp8 else 0), 4 * self.El) // 16) * 16

    @property
    def C(self) -> int:
        top = max(t * self.k for t in self.T)
        return {"full": top, "plus3": top + 3, "one": 1}[self.cap]


CASES = [
    Case("w1e1-one", 1, 1, 1, 8, False, 8, "one", "one", (1,)),
    Case("w1e64-header-slot", 1, 64, 2, 8, False, 264, "plus3", "holes", (9,)),
    Case("w1e64-fp8", 1, 64, 8, 16, True, 16, "plus3", "random", (5,)),
    Case("w2e4-full", 2, 4, 2, 264, False, 264, "full", "single", (5, 3)),
    Case("w2e4-fp8", 2, 4, 2, 16, True, 264, "plus3", "random", (6, 4)),
    Case("w2e4-long-rows", 2, 4, 2, 2056, False, 2056, "plus3", "random", (3, 4)),
    Case("w3e2-starved", 3, 2, 1, 2056, False, 264, "plus3", "starved", (3, 2, 4)),
    Case("w3e2-k8-full", 3, 2, 8, 8, False, 264, "full", "single", (3, 2, 1)),
    Case("w4e8-fp8-idle", 4, 8, 2, 4112, True, 4112, "plus3", "idle", (3, 2, 0, 4)),
    Case("w4e8-fp8-one", 4, 8, 1, 16, True, 264, "one", "one", (0, 0, 1, 0)),
    Case("w8e1-full", 8, 1, 1, 8, False, 8, "full", "single", (4, 2, 1, 3, 2, 1, 2, 3)),
    Case("w8e8-k8-holes-idle", 8, 8, 8, 264, False, 264, "plus3", "holes", (2, 1, 3, 2, 1, 2, 0, 2)),
    Case("w8e8-k8-fp8-full", 8, 8, 8, 16, True, 16, "full", "single", (2, 1, 1, 2, 1, 1, 2, 1)),
]
CASE = {c.name: c for c in CASES}
COMBINE_CASES = ["w1e64-header-slot", "w2e4-full", "w2e4-long-rows", "w3e2-k8-full", "w4e8-fp8-one",
                 "w8e8-k8-holes-idle", "w8e1-full"]
CHAIN = Case("w2e4-routed", 2, 4, 2, 264, False, 264, "plus3", "router", (7, 5))


def _gen(c: Case) -> torch.Generator:
    return torch.Generator().manual_seed(1009 * c.W + 101 * c.El + 11 * c.k + c.d + sum(c.T))


def hole_experts(El: int) -> List[int]:
    """The local experts a "holes" routing leaves empty: the first, the last and two adjacent middle ones."""
    m = El // 2
    return [0, m - 1, m, El - 1]


def expert_ids(c: Case, gen: torch.Generator) -> List[torch.Tensor]:
    """ids [T_r, k] per rank, written as integer tables (a token may name an expert twice: the exchange kernels
    only see rows)."""
    out = []
    for r, T in enumerate(c.T):
        ids = torch.randint(0, c.E, (T, c.k), generator=gen)
        if c.routing == "single" and r == 0:
            ids[:] = c.E - 2 if c.E > 2 else c.E - 1          # one expert of the last destination
        elif c.routing == "starved":
            ids = ids % (c.E - c.El)                          # nobody sends to the last rank
        elif c.routing == "holes":
            allowed = torch.tensor([e for e in range(c.El) if e not in hole_experts(c.El)])
            ids = (ids // c.El) * c.El + allowed[ids % len(allowed)]
        elif c.routing == "one":
            ids[:] = c.E - 1
        if c.k == 1:                                          # experts descend with the token: src is no identity
            ids = ids.sort(0, descending=True).values
        out.append(ids)
    return out


def route_tables(ids: torch.Tensor, E: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(row_off [E + 1], src [T k], inv [T k]) int32: rows sorted by expert, the rows of one expert from the LAST
    token down (the contract fixes no order inside an expert; this one keeps src from ever being the identity)."""
    T, k = ids.shape
    rows = sorted((int(ids[t, j]), -t, j) for t in range(T) for j in range(k))
    rows = [(e, -t, j) for e, t, j in rows]
    row_off, src, inv = [0] * (E + 1), [0] * (T * k), [0] * (T * k)
    for p, (e, t, j) in enumerate(rows):
        row_off[e + 1] += 1
        src[p] = t
        inv[t * k + j] = p
    for e in range(E):
        row_off[e + 1] += row_off[e]
    return torch.tensor(row_off, dtype=I32), torch.tensor(src, dtype=I32), torch.tensor(inv, dtype=I32)


def tame(x: torch.Tensor) -> torch.Tensor:
    """bf16 codes with the exponent fields below 0x10 and from 0xF0 moved to the middle (their top bit flipped):
    times 2^+-2 stays normal and finite."""
    b = bits(x.clone())
    ex = (b.to(torch.int32) >> 7) & 0xFF
    b[(ex < 0x10) | (ex >= 0xF0)] ^= 0x4000
    return b.view(BF)


@dataclass
class Rank:
    x: torch.Tensor                       # [T, d] bf16, or uint8 codes of e4m3 rows
    xs: Optional[torch.Tensor]            # [T] f32
    ids: torch.Tensor
    row_off: torch.Tensor
    src: torch.Tensor
    inv: torch.Tensor
    w: torch.Tensor                       # [T, k] f32, one-hot
    o: Dict[str, torch.Tensor] = field(default_factory=dict)   # the oracle's buffers


def inputs(c: Case, ids: Optional[Sequence[torch.Tensor]] = None) -> List[Rank]:
    gen = _gen(c)
    ids = expert_ids(c, gen) if ids is None else ids
    total = sum(c.T)
    if c.fp8:
        allx = (torch.arange(total * c.d) * 3 + 1).remainder(256).to(U8).view(total, c.d)
        i = torch.arange(total)
        alls = ((2 * i + 1).float() * torch.exp2((i % 7 - 3).float()))
    else:
        allx, alls = tame(distinct((total, c.d), start=257)), None
    out, t0 = [], 0
    for r, T in enumerate(c.T):
        ro, src, inv = route_tables(ids[r], c.E)
        w = torch.zeros(T, c.k)
        if T:
            w[torch.arange(T), torch.randint(0, c.k, (T,), generator=gen)] = 1.0
        out.append(Rank(allx[t0:t0 + T].contiguous(), alls[t0:t0 + T].contiguous() if c.fp8 else None, ids[r], ro,
                        src, inv, w))
        t0 += T
    return out


# ---------------------------------------------------------------------------------------------------------
# the oracle: explicit loops over (source, expert, row), from the contract above


def as_bytes(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(U8).reshape(-1)


def factor(r: int, El: int, e: int) -> float:
    return 2.0 ** ((r * El + e) % 5 - 2)


def expert_rows(x: torch.Tensor, s: Optional[torch.Tensor], f: float, d_out: int) -> torch.Tensor:
    """The expert function on rows x [n, d] (bf16, or uint8 with scales s): bf16 [n, d_out]."""
    col = torch.arange(d_out) % x.shape[1]
    v = x[:, col].float()
    if s is not None:
        v = v * s.float()[:, None]
    return rne(v * f)


def oracle_send(c: Case, rk: Rank) -> Tuple[torch.Tensor, torch.Tensor]:
    """(send [W, (C + 1) RB] uint8, mask of the specified bytes)."""
    W, El, C, RB, rb = c.W, c.El, c.C, c.RB, c.row_bytes
    send = torch.zeros(W, C + 1, RB, dtype=U8)
    mask = torch.ones(W, C + 1, RB, dtype=torch.bool)
    xb = rk.x.contiguous().view(U8).view(rk.x.shape[0], rb)
    for r in range(W):
        for e in range(El):
            n = int(rk.row_off[r * El + e + 1]) - int(rk.row_off[r * El + e])
            send[r, 0, 4 * e:4 * e + 4] = as_bytes(torch.tensor([n], dtype=I32))
        base = int(rk.row_off[r * El])
        for j in range(int(rk.row_off[(r + 1) * El]) - base):
            t = int(rk.src[base + j])
            send[r, 1 + j, :rb] = xb[t]
            end = rb
            if c.fp8:
                send[r, 1 + j, rb:rb + 4] = as_bytes(rk.xs[t:t + 1])
                end = rb + 4
            mask[r, 1 + j, end:] = False
    return send.view(W, -1), mask.view(W, -1)


def header_counts(recv: torch.Tensor, W: int, El: int, C: int, RB: int) -> List[List[int]]:
    chunks = recv.view(W, C + 1, RB)
    return [[int(v) for v in chunks[s, 0, :4 * El].contiguous().view(I32)] for s in range(W)]


def sane(counts: List[List[int]], C: int) -> List[List[int]]:
    """A source with a negative count or a sum above C (Python integers: any width) sends nothing."""
    return [[0] * len(row) if (min(row) < 0 or sum(row) > C) else list(row) for row in counts]


def oracle_unpack(recv: torch.Tensor, W: int, El: int, C: int, RB: int, rb: int, fp8: bool) -> Dict[str, torch.Tensor]:
    """x_local (uint8 [W C, rb]; rows from ``n`` on unspecified, left zero), s_local, map, row_off_local, n."""
    chunks = recv.view(W, C + 1, RB)
    cnt = sane(header_counts(recv, W, El, C, RB), C)
    x_local = torch.zeros(W * C, rb, dtype=U8)
    s_local = torch.zeros(W * C, dtype=F32)
    rmap = torch.full((W * C,), -1, dtype=I32)
    rol = torch.zeros(El + 1, dtype=I32)
    pos = 0
    for e in range(El):
        for s in range(W):
            first = sum(cnt[s][:e])
            for i in range(cnt[s][e]):
                slot = chunks[s, 1 + first + i]
                x_local[pos] = slot[:rb]
                if fp8:
                    s_local[pos] = slot[rb:rb + 4].contiguous().view(F32)[0]
                rmap[s * C + first + i] = pos
                pos += 1
        rol[e + 1] = pos
    return {"x_local": x_local, "s_local": s_local, "map": rmap, "row_off_local": rol, "n": torch.tensor(pos)}


def oracle_experts(c: Case, r: int, o: Dict[str, torch.Tensor]) -> torch.Tensor:
    """y_local [W C, d_out] bf16, the NaN sentinel in the rows no segment names."""
    y = torch.empty(c.W * c.C, c.d_out, dtype=BF)
    bits(y).fill_(SENTINEL)
    x = o["x_local"] if c.fp8 else o["x_local"].view(BF)
    for e in range(c.El):
        a, b = int(o["row_off_local"][e]), int(o["row_off_local"][e + 1])
        y[a:b] = expert_rows(x[a:b], o["s_local"][a:b] if c.fp8 else None, factor(r, c.El, e), c.d_out)
    return y


def oracle_back(y_local: torch.Tensor, rmap: torch.Tensor, W: int, C: int) -> torch.Tensor:
    back = torch.zeros(W * C, y_local.shape[1], dtype=y_local.dtype)
    for s in range(W):
        for i in range(C):
            m = int(rmap[s * C + i])
            if m >= 0:
                back[s * C + i] = y_local[m]
    return back


def ret_position(row_off: torch.Tensor, p: int, El: int, C: int) -> int:
    E = row_off.numel() - 1
    r = next(q for q in range(E) if int(row_off[q]) <= p < int(row_off[q + 1])) // El
    return r * C + p - int(row_off[r * El])


def oracle_combine(ret: torch.Tensor, row_off, inv, w, El: int, C: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp64 sum, magnitude) [T, d_out]."""
    T = w.shape[0]
    out = torch.zeros(T, ret.shape[1], dtype=torch.float64)
    mag = torch.zeros_like(out)
    for t in range(T):
        for j in range(k):
            term = float(w[t, j]) * ret[ret_position(row_off, int(inv[t * k + j]), El, C)].double()
            out[t] += term
            mag[t] += term.abs()
    return out, mag


def exchange(bufs: Sequence[torch.Tensor], W: int) -> List[torch.Tensor]:
    """The all-to-all on [W, chunk] buffers: recv_r[s] = send_s[r]."""
    return [torch.stack([bufs[s].view(W, -1)[r] for s in range(W)]) for r in range(W)]


def oracle(c: Case, ranks: List[Rank]) -> List[Rank]:
    W, C = c.W, c.C
    for rk in ranks:
        rk.o["send"], rk.o["send_mask"] = oracle_send(c, rk)
    for r, recv in enumerate(exchange([rk.o["send"] for rk in ranks], W)):
        o = ranks[r].o
        o["recv"] = recv
        o["recv_mask"] = exchange([rk.o["send_mask"] for rk in ranks], W)[r]
        o.update(oracle_unpack(recv, W, c.El, C, c.RB, c.row_bytes, c.fp8))
        o["y_local"] = oracle_experts(c, r, o)
        o["back"] = oracle_back(o["y_local"], o["map"], W, C)
    for r, ret in enumerate(exchange([rk.o["back"].view(W, -1) for rk in ranks], W)):
        rk = ranks[r]
        rk.o["ret"] = ret.view(W * C, c.d_out)
        rk.o["out"], rk.o["mag"] = oracle_combine(rk.o["ret"], rk.row_off, rk.inv, rk.w, c.El, C, c.k)
    return ranks


def sorted_expert_outputs(c: Case, rk: Rank) -> torch.Tensor:
    """Y [R, d_out]: the expert output of sorted row p, straight from the token rows (no exchange)."""
    R = rk.src.numel()
    Y = torch.zeros(R, c.d_out, dtype=BF)
    for e in range(c.E):
        for p in range(int(rk.row_off[e]), int(rk.row_off[e + 1])):
            t = int(rk.src[p])
            Y[p] = expert_rows(rk.x[t:t + 1], rk.xs[t:t + 1] if c.fp8 else None, factor(e // c.El, c.El, e % c.El),
                               c.d_out)[0]
    return Y


def ret_from_sorted(Y: torch.Tensor, row_off: torch.Tensor, W: int, El: int, C: int) -> torch.Tensor:
    """The returned chunks [W C, d] that hold sorted rows Y, the NaN sentinel in every slot nothing names."""
    ret = torch.empty(W * C, Y.shape[1], dtype=BF)
    bits(ret).fill_(SENTINEL)
    for p in range(int(row_off[W * El])):
        ret[ret_position(row_off, p, El, C)] = Y[p]
    return ret


# ---------------------------------------------------------------------------------------------------------
# unspecified bytes, cages, messages


def fill_unspecified_send(buf: torch.Tensor, mask: torch.Tensor, fp8: bool) -> torch.Tensor:
    """``buf`` [W, (C + 1) RB] uint8 with the bytes outside ``mask`` replaced by the NaN sentinel (in place)."""
    n = buf.numel()
    if fp8:
        fill = torch.full((n,), 0xFF, dtype=U8, device=buf.device)
    else:
        fill = torch.tensor([SENTINEL & 0xFF, SENTINEL >> 8], dtype=U8, device=buf.device).repeat(n // 2)
    flat = buf.view(-1)
    m = ~mask.to(buf.device).view(-1)
    flat[m] = fill[m]
    return buf


def fill_unspecified_rows(x_local: torch.Tensor, s_local: Optional[torch.Tensor], n: int, fp8: bool) -> None:
    """Rows of x_local / s_local from ``n`` on take the NaN sentinel (in place; x_local uint8 or bf16)."""
    if x_local.dtype == U8:
        if fp8:
            x_local[n:] = 0xFF
        else:
            x_local[n:].view(torch.int16).fill_(SENTINEL)
    else:
        bits(x_local)[n:] = SENTINEL
    if s_local is not None:
        s_local.view(I32)[n:] = SENT32


class PadCage:
    """``rows`` rows of ``cols`` elements with ``pad`` sentinel rows before and after (pad a multiple of 16), inside a
    RowCage: ``view`` is contiguous and 16-byte aligned; ``touched`` counts every sentinel lost around it."""

    def __init__(self, rows: int, cols: int, device="cpu", dtype=BF, pad: int = 16):
        assert pad % 16 == 0
        self.rows, self.pad = rows, pad
        self.cage = RowCage((rows + 2 * pad, cols), device, dtype)
        self.view = self.cage.view[pad:pad + rows]
        self.flat = self.view.view(-1)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0

    def touched(self) -> int:
        v, p = self.cage.view.view(self.cage.raw_dtype), self.pad
        return int((v[:p] != self.cage.code).sum()) + int((v[p + self.rows:] != self.cage.code).sum()) + \
            self.cage.outside_touched()

    def unwritten(self) -> int:
        return int((self.view.reshape(-1).view(self.cage.raw_dtype) == self.cage.code).sum())

    def same_as(self, other: "PadCage") -> bool:
        return torch.equal(self.cage.buf.view(self.cage.raw_dtype), other.cage.buf.view(other.cage.raw_dtype))


def poison_pad(W: int, El: int, C: int) -> int:
    """Pad rows around x_local / s_local / map for the poisoned headers: at least C + W El, a multiple of 16."""
    return -(-(C + W * El) // 16) * 16


def first_byte(kernel: str, rank: int, got: torch.Tensor, want: torch.Tensor, mask: Optional[torch.Tensor],
               chunk_rows: int, row_bytes: int, header: bool) -> Optional[str]:
    """None if the bytes agree (under ``mask``), else a message naming kernel, rank, source / destination chunk, slot
    and first differing byte.  Buffers are [W chunks][chunk_rows rows][row_bytes]."""
    g, w = as_bytes(got.cpu()), as_bytes(want.cpu())
    bad = g != w
    if mask is not None:
        bad &= mask.reshape(-1)
    if not bool(bad.any()):
        return None
    i = int(bad.nonzero()[0])
    row, byte = divmod(i, row_bytes)
    chunk, slot = divmod(row, chunk_rows)
    where = f"chunk {chunk} slot {slot}" + (" (header)" if header and slot == 0 else "")
    return (f"{kernel} rank {rank}: {int(bad.sum())} bytes differ, first at {where} byte {byte}: got {int(g[i]):#04x} "
            f"want {int(w[i]):#04x}")


def rows_message(kernel: str, rank: int, got: torch.Tensor, want: torch.Tensor, n: int, o: Dict[str, torch.Tensor],
                 C: int) -> Optional[str]:
    """x_local-style rows [W C, *] compared over the first n rows; names the (source, slot) whose row it is."""
    g, w = got.cpu().contiguous().view(U8).view(got.shape[0], -1)[:n], want.contiguous().view(U8).view(
        want.shape[0], -1)[:n]
    bad = g != w
    if not bool(bad.any()):
        return None
    row, byte = (int(v) for v in bad.nonzero()[0])
    at = (o["map"] == row).nonzero()
    s, i = divmod(int(at[0]), C) if at.numel() else (-1, -1)
    return (f"{kernel} rank {rank}: {int(bad.sum())} bytes differ, first in row {row} (source {s} slot {i}) byte "
            f"{byte}: got {int(g[row, byte]):#04x} want {int(w[row, byte]):#04x}")


def ints_message(kernel: str, rank: int, what: str, got: torch.Tensor, want: torch.Tensor, C: int = 0) -> Optional[str]:
    bad = same32(got.cpu(), want)
    if not bool(bad.any()):
        return None
    i = int(bad.nonzero()[0])
    at = f"source {i // C} slot {i % C}" if C else f"entry {i}"
    return (f"{kernel} rank {rank}: {int(bad.sum())} entries of {what} differ, first at {at}: got "
            f"{got.view(-1)[i].item()!r} want {want.view(-1)[i].item()!r}")


# ---------------------------------------------------------------------------------------------------------
# poisoned headers (ep_unpack only; recv built on the host)


POISONS = ["all_ones", "minus_one", "over_capacity", "int32_wrap"]
POISON_GEOS = [(3, 4, 8, False), (2, 4, 16, True)]          # (W, El, d, fp8)


def poisoned_recv(W: int, El: int, d: int, fp8: bool, kind: str):
    """(recv [W, (C + 1) RB] uint8, C, RB, row_bytes, bad source).  The last source is poisoned; the others send rows
    for every local expert but expert 1, so that an unsanitised kernel's indices stay near the buffers (see
    ``emul_unpack(sanitise=False)`` and tests/test_ep_probes.py)."""
    rb = d * (1 if fp8 else 2)
    RB = -(-max(rb + (4 if fp8 else 0), 4 * El) // 16) * 16
    counts = [[(2 + s + e) % 3 + (1 if e == 0 else 0) if e != 1 else 0 for e in range(El)] for s in range(W)]
    C = max(sum(row) for row in counts) + 2
    bad = W - 1
    recv = torch.zeros(W, C + 1, RB, dtype=U8)
    for s in range(W):
        recv[s, 0, :4 * El] = as_bytes(torch.tensor(counts[s], dtype=I32))
        for i in range(C):                                   # every slot holds a row: a poisoned chunk's too
            recv[s, 1 + i] = ((torch.arange(RB) * 5 + 31 * i + 97 * s + 1) % 251).to(U8)
            if fp8:
                recv[s, 1 + i, rb:rb + 4] = as_bytes(torch.tensor([(2 * (s * C + i) + 1) * 0.125], dtype=F32))
    if kind == "all_ones":
        recv[bad] = 0xFF
    else:
        row = {"minus_one": [1, 0, -1, 2] + [0] * (El - 4),
               "over_capacity": [C - 1, 0, 1, 1] + [0] * (El - 4),
               "int32_wrap": [2 ** 31 - 1, 2 ** 31 - 1, 2] + [0] * (El - 3)}[kind]
        recv[bad, 0, :4 * El] = as_bytes(torch.tensor(row, dtype=I32))
    return recv.view(W, -1), C, RB, rb, bad


# ---------------------------------------------------------------------------------------------------------
# emulations of the four kernels (after their code, block by block), each with switches that break it one way


def _i32(v: int) -> int:
    """Two's-complement wrap to int32, as the kernel's ``int`` arithmetic behaves on the device."""
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def emul_pack(x: torch.Tensor, xs: Optional[torch.Tensor], src: Optional[torch.Tensor], row_off: torch.Tensor,
              W: int, El: int, C: int, RB: int, send: torch.Tensor, *, ignore_src: bool = False,
              shift_header: bool = False) -> None:
    """Writes ``send`` [W, (C + 1) RB] uint8 in place, one (slot, r) block at a time."""
    rb = x.shape[1] * x.element_size()
    xb = x.contiguous().view(U8).view(x.shape[0], rb)
    chunks = send.view(W, C + 1, RB)
    ro = [int(v) for v in row_off] + [int(row_off[-1])]
    for r in range(W):
        base, n = ro[r * El], ro[(r + 1) * El] - ro[r * El]
        for slot in range(C + 1):
            dst = chunks[r, slot]
            if slot == 0:
                dst.zero_()
                h = 1 if shift_header else 0
                dst[:4 * El] = as_bytes(torch.tensor([ro[r * El + e + 1 + h] - ro[r * El + e + h] for e in range(El)],
                                                     dtype=I32))
            elif slot - 1 >= n:
                dst.zero_()
            else:
                p = base + slot - 1
                row = p if (src is None or ignore_src) else int(src[p])
                dst[:rb] = xb[row % max(xb.shape[0], 1)]
                if xs is not None:
                    dst[rb:rb + 4] = as_bytes(xs[row % max(xs.shape[0], 1)].reshape(1))


def emul_counts(recv: torch.Tensor, W: int, El: int, C: int, RB: int, *, sanitise: bool = True,
                int32_sum: bool = False, allow_negative: bool = False):
    """(cnt, em, cum, tot) as ``ep_counts`` leaves them (flat [W El] / [W] lists of wrapped ints)."""
    raw = header_counts(recv, W, El, C, RB)
    cnt = [v for row in raw for v in row]
    cum, tot, em = [0] * (W * El), [0] * W, [0] * (W * El)
    for s in range(W):
        total, bad = 0, False
        for e in range(El):
            v = cnt[s * El + e]
            bad |= (v < 0) and not allow_negative
            total = _i32(total + v) if int32_sum else total + v
        bad |= total > C
        acc = 0
        for e in range(El):
            if bad and sanitise:
                cnt[s * El + e] = 0
            cum[s * El + e] = acc
            acc = _i32(acc + cnt[s * El + e])
        tot[s] = acc
    return cnt, em, cum, tot


def emul_unpack(recv: torch.Tensor, W: int, El: int, C: int, RB: int, rb: int, fp8: bool, x_local: torch.Tensor,
                s_local: Optional[torch.Tensor], rmap: torch.Tensor, rol: torch.Tensor, *, sanitise: bool = True,
                int32_sum: bool = False, allow_negative: bool = False, rank_major: bool = False,
                scale_at_end: bool = False, trace: Optional[List[Tuple[str, int]]] = None) -> None:
    """Writes x_local (uint8 [W C, rb]), s_local, map, row_off_local in place.  Every row index formed is appended to
    ``trace`` as (buffer, row); a write outside a buffer is recorded and not made."""
    chunks = recv.view(W, C + 1, RB)
    cnt, em, cum, tot = emul_counts(recv, W, El, C, RB, sanitise=sanitise, int32_sum=int32_sum,
                                    allow_negative=allow_negative)
    acc = 0
    order = [(s, e) for s in range(W) for e in range(El)] if rank_major else \
        [(s, e) for e in range(El) for s in range(W)]
    for s, e in order:
        em[s * El + e] = acc
        acc = _i32(acc + cnt[s * El + e])
    acc = 0
    rol[0] = 0
    for e in range(El):
        for q in range(W):
            acc = _i32(acc + cnt[q * El + e])
        rol[e + 1] = acc
    note = trace.append if trace is not None else (lambda item: None)
    for s in range(W):
        for i in range(C):
            note(("map", s * C + i))
            if i >= tot[s]:
                rmap[s * C + i] = -1
                continue
            e = 0
            while e + 1 < El and i >= cum[s * El + e + 1]:
                e += 1
            dest = _i32(em[s * El + e] + (i - cum[s * El + e]))
            note(("x_local", dest))
            rmap[s * C + i] = dest
            if not 0 <= dest < W * C:
                continue
            row = chunks[s, 1 + i]
            x_local[dest] = row[:rb]
            if fp8:
                at = RB - 4 if scale_at_end else rb
                s_local.view(I32)[dest] = row[at:at + 4].contiguous().view(I32)[0]


def emul_back(y_local: torch.Tensor, rmap: torch.Tensor, W: int, C: int, back: torch.Tensor, *,
              skip_unused: bool = False) -> None:
    for q in range(W * C):
        m = int(rmap[q])
        if m < 0:
            if not skip_unused:
                bits(back)[q] = 0
        else:
            bits(back)[q] = bits(y_local)[m]


def emul_combine(ret: torch.Tensor, row_off: torch.Tensor, inv: torch.Tensor, w: torch.Tensor, El: int, C: int,
                 k: int, *, base_from_expert: bool = False, w_bf16: bool = False) -> torch.Tensor:
    """bf16 [T, d] from an unfused fp32 sum in slot order."""
    E, T = row_off.numel() - 1, w.shape[0]
    ro = [int(v) for v in row_off]
    acc = torch.zeros(T, ret.shape[1])
    for t in range(T):
        for j in range(k):
            p, e = int(inv[t * k + j]), 0
            while e + 1 < E and p >= ro[e + 1]:
                e += 1
            r = e // El
            pos = r * C + p - (ro[e] if base_from_expert else ro[r * El])
            wj = w[t, j].to(BF).float() if w_bf16 else w[t, j].float()
            acc[t] = acc[t] + wj * ret[pos % ret.shape[0]].float()
    return acc.to(BF)
