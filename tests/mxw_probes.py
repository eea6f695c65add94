"""Packed weights, an independent reference, exact operands and deliberately wrong readers for the four kernels that
read an MXFP4 weight: mxfp4_dequant and skinny_mxfp4 (mxfp4.hip), moe_skinny_mxfp4 (moe_mxfp4.hip) and gemm_mxfp4_a8
(mxfp4_a8.hip).

Weights are built as code bytes and scale bytes, not through ``quant_mxfp4_weight``: all 16 codes (``-0``, code 8,
included) under any admitted scale byte.  The reference value of a (code, byte) pair is this module's own table
times 2^(byte - 127) in fp64; it never calls ``ops.dequant_mxfp4`` (tests/test_mxw_probes.py pins that the two
agree on all 16 x 255 pairs).

Families:
  range     ``range_weight``: row n under scale byte n (its odd blocks under 254 - n), every block holding all 16
            codes twice.  ``full`` (bytes 0 to 254) for the dequantiser; ``finite`` for the GEMMs, where a block whose
            byte overflows some code keeps only the codes that stay finite (0 * inf would poison a one-hot row).
  dense     ``dense``: random codes, one scale byte per W row (13 exponents), A = +-1 at one k of every 8.  The sum of
            |terms| of any output is below 2^24 smallest products (``headroom``), so every partial sum in any order is
            exact in fp32 and the kernel's answer is ``want`` = RNE_bf16(exact) bit for bit whatever its reduction
            order; 1-in-8 density keeps the sums small enough that at least 90 % of the exact values are themselves
            bf16 numbers (``exact_share``), where an error of one product changes the stored bits.  ``wide`` rows
            (odd groups +-2^-5) keep the first premise and make the partial sums wider than bf16.
  swiglu    ``swiglu``: gate|up stacks whose gate is decided by two activation columns (k = 0 and k = 32, two blocks
            under different scales): zero, moderate (|g| <= 8) and saturated (+-96, +-200) by column, ups random.  The
            saturated premise is that of tests/mx_probes.py: 1 + exp(-g) is 1 in fp32 from g = 17 up, so silu(g) = g
            and the output is RNE(g * u); at g <= -89 exp(-g) is inf in fp32 and silu must come out as a zero.
  segments  ``segments``: 9 experts with rows [33, 48, 0, 49, 63, 1, 64, 17, 80], every expert its own codes, a
            gather with repeated source rows and the expert-major form.

The last part holds the emulated readers and their mutants for tests/test_mxw_probes.py.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import torch

from tests import gemm_probes as gp

GRID16 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)
SEG_LENS = (33, 48, 0, 49, 63, 1, 64, 17, 80)
SATURATED = (96.0, -96.0, 200.0, -200.0)
SAT_POS, SAT_NEG = 17.0, -89.0   # 1 + exp(-17) rounds to 1 in fp32; exp(89) is above fp32's largest value


# ---------------------------------------------------------------------------------------------------------
# packed weights and the reference


def pack(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes [..., K] -> bytes [..., K / 2]: k = 2j in the low nibble of byte j."""
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).contiguous()


def unpack(q: torch.Tensor) -> torch.Tensor:
    return torch.stack([q & 0xF, q >> 4], dim=-1).reshape(*q.shape[:-1], -1)


def values(codes: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp64 [..., K] of codes [..., K] under scale bytes [..., K / 32]: GRID16[code] * 2^(byte - 127)."""
    t = torch.tensor(GRID16, dtype=torch.float64)
    return t[codes.long()] * torch.exp2(s.double() - 127.0).repeat_interleave(32, dim=-1)


def pair_weight():
    """Every (code, byte) pair: q [255, 16], s [255, 1]; row b is one block under byte b, code c at k = c and
    k = 16 + c."""
    codes = (torch.arange(32) % 16).to(torch.uint8).expand(255, 32)
    return pack(codes), torch.arange(255, dtype=torch.uint8).view(255, 1)


def pair_values() -> torch.Tensor:
    """fp64 [255, 16]: the value of code c under byte b."""
    q, s = pair_weight()
    return values(unpack(q), s)[:, :16]


def nonfinite_pairs() -> List[tuple]:
    """The (code, byte) pairs whose value is not a finite bf16, computed from the format."""
    bad = ~torch.isfinite(gp.rne(pair_values()).float())
    return [(int(c), int(b)) for b, c in bad.nonzero().tolist()]


def range_weight(variant: str = "full"):
    """codes [256, 256], q [256, 128] and s [256, 8]: row n under byte n in its even blocks and byte 254 - n in its
    odd ones (a reader that takes a neighbouring block's scale must show; row 255, whose byte the format does not
    admit, under 127); block b of row n holds all 16 codes twice, code (j + 5 n + 3 b) % 16 at its position j.
    ``finite``: where a block's byte overflows a magnitude, the magnitude index is folded onto the finite ones."""
    assert variant in ("full", "finite")
    n = torch.arange(256).view(256, 1, 1)
    b = torch.arange(8).view(1, 8, 1)
    j = torch.arange(32).view(1, 1, 32)
    codes = ((j + 5 * n + 3 * b) % 16).expand(256, 8, 32)
    byte = torch.where(b % 2 == 0, n, 254 - n).expand(256, 8, 1)
    byte = torch.where(n <= 254, byte, torch.full_like(byte, 127))
    if variant == "finite":
        bad = ~torch.isfinite(gp.rne(pair_values()).float())             # [255 bytes, 16 codes]
        nfin = (~bad[:, :8]).sum(1)[byte.reshape(-1)].view(256, 8, 1)   # finite magnitudes: a prefix of the grid
        codes = (codes & 8) | ((codes & 7) % nfin)
    codes = codes.reshape(256, 256).to(torch.uint8)
    s = byte.reshape(256, 8).to(torch.uint8).contiguous()
    return SimpleNamespace(codes=codes, q=pack(codes), s=s, W=values(codes, s))


def range_ks() -> List[int]:
    """128 k of the range weight's 256: positions 0..15 of the even blocks and 16..31 of the odd ones, so every
    block shows all 16 codes and both halves of a block are read."""
    return [32 * b + 16 * (b % 2) + j for b in range(8) for j in range(16)]


def a_scales(M: int) -> torch.Tensor:
    return torch.exp2(((torch.arange(M) % 5) - 2).float())


def one_hot_law(W: torch.Tensor, ks, a: torch.Tensor) -> torch.Tensor:
    """bf16 [M, N] a GEMM reader owes for one-hot rows (row m: ``a[m]`` at k = ks[m], or 1 there and ``a`` as the
    row scale) over the fp64 weight ``W``: RNE(W[n, k_m] * a[m]), with +0 where that is -0.  The dequantiser stores
    code 8 as -0; a GEMM adds the product -0 to an accumulator that starts at +0, and (+0) + (-0) = +0 in
    round-to-nearest, so the sign of a zero weight does not reach the output.  An overflow to inf does."""
    return gp.rne(W.double()[:, list(ks)].t() * a.double()[:, None] + 0.0)


# ---------------------------------------------------------------------------------------------------------
# dense exact operands


def row_bytes(N: int) -> torch.Tensor:
    return (127 + (torch.arange(N) % 13) - 6).to(torch.uint8)


WIDE_STEP = 2.0 ** -5   # the odd groups of a ``wide`` row


def thin_rows(M: int, K: int, gen: torch.Generator, wide: bool = False) -> torch.Tensor:
    """fp32 A [M, K]: +-1 at one k of every 8, position (m + 3 group) % 8, so 8 consecutive rows cover every k.
    ``wide``: the odd groups hold +-2^-5 (a bf16 and an e4m3 number), so a sum over as few as two groups needs more
    than bf16's 8 bits: a partial that went through bf16 shows.  The plain rows cannot see that: a wave's partial is
    at most 32 terms of at most 12 half-units, nearly always a bf16."""
    G = K // 8
    m, g = torch.arange(M).view(M, 1), torch.arange(G).view(1, G)
    A = torch.zeros(M, K)
    v = gp._signs((M, G), gen)
    if wide:
        v = v * torch.where(g % 2 == 1, WIDE_STEP, 1.0)
    A[m.expand(M, G), (8 * g + (m + 3 * g) % 8)] = v
    return A


def dense(M: int, N: int, K: int, gen: torch.Generator, wide: bool = False):
    """Random codes [N, K] under one byte per row, A = thin_rows.  ``acc`` is the exact fp64 product, ``want`` its
    RNE bf16, ``exact_share`` the share of outputs whose exact value is a bf16, ``headroom`` the largest sum of
    |terms| of an output in units of its smallest non-zero product (0.5 * 2^(byte - 127), ``wide``: times 2^-5)."""
    assert K % 128 == 0
    codes = torch.randint(0, 16, (N, K), generator=gen).to(torch.uint8)
    s = row_bytes(N).view(N, 1).expand(N, K // 32).contiguous()
    A = thin_rows(M, K, gen, wide)
    W = values(codes, s)
    acc = A.double() @ W.t()
    want = gp.rne(acc)
    unit = 0.5 * torch.exp2(row_bytes(N).double() - 127.0) * (WIDE_STEP if wide else 1.0)
    headroom = float(((A.abs().double() @ W.abs().t()) / unit[None, :]).max())
    share = float((want.double() == acc).double().mean())
    return SimpleNamespace(A=A, codes=codes, q=pack(codes), s=s, W=W, acc=acc, want=want, exact_share=share,
                           headroom=headroom)


SKINNY_M = (1, 7, 16, 17, 32, 33, 48, 49, 64)
SKINNY_SHAPES = ((16, 128), (48, 384), (64, 1152), (6144, 1152))   # the last: 32 columns per workgroup
A8_M = (1, 16, 127, 128, 129, 257)
A8_SHAPES = ((16, 128), (144, 256), (112, 512), (1040, 384), (128, 1152))
SHIFTS = 8   # a launch of M < 8 rows is repeated on rows [s, s + M) for s < 8: together they cover every k
_dense = {}


WIDE_SHAPES = ((48, 384), (64, 1152))   # the weight-stream shapes that are also run on ``wide`` rows


def dense_case(N: int, K: int, rows: int, wide: bool = False):
    """``dense(rows + 8, N, K)``, built once per shape and never changed; a test of M rows takes rows [s, s + M)."""
    key = (N, K, rows, wide)
    if key not in _dense:
        _dense[key] = dense(rows + SHIFTS, N, K, torch.Generator().manual_seed(1000 * N + K + wide), wide)
    return _dense[key]


def shifts(M: int) -> range:
    return range(SHIFTS if M < 8 else 1)


# ---------------------------------------------------------------------------------------------------------
# gate|up stacks


def interleave(x: torch.Tensor) -> torch.Tensor:
    """[gate (F rows); up (F rows)] -> gate[0:32], up[0:32], gate[32:64], ... (what the kernels read)."""
    F = x.shape[0] // 2
    return torch.stack([x[:F].reshape(F // 32, 32, -1), x[F:].reshape(F // 32, 32, -1)], 1).reshape(x.shape)


def gated_rows(M: int, K: int, gen: torch.Generator) -> torch.Tensor:
    """thin_rows with the groups of k = 0 and k = 32 replaced by a row sign at k = 0 and k = 32 (row m: + for
    even m): the two columns the gate weights read."""
    A = thin_rows(M, K, gen)
    A[:, 0:8], A[:, 32:40] = 0, 0
    sgn = 1.0 - 2.0 * (torch.arange(M) % 2).float()
    A[:, 0], A[:, 32] = sgn, sgn
    return A


def gate_up_weight(F: int, K: int, gen: torch.Generator, moderate: bool = True, rot: int = 0):
    """codes [2 F, K] and bytes [2 F, K / 32] in [gate; up] order and ``g`` [F], the gate a row of sign + reaches.
    Gate rows hold code 0 except at k = 0 and k = 32; column f's class is (f + rot) % 3 (0 zero, 1 moderate, 2
    saturated; without ``moderate`` class 1 is saturated too).  Zero: +-0 codes everywhere.  Moderate: +-(0.5..6) at
    k = 0 and (0..2) of the same sign at k = 32 under byte 127.  Saturated: +-96 = 6 * 2^4 at k = 0, or +-200 = 6 * 2^5 at k = 0
    plus 4 * 2^1 at k = 32.  Up rows: random codes under byte 127 - f % 4."""
    assert F % 32 == 0 and K >= 128
    codes = torch.zeros(2 * F, K, dtype=torch.uint8)
    s = torch.full((2 * F, K // 32), 127, dtype=torch.uint8)
    codes[F:] = torch.randint(0, 16, (F, K), generator=gen).to(torch.uint8)
    s[F:] = (127 - torch.arange(F) % 4).to(torch.uint8).view(F, 1)
    cls = torch.zeros(F, dtype=torch.int64)
    for f in range(F):
        c = (f + rot) % 3
        if c == 1 and not moderate:
            c = 2
        cls[f] = c
        if c == 0:
            codes[f] = (torch.randint(0, 2, (K,), generator=gen) * 8).to(torch.uint8)
        elif c == 1:
            neg = 8 * int(torch.randint(0, 2, (1,), generator=gen))
            codes[f, 0] = int(torch.randint(1, 8, (1,), generator=gen)) | neg
            codes[f, 32] = int(torch.randint(0, 5, (1,), generator=gen)) | neg
        else:
            v = SATURATED[(f // 3 + rot) % 4]
            neg = 8 if v < 0 else 0
            if abs(v) == 96.0:
                codes[f, 0], s[f, 0] = 7 | neg, 131
            else:
                codes[f, 0], s[f, 0] = 7 | neg, 132
                codes[f, 32], s[f, 1] = 6 | neg, 128
    W = values(codes, s)
    g = W[:F, 0] + W[:F, 32]
    return SimpleNamespace(codes=codes, s=s, W=W, g=g, cls=cls, F=F)


def swiglu(M: int, F: int, K: int, gen: torch.Generator, moderate: bool = True):
    """A = gated_rows and one gate|up weight: ``q`` / ``s`` interleaved as the kernels read them, ``gate`` / ``up``
    fp64 [M, F] (exact small integers times powers of two), ``want`` = the fp64 silu(gate) * up."""
    w = gate_up_weight(F, K, gen, moderate)
    A = gated_rows(M, K, gen)
    gu = A.double() @ w.W.t()
    gate, up = gu[:, :F].contiguous(), gu[:, F:].contiguous()
    return SimpleNamespace(A=A, q=pack(interleave(w.codes)), s=interleave(w.s).contiguous(), W=w.W, gate=gate, up=up,
                           cls=w.cls, want=gp.silu_mul(gate, up), F=F)


def swiglu_violations(got: torch.Tensor, gate: torch.Tensor, up: torch.Tensor) -> List[str]:
    """What a SwiGLU epilogue got wrong on exact gate / up sums (fp64, same shape as ``got``): anything non-finite;
    a zero gate must give the bits of 0 * up (a zero with up's sign); a gate >= 17 the bits of RNE(gate * up); a gate
    <= -89 a zero of either sign; anything else is held to ``one_step`` of the fp64 value."""
    gate, up = gate.to(got.device), up.to(got.device)
    out = []
    fin = torch.isfinite(got.float())
    if not bool(fin.all()):
        i = [int(v) for v in (~fin).nonzero()[0]]
        out.append(f"{int((~fin).sum())} non-finite outputs; first at {i} (gate {float(gate[tuple(i)]):g})")
    zero, pos, neg = gate == 0, gate >= SAT_POS, gate <= SAT_NEG
    rules = (("zero gate", zero, gp.bitwise(got, gate * up)),
             ("saturated gate", pos, gp.bitwise(got, gate * up)),
             ("negative saturated gate", neg, got.float() != 0),
             ("moderate gate", ~(zero | pos | neg), gp.one_step(got, gp.silu_mul(gate, up))))
    for name, where, bad in rules:
        bad = bad & where
        if bool(bad.any()):
            i = [int(v) for v in bad.nonzero()[0]]
            out.append(f"{name}: {int(bad.sum())} of {int(where.sum())} outputs off; first at {i}: got "
                       f"{float(got[tuple(i)]):.8g}, gate {float(gate[tuple(i)]):g}, up {float(up[tuple(i)]):g}")
    return out


# ---------------------------------------------------------------------------------------------------------
# segments


def segments(N: int, K: int, gen: torch.Generator, swiglu_: bool = False, T: int = 40):
    """9 experts over SEG_LENS rows: ``A`` [T, K] source rows, ``a_rows`` (row i reads source row (7 i + 3) % T:
    repeats), ``A_em`` = A[a_rows] (the expert-major form), ``row_off`` [10] and the stack ``q`` [9, N, K / 2], ``s``
    [9, N, K / 32].  Plain: ``acc`` fp64 [rows, N] per expert from the fp64 product.  SwiGLU: W[e] is a gate|up
    weight (N = 2 F, no moderate class, classes rotated per expert) and ``gate`` / ``up`` are fp64 [rows, F]."""
    E, rows = len(SEG_LENS), sum(SEG_LENS)
    row_off = torch.tensor((0,) + SEG_LENS).cumsum(0).to(torch.int32)
    a_rows = ((torch.arange(rows) * 7 + 3) % T).to(torch.int32)
    A = gated_rows(T, K, gen) if swiglu_ else thin_rows(T, K, gen)
    A_em = A[a_rows.long()]
    out = SimpleNamespace(A=A, a_rows=a_rows, A_em=A_em, row_off=row_off, rows=rows, E=E, lens=SEG_LENS)
    qs, ss, Ws = [], [], []
    for e in range(E):
        if swiglu_:
            w = gate_up_weight(N // 2, K, gen, moderate=False, rot=e)
            qs.append(pack(interleave(w.codes)))
            ss.append(interleave(w.s))
            Ws.append(w.W)
        else:
            codes = torch.randint(0, 16, (N, K), generator=gen).to(torch.uint8)
            s = torch.roll(row_bytes(N), e).view(N, 1).expand(N, K // 32)
            qs.append(pack(codes))
            ss.append(s)
            Ws.append(values(codes, s))
    out.q, out.s, out.W = torch.stack(qs), torch.stack(ss).contiguous(), torch.stack(Ws)
    acc = segment_product(out)
    if swiglu_:
        out.gate, out.up = acc[:, :N // 2].contiguous(), acc[:, N // 2:].contiguous()
    else:
        out.acc = acc
    return out


def segment_product(sg, shift_expert: int = 0, identity_gather: bool = False) -> torch.Tensor:
    """fp64 [rows, N]: rows of expert e times W[e] ([gate; up] order for a gate|up stack).  Wrong references:
    ``shift_expert`` = 1 reads W[e + 1] (the last expert W[0]); ``identity_gather`` takes source row i for row i."""
    x = sg.A[(torch.arange(sg.rows) % sg.A.shape[0])] if identity_gather else sg.A_em
    ro = sg.row_off.tolist()
    parts = [x[ro[e]:ro[e + 1]].double() @ sg.W[(e + shift_expert) % sg.E].t() for e in range(sg.E)]
    return torch.cat(parts)


# ---------------------------------------------------------------------------------------------------------
# reporting: first mismatch as (row, column, k, byte)


def bit_violations(cage: gp.Cage, want: torch.Tensor, ks=None, s: Optional[torch.Tensor] = None) -> List[str]:
    """Bitwise comparison that admits non-finite references (the overflowing pairs): differing bits inside, touched
    sentinels outside.  ``ks`` [M]: the k a one-hot row probes; ``s`` [N, K / 32]: the weight's scale bytes."""
    out = []
    want = gp.rne(want) if want.dtype != torch.bfloat16 else want
    want = want.to(cage.view.device)
    bad = gp.bits(cage.view) != gp.bits(want)
    if bool(bad.any()):
        m, n = (int(v) for v in bad.nonzero()[0])
        where = f"(row {m}, column {n}"
        if ks is not None:
            where += f", k {int(ks[m])}"
            if s is not None:
                where += f", byte {int(s[n, int(ks[m]) // 32])}"
        out.append(f"{int(bad.sum())} of {bad.numel()} outputs differ; first at {where}): got "
                   f"0x{int(gp.bits(cage.view)[m, n]) & 0xFFFF:04x} ({float(cage.view[m, n]):.6g}) want "
                   f"0x{int(gp.bits(want)[m, n]) & 0xFFFF:04x} ({float(want[m, n]):.6g})")
    t = cage.outside_touched()
    if t:
        out.append(f"{t} sentinels outside [:{cage.M}, :{cage.NC}] overwritten")
    return out


# ---------------------------------------------------------------------------------------------------------
# emulated readers and their mutants (CPU tests only)


def _flush_subnormal(x: torch.Tensor) -> torch.Tensor:
    f = x.float()
    return torch.where(f.abs() < 2.0 ** -126, torch.copysign(torch.zeros_like(f), f), f).to(torch.bfloat16)


def read_weight(q: torch.Tensor, s: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    """The dequantiser written from the kernel: per 8 codes a convert with the block's scale -> bf16 [N, K].
    Mutants: ``nibbles`` (k = 2j in the high nibble), ``block`` (the scale of block b ^ 1), ``byte0`` (byte 0 read as
    the float 0.0: ``s << 23``), ``flush`` (bf16 subnormal results flushed to zero), ``saturate`` (overflow gives the
    largest finite bf16), ``plus_zero`` (code 8 stored as +0)."""
    codes = unpack(q)
    if mutant == "nibbles":
        codes = torch.stack([q >> 4, q & 0xF], dim=-1).reshape(codes.shape)
    if mutant == "block":
        s = s[:, torch.arange(s.shape[1]) ^ 1]
    scale = torch.exp2(s.double() - 127.0)
    if mutant == "byte0":
        scale = torch.where(s == 0, torch.zeros_like(scale), scale)
    v = torch.tensor(GRID16, dtype=torch.float64)[codes.long()] * scale.repeat_interleave(32, dim=-1)
    out = gp.rne(v)
    if mutant == "flush":
        out = _flush_subnormal(out)
    if mutant == "saturate":
        big = torch.tensor(0x7F7F, dtype=torch.int16).view(torch.bfloat16).float()
        f = out.float()
        out = torch.where(torch.isinf(f), torch.copysign(big, f), f).to(torch.bfloat16)
    if mutant == "plus_zero":
        out = torch.where(out == 0, torch.zeros_like(out), out)
    return out


def wave_batches(K: int, w: int):
    """The 128-k batches [b0, b0 + nb) of wave w of the 8-wave K split of skinny_mxfp4 / moe_skinny_mxfp4."""
    nbt = K // 128
    b0 = (w * nbt) // 8
    return b0, ((w + 1) * nbt) // 8 - b0


def read_stream(A: torch.Tensor, W: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    """The weight-stream kernels' sum, fp64 [M, N]: per wave the batches of its K share, then the 8 partials in wave
    order.  Mutants: ``twice`` / ``dropped`` (the last batch of the first wave with an odd batch count is added twice
    / left out: the ``past`` branch of the two-batch register sets), ``bf16_partial`` (a wave's partial rounded to
    bf16 before the cross-wave sum)."""
    A, W = A.double(), W.double()
    K = A.shape[1]
    total = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float64)
    hit = False
    for w in range(8):
        b0, nb = wave_batches(K, w)
        part = torch.zeros_like(total)
        for b in range(b0, b0 + nb):
            k = slice(128 * b, 128 * b + 128)
            times = 1.0
            if nb % 2 == 1 and b == b0 + nb - 1 and not hit and mutant in ("twice", "dropped"):
                times, hit = (2.0 if mutant == "twice" else 0.0), True
            part += times * (A[:, k] @ W[:, k].t())
        if mutant == "bf16_partial":
            part = gp.rne(part).double()
        total += part
    return total


def read_tiles(A: torch.Tensor, W: torch.Tensor, stale: bool = False) -> torch.Tensor:
    """gemm_mxfp4_a8's sum over 128-k tiles, fp64; ``stale``: tile 1 is computed from the registers of tile 0."""
    A, W = A.double(), W.double()
    total = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float64)
    for t in range(A.shape[1] // 128):
        src = 0 if (stale and t == 1) else t
        k = slice(128 * src, 128 * src + 128)
        total += A[:, k] @ W[:, k].t()
    return total


def epilogue(gate: torch.Tensor, up: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    """The kernels' SwiGLU in fp32 -> bf16: x * rcp(1 + exp(-x)) * up.  Mutants: ``swapped`` (gate and up),
    ``up_off`` (the up tile 16 columns off), ``ratio`` (the algebraically equal x / (1 + exp(-x)) in its tanh form
    x (1 + (1 - e) / (1 + e)) / 2 with e = exp(-x): inf / inf at a saturated negative gate)."""
    g, u = gate.float(), up.float()
    if mutant == "swapped":
        g, u = u, g
    if mutant == "up_off":
        u = torch.roll(u, 16, dims=1)
    e = torch.exp(-g)
    if mutant == "ratio":
        sig = 0.5 * (1.0 + (1.0 - e) / (1.0 + e))
    else:
        sig = 1.0 / (1.0 + e)
    return gp.rne(g * sig * u)


def write_segments(cage: gp.Cage, out: torch.Tensor, row_off, tile_further: Optional[int] = None) -> gp.Cage:
    """What the grouped kernel leaves in ``cage``.  ``tile_further`` = e: the last row of expert e's segment is
    stored 16 rows further (an m-tile past ``hi`` that stores)."""
    cage.view.copy_(out)
    if tile_further is not None:
        last = int(row_off[tile_further + 1]) - 1
        cage.buf[last + 16, :cage.NC] = out[last]
    return cage
