"""Exact inputs, oracle, poisoned surroundings and deliberately wrong references for the GEMM kernels.

Every dense and grouped GEMM here accumulates in fp32 and stores bf16 with round-to-nearest-even; split-K and
stream-K partials are fp32.  With operands whose products and partial sums are all exact in fp32, the order of
summation cannot matter and every output is determined bit for bit:

    out = RNE_bf16(fp32(A.double() @ W.double().T + residual or bias))

Input families (bf16; ``fp8_operands`` is the e4m3 analogue):
  sign     every element +-1.  A sum over an even K is an even integer with |sum| <= K, so one dropped, doubled
           or misread element makes it odd; bf16 holds every integer up to 256, so wherever |sum| <= 255 that
           changes the stored bits (``unit_visible`` is the fraction of such outputs, asserted >= 95 %).
  scaled   sign with row m of A times 2^(m % 7 - 3) and row n of W times 2^(n % 5 - 2): as exact, and
           neighbouring rows and columns no longer look alike, so a row / column mix-up that happens to pick
           equal signs still shows.
  wide     integers of magnitude 1..8: sums need more than bf16's 8 bits (and stay below 2^24), so a partial
           that went through bf16 on its way to the final sum shows.  The sign families cannot see that: their
           partial sums are integers below 256, which bf16 holds.
  one-hot  row m of A holds one N(0, 1) bf16 value at column k_m (``probe_ks``), W is randn / sqrt(K): the
           accumulator is the 16-bit product a_m * W[n, k_m], exact in fp32 and generally not a bf16 number.
           Pins the rounding of the store on full-mantissa values (about 1 in 256 is an exact tie), the k
           position every lane reads, and an epilogue that adds its operand after rounding the product.

Epilogue operands: ``quarters`` (multiples of 0.25 within +-64: accumulator + operand is exact in fp32 for the
integer families, and for one-hot the kernel's single fp32 add is the oracle's ``.float()``) and ``big_integers``
(magnitude 256..1024, where bf16 steps are 2 and 4, so the store meets ties).

Rules: ``bitwise`` (equal int16 views) and ``one_step`` for epilogues with a transcendental or an rsqrt.
Derivation of one_step: silu(x) = x * rcp(1 + __expf(-x)) carries only multiplicative errors, below 1e-5 for
|x| <= 32, and rsqrt is about one fp32 ulp; both are far below the 2^-9 half-step of the bf16 store, so the
stored code is the RNE code of the fp64 reference or its neighbour in the ordered-integer view; an exactly
zero reference stays zero.

Surroundings: ``poison_a`` / ``poison_w`` put NaN behind A's K columns, below A's M rows and below W's N rows;
``Cage`` is an output whose [:M, :NC] view sits in a buffer filled with a NaN bit pattern that must survive
every launch.

The last part holds what tests/test_gemm_probes.py needs to show that these checks reject a broken kernel.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

SENTINEL = 0x7FA5    # a bf16 NaN no kernel produces (canonical NaN is 0x7FC0)
SENTINEL8 = 0x7F     # e4m3fn NaN
EXACT_MAX = 255      # bf16 holds every integer of magnitude <= 256; a unit error from <= 255 stays in that range
BAND = 128           # |accumulator| below which the one_step probes are asserted to be dense (>= 90 %)
SURE = 32            # |accumulator| up to which a unit error provably moves a product by >= 2 bf16 steps
PAD_ROWS, PAD_COLS, PAD_W_ROWS, PAD_A_COLS = 8, 16, 16, 64


# ---------------------------------------------------------------------------------------------------------
# input families


def _signs(shape, gen: torch.Generator) -> torch.Tensor:
    return (torch.randint(0, 2, tuple(shape), generator=gen) * 2 - 1).float()


def row_scales(M: int) -> torch.Tensor:
    return torch.exp2((torch.arange(M) % 7 - 3).float())


def col_scales(N: int) -> torch.Tensor:
    return torch.exp2((torch.arange(N) % 5 - 2).float())


def sign(M: int, N: int, K: int, gen: torch.Generator, scaled: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 A [M, K], W [N, K] of +-1 (``scaled``: times the row stairs of powers of two)."""
    assert K % 2 == 0
    A, W = _signs((M, K), gen), _signs((N, K), gen)
    if scaled:
        A, W = A * row_scales(M)[:, None], W * col_scales(N)[:, None]
    return A.to(torch.bfloat16), W.to(torch.bfloat16)


def unit(M: int, N: int, scaled: bool = False) -> torch.Tensor:
    """fp64 [M, N] magnitude of one product of the sign family at each output."""
    if not scaled:
        return torch.ones(M, N, dtype=torch.float64)
    return (row_scales(M)[:, None] * col_scales(N)[None, :]).double()


def wide(M: int, N: int, K: int, gen: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 A, W of non-zero integers in +-1..8: |sum| <= 64 K < 2^24, exact in fp32 in any order."""
    assert 64 * K < (1 << 24)
    A = _signs((M, K), gen) * torch.randint(1, 9, (M, K), generator=gen).float()
    W = _signs((N, K), gen) * torch.randint(1, 9, (N, K), generator=gen).float()
    return A.to(torch.bfloat16), W.to(torch.bfloat16)


def probe_ks(K: int, shares: int = 1) -> List[int]:
    """The k positions a one-hot family walks, most telling first: the first and last k of each of ``shares``
    equal K ranges (the waves of a K-split kernel), both sides of every 64-k and then every 32-k boundary,
    every k of the first 64-k tile, every k of the last one, then a stride of 61 over the rest."""
    ks: List[int] = []
    per = K // shares
    for s in range(shares):
        ks += [s * per, s * per + per - 1]
    for b in range(64, K, 64):
        ks += [b - 1, b]
    for b in range(32, K, 64):
        ks += [b - 1, b]
    ks += list(range(min(64, K))) + list(range(max(K - 64, 0), K)) + list(range(0, K, 61))
    seen, out = set(), []
    for k in ks:
        if 0 <= k < K and k not in seen:
            seen.add(k)
            out.append(k)
    return out


def one_hot(M: int, N: int, K: int, gen: torch.Generator, ks: Optional[Sequence[int]] = None,
            start: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """bf16 A [M, K] with one non-zero N(0, 1) value per row at column ks[(start + m) % len(ks)], W [N, K] =
    randn / sqrt(K), and the columns k_m [M]."""
    ks = list(ks) if ks is not None else probe_ks(K)
    km = torch.tensor([ks[(start + m) % len(ks)] for m in range(M)])
    a = torch.randn(M, generator=gen).to(torch.bfloat16)
    a = torch.where(a == 0, torch.ones_like(a), a)
    A = torch.zeros(M, K, dtype=torch.bfloat16)
    A[torch.arange(M), km] = a
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).to(torch.bfloat16)
    return A, W, km


def quarters(shape, gen: torch.Generator) -> torch.Tensor:
    """bf16 multiples of 0.25 within +-64 (8 significant bits: bf16-exact)."""
    return (torch.randint(-256, 257, tuple(shape), generator=gen).float() * 0.25).to(torch.bfloat16)


def big_integers(shape, gen: torch.Generator) -> torch.Tensor:
    """bf16 integers of magnitude 256..1024 (multiples of 4, so bf16-exact), random sign."""
    return (_signs(shape, gen) * 4 * torch.randint(64, 257, tuple(shape), generator=gen).float()).to(torch.bfloat16)


def swiglu_gate_shift(K: int) -> int:
    """c with |sum| * 2^-c <= 32 for every sign sum over K."""
    return max(0, (K // 32 - 1).bit_length())


def swiglu_sign(M: int, F: int, K: int, gen: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """Sign operands for a SwiGLU probe: W [2 F, K] = [gate; up] with the gate rows scaled by
    2^-ceil(log2(K / 32)), so |gate| <= 32 and still exact."""
    A, W = sign(M, 2 * F, K, gen)
    W = W.float()
    W[:F] *= 2.0 ** -swiglu_gate_shift(K)
    return A, W.to(torch.bfloat16)


def fp8_operands(M: int, N: int, K: int, gen: torch.Generator, max_exp: int = 6):
    """e4m3 A [M, K], W [N, K] in {+-1, +-2} and power-of-two scales a_s [M], w_s [N] in 2^-max_exp..2^max_exp:
    |accumulator| <= 4 K and the scaling is exact."""
    A = _signs((M, K), gen) * torch.randint(1, 3, (M, K), generator=gen).float()
    W = _signs((N, K), gen) * torch.randint(1, 3, (N, K), generator=gen).float()
    a_s = torch.exp2(torch.randint(-max_exp, max_exp + 1, (M,), generator=gen).float())
    w_s = torch.exp2(torch.randint(-max_exp, max_exp + 1, (N,), generator=gen).float())
    return A.to(torch.float8_e4m3fn), W.to(torch.float8_e4m3fn), a_s, w_s


# ---------------------------------------------------------------------------------------------------------
# oracle and rules


def exact(A: torch.Tensor, W: torch.Tensor, residual: Optional[torch.Tensor] = None,
          bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 A . W^T (+ residual [M, N] or bias [N])."""
    x = A.double() @ W.double().t()
    if residual is not None:
        x = x + residual.double()
    if bias is not None:
        x = x + bias.double()
    return x


def rne(x: torch.Tensor) -> torch.Tensor:
    """The kernels' store: the fp32 value, rounded to nearest even bf16."""
    return x.float().to(torch.bfloat16)


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    gate, up = gate.double(), up.double()
    return gate / (1 + torch.exp(-gate)) * up


def unit_visible(acc: torch.Tensor, unit_: Optional[torch.Tensor] = None) -> float:
    """Fraction of outputs whose exact accumulator is at most EXACT_MAX products in magnitude."""
    lim = EXACT_MAX if unit_ is None else EXACT_MAX * unit_.to(acc.device)
    return float((acc.abs() <= lim).double().mean())


def in_band(acc: torch.Tensor, width: float = BAND) -> float:
    return float((acc.abs() < width).double().mean())


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16)


def ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 codes as integers that rise with the value (+0 and -0 both 0)."""
    b = bits(t).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def bitwise(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Mask of outputs whose bits differ from ``want`` (fp64 values are stored with ``rne`` first)."""
    if want.dtype != torch.bfloat16:
        want = rne(want)
    return bits(got) != bits(want)


def steps(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Distance in bf16 codes (ordered-integer view) from the RNE code of the fp64 reference."""
    return (ordered(got) - ordered(rne(want))).abs()


def one_step(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Mask of outputs more than one bf16 code from the RNE code of the fp64 reference, non-finite, or
    non-zero where the reference is exactly zero."""
    return (steps(got, want) > 1) | ~torch.isfinite(got.float()) | ((want == 0) & (got.float() != 0))


RULES = {"bitwise": bitwise, "one_step": one_step}


# ---------------------------------------------------------------------------------------------------------
# surroundings


def _raw(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.element_size() == 2 else torch.uint8)


def _nan_buffer(rows: int, cols: int, like: torch.Tensor, device) -> torch.Tensor:
    code = SENTINEL if like.element_size() == 2 else SENTINEL8
    raw = torch.full((rows, cols), code, dtype=_raw(like).dtype, device=device)
    return raw.view(like.dtype)


def poison_a(A: torch.Tensor, device=None) -> torch.Tensor:
    """A as the [:M, :K] view of a NaN-filled [M + 8, K + 64] buffer (e4m3: 64 bytes, stride % 16 == 0)."""
    device = device if device is not None else A.device
    M, K = A.shape
    buf = _nan_buffer(M + PAD_ROWS, K + PAD_A_COLS, A, device)
    _raw(buf)[:M, :K] = _raw(A).to(device)
    return buf[:M, :K]


def poison_w(W: torch.Tensor, device=None) -> torch.Tensor:
    """W ([N, K] or [G, N, K]) as the leading rows of a contiguous buffer whose last 16 rows are NaN."""
    device = device if device is not None else W.device
    K = W.shape[-1]
    rows = W.numel() // K
    buf = _nan_buffer(rows + PAD_W_ROWS, K, W, device)
    _raw(buf)[:rows] = _raw(W).reshape(rows, K).to(device)
    out = buf[:rows].view(W.shape)
    assert out.is_contiguous()
    return out


class Cage:
    """A bf16 output [M, NC] as the [:M, :NC] view of a [M + 8, NC + 16] buffer of SENTINEL."""

    def __init__(self, M: int, NC: int, device="cpu"):
        self.M, self.NC = M, NC
        self.buf = torch.empty(M + PAD_ROWS, NC + PAD_COLS, dtype=torch.bfloat16, device=device)
        self.view = self.buf[:M, :NC]
        self.poison()

    def poison(self) -> "Cage":
        bits(self.buf).fill_(SENTINEL)
        return self

    def load(self, R: torch.Tensor) -> torch.Tensor:
        """Poison everything, then put an in-place residual into the view; returns the view."""
        self.poison()
        self.view.copy_(R)
        return self.view

    def outside_touched(self) -> int:
        b = bits(self.buf)
        return int((b[self.M:] != SENTINEL).sum()) + int((b[:self.M, self.NC:] != SENTINEL).sum())


def violations(cage: Cage, want: torch.Tensor, rule: str, rows: Optional[slice] = None) -> List[str]:
    """What a launch into ``cage`` got wrong: non-finite or off-rule outputs inside (``rows``: only those rows
    are held to the rule), touched sentinels outside.  Empty = accepted."""
    out = []
    got = cage.view if rows is None else cage.view[rows]
    if not bool(torch.isfinite(got.float()).all()):
        n = int((~torch.isfinite(got.float())).sum())
        out.append(f"{n} non-finite outputs (unwritten or poisoned)")
    bad = RULES[rule](got, want)
    if bool(bad.any()):
        i = [int(v) for v in bad.nonzero()[0]]
        ref = rne(want) if want.dtype != torch.bfloat16 else want
        out.append(f"{int(bad.sum())} of {bad.numel()} outputs fail {rule}; first at {i}: got "
                   f"{float(got[tuple(i)]):.8g} want {float(ref[tuple(i)]):.8g}")
    n = cage.outside_touched()
    if n:
        out.append(f"{n} sentinels outside [:{cage.M}, :{cage.NC}] overwritten")
    return out


def check(cage: Cage, want: torch.Tensor, rule: str, what: str = "", rows: Optional[slice] = None) -> None:
    v = violations(cage, want, rule, rows)
    assert not v, f"{what}: " + "; ".join(v)


# ---------------------------------------------------------------------------------------------------------
# wrong references (CPU tests only).  Accumulator mutants return an fp64 accumulator, store mutants a bf16
# tensor, write mutants fill a Cage.


def drop_k(acc, A, W, k: int, r0: int = 0, c0: int = 0, times: float = -1.0):
    """k left out of the sums of the 16 x 16 output block at (r0, c0) (``times`` = +1: counted twice)."""
    acc = acc.clone()
    acc[r0:r0 + 16, c0:c0 + 16] += times * torch.outer(A[r0:r0 + 16, k].double(), W[c0:c0 + 16, k].double())
    return acc


def double_k(acc, A, W, k: int, r0: int = 0, c0: int = 0):
    return drop_k(acc, A, W, k, r0, c0, times=1.0)


def group_from_row(acc, A, W, m: int, k0: int, src: int):
    """Row m's 8-wide k group [k0, k0 + 8) read from row ``src`` of A."""
    acc = acc.clone()
    acc[m] += (A[src, k0:k0 + 8].double() - A[m, k0:k0 + 8].double()) @ W[:, k0:k0 + 8].double().t()
    return acc


def store_trunc(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits."""
    b = x.float().contiguous().view(torch.int32)
    return (b >> 16).to(torch.int16).view(torch.bfloat16)


def store_half_up(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by adding half a step to the magnitude and truncating (ties away from zero)."""
    b = x.float().contiguous().view(torch.int32)
    return ((b + 0x8000) >> 16).to(torch.int16).view(torch.bfloat16)


def split_bf16_partial(A, W, splits: int = 2) -> torch.Tensor:
    """fp64 accumulator of a split-K whose first partial went through bf16 before the add."""
    K = A.shape[1]
    edge = K // splits
    first = rne(exact(A[:, :edge], W[:, :edge])).double()
    return first + exact(A[:, edge:], W[:, edge:])


def residual_after_rounding(acc, R) -> torch.Tensor:
    """bf16(bf16(acc) + R): the product rounded before the epilogue's add (also a bias added in bf16)."""
    return rne(rne(acc).double() + R.double())


def write(cage: Cage, out: torch.Tensor, skip_tail: Optional[Tuple[int, int]] = None,
          row_past_m: bool = False) -> Cage:
    """What a kernel storing ``out`` leaves in ``cage``.  ``skip_tail`` = (r0, rows): the last 16 columns of
    those rows are never stored; ``row_past_m``: row M is stored as well."""
    keep = cage.view.clone()
    cage.view.copy_(out)
    if skip_tail is not None:
        r0, n = skip_tail
        cage.view[r0:r0 + n, cage.NC - 16:] = keep[r0:r0 + n, cage.NC - 16:]
    if row_past_m:
        cage.buf[cage.M, :cage.NC] = out[cage.M - 1]
    return cage
