"""Exact inputs, fp64 oracles, sentinel cages and deliberately wrong references for the row-wise kernels that
run between the GEMMs: rmsnorm / rmsnorm_quant_fp8 / layernorm / rms_rowsumsq (csrc/kernels/norm.hip),
rope_kv_write / silu_mul / embedding / kv_gather / kv_block_copy (elementwise.hip), qknorm_rope_kv_write
(qknorm.hip) and quant_fp8_rows / silu_mul_quant_fp8 (moe.hip).

Rules (``rne``, ``bitwise``, ``one_step``, ``steps`` are those of tests/gemm_probes.py):

  bitwise    wherever the stored value is determined bit for bit: every intermediate exact in fp32 (copies, the
             residual sum ``x + r`` of two bf16 values, a rotation by table entries in {0, +-1, +-0.5, +-0.25},
             integer sums of squares below 2^24, a LayerNorm row of zero variance), or the fp32 value provably
             within 2^-10 of a bf16 number (the ``pinned`` rows below).  Oracle: fp64, then ``rne``.
  one_step   wherever an rsqrt, an rcp / exp or an fp32 sum of inexact terms is involved.  Derivation for these
             kernels: the stored value is RNE_bf16(f) with f = true * (1 + e).  e collects (a) the fp32 sum of
             squares (or of squared deviations) of n <= 32768 non-negative terms, each rounded once (2^-24):
             per-lane runs of at most 128 terms, then at most 10 levels of shuffles / LDS, so at most
             (128 + 10) * 2^-24 < 2^-16.8 in any such order, which the root halves: 4.4e-6; (b) the division by
             d and the add of eps, 2^-24 each; (c) v_rsq_f32 / v_rcp_f32, one ulp = 2^-23; __expf(-x) =
             exp2(-x * log2 e), whose argument is rounded once: |x| * 1.4427 * 2^-24 * ln 2 <= 64 * 2^-24 =
             3.8e-6 for |x| <= 64, plus one ulp of v_exp_f32 (this extends the |x| <= 32 bound of gemm_probes to
             the +-64 grid used here; exp(64) = 6.2e27 and its reciprocal are normal fp32 numbers); (d) two or
             three fp32 products, 2^-24 each.  Together |e| < 1e-5 << 1e-4 << 2^-9, the half step of the bf16
             store, so the stored code is the RNE code of the fp64 value or its neighbour; an exactly zero
             reference stays zero.
  decided    one_step, and bit-equal to the RNE code wherever the fp64 value is at least 2^-12 (relative) away
             from the nearest midpoint of two bf16 numbers: with |e| < 1e-5 = 2^-16.6 the fp32 value then lies on
             the same side of every midpoint as the fp64 value, so the store has no choice.  2^-12 leaves a
             factor 24 over the error bound and still decides about 9 outputs in 10.  Used where one_step alone
             is blind: a sigmoid that went through bf16, a divisor d - 8 at d >= 4096 (a shift of 4 / d).
  one_step_cond  one_step for a value that ends in a sum a + b whose terms may cancel (LayerNorm's ``t g + b``,
             RoPE's ``x1 cos - x2 sin`` with the model's tables): the fp32 error ``err`` is relative to
             mag = |a| + |b|, not to the result, and an honest fp32 kernel is several codes off where the terms
             cancel hard (tests/test_rowwise_probes.py builds such outputs and shows an fp32 emulation breaking
             plain one_step on them).  Where |want| >= 2^10 err mag the error is below 2^-10 |want| and one_step
             holds as derived; the outputs that cancel harder are held to |got - want| <= err mag + one bf16 step
             of want (the error bound plus the rounding of the store), and the caller asserts that they are at
             most 5 % of the outputs.  err = ROPE_ERR = 2^-22 for a bare rotation (two products and a sum,
             2^-24 each: below 2^-23 mag), so the loose branch starts below 2^-12 mag; err = NORM_ERR = 2^-16
             (the 1e-5 above) where a term carries an rsqrt and a reduction: LayerNorm, the per-head norm.

fp32 outputs: row sums of squares of small integers are bitwise; a quantiser's scale must lie within one fp32 ulp
of max(amax, 1e-12) / 448 computed in fp32 on the CPU.  e4m3 codes must equal RNE_e4m3(fp32(v) * fp32(1 / s))
with s the kernel's own scale (``e4m3_codes``; torch's CPU conversion is RNE and saturates 448 (1 + 2^-23) to 448).

Input families:
  spike walk   a zero row (LayerNorm: a row of 0.125) with two spikes of magnitude 1.375: one fixed at column 3,
               the other at column 8 i + i % 8 of vector slot i, one row per slot, every slot at every width
               (a 32768-wide walk is generated and run in chunks of 512 rows).  Leaving either spike out of
               the reduction, or counting it twice, turns sqrt(d/2) into sqrt(d) or sqrt(d/3): every non-zero
               output moves by >= 18 %, dozens of bf16 codes, in EVERY row of the walk.
  eps rows     |x| ~ 2^-20, so eps is the whole radicand: eps left out or added outside the root shows.
  heads        the 16-row walk at d = 128 and 16 eps rows as the q and k heads of qknorm_rope_kv_write, at an
               identity table row: the per-head norm under plain one_step (see ``head_qkv``).
  random rows  N(0, 1), optionally times 2^(r % 13 - 6) per row (neighbouring rows then have different inv).
  residual     x and r with exponents within 2^+-7 (fp32 sum exact), ties planted in both RNE directions.
  pinned       the residual rows normalised with eps = 2^40 (1 + 2^-12) and power-of-two weights:
               inv = 2^-20 (1 - 2^-13) whatever the row holds (the mean square vanishes below eps's ulp), so
               y = RNE(h * w * inv) is h * w * 2^-20 bit for bit when h is the bf16 stream value, and one code
               lower at every planted upward tie when h is the unrounded fp32 sum: this pins "the normalised
               value is computed from the bf16-rounded sum" and RNE at the norm's own store.
  constant     LayerNorm rows of one small integer: variance zero, output = bias bit for bit.
  offset       LayerNorm rows 100 + 0.5 {0, 1}: a one-pass E[x^2] - mean^2 variance in fp32 loses them.
  rope exact   q|k|v = +-(1 + m/128) 2^(-1..1) and tables in {0, +-1, +-0.5, +-0.25} that depend on position and
               column (position 1: cos 0, sin 1, the pure swap): the rotation is exact in fp32, bitwise.
  silu grid    gates: every multiple of 0.25 within +-64, +-0, and +-2^-k; ups +-(1 + m/128) 2^e.
  amax walk    the row maximum walks the vector slots, the rest of the row is at most half of it.
  e4m3 ties    amax = 448 * 2^k (scale exactly 2^k), the rest of the row on e4m3 midpoints and subnormals.

``RowCage`` is the Cage idea of gemm_probes for ops that take contiguous tensors (gemm_probes.Cage's [:M, :NC]
view of a wider buffer is refused by these bindings): the tensor is a window of a flat buffer with 64 sentinel
elements before and after it.  Caches are filled with the sentinel outright.

The last part holds the wrong references tests/test_rowwise_probes.py rejects.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from tests.gemm_probes import SENTINEL, bits, bitwise, one_step, ordered, rne, steps  # noqa: F401
from tests.gemm_probes import store_half_up, store_trunc  # noqa: F401

BF = torch.bfloat16
SPIKE = 1.375            # bf16, not a power of two
FIXED_COL = 3            # the spike that stays
LN_OFFSET = 0.125        # LayerNorm walks: every other element (sums of multiples of 2^-3 are exact in fp32)
PIN_EPS = 2.0 ** 40 * (1 + 2.0 ** -12)   # fp32-exact; rsqrt = 2^-20 (1 - 2^-13 + ...)
PIN_INV = 2.0 ** -20
PAD = 64
SENT32 = 0x7FA5A5A5      # an fp32 NaN
SENT8 = 0x7F             # e4m3fn NaN
ROPE_ERR = 2.0 ** -22    # fp32 error of x1 cos - x2 sin relative to |x1 cos| + |x2 sin|
NORM_ERR = 2.0 ** -16    # the same where a term went through a reduction and an rsqrt
HEAD_D = 128


# ---------------------------------------------------------------------------------------------------------
# surroundings


class RowCage:
    """A contiguous tensor of ``shape`` as a window of a flat sentinel-filled buffer, PAD elements on each side
    (bf16: SENTINEL, fp32: SENT32, e4m3: SENT8)."""

    _RAW = {2: (torch.int16, SENTINEL), 4: (torch.int32, SENT32), 1: (torch.uint8, SENT8)}

    def __init__(self, shape, device="cpu", dtype=BF):
        self.n = 1
        for s in shape:
            self.n *= int(s)
        self.raw_dtype, self.code = self._RAW[torch.empty(0, dtype=dtype).element_size()]
        self.buf = torch.empty(self.n + 2 * PAD, dtype=dtype, device=device)
        self.view = self.buf[PAD:PAD + self.n].view(*shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0
        self.poison()

    def poison(self) -> "RowCage":
        self.buf.view(self.raw_dtype).fill_(self.code)
        return self

    def load(self, t: torch.Tensor) -> torch.Tensor:
        self.poison()
        self.view.copy_(t.view(self.view.shape))
        return self.view

    def outside_touched(self) -> int:
        b = self.buf.view(self.raw_dtype)
        return int((b[:PAD] != self.code).sum()) + int((b[PAD + self.n:] != self.code).sum())

    def unwritten(self) -> int:
        return int((self.view.reshape(-1).view(self.raw_dtype) == self.code).sum())


def sentinel_cache(shape, device="cpu") -> torch.Tensor:
    t = torch.empty(*shape, dtype=BF, device=device)
    bits(t).fill_(SENTINEL)
    return t


def well_conditioned(want: torch.Tensor, mag: torch.Tensor, err: float = NORM_ERR) -> torch.Tensor:
    return want.double().abs() >= 2.0 ** 10 * err * mag.double()


def one_step_cond(got: torch.Tensor, want: torch.Tensor, mag: torch.Tensor,
                  err: float = NORM_ERR) -> Tuple[torch.Tensor, float]:
    """(mask of outputs off the rule, share of well-conditioned outputs): see the module docstring."""
    want, mag = want.double(), mag.double()
    well = well_conditioned(want, mag, err)
    step = (rne(want).double().abs() * 2.0 ** -7).clamp(min=2.0 ** -133)
    loose = (got.double() - want).abs() > err * mag + step
    bad = torch.where(well, one_step(got, want), loose | ~torch.isfinite(got.float()))
    return bad, float(well.double().mean())


def decided(got: torch.Tensor, want: torch.Tensor, margin: float = 2.0 ** -12) -> torch.Tensor:
    """Mask of outputs off one_step, or off the RNE code where ``want`` is ``margin`` away from every midpoint."""
    want = want.double().to(got.device)
    code = bits(rne(want))
    clear = (bits(rne(want * (1 + margin))) == code) & (bits(rne(want * (1 - margin))) == code)
    return one_step(got, want) | (clear & (bits(got) != code))


def decided_share(want: torch.Tensor, margin: float = 2.0 ** -12) -> float:
    code = bits(rne(want))
    return float(((bits(rne(want * (1 + margin))) == code) & (bits(rne(want * (1 - margin))) == code)).double().mean())


def describe(bad: torch.Tensor, got: torch.Tensor, want: torch.Tensor, rule: str) -> str:
    i = tuple(int(v) for v in bad.nonzero()[0])
    ref = want if want.dtype == BF else rne(want)
    return (f"{int(bad.sum())} of {bad.numel()} outputs fail {rule}; first at {list(i)}: got {float(got[i]):.8g} "
            f"want {float(ref[i]):.8g}")


def violations(cage: RowCage, want: torch.Tensor, rule: str, mag: Optional[torch.Tensor] = None,
               err: float = NORM_ERR) -> List[str]:
    """What a launch into ``cage`` got wrong (empty = accepted)."""
    out, got = [], cage.view
    want = want.to(got.device)
    if rule == "one_step_cond":
        bad, share = one_step_cond(got, want, mag.to(got.device), err)
        if share < 0.95:
            out.append(f"only {share:.4f} of the outputs are well conditioned")
    else:
        bad = {"bitwise": bitwise, "one_step": one_step, "decided": decided}[rule](got, want)
    if bool(bad.any()):
        out.append(describe(bad, got, want, rule))
    n = cage.outside_touched()
    if n:
        out.append(f"{n} sentinels outside the output overwritten")
    return out


def worst(got: torch.Tensor, want: torch.Tensor) -> int:
    return int(steps(got, want.to(got.device)).max()) if got.numel() else 0


# ---------------------------------------------------------------------------------------------------------
# norm families


def walk_slots(nvec: int) -> List[int]:
    """Every vector slot of a row."""
    return list(range(nvec))


def walk_chunks(d: int, rows: int = 512) -> List[List[int]]:
    """The slots of a d-wide walk in runs of at most ``rows`` (a 32768-wide walk has 4096 rows of 64 KiB)."""
    slots = walk_slots(d // 8)
    return [slots[i:i + rows] for i in range(0, len(slots), rows)]


def walk_cols(slots: Sequence[int]) -> torch.Tensor:
    return torch.tensor([8 * i + i % 8 for i in slots])


def spike_walk(d: int, slots: Optional[Sequence[int]] = None, offset: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x [len(slots), d] bf16, walker columns): ``offset`` everywhere, offset + SPIKE at FIXED_COL and (negated
    on odd rows when offset == 0) at the walker's column.  d = 8 has only slot 0; its walker sits at column 0."""
    slots = list(slots) if slots is not None else walk_slots(d // 8)
    cols = walk_cols(slots)
    assert int(cols.max()) < d and FIXED_COL < d and not bool((cols == FIXED_COL).any())
    x = torch.full((len(slots), d), offset, dtype=torch.float32)
    x[:, FIXED_COL] = offset + SPIKE
    sign = torch.where(torch.arange(len(slots)) % 2 == 1, -1.0, 1.0) if offset == 0.0 else torch.ones(len(slots))
    x[torch.arange(len(slots)), cols] = offset + sign * SPIKE
    xb = x.to(BF)
    assert bool((xb.float() == x).all())
    return xb, cols


def weights(d: int, gen: torch.Generator, spread: float = 0.5) -> torch.Tensor:
    return (1 + spread * torch.randn(d, generator=gen)).to(BF)


def pow2_weights(d: int) -> torch.Tensor:
    sign = torch.where(torch.arange(d) % 3 == 0, -1.0, 1.0)
    return (sign * torch.exp2((torch.arange(d) % 5 - 2).float())).to(BF)


def random_rows(rows: int, d: int, gen: torch.Generator, spread: bool = False) -> torch.Tensor:
    x = torch.randn(rows, d, generator=gen)
    if spread:
        x = x * torch.exp2((torch.arange(rows) % 13 - 6).float())[:, None]
    return x.to(BF)


def eps_rows(rows: int, d: int, gen: torch.Generator) -> torch.Tensor:
    m = 1 + torch.randint(0, 128, (rows, d), generator=gen).float() / 128
    s = torch.randint(0, 2, (rows, d), generator=gen).float() * 2 - 1
    return (s * m * 2.0 ** -20).to(BF)


def residual_rows(rows: int, d: int, gen: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """x, r bf16 with exponents in -3..3 (|exponent difference| <= 6: the fp32 sum is exact) and, in columns
    c % 4 == 1 / == 3, planted ties that RNE rounds up (1 + 2^-7 + 2^-8 -> 1 + 2^-6) / down (1 + 2^-8 -> 1)."""
    def draw():
        m = 1 + torch.randint(0, 128, (rows, d), generator=gen).float() / 128
        s = torch.randint(0, 2, (rows, d), generator=gen).float() * 2 - 1
        return s * m * torch.exp2(torch.randint(-3, 4, (rows, d), generator=gen).float())
    x, r = draw(), draw()
    c = torch.arange(d)
    sgn = torch.where(torch.arange(rows) % 2 == 1, -1.0, 1.0)[:, None]
    up, down = (c % 4 == 1), (c % 4 == 3)
    x[:, up] = (sgn * (1 + 2.0 ** -7)).expand(rows, int(up.sum()))
    r[:, up] = (sgn * 2.0 ** -8).expand(rows, int(up.sum()))
    x[:, down] = sgn.expand(rows, int(down.sum())) * 1.0
    r[:, down] = (sgn * 2.0 ** -8).expand(rows, int(down.sum()))
    return x.to(BF), r.to(BF)


def stream(x: torch.Tensor, r: Optional[torch.Tensor]) -> torch.Tensor:
    """The updated residual stream: RNE_bf16(fp32(x + r)) (x itself without a residual)."""
    return x if r is None else rne(x.double() + r.double())


def rms(h: torch.Tensor, w: torch.Tensor, eps: float, ss: Optional[torch.Tensor] = None,
        div: Optional[float] = None) -> torch.Tensor:
    """fp64 RMSNorm of the rows ``h`` (``ss`` / ``div``: another sum of squares / divisor, for the mutants)."""
    h = h.double()
    ss = (h * h).sum(-1, keepdim=True) if ss is None else ss
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    return h * torch.rsqrt(ss / (div or h.shape[-1]) + eps32) * w.double()


def rms_fp32(h: torch.Tensor, w: torch.Tensor, eps: float, chunk: int = 8) -> torch.Tensor:
    """An honest fp32 RMSNorm that reduces in another order (runs of ``chunk``, then pairwise) and rounds at
    every step as the kernels do: what one_step has to accept."""
    h32 = h.float()
    p = (h32 * h32).view(h.shape[0], -1, chunk)
    acc = torch.zeros(p.shape[:2])
    for j in range(chunk):
        acc = acc + p[:, :, j]
    while acc.shape[1] > 1:
        if acc.shape[1] % 2:
            acc = torch.cat([acc, torch.zeros(acc.shape[0], 1)], 1)
        acc = acc[:, 0::2] + acc[:, 1::2]
    inv = torch.rsqrt(acc / torch.tensor(float(h.shape[1])) + torch.tensor(eps, dtype=torch.float32))
    return ((h32 * inv) * w.float()).to(BF)


def pinned(h: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """bf16 output of the pinned rows: h * w * 2^-20 exactly (w powers of two)."""
    y = h.double() * w.double() * PIN_INV
    assert bool((rne(y).double() == y).all())
    return rne(y)


def small_int_rows(rows: int, d: int, gen: torch.Generator, top: int = 8) -> torch.Tensor:
    """Integers in -top..top: sums of squares <= 64 d < 2^24 are exact in fp32 in any order."""
    assert top * top * d < (1 << 24)
    return torch.randint(-top, top + 1, (rows, d), generator=gen).float().to(BF)


def layernorm(x, g, b, eps, r=None, pb=None, count: Optional[float] = None, one_pass: bool = False):
    """(fp64 LayerNorm, magnitude |t g| + |b| for one_step_cond).  ``count``: the divisor of the mean (mutant);
    ``one_pass``: variance as fp32 E[h^2] - mean^2 (mutant)."""
    h = x.double()
    if r is not None:
        h = h + r.double()
    if pb is not None:
        h = h + pb.double()
    d = h.shape[-1]
    mean = h.sum(-1, keepdim=True) / (count or d)
    if one_pass:
        h32 = h.float()
        m32 = h32.sum(-1, keepdim=True) / d
        var = ((h32 * h32).sum(-1, keepdim=True) / d - m32 * m32).clamp(min=0).double()
    else:
        var = ((h - mean) ** 2).sum(-1, keepdim=True) / d
    t = (h - mean) * torch.rsqrt(var + float(torch.tensor(eps, dtype=torch.float32))) * g.double()
    return t + b.double(), t.abs() + b.double().abs()


def offset_rows(rows: int, d: int, gen: torch.Generator, base: float = 100.0) -> torch.Tensor:
    return (base + 0.5 * torch.randint(0, 2, (rows, d), generator=gen).float()).to(BF)


LN_OFFSET_DS = [256, 520, 768, 1024, 1032, 2048, 32768]   # every LayerNorm width of the GPU file but 8


def ln_offset_case(d: int, rows: int = 16):
    """(x, g, b) of the offset rows both test files use at width d: the CPU file shows which of these very rows
    reject the one-pass variance, the GPU file runs them."""
    gen = torch.Generator().manual_seed(1000 + d)
    x = offset_rows(rows, d, gen)
    return x, weights(d, gen, 0.2), (0.2 * torch.randn(d, generator=gen)).to(BF)


# ---------------------------------------------------------------------------------------------------------
# per-head RMSNorm (qknorm_rope_kv_write): the norm families as q and k heads, all at position 0 of a table
# whose row 0 is the identity, so the kernel's output for a head is rms(head + bias, w, eps) and the rule
# stays one_step.  One thread holds columns [8 u, 8 u + 8) and [64 + 8 u, 64 + 8 u + 8) of a head, the 8 threads
# of a head reduce by DPP: the 16 rows of spike_walk(128) put the walker into each half of each thread.

HEAD_BIAS = 2.0 ** -6


def head_qkv(heads: torch.Tensor, T: int, Hq: int, Hkv: int, gen: torch.Generator) -> torch.Tensor:
    """qkv [T, (Hq + 2 Hkv) * 128] whose q / k head h of token t is row (t + h) % R of ``heads`` [R, 128] (T >= R:
    every head sees every row) and whose v heads are exact_values."""
    R = heads.shape[0]
    idx = (torch.arange(T)[:, None] + torch.arange(Hq + Hkv)[None, :]) % R
    qk = heads[idx].reshape(T, (Hq + Hkv) * HEAD_D)
    return torch.cat([qk, exact_values((T, Hkv * HEAD_D), gen)], 1).contiguous()


def head_bias(Hq: int, Hkv: int, gen: torch.Generator) -> torch.Tensor:
    """+-2^-6 on the q and k columns (3 % of a walk head's energy: a dropped or doubled spike still moves the
    outputs by more than 17 %), exact_values on the v columns."""
    n = (Hq + Hkv) * HEAD_D
    qk = torch.where(torch.arange(n) % 2 == 0, HEAD_BIAS, -HEAD_BIAS).to(BF)
    return torch.cat([qk, exact_values((Hkv * HEAD_D,), gen)])


# ---------------------------------------------------------------------------------------------------------
# RoPE, qk-norm and the caches


TABLE_VALUES = torch.tensor([0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25])


def synthetic_tables(P: int, half: int, gen: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 cos / sin [P, half] with entries in {0, +-1, +-0.5, +-0.25} drawn per (position, column); position 0
    is the identity (cos 1, sin 0) and position 1 the pure swap (cos 0, sin 1)."""
    cos = TABLE_VALUES[torch.randint(0, 7, (P, half), generator=gen)]
    sin = TABLE_VALUES[torch.randint(0, 7, (P, half), generator=gen)]
    cos[0], sin[0] = 1.0, 0.0
    if P > 1:
        cos[1], sin[1] = 0.0, 1.0
    return cos.contiguous(), sin.contiguous()


def exact_values(shape, gen: torch.Generator) -> torch.Tensor:
    """bf16 +-(1 + m/128) 2^e, e in -1..1: sums and table-scaled sums of two of them stay below 2^16 ulps."""
    m = 1 + torch.randint(0, 128, tuple(shape), generator=gen).float() / 128
    s = torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 - 1
    return (s * m * torch.exp2(torch.randint(-1, 2, tuple(shape), generator=gen).float())).to(BF)


def probe_positions(T: int, P: int, gen: torch.Generator) -> torch.Tensor:
    """int32 positions that include 0, 1 and the table's last row."""
    pos = torch.randint(0, P, (T,), generator=gen)
    for i, p in enumerate([P - 1, 0, 1][:T]):
        pos[(i * 7) % T] = p
    if T >= 1:
        pos[0] = P - 1
    return pos.to(torch.int32)


def probe_slots(T: int, NB: int, BS: int, gen: torch.Generator, variant: str = "slots") -> Optional[torch.Tensor]:
    """int32 slots [T]: a permutation in which (for T >= 2 BS) every offset of the first and of the last block
    occurs, the rest in the blocks between.  ``variant``: "slots", "padded" (every third row -1), "allpad",
    "none"."""
    if variant == "none":
        return None
    if variant == "allpad":
        return torch.full((T,), -1, dtype=torch.int32)
    assert NB >= 3
    edge = list(range(BS)) + [(NB - 1) * BS + o for o in range(BS)]
    mid = [BS + int(v) for v in torch.randperm((NB - 2) * BS, generator=gen)]
    pool = (edge + mid)[:max(T, 1)] if T >= 2 * BS else None
    if pool is None:   # short steps: ends of both edge blocks first, then the middle
        pool = ([0, NB * BS - 1, BS - 1, (NB - 1) * BS, 5 % BS, (NB - 1) * BS + 6 % BS, 3 % BS] + mid)[:T]
    assert len(set(pool)) == len(pool) == T
    slots = torch.tensor(pool)[torch.randperm(T, generator=gen)].to(torch.int32)
    if variant == "padded":   # slot 0 stays free, so a padding row that is written there shows
        slots[::3] = -1
        slots[slots == 0] = -1
    return slots


def rotate(x: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, pairs: str = "half",
           sin_sign: float = 1.0, row_shift: int = 0, col_shift: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp64 rotate-half of x [T, H, D] and the magnitude |x1 c| + |x2 s| (the keyword arguments are mutants)."""
    x = x.double()
    D = x.shape[-1]
    rows = (pos.long() + row_shift).clamp(0, cos.shape[0] - 1)
    c = cos.double()[rows][:, None, :].roll(col_shift, -1)
    s = sin.double()[rows][:, None, :].roll(col_shift, -1) * sin_sign
    if pairs == "half":
        x1, x2 = x[..., : D // 2], x[..., D // 2:]
        out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
        mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
        return out, mag
    x1, x2 = x[..., 0::2], x[..., 1::2]   # the interleaved convention
    out = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], -1).flatten(-2)
    return out, out.abs()


class RopeWant:
    """What a rope / qknorm launch must leave: fp64 ``qkv`` [T, W] (values the kernel does not write hold the
    input), ``k`` / ``v`` [T, Hkv, D] fp64 cache lines, and the magnitudes for one_step_cond."""

    def __init__(self, qkv, mag, k, kmag, v):
        self.qkv, self.mag, self.k, self.kmag, self.v = qkv, mag, k, kmag, v


def rope_want(qkv: torch.Tensor, pos, cos, sin, slots, Hq: int, Hkv: int, D: int, rope_q: bool, *,
              bias: Optional[torch.Tensor] = None, qw: Optional[torch.Tensor] = None,
              kw: Optional[torch.Tensor] = None, eps: float = 1e-6, qknorm: bool = False,
              round_after: Optional[str] = None, rotate_q_anyway: bool = False, **mut) -> RopeWant:
    """The single-rounding oracle of rope_kv_write (``qknorm``: of qknorm_rope_kv_write).  Everything in fp64
    from the bf16 inputs.  ``round_after`` = "bias" / "norm": a bf16 rounding there (mutants)."""
    T = qkv.shape[0]
    x = qkv.double().view(T, Hq + 2 * Hkv, D)
    if bias is not None:
        x = x + bias.double().view(1, -1, D)
        if round_after == "bias":
            x = rne(x).double()
    q, k, v = x[:, :Hq], x[:, Hq:Hq + Hkv], x[:, Hq + Hkv:]
    eps32 = float(torch.tensor(eps, dtype=torch.float32))

    def norm(t, w):
        if w is None:
            return t
        t = t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps32) * w.double()
        return rne(t).double() if round_after == "norm" else t
    q, k = norm(q, qw), norm(k, kw)
    kr, kmag = rotate(k, pos, cos, sin, **mut)
    if rope_q or rotate_q_anyway:
        qr, qmag = rotate(q, pos, cos, sin, **mut)
    else:
        qr, qmag = q, q.abs()
    pad = torch.ones(T, dtype=torch.bool) if slots is None else slots < 0
    back = (pad | bool(rope_q))[:, None, None]           # rows whose k (qknorm + bias: and v) goes back to qkv
    x0 = qkv.double().view(T, Hq + 2 * Hkv, D)
    k_back = torch.where(back, kr, x0[:, Hq:Hq + Hkv])
    v_back = torch.where(back, v, x0[:, Hq + Hkv:]) if (qknorm and bias is not None) else x0[:, Hq + Hkv:]
    want = torch.cat([qr, k_back, v_back], 1).reshape(T, -1)
    mag = torch.cat([qmag, torch.where(back, kmag, k_back.abs()), v_back.abs()], 1).reshape(T, -1)
    return RopeWant(want, mag, kr, kmag, v)


def scatter(lines_k: torch.Tensor, lines_v: torch.Tensor, slots: Optional[torch.Tensor], NB: int, BS: int, *,
            v_layout: str = "interleaved", swap_off: bool = False, pad_to_zero: bool = False,
            k_transposed: bool = False, stray: bool = False):
    """(k cache [NB, Hkv, BS, D], v cache [NB, Hkv, BS/4, D, 4], written masks) holding the bf16 lines at
    ``slots`` and SENTINEL elsewhere.  The keyword arguments are the cache mutants."""
    T, Hkv, D = lines_k.shape
    kc, vc = sentinel_cache((NB, Hkv, BS, D)), sentinel_cache((NB, Hkv, BS // 4, D, 4))
    km, vm = torch.zeros(kc.shape, dtype=torch.bool), torch.zeros(vc.shape, dtype=torch.bool)
    lk = lines_k if lines_k.dtype == BF else rne(lines_k)
    lv = lines_v if lines_v.dtype == BF else rne(lines_v)
    for t in range(T if slots is not None else 0):
        s = int(slots[t])
        if s < 0:
            if not pad_to_zero:
                continue
            s = 0
        blk, off = divmod(s, BS)
        if k_transposed:
            kc[blk].view(BS, Hkv, D)[off] = lk[t]
            km[blk].view(BS, Hkv, D)[off] = True
        else:
            kc[blk, :, off] = lk[t]
            km[blk, :, off] = True
        if v_layout == "token_major":
            vc[blk].view(Hkv, BS, D)[:, off] = lv[t]
            vm[blk].view(Hkv, BS, D)[:, off] = True
        else:   # element d of a head at ((off >> 2) * D + d) * 4 + (off & 3) of the head's BS * D elements
            a, b = (off & 3, off >> 2) if swap_off else (off >> 2, off & 3)
            idx = (a * D + torch.arange(D)) * 4 + b
            vc[blk].view(Hkv, BS * D)[:, idx] = lv[t]
            vm[blk].view(Hkv, BS * D)[:, idx] = True
    if stray:
        free = (~km).nonzero()[-1]
        kc[tuple(free)] = 1.0
    return kc, vc, km, vm


def cache_violations(got: torch.Tensor, want: torch.Tensor, mask: torch.Tensor, rule: str = "bitwise",
                     lines64: Optional[torch.Tensor] = None) -> List[str]:
    """Every element outside ``mask`` must hold SENTINEL; inside, ``got`` must match ``want`` (bf16, bitwise) or,
    for one_step, be within a code of it with both finite."""
    out = []
    want, mask = want.to(got.device), mask.to(got.device)
    n = int((bits(got)[~mask] != SENTINEL).sum())
    if n:
        out.append(f"{n} cache elements outside the written lines overwritten")
    g, w = got[mask], want[mask]
    bad = bitwise(g, w) if rule == "bitwise" else ((ordered(g) - ordered(w)).abs() > 1) | ~torch.isfinite(g.float())
    if bool(bad.any()):
        out.append(f"{int(bad.sum())} of {bad.numel()} cached elements fail {rule}")
    return out


# ---------------------------------------------------------------------------------------------------------
# SwiGLU


def silu_grid() -> torch.Tensor:
    """bf16 gates: every multiple of 0.25 within +-64 (8 significant bits), +-0 and +-2^-k, k = 1..20."""
    q = torch.arange(-256, 257).float() * 0.25
    small = torch.exp2(-torch.arange(1, 21).float())
    return torch.cat([q, torch.tensor([-0.0]), small, -small]).to(BF)


def silu_inputs(T: int, F: int, block: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(gate_up [T, 2F] bf16 in the layout ``block`` asks for, gate [T, F], up [T, F]): gates walk the grid, ups
    are +-(1 + m/128) 2^e with a period coprime to the grid's."""
    grid = silu_grid()
    i = torch.arange(T * F)
    gate = grid[i % grid.numel()].view(T, F)
    j = (i * 7 + 3) % 509
    up = ((1 + (j % 128).float() / 128) * torch.exp2((j % 7 - 3).float()) * torch.where(j % 2 == 0, 1.0, -1.0))
    up = up.to(BF).view(T, F)
    return pack_gate_up(gate, up, block), gate, up


def pack_gate_up(gate: torch.Tensor, up: torch.Tensor, block: int = 0) -> torch.Tensor:
    T, F = gate.shape
    b = block or F
    return torch.stack([gate.view(T, F // b, b), up.view(T, F // b, b)], 2).reshape(T, 2 * F).contiguous()


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    g, u = gate.double(), up.double()
    return g * torch.sigmoid(g) * u


# ---------------------------------------------------------------------------------------------------------
# quantisers


def amax_walk(d: int, rows: Optional[int] = None, gen: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x [R, d] bf16, column of the maximum): row i's maximum 3.5 * 2^(i % 5) (sign alternating) sits in vector
    slot s_i at column 8 s_i + s_i % 8; everything else is at most half of it.  ``rows``: that many slots —
    the first, the last, both sides of every multiple of 256, then a stride."""
    nvec = d // 8
    slots = list(range(nvec))
    if rows is not None and rows < nvec:
        pick = [0, nvec - 1] + [s for b in range(256, nvec, 256) for s in (b - 1, b)]
        pick += list(range(1, nvec, max(1, nvec // rows)))
        slots = list(dict.fromkeys(pick))[:rows]
    elif rows is not None:
        slots = [slots[i % nvec] for i in range(rows)]
    gen = gen or torch.Generator().manual_seed(d)
    R = len(slots)
    top = 3.5 * torch.exp2((torch.arange(R) % 5).float())
    x = (torch.rand(R, d, generator=gen) - 0.5) * top[:, None]
    cols = walk_cols(slots)
    x[torch.arange(R), cols] = top * torch.where(torch.arange(R) % 2 == 1, -1.0, 1.0)
    xb = x.to(BF)
    assert bool((xb.float().abs().amax(1) == top).all())
    return xb, cols


def subnormal_rows(rows: int, d: int, gen: torch.Generator) -> torch.Tensor:
    """bf16 subnormals (|x| < 2^-126), both signs."""
    code = torch.randint(1, 128, (rows, d), generator=gen).to(torch.int16)
    code = code | (torch.randint(0, 2, (rows, d), generator=gen).to(torch.int16) << 15)
    return code.view(BF)


def e4m3_tie_rows(rows: int, d: int) -> torch.Tensor:
    """Row r: column 0 = 448 * 2^(r % 7 - 3) (the scale is then exactly 2^(r % 7 - 3)); the other columns cycle,
    with alternating sign, through the midpoints (1 + (2 m + 1)/16) 2^e of neighbouring e4m3 numbers, the
    subnormals j 2^-9 and their midpoints (j + 0.5) 2^-9, all times the scale."""
    mids = [(1 + (2 * m + 1) / 16) * 2.0 ** e for e in range(-6, 8) for m in range(8)]
    subs = [j * 2.0 ** -9 for j in range(1, 8)] + [(j + 0.5) * 2.0 ** -9 for j in range(0, 8)]
    vals = torch.tensor(mids + subs)
    c = torch.arange(d)
    body = vals[c % vals.numel()] * torch.where(c % 2 == 0, 1.0, -1.0)
    sc = torch.exp2((torch.arange(rows) % 7 - 3).float())
    x = body[None, :] * sc[:, None]
    x[:, 0] = 448.0 * sc
    xb = x.to(BF)
    assert bool((xb.float() == x).all())
    return xb


def scale_ref(x: torch.Tensor, top: float = 448.0) -> torch.Tensor:
    """fp32 max(amax, 1e-12) / 448, computed in fp32 (IEEE division)."""
    amax = x.float().abs().amax(-1)
    return torch.maximum(amax, torch.tensor(1e-12)) / torch.tensor(top)


def ulps32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance of positive fp32 numbers in ulps."""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


def e4m3_codes(x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """uint8 codes RNE_e4m3(fp32(x) * fp32(1 / s)), s [rows] the scale the kernel used."""
    x, s = x.cpu(), s.cpu().float()
    inv = torch.tensor(1.0) / s
    return (x.float().view(s.numel(), -1) * inv[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).view(x.shape)


def e4m3_codes_trunc(x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """Mutant: the scaled value's magnitude truncated to e4m3 instead of rounded."""
    v = x.float().view(s.numel(), -1) * (torch.tensor(1.0) / s.float())[:, None]
    q = v.to(torch.float8_e4m3fn)
    over = q.float().abs() > v.abs()
    code = q.view(torch.uint8)
    return torch.where(over, code - 1, code).view(x.shape)


# ---------------------------------------------------------------------------------------------------------
# copies


def distinct(shape, start: int = 1) -> torch.Tensor:
    """bf16 tensor whose elements' bit patterns count up (mod 0x7F00, skipping nothing a NaN would need), so no
    two elements within 32512 of each other are equal and none equals SENTINEL."""
    n = 1
    for s in shape:
        n *= int(s)
    code = ((torch.arange(n) * 7 + start) % 0x7F00).to(torch.int16)
    return code.view(BF).view(*shape)
