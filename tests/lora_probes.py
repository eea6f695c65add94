"""Exact inputs, fp64 oracles, cages and deliberately wrong emulations for the batched LoRA kernels of
csrc/kernels/lora.hip (lora_shrink, lora_expand_add).  tests/test_lora_gpu.py holds them to 2^-7 of the magnitude at
four ranks and three adapters; what that leaves open is one k of the permuted operand order, one wave's share of K,
one adapter bit above 31, the zero-filled half of the last k-step.

``RowCage``, ``SENTINEL``, ``distinct``, ``rne`` and ``bitwise`` are those of tests/gemm_probes.py and
tests/rowwise_probes.py.

Contract tested (the header comment of lora.hip)
------------------------------------------------
  shrink      T[m, :] = X[m, :] . A[ids[m]]^T, fp32 accumulation, RNE bf16; X [M, K] rows strided (ldx >= K).
  expand-add  Y[m, :] = RNE(Y[m, :] + T[m, :] . B[ids[m]]^T), ONE rounding of the fp32 sum; Y rows strided (ldy >= N).
  ids outside [0, n_adapters) mean "no adapter": shrink does not write that row of T, expand-add does not read it
  and leaves the row of Y bitwise unchanged; a group without any adapter writes nothing.

Families (every comparison bitwise)
-----------------------------------
  spike walk, shrink   M = K rows, row m a single 1.0 at column m, A ``distinct`` codes: T[m, r] = A[id_m, r, m],
                       a copy (1.0 * a exact, every other term +0): no bound needed.  Walks EVERY k: the k order of
                       the two operands inside a 64-chunk, the chunk a wave owns, the waves summed.
  spike walk, expand   T one-hot (1.0) at r_m = (number of rows with an adapter before m) % R, B ``distinct`` codes,
                       Y0 = 0: Y[m, n] = B[id_m, n, r_m], a copy.  M = 300 has at least 192 such rows, so every r is
                       walked, the last k-step's zero-filled upper half included (R % 32 == 16).
  sign, shrink         X = +-2^(m % 5 - 2), A = +-2^(r % 3 - 1): terms multiples of 2^-3 of magnitude <= 8, K <= 4096
                       of them: 64 * 4096 = 2^18 < 2^24, exact in fp32 in any order; T = RNE of the exact sum.
  sign, expand         T integers within +-32, B = +-2^(n % 3 - 1), Y0 integers within +-8: terms multiples of 2^-1 of
                       magnitude <= 64, R <= 192 of them plus Y0: (128 * 192 + 16) = 24592 < 2^24 units; Y = RNE of
                       the exact value (sums beyond +-128 are common at R = 192: a delta rounded on its own shows).
                       Rows without an adapter hold the NaN sentinel in T.
tests/test_lora_probes.py evaluates ``shrink_bound`` / ``expand_bound`` for every shape used.

Shapes and the launcher instantiation each reaches
--------------------------------------------------
``shrink_form(M, R)`` is launch_shrink's choice: M <= 8192: one 16-row tile per workgroup, 16 / 8 / 4 waves splitting
K for R <= 48 / 96 / 192; above: 4 waves on 4 / 2 / 1 row tiles.  NRT = R / 16 = 1..12 all run (SHRINK_WALK at K = 64
and SHRINK_SIGN at M = 300, K = 128).  K = 64 is one chunk for up to 16 waves (15 idle waves whose zero partials
are summed), 128 two chunks, 1088 seventeen (a remainder over 16, 8 and 4 waves), 4096 the long loop.  M = 1, 16, 17,
300: a partial tile, a full one, one row into the second, many groups.  M = 8200, K = 64 at R = 16, 80, 112, 192 are
the MT = 4, 2, 1 forms.  Expand: KS = ceil(R / 32) = 1..6 with both parities of R / 16 (R = 16, 32, 48, 80, 96, 128,
144, 176, 192); N = 8, 24, 520 (N % 16 == 8: the last column tile half outside); M = 2100 gives 33 row groups, the
4-column-tiles-per-wave form.  X and Y are column windows of caged buffers with ld = K + 8 / N + 8.

Ids: ``ids64``: n_adapters = 64, id = m % 64 (a 16-row tile holds 16 adapters, rows 0..63 all 64, ids 0, 31, 32, 63
among them at M >= 128), -1 on every fifth row from row 64 (from row 0 at M <= 64) and on the whole 64-row group
128..191.  ``ids3``: n_adapters = 3, ids cycling through 0, 1, 2, 3, 1000, -1: 3 and 1000 must behave as -1.

The last part holds emulations of the two kernels with switches that break them in one way each.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

from tests.gemm_probes import SENTINEL, _signs, bits, bitwise, rne  # noqa: F401
from tests.rowwise_probes import BF, RowCage, distinct  # noqa: F401

I32 = torch.int32
ALL_R = list(range(16, 193, 16))
EXPAND_R = [16, 32, 48, 80, 96, 128, 144, 176, 192]      # KS = 1, 1, 2, 3, 3, 4, 5, 6, 6

# (M = K, R, ids family)
SHRINK_WALK = [(64, R, "ids64") for R in ALL_R] + [(128, 16, "ids64"), (128, 96, "ids64"), (128, 192, "ids64"),
                                                    (1088, 48, "ids3"), (1088, 80, "ids64"), (1088, 176, "ids3"),
                                                    (4096, 16, "ids3"), (4096, 144, "ids3")]
# (M, K, R, ids family)
SHRINK_SIGN = [(300, 128, R, "ids64") for R in ALL_R] + \
              [(1, 64, 32, "ids3"), (1, 1088, 192, "ids64"), (16, 1088, 64, "ids64"), (17, 4096, 32, "ids3"),
               (17, 4096, 112, "ids3"), (300, 1088, 160, "ids3"), (300, 4096, 96, "ids3")] + \
              [(8200, 64, R, "ids64") for R in (16, 80, 112, 192)]
# (M, N, R, ids family)
EXPAND_WALK = [(300, 24, R, "ids64") for R in EXPAND_R] + [(300, 520, 48, "ids3"), (2100, 520, 176, "ids64")]
EXPAND_SIGN = [(300, 520, R, "ids3") for R in EXPAND_R] + \
              [(1, 8, 16, "ids3"), (16, 8, 80, "ids64"), (17, 24, 144, "ids64"), (1, 520, 192, "ids64"),
               (2100, 520, 48, "ids64"), (2100, 24, 16, "ids3")]
CHAIN = (300, 128, 80, 520)          # M, K, R, N


def shrink_form(M: int, R: int) -> Tuple[int, int]:
    """(MT row tiles per workgroup, NW waves) of launch_shrink."""
    nrt = R // 16
    if M <= 8192:
        return 1, (16 if nrt <= 3 else 8 if nrt <= 6 else 4)
    return (4 if nrt <= 3 else 2 if nrt <= 6 else 1), 4


def shrink_bound(K: int) -> int:
    """Units of 2^-3 the sign family's sums can reach; must stay below 2^24."""
    return 64 * K


def expand_bound(R: int) -> int:
    """Units of 2^-1 the sign family's Y0 + sum can reach."""
    return 128 * R + 16


def make_ids(family: str, M: int) -> Tuple[torch.Tensor, int]:
    """(ids [M] int32, n_adapters)."""
    m = torch.arange(M)
    if family == "ids64":
        ids = m % 64
        off = (m % 5 == 3) & ((m >= 64) | (M <= 64))
        ids = torch.where(off | ((m >= 128) & (m < 192)), -1, ids)
        return ids.to(I32), 64
    if family == "ids3":
        return torch.tensor([0, 1, 2, 3, 1000, -1])[(m + m // 6) % 6].to(I32), 3
    raise ValueError(family)


def has_adapter(ids: torch.Tensor, n: int) -> torch.Tensor:
    return (ids >= 0) & (ids < n)


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 77)


def window(t: torch.Tensor, device="cpu", extra: int = 8) -> Tuple[RowCage, torch.Tensor]:
    """t [M, C] as the [:, :C] window of a caged [M, C + extra] buffer whose other columns hold the NaN sentinel."""
    M, C = t.shape
    cage = RowCage((M, C + extra), device, BF)
    cage.view[:, :C] = t.to(device)
    return cage, cage.view[:, :C]


def window_touched(cage: RowCage, C: int) -> int:
    return int((bits(cage.view[:, C:]) != SENTINEL).sum()) + cage.outside_touched()


# ---------------------------------------------------------------------------------------------------------
# inputs and oracles


def shrink_walk(K: int, R: int, family: str):
    """(X [K, K], A [n, R, K], ids, n, want T [K, R] bf16)."""
    ids, n = make_ids(family, K)
    A = distinct((n, R, K), start=3 * R + K)
    X = torch.eye(K).to(BF)
    safe = ids.long().clamp(0, n - 1)
    want = A[safe, :, torch.arange(K)]
    return X, A, ids, n, want


def shrink_sign(M: int, K: int, R: int, family: str):
    """(X, A, ids, n, want fp64)."""
    assert shrink_bound(K) < (1 << 24)
    ids, n = make_ids(family, M)
    gen = _gen(M, K, R)
    X = (_signs((M, K), gen) * torch.exp2((torch.arange(M) % 5 - 2).float())[:, None]).to(BF)
    A = (_signs((n, R, K), gen) * torch.exp2((torch.arange(R) % 3 - 1).float())[None, :, None]).to(BF)
    return X, A, ids, n, product(X, A, ids, n)


def product(X: torch.Tensor, W: torch.Tensor, ids: torch.Tensor, n: int) -> torch.Tensor:
    """fp64 X[m] . W[ids[m]]^T per row, zero for rows without an adapter (X [M, K], W [n, R, K])."""
    out = torch.zeros(X.shape[0], W.shape[1], dtype=torch.float64)
    for a in range(n):
        rows = (ids == a).nonzero().flatten()
        if rows.numel():
            out[rows] = X[rows].double() @ W[a].double().t()
    return out


def walk_r(ids: torch.Tensor, n: int, R: int) -> torch.Tensor:
    """The hot column of every row of an expand walk: rows with an adapter count through 0 .. R - 1."""
    return (has_adapter(ids, n).long().cumsum(0) - 1).clamp(min=0) % R


def expand_walk(M: int, N: int, R: int, family: str):
    """(T [M, R], B [n, N, R], Y0 [M, N], ids, n, want Y bf16): T holds the NaN sentinel on rows without an adapter."""
    ids, n = make_ids(family, M)
    B = distinct((n, N, R), start=5 * R + N)
    hot = walk_r(ids, n, R)
    T = torch.zeros(M, R)
    T[torch.arange(M), hot] = 1.0
    T = T.to(BF)
    has = has_adapter(ids, n)
    bits(T)[~has] = SENTINEL
    want = B[ids.long().clamp(0, n - 1), :, hot]
    want[~has] = 0
    return T, B, torch.zeros(M, N, dtype=BF), ids, n, want


def expand_sign(M: int, N: int, R: int, family: str):
    assert expand_bound(R) < (1 << 24)
    ids, n = make_ids(family, M)
    gen = _gen(M, N, R, 1)
    T = torch.randint(-32, 33, (M, R), generator=gen).float().to(BF)
    B = (_signs((n, N, R), gen) * torch.exp2((torch.arange(N) % 3 - 1).float())[None, :, None]).to(BF)
    Y0 = torch.randint(-8, 9, (M, N), generator=gen).float().to(BF)
    has = has_adapter(ids, n)
    want = Y0.double() + product(torch.where(has[:, None], T, torch.zeros_like(T)), B, ids, n)
    bits(T)[~has] = SENTINEL
    return T, B, Y0, ids, n, want


def shrink_violations(cage: RowCage, want: torch.Tensor, ids: torch.Tensor, n: int) -> List[str]:
    out, got = [], cage.view.cpu()
    has = has_adapter(ids, n)
    bad = bitwise(got, want) & has[:, None]
    if bool(bad.any()):
        m, r = (int(v) for v in bad.nonzero()[0])
        out.append(f"{int(bad.sum())} of {int(has.sum()) * got.shape[1]} outputs differ; first T[{m}, {r}] (id "
                   f"{int(ids[m])}): got {float(got[m, r]):.8g} want {float(rne(want)[m, r]):.8g}")
    wrote = (bits(got) != SENTINEL) & ~has[:, None]
    if bool(wrote.any()):
        m = int(wrote.any(1).nonzero()[0])
        out.append(f"{int(wrote.any(1).sum())} rows without an adapter written; first row {m} (id {int(ids[m])})")
    if cage.outside_touched():
        out.append(f"{cage.outside_touched()} sentinels outside T overwritten")
    return out


def expand_violations(cage: RowCage, N: int, want: torch.Tensor, Y0: torch.Tensor, ids: torch.Tensor,
                      n: int) -> List[str]:
    out, got = [], cage.view[:, :N].cpu()
    has = has_adapter(ids, n)
    bad = bitwise(got, want) & has[:, None]
    if bool(bad.any()):
        m, c = (int(v) for v in bad.nonzero()[0])
        out.append(f"{int(bad.sum())} of {int(has.sum()) * N} outputs differ; first Y[{m}, {c}] (id {int(ids[m])}): "
                   f"got {float(got[m, c]):.8g} want {float(rne(want)[m, c]):.8g}")
    moved = bitwise(got, Y0) & ~has[:, None]
    if bool(moved.any()):
        m = int(moved.any(1).nonzero()[0])
        out.append(f"{int(moved.any(1).sum())} rows without an adapter changed; first row {m} (id {int(ids[m])})")
    if bool(torch.isnan(got.float()).any()):
        out.append(f"{int(torch.isnan(got.float()).sum())} NaN in Y")
    if window_touched(cage, N):
        out.append(f"{window_touched(cage, N)} sentinels around Y overwritten")
    return out


# ---------------------------------------------------------------------------------------------------------
# emulations


def shrink_emul(X: torch.Tensor, A: torch.Tensor, ids: torch.Tensor, n: int, T: torch.Tensor, *,
                mask32: bool = False, accept_n: bool = False, drop_partial: bool = False,
                swap_sub_blocks: bool = False, write_none: bool = False) -> None:
    """Writes T [M, R] bf16 in place: K in chunks of 64 dealt to NW waves, the waves' fp32 partials summed in wave
    order.  Mutants: the adapter mask built with a 32-bit shift (adapters from 32 on are never found), id ==
    n_adapters accepted (it reads what follows the last adapter: emulated as adapter 0), the partial of the wave
    that holds the last chunk dropped when chunks % NW != 0, the two 8-element sub-blocks of every 16 k swapped in X
    only, rows with id -1 written (with adapter 0's product)."""
    M, K = X.shape
    R = A.shape[1]
    _, NW = shrink_form(M, R)
    nchunks = K // 64
    idl = ids.long().clone()
    if accept_n:
        idl[idl == n] = 0
    if write_none:
        idl[idl == -1] = 0
    ok = (idl >= 0) & (idl < n)
    if mask32:
        ok &= idl < 32
    Xf = X.float()
    if swap_sub_blocks:
        Xf = Xf[:, torch.arange(K) ^ 8]
    kcol = torch.arange(K)
    for a in range(n):
        rows = (ok & (idl == a)).nonzero().flatten()
        if not rows.numel():
            continue
        total = torch.zeros(rows.numel(), R)
        for w in range(NW):
            if drop_partial and nchunks % NW != 0 and w == (nchunks - 1) % NW:
                continue
            ks = kcol[(kcol // 64) % NW == w]
            if ks.numel():
                total = total + Xf[rows][:, ks] @ A[a].float()[:, ks].t()
        T[rows] = total.to(BF)


def expand_emul(Y: torch.Tensor, T: torch.Tensor, B: torch.Tensor, ids: torch.Tensor, n: int, *,
                mask32: bool = False, read_upper_half: bool = False, round_twice: bool = False) -> None:
    """Y [M, N] bf16 in place.  Mutants: the 32-bit mask, the upper half of the last k-step read (from what follows
    in T and B: the next rows, the NaN sentinel after the last) when R % 32 == 16, the delta rounded to bf16 before
    the add."""
    M, N = Y.shape
    R = T.shape[1]
    ok = has_adapter(ids, n) & ((ids < 32) | (not mask32))
    ext = 16 if (read_upper_half and R % 32 == 16) else 0
    nan = torch.full((ext,), float("nan"))
    Tflat = torch.cat([T.float().reshape(-1), nan])
    Bflat = torch.cat([B.float().reshape(-1), nan])
    for a in range(n):
        rows = (ok & (ids == a)).nonzero().flatten()
        if not rows.numel():
            continue
        k = torch.arange(R + ext)
        t = Tflat[rows[:, None] * R + k[None, :]]
        b = Bflat[((a * N + torch.arange(N))[:, None]) * R + k[None, :]]
        delta = t @ b.t()
        if round_twice:
            delta = delta.to(BF).float()
        Y[rows] = (Y[rows].float() + delta).to(BF)


def chain_case():
    """(X, A, B, Y0, ids, n, want T fp64, want Y fp64) at CHAIN: shrink's sign family feeds expand.  T = RNE of
    multiples of 2^-3 within 8 * 128 = 2^10, B = +-2^(n % 3 - 1): terms multiples of 2^-4 within 2^11, 80 of them
    plus Y0: 2^15 * 80 + 2^7 < 2^24 units, so Y = RNE(Y0 + RNE(T) . B) is determined."""
    M, K, R, N = CHAIN
    X, A, ids, n, want_t = shrink_sign(M, K, R, "ids64")
    gen = _gen(M, K, R, N)
    B = (_signs((n, N, R), gen) * torch.exp2((torch.arange(N) % 3 - 1).float())[None, :, None]).to(BF)
    Y0 = torch.randint(-8, 9, (M, N), generator=gen).float().to(BF)
    assert (1 << 15) * R + (1 << 7) < (1 << 24)
    return X, A, B, Y0, ids, n, want_t, Y0.double() + product(rne(want_t), B, ids, n)
