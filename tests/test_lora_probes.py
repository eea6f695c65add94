"""What the comparisons of tests/test_lora_probes_gpu.py accept and reject, shown on the CPU: the emulations of
lora_shrink and lora_expand_add in tests/lora_probes.py pass every case, the exactness bounds of the sign families
hold for every shape used, and each mutant is rejected by the named case:

  shrink   adapter mask built with a 32-bit shift          walk (64, 16, ids64): adapters 32..63 never found
           id == n_adapters accepted                       sign (300, 1088, 160, ids3): id 3 of 3 adapters
           a wave's partial dropped (chunks % NW != 0)     walk (1088, 48 / 80 / 176): 17 chunks over 16 / 8 / 4 waves
           two k sub-blocks swapped in one operand         walk (64, 16, ids64)
           T rows written for ids of -1                    walk (64, 16, ids64)
  expand   the last k-step's upper half read, not zeroed   walk (300, 24, 48 / 80 / 144 / 176): R % 32 == 16
           mask built with a 32-bit shift                  walk (300, 24, 16, ids64)
           Y rounded twice                                 sign (300, 520, 192, ids3)"""
import pytest
import torch

from tests import lora_probes as lp
from tests.lora_probes import BF, RowCage, bits


def _shrink(X, A, ids, n, **mut):
    cage = RowCage((X.shape[0], A.shape[1]))
    lp.shrink_emul(X, A, ids, n, cage.view, **mut)
    return cage


def _expand(T, B, Y0, ids, n, **mut):
    cage, y = lp.window(Y0)
    lp.expand_emul(y, T, B, ids, n, **mut)
    return cage


def test_shapes_cover_every_instantiation_and_the_bounds_hold():
    shrink = [(K, K, R) for K, R, _ in lp.SHRINK_WALK] + [(M, K, R) for M, K, R, _ in lp.SHRINK_SIGN]
    assert {R for M, _, R in shrink if M <= 8192} == set(lp.ALL_R)
    assert {R for M, _, R in shrink if M == 8200} == {16, 80, 112, 192}
    assert {lp.shrink_form(8200, R)[0] for R in (16, 80, 112, 192)} == {4, 2, 1}
    assert {K for _, K, _ in shrink} == {64, 128, 1088, 4096}
    for K in (64, 128, 1088, 4096):                      # every wave count meets every kind of chunk count
        assert {lp.shrink_form(M, R)[1] for M, k, R in shrink if k == K and M <= 8192} == {16, 8, 4}
    assert {M for M, _, _, _ in lp.SHRINK_SIGN} >= {1, 16, 17, 300}
    expand = lp.EXPAND_WALK + lp.EXPAND_SIGN
    assert {R for _, _, R, _ in expand} == set(lp.EXPAND_R)
    assert {(R + 31) // 32 for R in lp.EXPAND_R} == set(range(1, 7))
    assert {N for _, N, _, _ in expand} == {8, 24, 520} and {M for M, _, _, _ in expand} == {1, 16, 17, 300, 2100}
    assert all(lp.shrink_bound(K) < (1 << 24) for _, K, _ in shrink)
    assert all(lp.expand_bound(R) < (1 << 24) for _, _, R, _ in expand)


def test_the_id_families():
    ids, n = lp.make_ids("ids64", 300)
    assert n == 64 and set(ids[:64].tolist()) == set(range(64)) and {0, 31, 32, 63} <= set(ids.tolist())
    assert all(len(set(ids[t:t + 16].tolist())) == 16 for t in (0, 16, 32, 48))
    assert bool((ids[128:192] == -1).all()) and bool((ids[64:128] == -1).any()) and bool((ids[64:128] >= 0).any())
    ids, n = lp.make_ids("ids64", 64)
    assert -1 in ids.tolist() and {0, 31, 32, 62} <= set(ids.tolist())
    ids, n = lp.make_ids("ids3", 300)
    assert n == 3 and set(ids.tolist()) == {0, 1, 2, 3, 1000, -1}
    assert set(ids[:16].tolist()) == {0, 1, 2, 3, 1000, -1}
    assert lp.has_adapter(ids, n).tolist() == [i in (0, 1, 2) for i in ids.tolist()]


@pytest.mark.parametrize("K,R,fam", lp.SHRINK_WALK)
def test_shrink_walk_emulation_and_mutants(K, R, fam):
    X, A, ids, n, want = lp.shrink_walk(K, R, fam)
    has = lp.has_adapter(ids, n)
    assert not lp.shrink_violations(_shrink(X, A, ids, n), want, ids, n)
    if K > 1088:                                             # the long loop: the honest emulation only
        return
    assert not bool(lp.bitwise(lp.rne(lp.product(X, A, ids, n)), want)[has].any()), "the copy is not the product"
    assert lp.shrink_violations(_shrink(X, A, ids, n, swap_sub_blocks=True), want, ids, n)
    if -1 in ids.tolist():
        assert lp.shrink_violations(_shrink(X, A, ids, n, write_none=True), want, ids, n)
    if fam == "ids64":
        assert lp.shrink_violations(_shrink(X, A, ids, n, mask32=True), want, ids, n)
    else:
        assert lp.shrink_violations(_shrink(X, A, ids, n, accept_n=True), want, ids, n)
    if (K // 64) % lp.shrink_form(K, R)[1] != 0:
        assert lp.shrink_violations(_shrink(X, A, ids, n, drop_partial=True), want, ids, n)
    assert (K, R) != (1088, 48) or (17 % 16, lp.shrink_form(K, R)[1]) == (1, 16)


@pytest.mark.parametrize("M,K,R,fam", lp.SHRINK_SIGN)
def test_shrink_sign_emulation_and_mutants(M, K, R, fam):
    X, A, ids, n, want = lp.shrink_sign(M, K, R, fam)
    assert bool((want.float().double() == want).all()) and float(want.abs().max()) * 8 <= lp.shrink_bound(K)
    assert not lp.shrink_violations(_shrink(X, A, ids, n), want, ids, n)
    if (M, K, R) == (300, 1088, 160):
        assert lp.shrink_violations(_shrink(X, A, ids, n, accept_n=True), want, ids, n)
        assert lp.shrink_violations(_shrink(X, A, ids, n, drop_partial=True), want, ids, n)


@pytest.mark.parametrize("M,N,R,fam", lp.EXPAND_WALK)
def test_expand_walk_emulation_and_mutants(M, N, R, fam):
    T, B, Y0, ids, n, want = lp.expand_walk(M, N, R, fam)
    assert set(lp.walk_r(ids, n, R)[lp.has_adapter(ids, n)].tolist()) == set(range(R)), "some r is never walked"
    assert not lp.expand_violations(_expand(T, B, Y0, ids, n), N, want, Y0, ids, n)
    if R % 32 == 16:
        assert lp.expand_violations(_expand(T, B, Y0, ids, n, read_upper_half=True), N, want, Y0, ids, n)
    if fam == "ids64":
        assert lp.expand_violations(_expand(T, B, Y0, ids, n, mask32=True), N, want, Y0, ids, n)


@pytest.mark.parametrize("M,N,R,fam", lp.EXPAND_SIGN)
def test_expand_sign_emulation_and_mutants(M, N, R, fam):
    T, B, Y0, ids, n, want = lp.expand_sign(M, N, R, fam)
    assert bool(torch.isnan(T.float()).any(1).eq(~lp.has_adapter(ids, n)).all())
    assert float(want.abs().max()) * 2 <= lp.expand_bound(R)
    assert not lp.expand_violations(_expand(T, B, Y0, ids, n), N, want, Y0, ids, n)
    if (M, N, R) == (300, 520, 192):
        assert lp.expand_violations(_expand(T, B, Y0, ids, n, round_twice=True), N, want, Y0, ids, n)
    if R % 32 == 16 and M > 1:
        assert lp.expand_violations(_expand(T, B, Y0, ids, n, read_upper_half=True), N, want, Y0, ids, n)


def test_the_violations_see_what_they_should():
    T, B, Y0, ids, n, want = lp.expand_sign(17, 24, 16, "ids3")
    cage = _expand(T, B, Y0, ids, n)
    none = int((~lp.has_adapter(ids, n)).nonzero()[0])
    cage.view[none, 0] += 1                                  # a row without an adapter moved
    assert lp.expand_violations(cage, 24, want, Y0, ids, n)
    cage = _expand(T, B, Y0, ids, n)
    bits(cage.view)[0, 24] = 0                               # a padding column of the window written
    assert lp.expand_violations(cage, 24, want, Y0, ids, n)
    X, A, ids, n, want = lp.shrink_sign(17, 64, 16, "ids3")
    cage = _shrink(X, A, ids, n)
    cage.buf[0] = 0
    assert lp.shrink_violations(cage, want, ids, n)


def test_the_chain_case_is_determined_and_the_emulations_pass_it():
    X, A, B, Y0, ids, n, want_t, want_y = lp.chain_case()
    tc = _shrink(X, A, ids, n)
    assert not lp.shrink_violations(tc, want_t, ids, n)
    assert bool((want_y.float().double() == want_y).all())
    assert not lp.expand_violations(_expand(tc.view, B, Y0, ids, n), Y0.shape[1], want_y, Y0, ids, n)
