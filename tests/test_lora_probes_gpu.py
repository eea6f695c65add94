"""lora_shrink and lora_expand_add (csrc/kernels/lora.hip) under the exact inputs of tests/lora_probes.py; every
comparison is bitwise.

  shrink   spike walks over every k at K = 64 (all twelve ranks), 128, 1088 and 4096; the sign family at M = 1, 16,
           17, 300 and at M = 8200 (the 4-, 2- and 1-row-tile forms); X a window with ldx = K + 8 over NaN padding;
           rows without an adapter (-1, n_adapters, 1000) keep the sentinel in T.
  expand   spike walks over every r at R = 16 .. 192 (KS = 1 .. 6, the zero-filled half step at R % 32 == 16), the
           sign family at N = 8, 24, 520 and M = 1, 16, 17, 300, 2100; Y a window with ldy = N + 8; T holds the NaN
           sentinel on rows without an adapter, whose rows of Y must not change.
  chain    shrink's output feeds expand at (300, 128, 80, 520).

64 adapters with 16 different ones in a 16-row tile and all 64 in a 64-row group, ids 0, 31, 32, 63; a 64-row group
without any adapter.  tests/test_lora_probes.py shows on the CPU what these comparisons reject.

Observed on an MI355X: all 70 cases bitwise, 2 s for the file."""
import pytest
import torch

from tests import lora_probes as lp
from tests.lora_probes import RowCage

pytestmark = pytest.mark.gpu


def _ops():
    from llm_weighted_consensus_amd import ops
    return ops


def _shrink(gpu, X, A, ids, n, want, what):
    xc, xv = lp.window(X, gpu)
    tc = RowCage((X.shape[0], A.shape[1]), gpu)
    assert A.shape[0] == n
    _ops().lora_shrink(xv, A.to(gpu), ids.to(gpu), out=tc.view)
    v = lp.shrink_violations(tc, want, ids, n)
    assert not v, f"lora_shrink {what}: " + "; ".join(v)
    assert lp.window_touched(xc, X.shape[1]) == 0
    return tc


def _expand(gpu, T, B, Y0, ids, n, want, what):
    N = Y0.shape[1]
    yc, yv = lp.window(Y0, gpu)
    assert _ops().lora_expand_add_(yv, T.to(gpu), B.to(gpu), ids.to(gpu)) is yv
    v = lp.expand_violations(yc, N, want, Y0, ids, n)
    assert not v, f"lora_expand_add {what}: " + "; ".join(v)


@pytest.mark.parametrize("K,R,fam", lp.SHRINK_WALK)
def test_shrink_walk(gpu, K, R, fam):
    X, A, ids, n, want = lp.shrink_walk(K, R, fam)
    _shrink(gpu, X, A, ids, n, want, f"walk K={K} R={R} {fam} form={lp.shrink_form(K, R)}")


@pytest.mark.parametrize("M,K,R,fam", lp.SHRINK_SIGN)
def test_shrink_sign(gpu, M, K, R, fam):
    X, A, ids, n, want = lp.shrink_sign(M, K, R, fam)
    _shrink(gpu, X, A, ids, n, want, f"sign M={M} K={K} R={R} {fam} form={lp.shrink_form(M, R)}")


@pytest.mark.parametrize("M,N,R,fam", lp.EXPAND_WALK)
def test_expand_walk(gpu, M, N, R, fam):
    T, B, Y0, ids, n, want = lp.expand_walk(M, N, R, fam)
    _expand(gpu, T, B, Y0, ids, n, want, f"walk M={M} N={N} R={R} {fam}")


@pytest.mark.parametrize("M,N,R,fam", lp.EXPAND_SIGN)
def test_expand_sign(gpu, M, N, R, fam):
    T, B, Y0, ids, n, want = lp.expand_sign(M, N, R, fam)
    _expand(gpu, T, B, Y0, ids, n, want, f"sign M={M} N={N} R={R} {fam}")


def test_shrink_feeds_expand(gpu):
    X, A, B, Y0, ids, n, want_t, want_y = lp.chain_case()
    tc = _shrink(gpu, X, A, ids, n, want_t, "chain")
    _expand(gpu, tc.view, B, Y0, ids, n, want_y, "chain")     # rows without an adapter still hold the sentinel
    torch.cuda.synchronize()
