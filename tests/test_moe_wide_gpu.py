"""The wide MoE routing kernels (csrc/kernels/moe_wide.hip: moe_route_wide, moe_router_wide and the 128-entry
permutation behind both) under the exact inputs of tests/select_probes.py, by the rules of
tests/test_select_probes_gpu.py: ids are the stable descending sort of the logits, logits of the exact families
are bitwise RNE(h . r), weights within W_ERR, row_off the prefix sum, the permutation valid, every output in a
sentinel cage.  ``h`` is the [:T, :d] window of a NaN buffer, so a read outside the window is a NaN logit.

  moe_route_wide   tied logits at E = 65, 100, 128, T = 1 .. 4097 (8200 routed rows: the permutation re-reads ids).
  moe_router_wide  +-1 / scaled rows and one-hot rows at d = 8, 256, 2048, 2056, 4096, six (E, k) that cover 2 to 8
                   accumulator tiles and E that are no multiple of 16, T on both sides of the 16-token tile; random
                   rows at the Qwen3-30B-A3B shape within one bf16 step of the fp64 product, two launches bitwise equal.
  refusals, and ops.route: E = 128 takes the wide kernel, E = 8 and E = 33 what they took before."""
import pytest
import torch

from tests import select_probes as sp
from tests.select_probes import BF, RowCage, bitwise, one_step, poison_a
from tests.test_select_probes_gpu import _gen, _intact, _route_cages, _route_checks

pytestmark = pytest.mark.gpu

WIDE_ROUTE_SHAPES = [(1, 128, 8), (5, 128, 8), (255, 65, 2), (300, 100, 8), (300, 128, 8), (1025, 128, 8),
                     (4097, 128, 1)]
WIDE_EK = [(17, 1), (64, 8), (65, 2), (96, 4), (100, 8), (128, 8)]
WIDE_TS = [1, 15, 16, 17, 130]


def _ops():
    from llm_weighted_consensus_amd import ops
    return ops


@pytest.mark.parametrize("T,E,k", WIDE_ROUTE_SHAPES)
def test_route_wide_tied_logits(gpu, T, E, k):
    lg = sp.route_logits(T, E, k, _gen(T, E, k))
    cages = _route_cages(gpu, T, E, k)
    _ops().kernels().moe_route_wide(lg.to(gpu), k, *[c.view for c in cages])
    _route_checks(gpu, f"route_wide T={T} E={E} k={k}", cages, lg, T, E, k, 2.0)


def _router_wide(gpu, what, h, r, T, E, k, exact=True):
    """One fused launch on poisoned h: the logits (bitwise for the exact families), the selection on the kernel's
    own logits, and moe_route_wide on those logits giving the identical result.  Returns the logits cage."""
    ops = _ops()
    hv = poison_a(h, gpu)
    cages = _route_cages(gpu, T, E, k)
    cl = RowCage((T, E), gpu, BF)
    ops.kernels().moe_router_wide(hv, r.to(gpu), k, *[c.view for c in cages], cl.view)
    _intact(what, cl)
    if exact:
        want = sp.router_want(h, r)
        bad = bitwise(cl.view, want.to(gpu))
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} logits differ from RNE(h . r)"
    lg = cl.view.cpu()
    _route_checks(gpu, what, cages, lg, T, E, k, float(lg.float().abs().max()))
    n = T * k
    ids2, w2, ro2, _, _ = ops.moe_route_wide(cl.view, k)
    assert torch.equal(ids2.flatten(), cages[0].view[:n]) and torch.equal(ro2, cages[2].view), what
    torch.testing.assert_close(w2.flatten(), cages[1].view[:n], rtol=0, atol=0)
    return cl, cages


@pytest.mark.parametrize("E,k", WIDE_EK)
@pytest.mark.parametrize("d", sp.ROUTER_DS)
def test_router_wide_sign_rows(gpu, d, E, k):
    for T in WIDE_TS:
        for scaled in (False, True):
            h, r = sp.router_sign(T, E, d, _gen(T, E, d, k), scaled)
            _router_wide(gpu, f"router_wide sign T={T} E={E} k={k} d={d} scaled={scaled}", h, r, T, E, k)


@pytest.mark.parametrize("E,k", WIDE_EK)
@pytest.mark.parametrize("d", sp.ROUTER_DS)
def test_router_wide_one_hot(gpu, d, E, k):
    walks = [sp.router_chunks(d, T) for T in WIDE_TS]
    if (E, k) == (128, 8) and d == 2056:
        walks.append(sp.router_chunks(d))                   # every chunk once
    for ch in walks:
        h, r = sp.router_onehot(d, ch, E, _gen(len(ch), E, d))
        _router_wide(gpu, f"router_wide one-hot T={len(ch)} E={E} k={k} d={d}", h, r, len(ch), E, k)


def test_router_wide_random_rows(gpu):
    """h, router ~ N(0, 1) in bf16 at (T, E, k, d) = (130, 128, 8, 2048): fp32 accumulation of 2048 exact products
    is off by at most 2048 * 2^-24 of sum |h r|, far below the half step of the bf16 store, so every logit is
    within one bf16 step of the fp64 product; the selection is checked on the kernel's logits; a second launch
    gives the same bits."""
    T, E, k, d = 130, 128, 8, 2048
    gen = _gen(T, E, k, d)
    h, r = torch.randn(T, d, generator=gen).to(BF), torch.randn(E, d, generator=gen).to(BF)
    what = "router_wide random"
    cl, cages = _router_wide(gpu, what, h, r, T, E, k, exact=False)
    want = h.double() @ r.double().t()
    bad = one_step(cl.view, want.to(gpu))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} logits off one bf16 step"
    cl2, cages2 = _router_wide(gpu, what + " (again)", h, r, T, E, k, exact=False)
    assert not bool(bitwise(cl2.view, cl.view).any()), "two launches differ in their logits"
    n = T * k
    assert torch.equal(cages2[0].view[:n], cages[0].view[:n])
    assert not bool(sp.same32(cages2[1].view[:n], cages[1].view[:n]).any()), "two launches differ in their weights"


def test_wide_refusals(gpu):
    ops = _ops()
    z = lambda *s: torch.zeros(*s, dtype=BF, device=gpu)  # noqa: E731
    for E, k in [(129, 8), (16, 4), (128, 9), (17, 18), (128, 0)]:
        with pytest.raises(RuntimeError):
            ops.moe_route_wide(z(4, E), k)
        with pytest.raises(RuntimeError):
            ops.moe_router_wide(z(4, 64), z(E, 64), k)
    with pytest.raises(RuntimeError):                       # d % 8
        ops.moe_router_wide(z(4, 12), z(128, 12), 8)
    with pytest.raises(RuntimeError):                       # ldh = d + 4
        ops.moe_router_wide(z(4, 68)[:, :64], z(128, 64), 8)
    with pytest.raises(RuntimeError):                       # a CPU operand
        ops.moe_router_wide(z(4, 64), torch.zeros(128, 64, dtype=BF), 8)
    with pytest.raises(RuntimeError):
        ops.moe_route_wide(torch.zeros(4, 128, dtype=BF), 8)
    with pytest.raises(RuntimeError):                       # a strided router
        ops.moe_router_wide(z(4, 64), z(128, 128)[:, ::2], 8)
    with pytest.raises(RuntimeError):                       # the narrow kernel still refuses what it refused
        ops.moe_route(z(4, 65), 2)
    ids, w, ro, src, inv = ops.moe_route_wide(z(0, 128), 8)  # T = 0: empty segments, no launch
    assert ids.shape == (0, 8) and not bool(ro.any())
    torch.cuda.synchronize()


def test_route_sends_wide_shapes_to_the_wide_kernel(gpu, monkeypatch):
    """ops.route: E = 128 is moe_router_wide (fused) or F.linear + moe_route_wide (rows the fused kernel does not
    take); E = 8 and E = 33 return what moe_router and F.linear + moe_route return."""
    ops = _ops()
    gen = _gen(128, 8)
    T, d = 37, 256
    h = torch.randn(T, d, generator=gen).to(BF).to(gpu)
    calls = []
    for name in ("moe_router_wide", "moe_route_wide", "moe_router", "moe_route"):
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **kw: (calls.append(n), f(*a, **kw))[1])(
            getattr(ops, name), name))

    def same(got, want):
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
        assert not bool(sp.same32(got[1], want[1]).any())

    r = torch.randn(128, d, generator=gen).to(BF).to(gpu)
    got = ops.route(h, r, 8)
    assert calls == ["moe_router_wide"], calls
    same(got, ops.moe_router_wide(h, r, 8))
    calls.clear()
    h12 = torch.randn(T, 12, generator=gen).to(BF).to(gpu)     # d % 8 != 0: the unfused pair
    r12 = torch.randn(128, 12, generator=gen).to(BF).to(gpu)
    got = ops.route(h12, r12, 8)
    assert calls == ["moe_route_wide"], calls
    same(got, ops.moe_route_wide(torch.nn.functional.linear(h12, r12), 8))
    for E, k, fused in ((8, 2, True), (33, 8, False)):
        calls.clear()
        r = torch.randn(E, d, generator=gen).to(BF).to(gpu)
        got = ops.route(h, r, k)
        assert calls == ["moe_router" if fused else "moe_route"], calls
        same(got, ops.moe_router(h, r, k) if fused else ops.moe_route(torch.nn.functional.linear(h, r), k))
