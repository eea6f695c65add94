"""The scoring kernels (pool_l2norm, cosine_consensus, knn_topk, vote_tally) and the MoE selection and dispatch
kernels (moe_route, moe_router, moe_combine) under the exact inputs of tests/select_probes.py.

The tests of these kernels in tests/test_kernels_gpu.py compare unit-vector components of 1/32 under atol 1e-2, run
the consensus once at n = 37, allow 1e-5 on kNN values that exact inputs determine, accept either order of tied
experts and never launch the 64-expert top-k; moe_combine had no single-GPU test.  Here every index output is
held to a stable descending sort of exact scores, every determined value bitwise, and the rest to the bounds
derived in the helper module's docstring (POOL_ERR, W_ERR, the S sum bound, one_step / one_step_cond):

  pool_l2norm       spike walks over every column at d = 8, 256, 264, 1000, 4096 (cu = arange, LAST; the other
                    modes at 264), integer sequences of lengths 3, 1, 0, 30, 2, 1 in all three modes, contiguous and
                    with ld = d + 8 over NaN padding, out_bf16 = None; fp32 within POOL_ERR, bf16 one_step, exact
                    zeros for the zero-length sequence and the zero row; d = 4104 refused.
  cosine_consensus  +-1 / scaled rows at d = 32, 96, 1024, n = 1, 2, 15, 16, 17, 33, R = 1, 3 and n = 1024 at d = 32:
                    S, centrality and best bitwise with a planted tie; random and clustered unit rows at
                    n = 2, 5, 20, d = 384, 4096, tau = 0.05, 0.001: S within the sum bound, centrality bitwise the
                    serial sum of the kernel's S, best its first maximum, weights within W_ERR; n = 1040 refused.
  knn_topk          integer tables: values and rows bitwise at every shape of KNN_SHAPES (one, two and three merge
                    levels, -1 fillers, single-list merges), five families; k = 65 and k = n + 1 refused.
  vote_tally        C = 1024, a request without a valid voter, R = 0; C = 1025 refused.
  moe_route         tied logits at every shape of ROUTE_SHAPES (all three top-k instances, both permutation
                    paths): ids bitwise, weights within W_ERR(2), row_off exact, the permutation, caged tails.
  moe_router        +-1 / scaled and one-hot rows at d = 8, 256, 2048, 2056, 4096: logits bitwise, ids the stable
                    sort of them, everything identical to moe_route on those logits; strided rows over NaN padding.
  moe_combine       exact, fine, one-hot (bitwise) and random (one_step_cond) families on a permutation from
                    moe_route, NaN rows behind Y, a caged output; d = 12 refused.

Every output sits in a RowCage whose sentinels must survive.  tests/test_select_probes.py shows on the CPU what
these comparisons reject.  The tests print what they measured (pytest -s).

Observed on an MI355X: every bitwise comparison held.  pool_l2norm: worst fp32 error 0.29 x 2^-24 on the walks and
1.8 x 2^-24 on the integer sequences (POOL_ERR is 32 x 2^-24).  cosine_consensus on unit rows: S at most 1.3 % of
its sum bound, weights at most 1.1 % of W_ERR, finite at tau = 0.001.  moe_combine, random family: every
well-conditioned output within one code; plain one_step would have failed 3 of 4.3 million outputs (up to 8 codes,
all of them outputs whose terms cancel below 2^-10 of their magnitude).  The file's 147 cases ran in 6 s."""
import random

import pytest
import torch

from tests import select_probes as sp
from tests.select_probes import BF, RowCage, bitwise, one_step, poison_a

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32


def _ops():
    from llm_weighted_consensus_amd import ops
    return ops


def _K():
    return _ops().kernels()


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 43)


def _intact(what, *cages):
    for c in cages:
        assert c.outside_touched() == 0, f"{what}: {c.outside_touched()} sentinels around an output overwritten"
        assert c.unwritten() == 0, f"{what}: {c.unwritten()} outputs never written"


# ---------------------------------------------------------------------------------------------------------
# pool_l2norm


def _pool(gpu, view, cu, mode, want, what, bf16=True):
    n, d = cu.numel() - 1, view.shape[1]
    cf = RowCage((n, d), gpu, F32)
    cb = RowCage((n, d), gpu, BF) if bf16 else None
    _K().pool_l2norm(view, cu.to(gpu), mode, cf.view, cb.view if bf16 else None)
    v = sp.pool_violations(cf.view, cb.view if bf16 else None, want)
    assert not v, f"{what}: " + "; ".join(v)
    _intact(what, *([cf, cb] if bf16 else [cf]))
    return float(((cf.view.double() - want.to(gpu)).abs() / want.to(gpu).abs().clamp(min=1e-30)).max())


@pytest.mark.parametrize("d", sp.POOL_WALK_DS)
def test_pool_spike_walk(gpu, d):
    cols = sp.pool_cols(d)
    worst = 0.0
    for i in range(0, len(cols), 512):
        x = sp.pool_walk(d, cols[i:i + 512])
        want = x.double() / x.double().norm(dim=1, keepdim=True)
        cu = torch.arange(x.shape[0] + 1, dtype=I32)
        for pad in (0, 8):
            worst = max(worst, _pool(gpu, sp.framed(x, pad, device=gpu), cu, 2, want, f"walk d={d} cols {i}.. ld=d+{pad}"))
        if i == 0:
            _pool(gpu, sp.framed(x, 8, device=gpu), cu, 2, want, f"walk d={d} without a bf16 output", bf16=False)
            if d == 264:
                for mode in (0, 1):
                    _pool(gpu, sp.framed(x, 8, device=gpu), cu, mode, want, f"walk d={d} mode {mode}")
    print(f"\n[select] pool walk d={d}: worst fp32 error {worst / 2.0 ** -24:.2f} x 2^-24 (POOL_ERR = 32 x 2^-24)")


@pytest.mark.parametrize("d", [8, 264, 1024, 4096])
def test_pool_integer_sequences(gpu, d):
    h, cu = sp.pool_seqs(d, _gen(d))
    worst = 0.0
    for mode in (0, 1, 2):
        want = sp.pool_want(h, cu, mode)
        for pad in (0, 8):
            worst = max(worst, _pool(gpu, sp.framed(h, pad, device=gpu), cu, mode, want, f"seqs d={d} mode {mode} ld=d+{pad}"))
        _pool(gpu, sp.framed(h, 8, device=gpu), cu, mode, want, f"seqs d={d} mode {mode} fp32 only", bf16=False)
    print(f"\n[select] pool seqs d={d}: worst fp32 error {worst / 2.0 ** -24:.2f} x 2^-24")


def test_pool_refusals(gpu):
    ops = _ops()
    cu = torch.tensor([0, 2], dtype=I32, device=gpu)
    with pytest.raises(RuntimeError):
        ops.pool_l2norm(torch.zeros(2, 4104, dtype=BF, device=gpu), cu, ops.POOL_MEAN)
    with pytest.raises(RuntimeError):
        ops.pool_l2norm(torch.zeros(2, 64, dtype=BF, device=gpu), torch.tensor([0, 9, 2, 9], dtype=I32, device=gpu)[::2],
                        ops.POOL_MEAN)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# cosine_consensus


def _consensus(gpu, E, tau):
    R, n, d = E.shape
    n_pad = (n + 15) // 16 * 16
    cS, cc, cw, cb = (RowCage((R, n_pad, n_pad), gpu, F32), RowCage((R, n), gpu, F32), RowCage((R, n), gpu, F32),
                      RowCage((R,), gpu, I32))
    _K().cosine_consensus(E.to(gpu).contiguous(), cS.view, 1.0 / float(tau), cc.view, cw.view, cb.view)
    _intact(f"consensus {tuple(E.shape)}", cS, cc, cw, cb)
    return cS.view[:, :n, :n].cpu(), cc.view.cpu(), cw.view.cpu(), cb.view.cpu()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("d", sp.CONS_DS)
def test_consensus_exact(gpu, d, scaled):
    for R in sp.CONS_RS:
        for n in sp.CONS_NS:
            E = sp.plant_tie(sp.sign_rows(R, n, d, _gen(R, n, d), scaled))
            S, cen, w, best = _consensus(gpu, E, 0.05)
            v = sp.consensus_exact_violations(S, cen, best, E)
            x = sp.cen_exact(sp.gram(E)).double() * sp.inv_tau32(0.05)
            v += sp.softmax_violations(w, x, float(x.abs().max()))
            assert not v, f"R={R} n={n} d={d}: " + "; ".join(v)
            if n == 1:   # a sole candidate: centrality 1, weight 1, best 0
                assert cen.tolist() == [[1.0]] * R and w.tolist() == [[1.0]] * R and best.tolist() == [0] * R


def test_consensus_exact_largest_n(gpu):
    R, n, d = sp.CONS_BIG
    E = sp.plant_tie(sp.sign_rows(R, n, d, _gen(R, n, d), scaled=True))
    S, cen, w, best = _consensus(gpu, E, 0.05)
    v = sp.consensus_exact_violations(S, cen, best, E)
    assert not v, "; ".join(v)
    assert bool(torch.isfinite(w).all()) and abs(float(w.double().sum()) - 1) <= n * 2.0 ** -23


@pytest.mark.parametrize("clustered", [False, True])
@pytest.mark.parametrize("tau", [0.05, 0.001])
@pytest.mark.parametrize("n,d", [(2, 384), (5, 384), (20, 384), (2, 4096), (5, 4096), (20, 4096)])
def test_consensus_unit_rows(gpu, n, d, tau, clustered):
    E = sp.unit_rows(3, n, d, _gen(n, d, clustered), clustered)
    S, cen, w, best = _consensus(gpu, E, tau)
    v = sp.consensus_random_violations(S, cen, w, best, E, tau)
    assert not v, "; ".join(v)
    ref = E.double() @ E.double().transpose(1, 2)
    sm = torch.softmax(cen.double() * sp.inv_tau32(tau), -1)
    print(f"\n[select] consensus n={n} d={d} tau={tau}: S error {float(((S.double() - ref).abs() / sp.s_bound(E)).max()):.4f} "
          f"of its bound, weights {float(((w.double() - sm).abs() / sm.clamp(min=1e-30)).max()) / sp.W_ERR(1.01 / tau):.4f} "
          f"of W_ERR")


def test_consensus_refusals(gpu):
    ops = _ops()
    with pytest.raises(RuntimeError):
        ops.cosine_consensus(torch.ones(1, 1040, 32, dtype=BF, device=gpu))
    E = torch.ones(2, 4, 32, dtype=BF, device=gpu)
    S = torch.empty(2, 16, 16, dtype=F32, device=gpu)
    cen, w, best = (torch.empty(2, 8, dtype=F32, device=gpu), torch.empty(2, 4, dtype=F32, device=gpu),
                    torch.empty(2, dtype=I32, device=gpu))
    with pytest.raises(RuntimeError):       # a strided output would be written as if it were flat
        _K().cosine_consensus(E, S, 20.0, cen[:, ::2], w, best)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# knn_topk


@pytest.mark.parametrize("n,k", sp.KNN_SHAPES)
def test_knn_exact(gpu, n, k):
    ops = _ops()
    for d in sp.knn_d(n):
        for fam in sp.knn_families(n, k) + (["wide"] if d == 64 else []):
            E, q = sp.knn_case(fam, n, d, k, _gen(n, k, d))
            vals, rows = ops.knn_topk(E.to(gpu), q.to(gpu), k)
            v = sp.knn_violations(vals, rows, E, q, k)
            assert not v, f"n={n} k={k} d={d} {fam}: " + "; ".join(v)


def test_knn_refusals(gpu):
    ops = _ops()
    E, q = torch.ones(100, 4, device=gpu), torch.ones(4, device=gpu)
    for E_, k in [(E, 65), (E[:10], 11), (E, 0)]:
        with pytest.raises(RuntimeError):
            ops.knn_topk(E_, q, k)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# vote_tally


def test_vote_tally_edges(gpu):
    from llm_weighted_consensus_amd import _runtime as RT
    from llm_weighted_consensus_amd.score import tally_batch as TB
    from tests.test_vote_tally import _Choice, _request, _same

    ops = _ops()
    rng = random.Random(11)
    silent = [_Choice(None, rng.random()) for _ in range(5)]          # no voter has a vote: sum 0, confidence 0
    batches = [[(1024, _request(rng, 1024, 3))],
               [(4, _request(rng, 4, 6)), (4, silent), (7, _request(rng, 7, 9))]]
    for batch in batches:
        items = [TB.vote_rows(ch) + (C,) for C, ch in batch]
        for (votes, wts, C), t in zip(items, TB.tally_many_gpu(items, gpu)):
            r = RT.tally(votes, wts, C)
            _same(t.choice_weight, r.choice_weight)
            _same(t.confidence, r.confidence)
            _same(t.voter_confidence, r.voter_confidence)
    got = TB.tally_many_gpu([TB.vote_rows(silent) + (4,)], gpu)[0]
    assert got.confidence == [0.0] * 4 and got.choice_weight == [0.0] * 4
    cw, conf, vconf = ops.vote_tally(torch.zeros(0, 3, 4, dtype=torch.float64, device=gpu),
                                     torch.zeros(0, 3, dtype=torch.float64, device=gpu),
                                     torch.zeros(0, 3, dtype=torch.uint8, device=gpu))
    assert cw.shape == (0, 4) and conf.shape == (0, 4) and vconf.shape == (0, 3)
    with pytest.raises(RuntimeError):
        ops.vote_tally(torch.zeros(1, 2, 1025, dtype=torch.float64, device=gpu),
                       torch.zeros(1, 2, dtype=torch.float64, device=gpu), torch.ones(1, 2, dtype=torch.uint8, device=gpu))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# moe_route / moe_router


def _route_cages(gpu, T, E, k):
    n = T * k
    return (sp.tail_cage(n, I32, gpu), sp.tail_cage(n, F32, gpu), RowCage((E + 1,), gpu, I32), sp.tail_cage(n, I32, gpu),
            sp.tail_cage(n, I32, gpu))


def _route_checks(gpu, what, cages, logits, T, E, k, x_max):
    from tests.test_kernels_gpu import _check_permutation

    n = T * k
    ids, w, ro, src, inv = cages
    for c in (ids, w, src, inv):
        assert sp.tail_touched(c, n) == 0, f"{what}: sentinels behind T k entries overwritten"
        assert int((c.view[:n].view(c.raw_dtype) == c.code).sum()) == 0, f"{what}: entries never written"
    _intact(what, ro)
    v = sp.route_violations(ids.view[:n], w.view[:n].cpu(), ro.view, logits, k, x_max)
    assert not v, f"{what}: " + "; ".join(v)
    _check_permutation(gpu, ids.view[:n].view(T, k), ro.view, src.view[:n], inv.view[:n], T, E, k)


@pytest.mark.parametrize("T,E,k", sp.ROUTE_SHAPES)
def test_route_tied_logits(gpu, T, E, k):
    lg = sp.route_logits(T, E, k, _gen(T, E, k))
    cages = _route_cages(gpu, T, E, k)
    _K().moe_route(lg.to(gpu), k, *[c.view for c in cages])
    _route_checks(gpu, f"route T={T} E={E} k={k}", cages, lg, T, E, k, 2.0)


def test_route_refusals(gpu):
    ops = _ops()
    for E, k in [(65, 2), (16, 9), (2, 3), (8, 0)]:
        with pytest.raises(RuntimeError):
            ops.moe_route(torch.zeros(4, E, dtype=BF, device=gpu), k)
    torch.cuda.synchronize()


def _router(gpu, what, h, r, T, E, k):
    ops = _ops()
    hv = poison_a(h, gpu)                                   # [:T, :d] of a NaN buffer: strided rows, NaN rows below
    cages = _route_cages(gpu, T, E, k)
    cl = RowCage((T, E), gpu, BF)
    _K().moe_router(hv, r.to(gpu), k, *[c.view for c in cages], cl.view)
    _intact(what, cl)
    want = sp.router_want(h, r)
    bad = bitwise(cl.view, want.to(gpu))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} logits differ from RNE(h . r)"
    lg = cl.view.cpu()
    _route_checks(gpu, what, cages, lg, T, E, k, float(want.float().abs().max()))
    n = T * k
    ids2, w2, ro2, _, _ = ops.moe_route(cl.view, k)          # the unfused pair on the same logits
    assert torch.equal(ids2.flatten(), cages[0].view[:n]) and torch.equal(ro2, cages[2].view), what
    torch.testing.assert_close(w2.flatten(), cages[1].view[:n], rtol=0, atol=0)


@pytest.mark.parametrize("E,k", sp.ROUTER_EK)
@pytest.mark.parametrize("d", sp.ROUTER_DS)
def test_router_sign_rows(gpu, d, E, k):
    for T in sp.ROUTER_TS:
        for scaled in (False, True):
            h, r = sp.router_sign(T, E, d, _gen(T, E, d, k), scaled)
            _router(gpu, f"router sign T={T} E={E} k={k} d={d} scaled={scaled}", h, r, T, E, k)


@pytest.mark.parametrize("E,k", sp.ROUTER_EK)
@pytest.mark.parametrize("d", sp.ROUTER_DS)
def test_router_one_hot(gpu, d, E, k):
    walks = [sp.router_chunks(d, T) for T in sp.ROUTER_TS]
    if (E, k) in ((8, 2), (16, 4)):
        walks.append(sp.router_chunks(d))                   # every chunk once
    for ch in walks:
        h, r = sp.router_onehot(d, ch, E, _gen(len(ch), E, d))
        _router(gpu, f"router one-hot T={len(ch)} E={E} k={k} d={d}", h, r, len(ch), E, k)


# ---------------------------------------------------------------------------------------------------------
# moe_combine


@pytest.mark.parametrize("d", sp.COMBINE_DS)
@pytest.mark.parametrize("k", sp.COMBINE_KS)
@pytest.mark.parametrize("T", sp.COMBINE_TS)
def test_combine(gpu, T, k, d):
    ops = _ops()
    gen = _gen(T, k, d)
    _, _, _, _, inv = ops.moe_route(sp.route_logits(T, 8, k, gen).to(gpu), k)
    assert torch.equal(inv.long().sort().values.cpu(), torch.arange(T * k))
    for kind in ("exact", "fine", "onehot", "random"):
        Y, w = sp.combine_inputs(kind, T, k, d, gen, rows=T * k + 8)
        sp.bits(Y)[T * k:] = sp.SENTINEL                    # rows no inv entry names
        want, mag = sp.combine_want(Y, inv, w, k)
        cage = RowCage((T, d), gpu, BF)
        _K().moe_combine(Y.to(gpu), inv, w.to(gpu), k, cage.view)
        v = sp.combine_violations(cage, want, mag, kind)
        assert not v, f"combine {kind} T={T} k={k} d={d}: " + "; ".join(v)
        _intact(f"combine {kind}", cage)
        if kind == "random":
            plain = one_step(cage.view, want.to(gpu))
            print(f"\n[select] combine random T={T} k={k} d={d}: {int(plain.sum())} of {plain.numel()} outputs off plain "
                  f"one_step, worst {int(sp.steps(cage.view, want.to(gpu)).max())} code(s)")


def test_combine_refusals(gpu):
    ops = _ops()
    Y = torch.zeros(8, 12, dtype=BF, device=gpu)
    inv = torch.arange(8, dtype=I32, device=gpu)
    w = torch.ones(4, 2, device=gpu)
    with pytest.raises(RuntimeError):
        ops.moe_combine(Y, inv, w, 2)
    Y = torch.zeros(8, 16, dtype=BF, device=gpu)
    with pytest.raises(RuntimeError):       # strided inv / w would be read as if they were flat
        ops.moe_combine(Y, torch.arange(16, dtype=I32, device=gpu)[::2], w, 2)
    with pytest.raises(RuntimeError):
        ops.moe_combine(Y, inv, torch.ones(4, 4, device=gpu)[:, ::2], 2)
    torch.cuda.synchronize()
