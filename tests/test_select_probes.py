"""The probes of tests/select_probes.py would notice the failures they target (CPU only).

For every check the GPU file makes, a plain torch emulation of the kernel's contract (fp32 where the kernel is,
summing in another order) passes on the probe inputs, and the same emulation broken in one way is rejected:

  pool_l2norm       mean over [t0, t1 - 1) and over [t0, t1], LAST reading t1, the row stride ignored, the last
                    column trip left out of ss, a zero-length / all-zero row giving NaN.
  cosine_consensus  centrality keeping the diagonal, dividing by n, ``best`` ties to the higher index, a softmax
                    without the max subtraction at tau = 0.001, an off-diagonal 16 x 16 tile of S transposed inside
                    itself, the last 32 columns of d skipped.
  knn_topk          ties to the higher row, missing rows of the last slab scored 0, a merge that drops a trailing
                    partial group, a slab's row offset lost.
  moe_route         ties to the higher expert, a top-k that reads 16 experts of 17.
  moe_router        logits not rounded to bf16 before the selection.
  moe_combine       weights rounded to bf16, inv read as [k, T].

Also: the integer oracles agree with fp64 matmul, every exact family's < 2^24 bound holds at the shapes the GPU
file runs, the planted ties are ties, and the three forms of the consensus (kernel contract, consensus_reference,
the CPU branch of ConsensusClient.build in score/multichat.py) agree for a sole candidate while the two CPU forms
are unchanged for n >= 2."""
import pytest
import torch

from tests import select_probes as sp
from tests.select_probes import RowCage, bitwise, rne


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 41)


# ---------------------------------------------------------------------------------------------------------
# pool_l2norm


def _walk_case(d, ncols=None, pad=0):
    cols = sp.pool_cols(d)
    if ncols is not None and ncols < len(cols):
        cols = list(dict.fromkeys([cols[0], cols[-1], 255, 256, d - 9] + cols[::max(1, len(cols) // ncols)]))
        cols = [c for c in cols if 0 <= c < d and c != sp.FIXED_COL]
    x = sp.pool_walk(d, cols)
    cu = torch.arange(len(cols) + 1, dtype=torch.int32)
    return sp.framed(x, pad), cu, sp.pool_want(x, cu, 2), torch.tensor(cols)


@pytest.mark.parametrize("d", sp.POOL_WALK_DS)
def test_pool_walk_accepts_fp32_and_has_two_spikes(d):
    view, cu, want, _ = _walk_case(d, 48)
    assert bool(((want != 0).sum(1) == 2).all()) and bool((want[want != 0].abs() - 0.5 ** 0.5).abs().max() < 1e-15)
    for pad in (0, 8):
        view, cu, want, _ = _walk_case(d, 48, pad)
        of, ob = sp.pool_emul(view, cu, 2)
        assert not sp.pool_violations(of, ob, want)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("d", [8, 264])
def test_pool_seqs_accept_fp32_and_reject_the_mutants(d, mode):
    h, cu = sp.pool_seqs(d, _gen(d))
    want = sp.pool_want(h, cu, mode)
    assert bool((want[2] == 0).all()) and bool((want[-1] == 0).all())       # zero length, zero row
    for pad in (0, 8):
        of, ob = sp.pool_emul(sp.framed(h, pad), cu, mode)
        assert not sp.pool_violations(of, ob, want), (pad, mode)
    view = sp.framed(h, 8)
    mutants = {0: [dict(ignore_stride=True)],
               1: [dict(hi=-1), dict(hi=1), dict(lo=1), dict(lo=-1), dict(ignore_stride=True)],
               2: [dict(last=0), dict(ignore_stride=True)]}[mode]
    for m in mutants + [dict(zero_nan=True)]:
        of, ob = sp.pool_emul(view, cu, mode, **m)
        assert sp.pool_violations(of, None, want), m          # the fp32 check alone
        assert sp.pool_violations(want.float(), ob, want), m  # the bf16 check alone


@pytest.mark.parametrize("d", [264, 1000, 4096])
def test_pool_walk_rejects_a_dropped_column_trip(d):
    view, cu, want, cols = _walk_case(d, 48)
    of, ob = sp.pool_emul(view, cu, 2, drop_chunk=True)
    bad = (of.double() - want).abs().amax(1) > 0.2          # 2^-1/2 became 1 in every row that walks the last trip
    last = cols >= (d - 1) // 256 * 256
    assert int(last.sum()) >= 2 and torch.equal(bad, last) and sp.pool_violations(of, ob, want)
    of, _ = sp.pool_emul(sp.framed(sp.pool_walk(d, sp.pool_cols(d)[:8]), 8), cu[:9], 2, ignore_stride=True)
    assert sp.pool_violations(of, None, want[:8])


# ---------------------------------------------------------------------------------------------------------
# cosine_consensus


CONS_SMALL = [(R, n, d) for R in sp.CONS_RS for n in sp.CONS_NS for d in sp.CONS_DS]


@pytest.mark.parametrize("scaled", [False, True])
def test_consensus_exact_bounds_oracle_and_ties(scaled):
    for R, n, d in CONS_SMALL + [sp.CONS_BIG]:
        assert 256 * n * d < 2 ** 24
        if n * d > 33 * 96 and (R, n, d) != sp.CONS_BIG and R > 1:
            continue
        E = sp.plant_tie(sp.sign_rows(R, n, d, _gen(R, n, d), scaled))
        G = sp.gram(E)
        assert torch.equal(G, E.double() @ E.double().transpose(1, 2))
        assert float(G.abs().max()) * 16 < 2 ** 24 and bool((G.float().double() == G).all())
        c = sp.cen_exact(G)
        if n >= 2:
            assert bool(((c == c.max(-1, keepdim=True).values).sum(-1) >= 2).all()), (R, n, d)
        if R > 1:
            assert not torch.equal(E[0], E[1])
        S, cen, w, best = sp.consensus_emul(E, 0.05)
        assert not sp.consensus_exact_violations(S, cen, best, E), (R, n, d)


@pytest.mark.parametrize("n", [2, 15, 17, 33])
def test_consensus_exact_rejects_the_mutants(n):
    R, d = 3, 96
    E = sp.plant_tie(sp.sign_rows(R, n, d, _gen(n), scaled=True))
    muts = [dict(keep_diag=True), dict(div_n=True), dict(tie_high=True), dict(skip_cols=32)]
    if n >= 32:
        muts.append(dict(transpose_tile=True))
    for m in muts:
        S, cen, w, best = sp.consensus_emul(E, 0.05, **m)
        assert sp.consensus_exact_violations(S, cen, best, E), m
    S, cen, w, best = sp.consensus_emul(sp.sign_rows(1, n, 32, _gen(n, 1)), 0.05, skip_cols=32)
    assert sp.consensus_exact_violations(S, cen, best, sp.sign_rows(1, n, 32, _gen(n, 1)))


@pytest.mark.parametrize("clustered", [False, True])
@pytest.mark.parametrize("tau", [0.05, 0.001])
@pytest.mark.parametrize("n,d", [(2, 384), (5, 4096), (20, 384)])
def test_consensus_random_accepts_fp32_and_rejects_the_mutants(n, d, tau, clustered):
    E = sp.unit_rows(2, n, d, _gen(n, d), clustered)
    S, cen, w, best = sp.consensus_emul(E, tau)
    assert not sp.consensus_random_violations(S, cen, w, best, E, tau)
    for m in (dict(keep_diag=True), dict(div_n=True), dict(skip_cols=32)):
        assert sp.consensus_random_violations(*sp.consensus_emul(E, tau, **m), E, tau), m
    if clustered and tau == 0.001:
        assert float(cen.max()) / tau > 120          # exp overflows in fp32 unless the maximum is subtracted
        S2, cen2, w2, best2 = sp.consensus_emul(E, tau, no_max=True)
        assert sp.consensus_random_violations(S2, cen2, w2, best2, E, tau)
    # the weights check has teeth of its own: one weight moved by 4 W_ERR
    x = cen.double() * sp.inv_tau32(tau)
    w3 = torch.softmax(x, -1)
    assert not sp.softmax_violations(w3.float(), x, 1.01 / tau)
    w3[:, 0] *= 1 + 4 * sp.W_ERR(1.01 / tau)
    assert sp.softmax_violations(w3, x, 1.01 / tau)


def _completion(n):
    from llm_weighted_consensus_amd.schema import chat as C
    return C.ChatCompletion(id="chatcmpl-1", created=1, model="m", choices=[
        C.UnaryChoice(message=C.UnaryMessage(content=f"a{i}"), finish_reason="stop", index=i) for i in range(n)])


def test_a_sole_candidate_has_centrality_one_in_all_three_forms():
    from llm_weighted_consensus_amd.embeddings.consensus import consensus_reference
    from llm_weighted_consensus_amd.score.multichat import ConsensusClient

    E = sp.unit_rows(2, 1, 384, _gen(1))
    S, cen, w, best = sp.consensus_emul(E, 0.05)                    # the kernel's contract
    ref = consensus_reference(E, 0.05)
    assert cen.tolist() == ref.centrality.tolist() == [[1.0], [1.0]]
    assert w.tolist() == ref.weights.tolist() == [[1.0], [1.0]] and best.tolist() == ref.best == [0, 0]
    out = ConsensusClient.build(_completion(1), E[0].float(), 3, "emb", 0.05)
    assert out.choices[0].weight == 1.0 and out.choices[0].confidence == 1.0


@pytest.mark.parametrize("n", [2, 5, 20])
def test_the_cpu_forms_are_unchanged_for_two_or_more(n):
    from llm_weighted_consensus_amd.embeddings.consensus import consensus_reference
    from llm_weighted_consensus_amd.score.multichat import ConsensusClient

    tau = 0.05
    E = sp.unit_rows(3, n, 384, _gen(n, 7), clustered=True)
    Ef = E.float()
    S = Ef @ Ef.transpose(1, 2)
    cen = (S.sum(-1) - S.diagonal(dim1=1, dim2=2)) / max(1, n - 1)          # the forms as they were
    ref = consensus_reference(E, tau)
    assert torch.equal(ref.centrality, cen) and torch.equal(ref.weights, torch.softmax(cen / tau, -1))
    assert ref.best == cen.argmax(-1).tolist() and torch.equal(ref.similarity, S)
    E0 = Ef[0]
    Sm = E0 @ E0.t()
    c0 = (Sm.sum(1) - Sm.diagonal()) / max(1, n - 1)
    out = ConsensusClient.build(_completion(n), E0, 3, "emb", tau)
    assert [c.weight for c in out.choices] == c0.tolist()
    assert [c.confidence for c in out.choices] == torch.softmax(c0 / tau, 0).tolist()


# ---------------------------------------------------------------------------------------------------------
# knn_topk


KNN_CPU = [s for s in sp.KNN_SHAPES if s[0] <= 16385]


@pytest.mark.parametrize("n,k", sp.KNN_SHAPES)
def test_knn_families_are_exact_and_the_structure_emulation_passes(n, k):
    for d in sp.knn_d(n)[:2]:
        for fam in sp.knn_families(n, k) + (["wide"] if d == 64 else []):
            E, q = sp.knn_case(fam, n, d, k, _gen(n, k, d))
            sc = sp.knn_scores(E, q)
            assert int(sc.abs().max()) < 2 ** 24 and torch.equal(sc.double(), E.double() @ q.double())
            if fam == "negative":
                assert int(sc.max()) < 0
            if fam in ("slab_tie", "group_tie"):
                lo = 250 if fam == "slab_tie" else sp.group_boundary(k) - k
                blk = sc[lo:min(n, lo + 2 * k)]
                assert bool((blk == sc.max()).all()) and blk.numel() >= 2
            if n <= 70000:
                v, r = sp.knn_emul(E, q, k)
                assert not sp.knn_violations(v, r, E, q, k), (fam, d)


def test_knn_three_merge_levels_at_the_largest_shape():
    n, k = sp.KNN_SHAPES[8]
    slabs = -(-n // 256)
    l2 = -(-slabs // (4096 // k))
    l3 = -(-l2 // (4096 // k))
    assert slabs > 4096 and l2 > 1 and l3 > 1 and -(-l3 // (4096 // k)) == 1     # 4097 -> 65 -> 2 -> 1 lists
    assert -(-16385 // 256) == 65 and 65 % 64 == 1           # (16385, 64): the second merging block gets one list


def test_knn_rejects_the_mutants():
    def rejected(n, k, d, fam, **m):
        E, q = sp.knn_case(fam, n, d, k, _gen(n, k, d, 3))
        v, r = sp.knn_emul(E, q, k, **m)
        return bool(sp.knn_violations(v, r, E, q, k))

    for n, k in [(64, 64), (255, 7), (257, 64), (300, 33), (513, 3)]:
        assert rejected(n, k, 4, "equal", tie_high=True), (n, k)
    assert rejected(513, 3, 64, "slab_tie", tie_high=True) and rejected(16385, 64, 4, "group_tie", tie_high=True)
    for n, k in [(255, 7), (257, 64), (300, 33), (513, 3)]:
        assert rejected(n, k, 64, "negative", missing_zero=True), (n, k)
    assert rejected(16385, 64, 4, "integers", drop_partial_group=True)
    for n, k in [(257, 64), (300, 33), (513, 3), (16385, 64)]:
        assert rejected(n, k, 4, "integers", lose_offset=True), (n, k)


# ---------------------------------------------------------------------------------------------------------
# moe_route / moe_router


@pytest.mark.parametrize("T,E,k", sp.ROUTE_SHAPES)
def test_route_logits_tie_and_the_mutants_are_rejected(T, E, k):
    lg = sp.route_logits(T, E, k, _gen(T, E, k))
    lf = lg.float()
    assert bool((lf[torch.isfinite(lf)].abs() <= 2).all()) and bool(((lf * 2) == (lf * 2).round())[torch.isfinite(lf)].all())
    s, _ = lf.sort(1, descending=True)
    if k < E:
        tied = s[:, k - 1] == s[:, k]                              # every row but the two special ones ties there
        assert bool(tied[[t for t in range(T) if t not in (1, T - 1)]].all())
        assert bool((torch.isfinite(lf).sum(1) >= k).all())
    if T > 1 and E > k:
        assert bool(torch.isinf(lf[T - 1, 0])) and bool((lf[(T - 1) // 2] == 0.5).all())
    ids, w, ro = sp.route_emul(lg, k)
    assert not sp.route_violations(ids, w, ro, lg, k, 2.0)
    if E > 1:
        ids, w, ro = sp.route_emul(lg, k, tie_high=True)
        assert sp.route_violations(ids, w, ro, lg, k, 2.0)
    if E == 17:
        ids, w, ro = sp.route_emul(lg, k, e_read=16)
        assert sp.route_violations(ids, w, ro, lg, k, 2.0)
    w2 = w.clone()
    w2[0, 0] *= 1 + 4 * sp.W_ERR(2.0)
    assert sp.route_violations(sp.route_emul(lg, k)[0], w2, sp.route_emul(lg, k)[2], lg, k, 2.0)


def _router_violations(ids, lg, want_lg, k):
    out = []
    if bool(bitwise(lg, want_lg).any()):
        out.append("logits")
    if not torch.equal(ids.long(), sp.stable_topk(lg.float(), k)[1]):
        out.append("ids")
    return out


@pytest.mark.parametrize("d", sp.ROUTER_DS)
def test_router_families_are_exact_and_unrounded_selection_is_rejected(d):
    assert 64 * d < 2 ** 24
    seen = 0
    for E, k in sp.ROUTER_EK:
        for scaled in (False, True):
            h, r = sp.router_sign(130, E, d, _gen(d, E, k), scaled)
            acc = h.double() @ r.double().t()
            assert bool((acc.float().double() == acc).all()) and float(acc.abs().max()) * 8 < 2 ** 24
            ids, w, ro, lg = sp.router_emul(h, r, k)
            assert not _router_violations(ids, lg, sp.router_want(h, r), k)
            seen += bool(_router_violations(sp.router_emul(h, r, k, round_first=False)[0], lg, sp.router_want(h, r), k))
        h, r = sp.router_onehot(d, sp.router_chunks(d), E, _gen(d, E))
        assert bool(((h != 0).sum(1) == 1).all()) and sorted(set((h != 0).nonzero()[:, 1].tolist())) == \
            [8 * c + c % 8 for c in range(d // 8)]
        prod = h.double() @ r.double().t()
        assert bool((prod.float().double() == prod).all())              # the 16-bit products are exact in fp32
        ids, w, ro, lg = sp.router_emul(h, r, k)
        assert not _router_violations(ids, lg, sp.router_want(h, r), k)
        seen += bool(_router_violations(sp.router_emul(h, r, k, round_first=False)[0], lg, sp.router_want(h, r), k))
    assert seen >= 1 or d <= 256, "no family at this width sees a selection made on the unrounded sums"


def test_router_chunks_cover_the_edges():
    for d in sp.ROUTER_DS:
        for T in sp.ROUTER_TS:
            ch = sp.router_chunks(d, T)
            assert len(ch) == T and ch[0] == d // 8 - 1 and max(ch) < d // 8
        if d // 8 > 256:
            assert {0, 255, 256, d // 8 - 1} <= set(sp.router_chunks(d, 130))


# ---------------------------------------------------------------------------------------------------------
# moe_combine


def _combine_case(kind, T, k, d):
    gen = _gen(T, k, d)
    ids, _, _ = sp.route_emul(sp.route_logits(T, 8, k, gen), k)
    _, _, inv = sp.permute_ref(ids, 8)
    Y, w = sp.combine_inputs(kind, T, k, d, gen, rows=T * k + 8)
    sp.bits(Y)[T * k:] = sp.SENTINEL
    return Y, w, inv


def _accepts(out, want, mag, kind):
    cage = RowCage(out.shape)
    cage.load(out)
    return not sp.combine_violations(cage, want, mag, kind)


@pytest.mark.parametrize("T", sp.COMBINE_TS)
@pytest.mark.parametrize("k", sp.COMBINE_KS)
@pytest.mark.parametrize("kind", ["exact", "fine", "onehot", "random"])
def test_combine_accepts_fp32_and_rejects_the_mutants(kind, T, k):
    d = 264
    Y, w, inv = _combine_case(kind, T, k, d)
    want, mag = sp.combine_want(Y, inv, w, k)
    if kind in ("exact", "fine"):
        unit = 0.25 if kind == "exact" else 2.0 ** -10
        assert float(mag.max()) / unit < 2 ** 24 and bool(((want / unit) == (want / unit).round()).all())
    if kind == "onehot":
        assert bool((bitwise(rne(want), Y[inv[torch.arange(T) * k + w.argmax(1)]]) == 0).all())
    assert _accepts(sp.combine_emul(Y, inv, w, k), want, mag, kind)
    if k > 1 and T > 1:
        assert not _accepts(sp.combine_emul(Y, inv, w, k, transposed=True), want, mag, kind)
    if kind == "fine" and T * k >= 5:
        assert not _accepts(sp.combine_emul(Y, inv, w, k, w_bf16=True), want, mag, kind)
    if kind == "exact":   # what {1, 0.5, 0.25, 0} cannot see
        assert _accepts(sp.combine_emul(Y, inv, w, k, w_bf16=True), want, mag, kind)
    out = sp.combine_emul(Y, inv, w, k)
    out[0, 0] = float("nan")
    assert not _accepts(out, want, mag, kind)


def test_combine_random_cancels_beyond_plain_one_step():
    """Why the random family is held to one_step_cond: an honest unfused fp32 sum is many codes from the fp64 sum
    at an output whose terms cancel (error <= 9 * 2^-24 of sum |w y|, not of the result), and only there."""
    from tests.rowwise_probes import well_conditioned

    T, k, d = 300, 8, 2056
    Y, w, inv = _combine_case("random", T, k, d)
    want, mag = sp.combine_want(Y, inv, w, k)
    out = sp.combine_emul(Y, inv, w, k)
    plain = sp.one_step(out, want)
    well = well_conditioned(want, mag, sp.COMBINE_ERR)
    assert int(plain.sum()) >= 1 and not bool((plain & well).any()) and float((~well).double().mean()) < 0.01
    assert bool(((out.double() - want).abs() <= 9 * 2.0 ** -24 * mag + rne(want).double().abs() * 2.0 ** -7)[~well].all())
    assert _accepts(out, want, mag, "random")
