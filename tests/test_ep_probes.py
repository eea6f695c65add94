"""What the comparisons of tests/test_ep_probes_gpu.py accept and reject, shown on the CPU: the emulations of the four
exchange kernels in tests/ep_probes.py pass every case against the oracle, and each of these mutants is rejected by
the named case:

  ep_unpack   rows ordered rank-major                    w2e4-full (two sources, rows for several local experts)
              counts summed in int32                     poison int32_wrap
              negative counts not treated as bad         poison minus_one
              scale read from the slot's last 4 bytes    w4e8-fp8-idle (RB = 4128: scale at 4112, last 4 at 4124)
  ep_pack     src ignored                                w2e4-full
              header counts shifted by one expert        w2e4-full
  ep_back     unused slots left unwritten                w2e4-fp8 (C = max R + 3: every chunk has unused slots)
  ep_combine  chunk base from row_off[e]                 w2e4-long-rows
              weights through bf16                       the ``fine`` family

The oracle's count handling is cross-checked against ExpertParallel._expert_major / _sane_counts, and the poisoned
headers are first run through the emulation WITHOUT sanitising: every index it forms stays inside the padded cages."""
import re

import pytest
import torch

from tests import ep_probes as ep
from tests.ep_probes import BF, CASES, F32, I32, U8, Case, bits, bitwise

NAMES = [c.name for c in CASES]


@pytest.fixture(scope="module")
def solved():
    """Inputs and oracle buffers of every case, computed once and left unchanged."""
    return {c.name: ep.oracle(c, ep.inputs(c)) for c in CASES}


def _sentinel_bytes(shape):
    return torch.full(shape, 0x7F, dtype=U8)


def _pack(c: Case, rk, **mut):
    send = _sentinel_bytes((c.W, (c.C + 1) * c.RB))
    ep.emul_pack(rk.x, rk.xs, rk.src, rk.row_off, c.W, c.El, c.C, c.RB, send, **mut)
    return send


def _unpack(c: Case, recv, **mut):
    W, C = c.W, c.C
    x = _sentinel_bytes((W * C, c.row_bytes))
    s = torch.zeros(W * C, dtype=F32)
    s.view(I32).fill_(ep.SENT32)
    m = torch.full((W * C,), ep.SENT32, dtype=I32)
    rol = torch.full((c.El + 1,), ep.SENT32, dtype=I32)
    ep.emul_unpack(recv, W, c.El, C, c.RB, c.row_bytes, c.fp8, x, s, m, rol, **mut)
    return x, s, m, rol


def _unpack_ok(c, o, got, r=0) -> bool:
    """The comparisons of the GPU test (the same message helpers) on an emulated unpack."""
    x, s, m, rol = got
    n = int(o["n"])
    x = x if c.fp8 else x.view(BF)
    msgs = [ep.ints_message("ep_unpack", r, "row_off_local", rol, o["row_off_local"]),
            ep.ints_message("ep_unpack", r, "map", m, o["map"], c.C),
            ep.rows_message("ep_unpack", r, x, o["x_local"], n, o, c.C),
            ep.ints_message("ep_unpack", r, "s_local", s[:n], o["s_local"][:n]) if c.fp8 else None]
    assert all(msg is None or f"ep_unpack rank {r}" in msg for msg in msgs)
    return all(msg is None for msg in msgs)


def _back(c, o, **mut):
    back = torch.empty(c.W * c.C, c.d_out, dtype=BF)
    bits(back).fill_(ep.SENTINEL)
    ep.emul_back(o["y_local"], o["map"], c.W, c.C, back, **mut)
    return back


def _stage_results(c: Case, ranks, pack={}, unpack={}, back={}, combine={}):
    """Which stages of the emulated chain agree with the oracle, each stage fed the oracle's input."""
    ok = dict(pack=True, unpack=True, back=True, combine=True)
    for r, rk in enumerate(ranks):
        o = rk.o
        send = _pack(c, rk, **pack)
        ok["pack"] &= ep.first_byte("ep_pack", r, send, o["send"], o["send_mask"], c.C + 1, c.RB, True) is None
        recv = ep.fill_unspecified_send(o["recv"].clone(), o["recv_mask"], c.fp8)
        ok["unpack"] &= _unpack_ok(c, o, _unpack(c, recv, **unpack), r)
        ok["back"] &= ep.first_byte("ep_back", r, _back(c, o, **back), o["back"], None, c.C, 2 * c.d_out, False) is None
        out = ep.emul_combine(o["ret"], rk.row_off, rk.inv, rk.w, c.El, c.C, c.k, **combine)
        ok["combine"] &= not bool(bitwise(out, o["out"]).any())
    return ok


def test_the_cases_cover_what_the_suite_never_ran():
    assert {(c.W, c.El) for c in CASES} == {(1, 1), (1, 64), (2, 4), (3, 2), (4, 8), (8, 1), (8, 8)}
    assert {c.k for c in CASES} == {1, 2, 8}
    assert {c.d for c in CASES if not c.fp8} == {8, 264, 2056} and {c.d for c in CASES if c.fp8} == {16, 4112}
    assert {c.cap for c in CASES} == {"full", "plus3", "one"}
    assert {c.routing for c in CASES} >= {"random", "single", "starved", "holes", "idle", "one"}
    assert all(c.d_out in (c.d, 264) for c in CASES) and any(c.d_out != c.d for c in CASES)
    assert any(0 in c.T and sum(c.T) > 1 for c in CASES)
    assert ep.CASE["w1e64-header-slot"].RB == 256 and ep.CASE["w4e8-fp8-idle"].RB == 4128
    assert any((c.W, c.El, c.k) == (8, 8, 8) for c in CASES)
    for c in CASES:
        assert c.W * c.El <= 64 and c.RB % 16 == 0 and c.row_bytes % 16 == 0 and c.C >= max(t * c.k for t in c.T)


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_what_the_docstring_says(solved, name):
    c, ranks = ep.CASE[name], solved[name]
    rows = torch.cat([rk.x.contiguous().view(U8).view(rk.x.shape[0], c.row_bytes) for rk in ranks])
    assert torch.unique(rows, dim=0).shape[0] == rows.shape[0], "token rows are not distinct across ranks"
    if c.fp8:
        s = torch.cat([rk.xs for rk in ranks])
        assert torch.unique(s).numel() == s.numel() and bool((s > 0).all())
    else:
        v = torch.cat([rk.x for rk in ranks]).float()
        assert bool(torch.isfinite(v * 4).all()) and bool(((v * 0.25).to(BF).float() * 4 == v).all())
    cnt = torch.stack([rk.row_off[1:] - rk.row_off[:-1] for rk in ranks])          # [source, expert]
    per_dest = cnt.view(c.W, c.W, c.El).sum(2)
    for rk in ranks:
        T = rk.x.shape[0]
        assert torch.equal(rk.inv.long().sort().values, torch.arange(T * c.k))
        if T * c.k > 1 and c.routing != "router":
            assert not torch.equal(rk.src.long(), torch.arange(T * c.k)), "src is the identity"
        if T:
            assert torch.equal(torch.bincount(rk.src.long(), minlength=T), torch.full((T,), c.k))
    if c.cap == "full":
        assert int(per_dest.max()) == c.C, "no chunk is exactly full"
    if c.cap == "one":
        assert int(cnt.sum()) == 1 and c.C == 1
    if c.routing == "single":
        assert int((cnt[0] > 0).sum()) == 1
    if c.routing == "starved":
        assert int(per_dest[:, -1].sum()) == 0
    if c.routing == "holes":
        holes = [r * c.El + e for r in range(c.W) for e in ep.hole_experts(c.El)]
        assert int(cnt[:, holes].sum()) == 0 and int(cnt.sum()) > 0


@pytest.mark.parametrize("name", NAMES)
def test_the_emulation_passes_every_case(solved, name):
    c = ep.CASE[name]
    assert _stage_results(c, solved[name]) == dict(pack=True, unpack=True, back=True, combine=True)


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_agrees_with_the_model_glue(solved, name):
    """Positions and segments against ExpertParallel._expert_major / _sane_counts on the same count tables, and the
    final output against the rows' own expert outputs (no exchange at all)."""
    from llm_weighted_consensus_amd.parallel.expert import ExpertParallel

    c, ranks = ep.CASE[name], solved[name]
    glue = ExpertParallel.__new__(ExpertParallel)
    glue.W, glue.El = c.W, c.El
    for r, rk in enumerate(ranks):
        rcnt = torch.tensor(ep.header_counts(rk.o["recv"], c.W, c.El, c.C, c.RB), dtype=torch.int64)
        dest, valid, rol = glue._expert_major(ExpertParallel._sane_counts(rcnt, c.C), c.C)
        assert torch.equal(rol, rk.o["row_off_local"])
        assert torch.equal(torch.where(valid, dest, -1).to(I32), rk.o["map"])
        Y = ep.sorted_expert_outputs(c, rk)
        want, _ = ep.combine_want(Y, rk.inv, rk.w, c.k) if rk.w.shape[0] else (torch.zeros(0, c.d_out), None)
        assert not bool(bitwise(ep.rne(rk.o["out"]), want).any()), f"rank {r}: out differs from the direct computation"


def test_the_routed_case_with_the_permutation_of_select_probes():
    """ep_probes.CHAIN on the CPU: logits -> route_emul / permute_ref of tests/select_probes.py -> the exchange;
    the emulated output equals combine_emul of the rows' own expert outputs (the same unfused fp32 sum)."""
    from tests import select_probes as sp

    c = ep.CHAIN
    routed = [sp.route_emul(sp.route_logits(T, c.E, c.k, torch.Generator().manual_seed(5 + r)), c.k)
              for r, T in enumerate(c.T)]
    ranks = ep.inputs(c, ids=[ids.long() for ids, _, _ in routed])
    for rk, (ids, w, _) in zip(ranks, routed):
        rk.row_off, rk.src, rk.inv = (t.to(I32) for t in sp.permute_ref(ids.long(), c.E))
        rk.w = w.float()
    ok = _stage_results(c, ep.oracle(c, ranks))
    assert ok["pack"] and ok["unpack"] and ok["back"]
    for rk in ranks:
        out = ep.emul_combine(rk.o["ret"], rk.row_off, rk.inv, rk.w, c.El, c.C, c.k)
        want = sp.combine_emul(ep.sorted_expert_outputs(c, rk), rk.inv, rk.w, c.k)
        assert not bool(bitwise(out, want).any())
        assert not bool(ep.one_step_cond(out, rk.o["out"], rk.o["mag"], ep.COMBINE_ERR)[0].any())


def test_a_failure_names_kernel_rank_chunk_slot_and_byte(solved):
    c = ep.CASE["w2e4-full"]
    rk = solved[c.name][0]
    o, geo = rk.o, (c.C + 1, c.RB, True)
    msg = ep.first_byte("ep_pack", 0, _pack(c, rk, ignore_src=True), o["send"], o["send_mask"], *geo)
    assert re.match(r"ep_pack rank 0: \d+ bytes differ, first at chunk 1 slot [1-9]\d* byte \d+: got 0x", msg), msg
    msg = ep.first_byte("ep_pack", 0, _pack(c, rk, shift_header=True), o["send"], o["send_mask"], *geo)
    assert "slot 0 (header)" in msg, msg


MUTANTS = [
    ("unpack", dict(rank_major=True), "w2e4-full"),
    ("unpack", dict(scale_at_end=True), "w4e8-fp8-idle"),
    ("pack", dict(ignore_src=True), "w2e4-full"),
    ("pack", dict(shift_header=True), "w2e4-full"),
    ("back", dict(skip_unused=True), "w2e4-fp8"),
    ("combine", dict(base_from_expert=True), "w2e4-long-rows"),
]


@pytest.mark.parametrize("stage,mut,name", MUTANTS, ids=[f"{s}-{next(iter(m))}" for s, m, _ in MUTANTS])
def test_each_mutant_is_rejected_by_its_named_case(solved, stage, mut, name):
    c = ep.CASE[name]
    ok = _stage_results(c, solved[name], **{stage: mut})
    assert ok == {s: s != stage for s in ok}, f"{mut} on {name}: {ok}"


@pytest.mark.parametrize("name", ep.COMBINE_CASES)
def test_combine_families_bounds_and_the_bf16_weight_mutant(solved, name):
    c, ranks = ep.CASE[name], solved[name]
    assert 64 * c.k < (1 << 24) and (1 << 14) * c.k < (1 << 24)
    fine_rejected = False
    for r, rk in enumerate(ranks):
        T, R = rk.x.shape[0], rk.src.numel()
        if T == 0:
            continue
        for kind in ("exact", "fine", "onehot", "random"):
            Y, w = ep.combine_inputs(kind, T, c.k, c.d_out, ep._gen(c), rows=R)
            ret = ep.ret_from_sorted(Y, rk.row_off, c.W, c.El, c.C)
            want, mag = ep.combine_want(Y, rk.inv, w, c.k)
            own, _ = ep.oracle_combine(ret, rk.row_off, rk.inv, w, c.El, c.C, c.k)
            assert torch.equal(own, want), "the two references disagree"

            def accepted(out):
                if kind == "random":
                    return not bool(ep.one_step_cond(out, want, mag, ep.COMBINE_ERR)[0].any())
                return not bool(bitwise(out, want).any())

            assert accepted(ep.emul_combine(ret, rk.row_off, rk.inv, w, c.El, c.C, c.k))
            if kind == "fine":
                fine_rejected |= not accepted(ep.emul_combine(ret, rk.row_off, rk.inv, w, c.El, c.C, c.k, w_bf16=True))
    assert fine_rejected or name == "w4e8-fp8-one", "the fine family did not show weights that went through bf16"


def test_combine_random_share_over_every_shape(solved):
    """At least 95 % of the random family's outputs are well conditioned, over all outputs of each shape's ranks."""
    for name in ep.COMBINE_CASES:
        c, well, total = ep.CASE[name], 0.0, 0
        for rk in solved[name]:
            T = rk.x.shape[0]
            if T == 0:
                continue
            Y, w = ep.combine_inputs("random", T, c.k, c.d_out, ep._gen(c), rows=rk.src.numel())
            want, mag = ep.combine_want(Y, rk.inv, w, c.k)
            well += float(ep.one_step_cond(ep.rne(want), want, mag, ep.COMBINE_ERR)[1]) * want.numel()
            total += want.numel()
        assert well / total >= 0.95, f"{name}: {well / total:.4f}"


# ---------------------------------------------------------------------------------------------------------
# poisoned headers


@pytest.mark.parametrize("geo", ep.POISON_GEOS, ids=lambda g: f"w{g[0]}e{g[1]}d{g[2]}{'fp8' if g[3] else 'bf16'}")
@pytest.mark.parametrize("kind", ep.POISONS)
def test_poisoned_headers(kind, geo):
    W, El, d, fp8 = geo
    recv, C, RB, rb, bad = ep.poisoned_recv(W, El, d, fp8, kind)
    c = Case("poison", W, El, 1, d, fp8, d, "plus3", "random", (C - 3,) * W)
    assert (c.C, c.RB, c.row_bytes) == (C, RB, rb)
    o = ep.oracle_unpack(recv, W, El, C, RB, rb, fp8)
    # the poisoned source is absent, the others are where a clean exchange without it puts them
    assert bool((o["map"][bad * C:(bad + 1) * C] == -1).all())
    clean = recv.clone().view(W, C + 1, RB)
    clean[bad, 0] = 0
    oc = ep.oracle_unpack(clean.view(W, -1), W, El, C, RB, rb, fp8)
    assert all(torch.equal(o[key], oc[key]) for key in o) and int(o["n"]) > 0
    raw = torch.tensor(ep.header_counts(recv, W, El, C, RB), dtype=torch.int64)
    from llm_weighted_consensus_amd.parallel.expert import ExpertParallel
    sane = ExpertParallel._sane_counts(raw, C)
    assert sane.tolist() == ep.sane(raw.tolist(), C) and int(sane[bad].sum()) == 0 and int(sane.sum()) == int(o["n"])
    glue = ExpertParallel.__new__(ExpertParallel)
    glue.W, glue.El = W, El
    dest, valid, rol = glue._expert_major(sane, C)
    assert torch.equal(rol, o["row_off_local"]) and torch.equal(torch.where(valid, dest, -1).to(I32), o["map"])
    # the guard is exercised, not relied on: without it every index stays inside the padded cages
    pad, trace = ep.poison_pad(W, El, C), []
    assert pad >= C + W * El
    _unpack(c, recv, sanitise=False, trace=trace)
    assert trace and all(-pad <= row < W * C + pad for _, row in trace), \
        f"unsanitised indices leave the cages: {[t for t in trace if not -pad <= t[1] < W * C + pad][:4]}"
    assert _unpack_ok(c, o, _unpack(c, recv))
    # the mutants
    if kind == "int32_wrap":
        assert not _unpack_ok(c, o, _unpack(c, recv, int32_sum=True))
    if kind == "minus_one":
        assert not _unpack_ok(c, o, _unpack(c, recv, allow_negative=True))
    back = torch.empty(W * C, 8, dtype=BF)
    bits(back).fill_(ep.SENTINEL)
    y = ep.distinct((W * C, 8))
    ep.emul_back(y, o["map"], W, C, back)
    assert bool((bits(back)[bad * C:(bad + 1) * C] == 0).all())
