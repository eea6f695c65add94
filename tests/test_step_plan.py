"""The decode step plan (models/step_plan.py), on the CPU, over the whole space of chain plans: what parses,
that every move gives a plan that parses and changes the step, that the summary depends on the live view only,
and that the kernel sequence LlamaModel._chain_layers runs never lets a row-scaled GEMM read partials that
nobody wrote for the rows it reads."""
import itertools

import pytest
import torch

from llm_weighted_consensus_amd.models import llama, step_plan
from llm_weighted_consensus_amd.models.step_plan import ChainPlan
from tests.op_recorder import Recorder

PRODUCERS = ("plain", "own32", "own64", "sumsq")
KEYS = ("attn", "mlp", "final", "qkv_bn", "qkv_var", "gu_var", "lm_var", "lm_split", "o", "down")
SPACE = [dict(zip(KEYS, v)) for v in itertools.product(
    (False, True), (False, True), (False, True), (192, 256), (32, 64), (32, 64), (32, 64), (False, True),
    PRODUCERS, PRODUCERS)]
# chain timings as tests/test_engine_plan.py records them: the own epilogues timed, the plain GEMMs not
TIMINGS = {"gu_rsv32": 660.0, "gu_rsv64": 650.0, "lm_rsv32": 3000.0, "lm_rsv64": 2990.0, "o_own32": 110.0,
           "o_own64": 101.0, "down_own32": 330.0, "down_own64": 320.0}
OWN = {n: "g4p" for n in step_plan.PROJECTIONS}


def _well_formed(d: dict) -> bool:
    return not (d["mlp"] and d["o"] == "plain") and not ((d["attn"] or d["final"]) and d["down"] == "plain")


@pytest.fixture(scope="module")
def accepted():
    return [d for d in SPACE if _well_formed(d)]


def test_from_dict_accepts_exactly_the_plans_whose_live_producers_exist(accepted):
    assert len(SPACE) == 4096 and len(accepted) == 2912
    for d in SPACE:
        if _well_formed(d):
            assert ChainPlan.from_dict(d).as_dict() == d  # dead entries kept verbatim
        else:
            with pytest.raises(ValueError, match="o='plain'" if d["mlp"] and d["o"] == "plain" else "down='plain'"):
                ChainPlan.from_dict(d)


def test_from_dict_defaults_and_errors_name_the_key():
    assert ChainPlan.from_dict({}) == ChainPlan.UNFOLDED == ChainPlan.from_dict(ChainPlan.UNFOLDED.as_dict())
    assert ChainPlan.UNFOLDED.as_dict() == {"attn": False, "mlp": False, "final": False, "qkv_bn": 192, "qkv_var": 32,
                                            "gu_var": 32, "lm_var": 32, "lm_split": False, "o": "plain",
                                            "down": "plain"}
    assert list(ChainPlan.UNFOLDED.as_dict()) == list(KEYS)
    p = ChainPlan.from_dict({"attn": True, "mlp": False, "final": False, "qkv_bn": 256, "o": "sumsq", "down": "own64"})
    assert (p.qkv_var, p.gu_var, p.lm_var, p.lm_split) == (32, 32, 32, False)
    assert p.o == "sumsq" and p.live().o == "plain"  # a dead entry: kept, and without effect
    with pytest.raises(ValueError, match="qkv_vr"):
        ChainPlan.from_dict({"attn": False, "qkv_vr": 32})
    for key, bad in (("qkv_bn", 128), ("gu_var", 48), ("o", "own"), ("down", "sumsqr"), ("attn", "yes"),
                     ("lm_split", 2)):
        with pytest.raises(ValueError, match=key):
            ChainPlan.from_dict({key: bad})
    with pytest.raises(ValueError, match="kv"):
        step_plan.check_plan({"choices": {"kv": "blas"}, "chain": None})


def test_live_view_owned_and_producer_modes():
    p = ChainPlan(attn=True, final=False, mlp=False, qkv_bn=256, lm_var=64, lm_split=True, o="own32", down="own64")
    assert p.live() == ChainPlan(attn=True, qkv_bn=256, down="own64")
    assert p.owned() == {"qkv", "down"}
    assert (p.down_mode(last=False), p.down_mode(last=True)) == ("own64", "plain")
    q = ChainPlan(final=True, lm_var=32, lm_split=True, down="sumsq")
    assert not q.live().lm_split and q.owned() == {"lm"}  # the split tail exists at VAR 64 only
    assert (q.down_mode(last=False), q.down_mode(last=True)) == ("plain", "sumsq")
    assert ChainPlan(mlp=True, o="own64").owned() == {"gu", "o"}


def test_candidate_table_names_plan_entries():
    names = [c for cands in step_plan.CHAIN_CANDIDATES.values() for c in cands]
    assert len(names) == len(set(names)) == 13
    for proj, cands in step_plan.CHAIN_CANDIDATES.items():
        for entries in cands.values():
            ChainPlan(attn=True, mlp=True, final=True, **dict({"o": "sumsq", "down": "sumsq"}, **entries))
    assert step_plan.CHAIN_CANDIDATES["qkv"]["qkv_rs256v64"] == {"qkv_bn": 256, "qkv_var": 64}
    assert step_plan.CHAIN_CANDIDATES["lm"]["lm_rsv64s"] == {"lm_var": 64, "lm_split": True}
    assert step_plan.fastest_candidate("lm", {"lm_rsv32": 2.0, "lm_rsv64": 3.0, "lm_rsv64s": 2.0}) == "lm_rsv32"
    t = {"o": 100.0, "sumsq": 5.0, "o_own32": 106.0, "o_own64": 104.0}
    assert step_plan.cheapest_producer("o", t) == "own64"
    assert step_plan.cheapest_producer("o", dict(t, sumsq=3.0)) == "sumsq"
    assert step_plan.cheapest_producer("down", None) == step_plan.cheapest_producer("down", {}) == "sumsq"


def _moves(chain, choices, t):
    plan = {"choices": dict(choices), "chain": None if chain is None else dict(chain)}
    return plan, [(lb, step_plan.with_move(plan, dl)) for lb, dl in step_plan.step_moves(plan, OWN, True, t)]


@pytest.mark.parametrize("t", [TIMINGS, None], ids=["timed", "untimed"])
def test_every_move_parses_and_changes_the_step(accepted, t):
    blas = {n: "blas" for n in step_plan.PROJECTIONS}
    total = 0
    for d in accepted + [ChainPlan.UNFOLDED.as_dict()]:
        plan, moved = _moves(d, blas, t)
        live = ChainPlan.from_dict(d).live()
        assert len({lb for lb, _ in moved}) == len(moved)
        for lb, p in moved:
            new = ChainPlan.from_dict(p["chain"])  # (with_move has checked it too)
            assert new.live() != live or p["choices"] != plan["choices"], (d, lb)
        total += len(moved)
    assert total == 30336 + 8  # the 2912 plans' moves, and the unfolded plan's once more


def test_fold_moves_bring_their_producer():
    lib = {"choices": {n: "blas" for n in step_plan.PROJECTIONS}, "chain": ChainPlan.UNFOLDED.as_dict()}
    for t, want in ((TIMINGS, "own64"), (None, "sumsq")):
        mv = dict(step_plan.step_moves(lib, OWN, True, t))
        assert mv["attn_fold=True"]["chain"] == {"attn": True, "down": want}
        assert mv["mlp_fold=True"]["chain"] == {"mlp": True, "o": want}
        assert mv["final_fold=True"]["chain"] == {"final": True, "down": want}
    # a producer that is already set stays, also where it was dead
    chain = dict(lib["chain"], o="own32", down="sumsq")
    mv = dict(step_plan.step_moves(dict(lib, chain=chain), OWN, True, TIMINGS))
    assert mv["mlp_fold=True"]["chain"] == {"mlp": True} and mv["attn_fold=True"]["chain"] == {"attn": True}
    # no chain at this batch: backend moves only
    assert [lb for lb, _ in step_plan.step_moves(lib, OWN, False, TIMINGS)] == [f"{n}=g4p" for n in lib["choices"]]


def test_summary_depends_on_choices_and_live_view_only(accepted):
    backends = {"qkv": "g4n192", "o": "blas", "gu": "g4p", "down": "g8", "lm": "blas"}
    by_live = {}
    for d in accepted:
        p = ChainPlan.from_dict(d)
        s = step_plan.plan_summary(backends, p)
        assert by_live.setdefault(p.live(), s) == s
        assert list(s) == list(backends)
    assert len(set(map(str, by_live.values()))) == len(by_live)  # and it tells every two steps apart
    assert step_plan.plan_summary(backends, None) == backends
    s = step_plan.plan_summary(backends, ChainPlan(attn=True, final=True, qkv_bn=256, lm_var=64, lm_split=True,
                                                   o="own32", down="sumsq"))
    assert s == {"qkv": "g4 rs256 v32", "o": "blas", "gu": "g4p", "down": "g8+sumsq", "lm": "g4 rs v64 split-K tail"}


def test_pin_step_plan_rejects_a_bad_plan_at_once():
    m = llama.LlamaModel.__new__(llama.LlamaModel)
    m.pinned = {}
    good = {"choices": {"qkv": "g4n192", "o": "blas"},
            "chain": {"attn": True, "mlp": False, "final": False, "qkv_bn": 192, "o": "sumsq", "down": "sumsq"}}
    m.pin_step_plan(4096, good)
    assert m.pinned[4096] == good
    with pytest.raises(ValueError, match="down"):
        m.pin_step_plan(2048, dict(good, chain=dict(good["chain"], down="plain")))
    with pytest.raises(ValueError, match="qkv_bm"):
        m.pin_step_plan(2048, dict(good, chain=dict(good["chain"], qkv_bm=256)))
    assert list(m.pinned) == [4096]


def test_chain_layers_never_reads_stale_partials(accepted, monkeypatch):
    """Three layers (the first, an inner and the last differ).  Every row-scaled consumer (gemm4w with ``chain=``
    and no residual) must follow a producer of partials (rms_rowsumsq, or a residual gemm4w with ``chain=``) with
    no update of the residual stream in between."""
    x = torch.zeros(1, 1)
    log = []
    rec = Recorder(log, x)
    monkeypatch.setattr(llama, "ops", rec)
    monkeypatch.setattr(llama, "gemm_plan", rec)
    m = llama.LlamaModel.__new__(llama.LlamaModel)
    m.cfg = type("Cfg", (), {"heads": 1, "kv_heads": 1, "head_dim": 1, "hidden": 1, "rms_eps": 1e-5})()
    m.layers = [type("L", (), {"wqkv": x, "wo": x, "w_gate_up": x, "w_down": x, "gu_block": 32, "bqkv": None,
                               "q_norm": None, "k_norm": None})() for _ in range(3)]
    m.on_gpu, m.weight_format, m.moe = True, "bf16", False
    m.chain, m.g8_ws, m.final_norm, m.lm_head, m.cos, m.sin = object(), object(), x, x, x, x
    cache = type("Cache", (), {"k": [x] * 3, "v": [x] * 3})()
    for d in accepted:
        del log[:]
        m._chain_layers(x, cache, None, None, lambda qkv, li: x, True, d)
        fresh, consumers = False, 0
        for name, kw in log:
            residual = name == "linear_add_" or (name == "gemm4w" and kw.get("residual") is not None)
            if name == "rms_rowsumsq" or (residual and "chain" in kw):
                fresh = True
            elif residual:  # the planned residual GEMM: a new residual stream, no partials
                fresh = False
            elif name == "gemm4w":
                assert "chain" in kw and fresh, (d, log)
                consumers += 1
            else:
                assert name in ("rmsnorm", "linear", "swiglu", "rope_kv_write"), name
        assert consumers == 3 * d["attn"] + 3 * d["mlp"] + d["final"]
