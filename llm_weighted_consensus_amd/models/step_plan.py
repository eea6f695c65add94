"""The decode step plan: which GEMM backend runs each projection and where the RMSNorm is folded into gemm4w.

A step plan is the wire dict ``{"choices": {projection: backend}, "chain": {...} or None}`` that the bench pins,
the engine's in-step A/B races and :class:`~.llama.LlamaModel` executes.  Its ``chain`` half (the folded-norm
chain) parses into :class:`ChainPlan`, the one place that knows which entries are legal, which of them change
the step, and that a folded norm point needs a producer of partial row sums of squares.  The functions below
build, change and print plans from recorded timings; nothing here touches the device.
"""
from __future__ import annotations

from dataclasses import asdict, dataclass, fields
from typing import ClassVar, Optional

PROJECTIONS = ("qkv", "o", "gu", "down", "lm")
# gemm4w's schedule for a residual epilogue that writes the partials itself (RS 2)
OWN_VAR = {"own32": 32, "own64": 64}
_PRODUCERS = ("plain", "own32", "own64", "sumsq")
_LEGAL = {"attn": (False, True), "mlp": (False, True), "final": (False, True), "qkv_bn": (192, 256),
          "qkv_var": (32, 64), "gu_var": (32, 64), "lm_var": (32, 64), "lm_split": (False, True),
          "o": _PRODUCERS, "down": _PRODUCERS}


@dataclass(frozen=True)
class ChainPlan:
    """Where a decode step folds the RMSNorm.  ``attn`` / ``mlp`` / ``final``: the norm before qkv / gate|up /
    lm_head is folded (the consumer scales its rows from the chain's partials: gemm4w tile width ``qkv_bn``,
    schedule ``*_var``, ``lm_split``: lm_head's ragged last round split along K, VAR 64 only).  ``o`` / ``down``:
    how that residual projection leaves the partials for the folded point after it ("own32" / "own64": its own
    gemm4w epilogue; "sumsq": one rms_rowsumsq pass after the planned GEMM; "plain": none).

    An entry whose norm point is unfolded is dead: legal, kept verbatim, and without effect (:meth:`live`)."""
    attn: bool = False
    mlp: bool = False
    final: bool = False
    qkv_bn: int = 192
    qkv_var: int = 32
    gu_var: int = 32
    lm_var: int = 32
    lm_split: bool = False
    o: str = "plain"
    down: str = "plain"

    UNFOLDED: ClassVar["ChainPlan"]  # no norm folded, every entry at its default

    def __post_init__(self):
        for f in fields(self):
            if getattr(self, f.name) not in _LEGAL[f.name]:
                raise ValueError(f"chain plan: {f.name}={getattr(self, f.name)!r} is not one of {_LEGAL[f.name]}")
        if self.mlp and self.o == "plain":
            raise ValueError("chain plan: mlp is folded but o leaves no partials (o='plain')")
        if (self.attn or self.final) and self.down == "plain":
            raise ValueError("chain plan: attn or final is folded but down leaves no partials (down='plain')")

    @classmethod
    def from_dict(cls, d: dict) -> "ChainPlan":
        unknown = [k for k in d if k not in _LEGAL]
        if unknown:
            raise ValueError(f"chain plan: unknown key {unknown[0]!r}")
        return cls(**d)

    def as_dict(self) -> dict:
        return asdict(self)

    @property
    def folds(self) -> bool:
        return bool(self.attn or self.mlp or self.final)

    def live(self) -> "ChainPlan":
        """The plan with dead entries at their defaults: two plans run the same step iff their live views are equal."""
        u = ChainPlan.UNFOLDED
        return ChainPlan(
            attn=bool(self.attn), mlp=bool(self.mlp), final=bool(self.final),
            qkv_bn=self.qkv_bn if self.attn else u.qkv_bn, qkv_var=self.qkv_var if self.attn else u.qkv_var,
            gu_var=self.gu_var if self.mlp else u.gu_var, lm_var=self.lm_var if self.final else u.lm_var,
            lm_split=bool(self.final and self.lm_split and self.lm_var == 64),
            o=self.o if self.mlp else "plain", down=self.down if self.attn or self.final else "plain")

    def down_mode(self, last: bool) -> str:
        """The down projection's producer mode in one layer: an inner layer's feeds the next qkv, the last
        layer's feeds lm_head."""
        return self.down if (self.final if last else self.attn) else "plain"

    def owned(self) -> set:
        """The projections whose kernel the chain fixes (their backend choice is not consulted)."""
        lv = self.live()
        return ({n for n, folded in (("qkv", lv.attn), ("gu", lv.mlp), ("lm", lv.final)) if folded}
                | {n for n in ("o", "down") if getattr(lv, n) in OWN_VAR})


ChainPlan.UNFOLDED = ChainPlan()

# The chain candidates that LlamaModel._tune_chain times alone, per projection: timing name -> the ChainPlan
# entries that name stands for (the names are the keys of TIMINGS[(M, hidden, 0, "norm_chain")])
CHAIN_CANDIDATES = {
    "qkv": {f"qkv_rs{bn}v{v}": {"qkv_bn": bn, "qkv_var": v} for bn in (192, 256) for v in (32, 64)},
    "gu": {f"gu_rsv{v}": {"gu_var": v} for v in (32, 64)},
    "lm": {"lm_rsv32": {"lm_var": 32, "lm_split": False}, "lm_rsv64": {"lm_var": 64, "lm_split": False},
           "lm_rsv64s": {"lm_var": 64, "lm_split": True}},
    "o": {f"o_{mode}": {"o": mode} for mode in OWN_VAR},
    "down": {f"down_{mode}": {"down": mode} for mode in OWN_VAR},
}


def fastest_candidate(proj: str, t: dict) -> str:
    """The timing name of ``proj``'s fastest chain candidate by the chain timings ``t`` (untimed ones last)."""
    return min(CHAIN_CANDIDATES[proj], key=lambda c: t.get(c, float("inf")))


def producer_costs(proj: str, t: dict) -> dict:
    """What each way for the o / down projection to leave partials costs by the chain timings ``t`` (the timed
    ones only): its own epilogue at either schedule, or the planned GEMM plus one rms_rowsumsq pass."""
    costs = {f[proj]: t[c] for c, f in CHAIN_CANDIDATES[proj].items() if c in t}
    if proj in t and "sumsq" in t:
        costs["sumsq"] = t[proj] + t["sumsq"]
    return costs


def cheapest_producer(proj: str, t: Optional[dict]) -> str:
    """The cheapest of :func:`producer_costs`; "sumsq" (which needs no gemm4w shape) when nothing was timed."""
    costs = producer_costs(proj, t or {})
    return min(costs, key=costs.get) if costs else "sumsq"


def check_plan(plan: dict) -> Optional[ChainPlan]:
    """Parse a wire plan: ValueError for an unknown projection or a bad chain; returns its ChainPlan (or None)."""
    for n in plan["choices"]:
        if n not in PROJECTIONS:
            raise ValueError(f"step plan: unknown projection {n!r}")
    ch = plan.get("chain")
    return ChainPlan.from_dict(ch) if ch is not None else None


def step_plans(choices: dict, own: dict, chain: Optional[dict], chain_t: Optional[dict]) -> dict:
    """The whole-plan candidates.  ``choices``: the planner's backend per projection; ``own``: each projection's
    fastest hand-written backend (None: none timed); ``chain`` / ``chain_t``: the planner's chain plan and the
    chain timings at this batch.  ``planner``: as tuned; ``library``: hipBLASLt everywhere, nothing folded;
    ``own``: the fastest hand-written backend everywhere and, where the chain was timed, every norm folded with
    the fastest consumer and own-epilogue producer."""
    plans = {"planner": {"choices": dict(choices), "chain": chain},
             "library": {"choices": {n: "blas" for n in choices},
                         "chain": ChainPlan.UNFOLDED.as_dict() if chain is not None else None}}
    own_chain = chain
    if chain is not None and chain_t:
        entries = {}
        for proj, cands in CHAIN_CANDIDATES.items():
            entries.update(cands[fastest_candidate(proj, chain_t)])
        own_chain = ChainPlan(attn=True, mlp=True, final=True, **entries).as_dict()
    plans["own"] = {"choices": {n: own[n] or choices[n] for n in choices}, "chain": own_chain}
    return plans


def step_moves(plan: dict, own: dict, chain_usable: bool, chain_t: Optional[dict]) -> list:
    """Single-decision changes of ``plan`` that change the step, as [(label, delta)] for :func:`with_move`: each
    projection's backend (hipBLASLt <-> ``own``) where the chain does not own it and, when the norm chain can
    run at this batch (``chain_usable``), each norm point folded or not, the live consumers' schedule / tile
    width and the live producers' mode.  Folding a point whose producer is "plain" also sets the producer
    (:func:`cheapest_producer` by ``chain_t``): a consumer never reads partials nobody wrote."""
    ch = check_plan(plan) if chain_usable else None
    owned = ch.owned() if ch is not None else set()
    moves = []

    def variant(label, choices=None, chain=None):
        moves.append((label, {"choices": dict(choices or {}), "chain": dict(chain or {})}))

    for n in PROJECTIONS:
        if n in owned or own[n] is None:
            continue
        to = own[n] if plan["choices"].get(n) == "blas" else "blas"
        variant(f"{n}={to}", {n: to})
    if ch is None:
        return moves
    for pt, prod in (("attn", "down"), ("mlp", "o"), ("final", "down")):
        delta = {pt: not getattr(ch, pt)}
        if delta[pt] and getattr(ch, prod) == "plain":
            delta[prod] = cheapest_producer(prod, chain_t)
        variant(f"{pt}_fold={delta[pt]}", chain=delta)
    if ch.final:
        variant(f"lm_split={not ch.lm_split}", chain={"lm_split": not ch.lm_split, "lm_var": 64})
    for key, pt in (("qkv_var", "attn"), ("gu_var", "mlp"), ("lm_var", "final"), ("qkv_bn", "attn")):
        for v in _LEGAL[key]:
            if v != getattr(ch, key) and getattr(ch, pt):
                variant(f"{key}={v}", chain={key: v})
    for key, live in (("o", ch.mlp), ("down", ch.attn or ch.final)):
        for v in ("own32", "own64", "sumsq"):
            if v != getattr(ch, key) and live:
                variant(f"{key}_producer={v}", chain={key: v})
    return moves


def with_move(plan: dict, delta: dict) -> dict:
    """``plan`` with one :func:`step_moves` delta applied (choices and chain entries overridden), checked."""
    ch = plan.get("chain")
    out = {"choices": dict(plan["choices"], **delta.get("choices", {})),
           "chain": dict(ch, **delta.get("chain", {})) if ch is not None else None}
    check_plan(out)
    return out


def plan_summary(backends: dict, chain: Optional[ChainPlan]) -> dict:
    """The kernels a decode step runs, compactly: ``backends`` per projection, overridden by what the live
    view of ``chain`` (None: the step folds nothing) puts there."""
    out = dict(backends)
    if chain is None:
        return out
    lv = chain.live()
    if lv.attn:
        out["qkv"] = f"g4 rs{lv.qkv_bn} v{lv.qkv_var}"
    if lv.mlp:
        out["gu"] = f"g4 rs v{lv.gu_var}"
    if lv.final:
        out["lm"] = f"g4 rs v{lv.lm_var}" + (" split-K tail" if lv.lm_split else "")
    for n in ("o", "down"):
        mode = getattr(lv, n)
        if mode == "sumsq":
            out[n] += "+sumsq"
        elif mode in OWN_VAR:
            out[n] = f"g4 rs2 v{OWN_VAR[mode]}"
    return out
