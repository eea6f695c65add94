"""LoRA adapters as distinct voters on one base model.

A :class:`LoraSet` holds every adapter of one model in the layout the batched kernels read
(``csrc/kernels/lora.hip``, ``ops.lora_shrink`` / ``ops.lora_expand_add_``): per layer and per ENGINE projection
(``qkv``, ``o``, ``gate_up``, ``down`` — the fused weights of ``models.llama.LayerWeights``) the stacked
``A [n_adapters, R, K]`` and ``B [n_adapters, N, R]`` in bf16, so a batch whose rows carry different adapters
(per-row int32 ids, -1 = none) is two launches per projection.

Fused projections: the HF targets q, k, v (gate, up) of one adapter become one pair: ``A`` is the targets'
A matrices stacked along the rank axis, ``B`` is block-diagonal — target t's B fills its own rows (the q, k or v
column range of the projection's output) and its own rank columns.  Only targets that some adapter of the set
carries get a rank slot; an adapter that lacks one has a zero block there.  Every rank is zero-padded to the
set's maximum rounded up to 16 (the MFMA k granularity), ``alpha / r`` is folded into ``B``.  For a gate|up
weight interleaved in blocks (``LayerWeights.gu_block``) the rows of ``B`` are permuted the same way.

Sources of an adapter (the ``weights`` key of its spec): ``"random:<seed>"`` — N(0, std) A and B (B non-zero,
unlike PEFT's init, so the adapter changes the output), or a PEFT directory (``adapter_config.json`` with
``r`` / ``lora_alpha`` / ``target_modules`` and ``adapter_model.safetensors``).  Loading is pure torch on CPU
tensors.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch

from .config import DecoderConfig

TARGETS = ("q", "k", "v", "o", "gate", "up", "down")
# engine projection -> its HF targets, in the row order of the fused weight
PROJ_TARGETS = {"qkv": ("q", "k", "v"), "o": ("o",), "gate_up": ("gate", "up"), "down": ("down",)}
_HF_NAME = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
            "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
MAX_FUSED_RANK = 192  # the kernels' R limit (csrc/kernels/lora.hip)
MAX_ADAPTERS = 64


def target_dims(cfg: DecoderConfig) -> Dict[str, Tuple[int, int]]:
    """target -> (out features, in features)."""
    d, q, kv, f = cfg.hidden, cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim, cfg.ffn
    return {"q": (q, d), "k": (kv, d), "v": (kv, d), "o": (d, q), "gate": (f, d), "up": (f, d), "down": (d, f)}


def check_targets(targets) -> Tuple[str, ...]:
    out = []
    for t in targets:
        t = str(t)
        t = t[:-5] if t.endswith("_proj") else t
        if t not in TARGETS:
            raise ValueError(f"LoRA target {t!r}: expected one of {', '.join(TARGETS)}")
        if t not in out:
            out.append(t)
    if not out:
        raise ValueError("a LoRA adapter needs at least one target")
    return tuple(out)


@dataclass
class Adapter:
    """One adapter on the CPU in fp32: ``layers[i][target] = (A [r, in], B [out, r])``, unscaled."""
    name: str
    rank: int
    alpha: float
    targets: Tuple[str, ...]
    layers: List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = field(default_factory=list)

    @property
    def scale(self) -> float:
        return float(self.alpha) / float(self.rank)


def random_adapter(name: str, cfg: DecoderConfig, seed: int, rank: int = 16, alpha: float = 32.0,
                   targets=TARGETS, std: float = 0.02) -> Adapter:
    targets = check_targets(targets)
    if rank < 1:
        raise ValueError(f"adapter {name!r}: rank must be positive")
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    dims = target_dims(cfg)
    layers = []
    for _ in range(cfg.layers):
        lw = {}
        for t in targets:
            n, k = dims[t]
            lw[t] = (torch.randn(rank, k, generator=g) * std, torch.randn(n, rank, generator=g) * std)
        layers.append(lw)
    return Adapter(name, int(rank), float(alpha), targets, layers)


def load_peft_adapter(name: str, path: str, cfg: DecoderConfig) -> Adapter:
    """A PEFT LoRA checkpoint directory: adapter_config.json + adapter_model.safetensors."""
    from safetensors.torch import load_file

    p = Path(path)
    with open(p / "adapter_config.json") as f:
        conf = json.load(f)
    rank, alpha = int(conf["r"]), float(conf.get("lora_alpha", conf["r"]))
    targets = check_targets(conf["target_modules"])
    sd = load_file(str(p / "adapter_model.safetensors"), device="cpu")
    dims = target_dims(cfg)
    layers = []
    for i in range(cfg.layers):
        lw = {}
        for t in targets:
            key = f"base_model.model.model.layers.{i}.{_HF_NAME[t]}."
            if key + "lora_A.weight" not in sd:
                continue  # (PEFT's layers_to_transform: a target on some layers only)
            a, b = sd[key + "lora_A.weight"].float(), sd[key + "lora_B.weight"].float()
            n, k = dims[t]
            if tuple(a.shape) != (rank, k) or tuple(b.shape) != (n, rank):
                raise ValueError(f"adapter {name!r} layer {i} {t}: A {tuple(a.shape)} / B {tuple(b.shape)} do not fit "
                                 f"rank {rank} on a {n} x {k} projection")
            lw[t] = (a, b)
        layers.append(lw)
    if not any(layers):
        raise ValueError(f"adapter {name!r}: no LoRA weights of its targets found in {path}")
    return Adapter(name, rank, alpha, targets, layers)


def load_adapter(name: str, spec: dict, cfg: DecoderConfig) -> Adapter:
    """An adapter from its spec: {"weights": "random:<seed>" | "<peft dir>", "rank", "alpha", "targets", "std"}
    (rank / alpha / targets describe a random adapter; a PEFT directory brings its own)."""
    if ":" in name or not name:
        raise ValueError(f"adapter name {name!r}: must be non-empty and hold no ':'")
    if "targets" in spec:
        check_targets(spec["targets"])
    w = str(spec.get("weights", "random:0"))
    if w.startswith("random:"):
        return random_adapter(name, cfg, int(w.split(":", 1)[1]), int(spec.get("rank", 16)),
                              float(spec.get("alpha", 2 * int(spec.get("rank", 16)))),
                              spec.get("targets", TARGETS), float(spec.get("std", 0.02)))
    return load_peft_adapter(name, w, cfg)


def check_model_spec(name: str, spec: dict, embedder: bool = False) -> Tuple[str, ...]:
    """The adapter names of a server model spec, refusing the combinations adapters do not run in (tensor
    parallelism, MoE decoders, fp8 weights, embedding models), what "mxfp4" / "mxfp4_act" / "expert_weights" / "expert_act" do not
    run in (``config.check_variant``) and malformed adapter entries: raised when the server is configured, before
    any weight is loaded."""
    from .config import DECODERS, check_variant

    ads = spec.get("adapters")
    check_variant(DECODERS.get(spec.get("arch")), tp=int(spec.get("tp", 1) or 1) > 1, fp8=bool(spec.get("fp8")),
                  mxfp4=bool(spec.get("mxfp4")), adapters=bool(ads), embedder=embedder, mxfp4_act=spec.get("mxfp4_act"),
                  expert_weights=spec.get("expert_weights"), expert_act=spec.get("expert_act"),
                  who=f"embedding model {name}" if embedder else f"model {name}")
    if not ads:
        return ()
    if not isinstance(ads, dict):
        raise ValueError(f"model {name}: \"adapters\" must map adapter names to their specs")
    if len(ads) > MAX_ADAPTERS:
        raise ValueError(f"model {name}: {len(ads)} adapters, at most {MAX_ADAPTERS} per model")
    for an, aspec in ads.items():
        if not an or ":" in str(an):
            raise ValueError(f"model {name}: adapter name {an!r} must be non-empty and hold no ':'")
        if not isinstance(aspec, dict):
            raise ValueError(f"model {name}: adapter {an!r} needs a spec object")
        if "targets" in aspec:
            check_targets(aspec["targets"])
    return tuple(str(a) for a in ads)


def _interleave_rows(b: torch.Tensor, block: int) -> torch.Tensor:
    """The row permutation the model applies to its gate|up weight: ``ops.swiglu_interleave`` itself."""
    from ..ops import swiglu_interleave

    return swiglu_interleave(b, block)


def load_adapters(cfg: DecoderConfig, spec: Dict[str, dict]) -> List[Adapter]:
    """The adapters of a model spec's ``adapters`` mapping (server/config.py), in its order, on the CPU."""
    return [load_adapter(str(n), dict(s or {}), cfg) for n, s in spec.items()]


def _same_device(a, b) -> bool:
    a, b = torch.device(a), torch.device(b)
    return a.type == b.type and (a.index or 0) == (b.index or 0)


class LoraSet:
    """Every adapter of one model, stacked for the batched kernels (module docstring).

    ``A[layer][proj]`` [n, R, K] / ``B[layer][proj]`` [n, N, R] bf16 on ``device``, or both None for a projection
    no adapter targets (the model then launches nothing for it).  ``gu_block``: the base model's gate|up row
    interleave (``LayerWeights.gu_block``)."""

    def __init__(self, cfg: DecoderConfig, adapters: List[Adapter], gu_block: int = 0, device="cpu",
                 dtype=torch.bfloat16):
        if not adapters:
            raise ValueError("LoraSet: no adapters")
        if len(adapters) > MAX_ADAPTERS:
            raise ValueError(f"LoraSet: {len(adapters)} adapters, at most {MAX_ADAPTERS} per model")
        names = [a.name for a in adapters]
        if len(set(names)) != len(names):
            raise ValueError("LoraSet: duplicate adapter names")
        self.cfg, self.adapters, self.names, self.gu_block = cfg, list(adapters), names, int(gu_block)
        self.device, self.dtype = torch.device(device), dtype
        self.rank = -(-max(a.rank for a in adapters) // 16) * 16  # per-target rank slot
        carried = {t for a in adapters for lw in a.layers for t in lw}
        self.slots = {p: tuple(t for t in ts if t in carried) for p, ts in PROJ_TARGETS.items()}
        for p, ts in self.slots.items():
            if len(ts) * self.rank > MAX_FUSED_RANK:
                raise ValueError(f"LoraSet: rank {self.rank} on {len(ts)} fused targets of {p} exceeds the kernels' "
                                 f"fused rank {MAX_FUSED_RANK}")
        dims = target_dims(cfg)
        # the kernels' shape contract (csrc/kernels/lora.hip): refused here, not at the first forward
        for p, ts in self.slots.items():
            if ts:
                k = dims[PROJ_TARGETS[p][0]][1]
                n_out = sum(dims[t][0] for t in PROJ_TARGETS[p])
                if k % 64 or n_out % 8:
                    raise ValueError(f"LoraSet: {cfg.name}'s {p} projection ({n_out} x {k}) does not fit the LoRA "
                                     f"kernels (input features a multiple of 64, output features of 8)")
        self.A: List[Dict[str, Optional[torch.Tensor]]] = []
        self.B: List[Dict[str, Optional[torch.Tensor]]] = []
        n, r = len(adapters), self.rank
        for li in range(cfg.layers):
            la, lb = {}, {}
            for p, all_ts in PROJ_TARGETS.items():
                ts = self.slots[p]
                if not ts:
                    la[p] = lb[p] = None
                    continue
                k = dims[all_ts[0]][1]
                n_out = sum(dims[t][0] for t in all_ts)
                row0 = {t: sum(dims[u][0] for u in all_ts[:all_ts.index(t)]) for t in all_ts}
                a_st = torch.zeros(n, len(ts) * r, k)
                b_st = torch.zeros(n, n_out, len(ts) * r)
                for ai, ad in enumerate(adapters):
                    for si, t in enumerate(ts):
                        if t not in ad.layers[li]:
                            continue
                        a, b = ad.layers[li][t]
                        a_st[ai, si * r:si * r + ad.rank] = a
                        b_st[ai, row0[t]:row0[t] + dims[t][0], si * r:si * r + ad.rank] = b * ad.scale
                if p == "gate_up" and self.gu_block:
                    b_st = torch.stack([_interleave_rows(b_st[ai], self.gu_block) for ai in range(n)])
                la[p] = a_st.to(device=device, dtype=dtype).contiguous()
                lb[p] = b_st.to(device=device, dtype=dtype).contiguous()
            self.A.append(la)
            self.B.append(lb)
        self.adapts_gate_up = bool(self.slots["gate_up"])

    def index(self, name: str) -> int:
        try:
            return self.names.index(name)
        except ValueError:
            raise ValueError(f"unknown adapter {name!r} (model has: {', '.join(self.names)})") from None

    def __len__(self) -> int:
        return len(self.adapters)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for l in self.A + self.B for t in l.values() if t is not None)

    def laid_out_for(self, gu_block: int, device) -> bool:
        """Whether the stacks already have a model's gate|up interleave and live on its device."""
        return self.gu_block == int(gu_block) and _same_device(self.device, device)

    @classmethod
    def from_spec(cls, cfg: DecoderConfig, spec: Dict[str, dict], gu_block: int = 0, device="cpu") -> "LoraSet":
        """``spec``: the ``adapters`` mapping of a model spec (server/config.py), in its order."""
        return cls(cfg, load_adapters(cfg, spec), gu_block, device)


def merged_weights(base_layer, adapter: Adapter, layer: int) -> Dict[str, torch.Tensor]:
    """``W + (alpha / r) B A`` of every engine projection of ``base_layer`` (a ``LayerWeights`` whose norms are
    NOT folded into its weights) for ``adapter``'s layer ``layer``, in fp32 and in the layer's own layout
    (fused q|k|v, gate|up interleaved by its ``gu_block``): what baking the adapter into the model gives."""
    lw = adapter.layers[layer]
    out = {}
    for p, attr in (("qkv", "wqkv"), ("o", "wo"), ("gate_up", "w_gate_up"), ("down", "w_down")):
        w = getattr(base_layer, attr).float().clone()
        ts = PROJ_TARGETS[p]
        sizes = None
        delta = torch.zeros_like(w)
        if any(t in lw for t in ts):
            rows = []
            for t in ts:
                if t in lw:
                    a, b = lw[t]
                    rows.append((b.to(w.device) @ a.to(w.device)) * adapter.scale)
                else:
                    rows.append(None)
            # row ranges of the fused weight in HF order (equal-sized gate / up; q, k, v from the shapes)
            if p == "qkv":
                n_kv = next((r.shape[0] for t, r in zip(ts, rows) if r is not None and t != "q"), None)
                n_q = next((r.shape[0] for t, r in zip(ts, rows) if r is not None and t == "q"), None)
                if n_kv is None:
                    n_kv = (w.shape[0] - n_q) // 2
                if n_q is None:
                    n_q = w.shape[0] - 2 * n_kv
                sizes = (n_q, n_kv, n_kv)
            else:
                sizes = tuple(w.shape[0] // len(ts) for _ in ts)
            o = 0
            for r, n in zip(rows, sizes):
                if r is not None:
                    delta[o:o + n] = r
                o += n
            if p == "gate_up" and getattr(base_layer, "gu_block", 0):
                delta = _interleave_rows(delta, base_layer.gu_block)
        out[attr] = w + delta
    return out
