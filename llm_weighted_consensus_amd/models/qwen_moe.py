"""Qwen3-MoE decoders (Qwen3-30B-A3B: 128 experts, 8 per token, per-expert FFN width 768).

`MixtralModel` with the Qwen3 attention block: a per-head RMSNorm of q and k before the rotation (one weight of
``head_dim`` values each, shared by all heads), applied by the shared attention body of `LlamaModel` through
``ops.qknorm_rope_kv_write`` as for the dense Qwen3 decoders.  The MoE layer is Mixtral's: the router's softmax
over all experts, top-k, renormalise (``norm_topk_prob``) equals the softmax over the k selected logits, which is
what the routing kernels compute.  With 128 experts ``ops.route`` takes the wide router
(csrc/kernels/moe_wide.hip); the grouped expert GEMMs, the SwiGLU / MX middle and the combine are unchanged.

One device only: tensor and expert parallelism are refused at construction, and so is the use as an embedder
(``config.check_variant``).  ``fp8=True`` quantises the experts at load (gate|up interleaved in blocks of 32) and
holds the attention projections as ``ops.Fp8Weight``, as for Mixtral.  ``expert_weights="mxfp4"`` holds the experts
as ``ops.Mxfp4Experts`` (weight-only, everything else bf16), as for Mixtral too, and ``expert_act="e4m3"`` runs their
large steps with e4m3 activations (``ops.moe_gemm_mxfp4_a8``).
"""
from __future__ import annotations

from pathlib import Path
from typing import Optional

import torch

from .config import DecoderConfig
from .mixtral import MixtralModel


class Qwen3MoeModel(MixtralModel):
    qk_norm_attention = True  # passes MixtralModel's qk_norm gate; a q|k|v bias stays refused there

    def __init__(self, cfg: DecoderConfig, device="cuda", dtype=torch.bfloat16, seed: int = 0,
                 weights_path: Optional[str] = None, max_position: Optional[int] = None, fp8: bool = False,
                 tp_size: int = 1, ep_size: int = 1, mxfp4: bool = False, expert_weights: str = "bf16",
                 expert_act: str = "bf16"):
        if not (cfg.num_experts and cfg.qk_norm):
            raise ValueError(f"{cfg.name} is not a Qwen3-MoE decoder (a MoE config with qk_norm)")
        if tp_size > 1 or ep_size > 1:
            raise ValueError(f"{cfg.name}: Qwen3-MoE decoders run on one device (tp_size {tp_size}, ep_size {ep_size})")
        super().__init__(cfg, device=device, dtype=dtype, seed=seed, weights_path=weights_path,
                         max_position=max_position, fp8=fp8, mxfp4=mxfp4, expert_weights=expert_weights,
                         expert_act=expert_act)

    def _random_init(self, seed: int) -> None:
        """Mixtral's tensors from Mixtral's generator, then the q / k norm weights of every layer from a generator
        of their own (1 + 0.3 N(0, 1) in fp32, one cast, as LlamaModel draws them for Qwen3): no other arch's
        random sequence moves."""
        super()._random_init(seed)
        g = torch.Generator(device=self.device)
        g.manual_seed(seed + 0x51E3)

        def norm_w():
            w = 1.0 + 0.3 * torch.randn(self.full_cfg.head_dim, generator=g, device=self.device, dtype=torch.float32)
            return w.to(self.dtype)

        for L in self.layers:
            L.q_norm, L.k_norm = norm_w(), norm_w()

    def _load(self, path: str) -> None:
        """HF Qwen3-MoE safetensors (model.layers.N.self_attn.{q,k,v,o}_proj / {q,k}_norm, mlp.gate,
        mlp.experts.<e>.{gate,up,down}_proj).  Every tensor is checked by name: one that is missing, or of
        another shape than the config's, refuses the checkpoint."""
        from safetensors.torch import load_file

        files = sorted(Path(path).glob("*.safetensors")) if Path(path).is_dir() else [Path(path)]
        sd = {}
        for f in files:
            sd.update(load_file(str(f), device="cpu"))
        dev, dt, cfg = self.device, self.dtype, self.full_cfg

        def req(name, shape):
            if name not in sd:
                raise ValueError(f"{path}: {cfg.name} needs {name}, which the checkpoint does not have")
            if tuple(sd[name].shape) != tuple(shape):
                raise ValueError(f"{path}: {name} has shape {tuple(sd[name].shape)}, {cfg.name} expects {tuple(shape)}")
            return sd[name].to(device=dev, dtype=dt).contiguous()

        d, F_, E, D = cfg.hidden, cfg.ffn, cfg.num_experts, cfg.head_dim
        self.embed = req("model.embed_tokens.weight", (cfg.vocab_size, d))
        self.layers = []
        for i in range(cfg.layers):
            p = f"model.layers.{i}."

            def ex(w, shape):
                return torch.stack([req(f"{p}mlp.experts.{e}.{w}.weight", shape) for e in range(E)])

            L = self._shard_layer(
                req(p + "input_layernorm.weight", (d,)), req(p + "self_attn.q_proj.weight", (cfg.heads * D, d)),
                req(p + "self_attn.k_proj.weight", (cfg.kv_heads * D, d)),
                req(p + "self_attn.v_proj.weight", (cfg.kv_heads * D, d)),
                req(p + "self_attn.o_proj.weight", (d, cfg.heads * D)),
                req(p + "post_attention_layernorm.weight", (d,)), req(p + "mlp.gate.weight", (E, d)),
                ex("gate_proj", (F_, d)), ex("up_proj", (F_, d)), ex("down_proj", (d, F_)))
            L.q_norm = req(p + "self_attn.q_norm.weight", (D,))
            L.k_norm = req(p + "self_attn.k_norm.weight", (D,))
            self.layers.append(L)
        self.final_norm = req("model.norm.weight", (d,))
        self.lm_head = req("lm_head.weight", (cfg.vocab_size, d)) if "lm_head.weight" in sd else self.embed
