"""Llama-family decoder (Llama-3 / Mistral shapes) on the gfx950 kernel set.

This is the local generation backend that replaces the reference's upstream providers
(reference: every voter is an OpenAI-compatible chat call, src/chat/completions/client.rs:308-332).

Per layer (decode, B sequences):
    rmsnorm                       K1
    qkv  = x @ Wqkv^T             K6 (fused q|k|v weight)
    rope + paged KV write         K2 (in place, one pass; Qwen: K2q, the q|k|v bias and the per-head q / k
                                      RMSNorm in the same pass, csrc/kernels/qknorm.hip)
    attn = paged GQA decode       K3 (cascade for forked candidates, else split-K)
    x   += attn @ Wo^T            K6 with the residual add in its epilogue, then K1
    act  = silu(x Wg^T) (x Wu^T)  K6 with SwiGLU in its epilogue (fused gate|up weight), or GEMM + K5
    x   += act @ Wd^T             K6 + residual, then K1
K6 is chosen per shape by ops/gemm_plan.py among hipBLASLt and the hand-written cores (gemm4w, gemm8p),
timed on the device.

Folded RMSNorm (decode chain, dense bf16 on the GPU): every norm weight is folded into the projection that
reads it at load (W_qkv diag(g_attn), W_gate_up diag(g_mlp), W_lm_head diag(g_final); the norm weights become
ones, so the unfolded path computes the same function), and a decode step where the chain was timed faster
(:meth:`LlamaModel.tune_gemms`) runs NO norm kernel: the o / down projections' residual epilogues emit the
partial row sums of squares of the new residual stream, from which the next projection (qkv, gate|up,
lm_head) scales its accumulator rows by 1/rms (gemm4w RS modes, csrc/kernels/gemm4w.hip):
    ss = rms_rowsumsq(embedding)                  (once)
    qkv = gemm4w(x, W_qkv', ss)   ...   x += gemm4w(attn, W_o) -> ss
    act = gemm4w(x, W_gu', ss, SwiGLU)   x += gemm4w(act, W_d) -> ss     ...   logits = gemm4w(x, W_lm', ss)  Prefill uses the same layer with the varlen causal flash-attention kernel (K4) over
the fresh k/v of the qkv buffer; mixed chunked-prefill steps (forward_mixed) send decode rows to K3 and
prompt-chunk rows to K4's paged-KV mode; the k/v are scattered into the paged cache in the RoPE pass.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import torch
import torch.nn.functional as F

from .. import ops
from ..ops import blas_tuning, gemm_plan
from ..ops.mxfp4 import Mxfp4Weight
from . import step_plan
from .config import DecoderConfig, check_decoder, check_variant
from .step_plan import ChainPlan


def rope_tables(cfg: DecoderConfig, device, max_pos: Optional[int] = None):
    """Host-built cos/sin tables [max_pos, D/2] f32 (Appendix B: no on-device trig), with the
    Llama-3 frequency scaling when configured."""
    D = cfg.head_dim
    max_pos = max_pos or cfg.max_position
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    if cfg.rope_scaling is not None:
        factor, lo_f, hi_f, orig = cfg.rope_scaling
        lo_wl, hi_wl = orig / lo_f, orig / hi_f
        wl = 2 * math.pi / inv
        smooth = (orig / wl - lo_f) / (hi_f - lo_f)
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        mid = (wl <= lo_wl) & (wl >= hi_wl)
        scaled = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
        inv = scaled
    t = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return ang.cos().float().to(device).contiguous(), ang.sin().float().to(device).contiguous()


@dataclass
class LayerWeights:
    attn_norm: torch.Tensor
    wqkv: torch.Tensor      # [(Hq+2Hkv)*D, d]
    wo: torch.Tensor        # [d, Hq*D]
    mlp_norm: torch.Tensor
    w_gate_up: torch.Tensor  # [2F, d]  rows: gate then up (gu_block 0) or interleaved in blocks of gu_block
    w_down: torch.Tensor    # [d, F]
    gu_block: int = 0
    # Qwen attention block (cfg.qkv_bias / cfg.qk_norm), applied by ops.qknorm_rope_kv_write
    bqkv: Optional[torch.Tensor] = None    # [(Hq+2Hkv)*D]  q|k|v projection bias
    q_norm: Optional[torch.Tensor] = None  # [D]  per-head RMSNorm weight of q, shared by all heads
    k_norm: Optional[torch.Tensor] = None  # [D]  the same for k


def _claim_gu_interleave(L: LayerWeights) -> bool:
    """The gate|up interleave rule, stated once: a GPU layer whose gate|up rows are still in the plain order and
    pair up in blocks of 32 (2F a multiple of 64) gets them interleaved in blocks of 32, so the GEMM epilogues
    (gemm8p, gemm8g, the MXFP4 stream) can apply the SwiGLU.  True: ``gu_block`` is now 32 and the caller
    permutes the rows it holds (``ops.swiglu_interleave``: a bf16 weight, or MXFP4 codes and scales)."""
    if L.gu_block != 0 or L.w_gate_up.shape[0] % 64 != 0:
        return False
    L.gu_block = 32
    return True


class KVCache:
    """One flat bf16 pool for all layers: [L, 2, num_blocks, Hkv*BS*D]; per-layer K view
    [NB, Hkv, BS, D] and 4-token-interleaved V view [NB, Hkv, BS/4, D, 4] (see attention_decode.hip)."""

    def __init__(self, cfg: DecoderConfig, num_blocks: int, block_size: int, device, dtype=torch.bfloat16):
        self.cfg, self.num_blocks, self.block_size = cfg, num_blocks, block_size
        self.block_elems = cfg.kv_heads * block_size * cfg.head_dim
        self.pool = torch.zeros(cfg.layers, 2, num_blocks, self.block_elems, dtype=dtype, device=device)
        Hkv, D = cfg.kv_heads, cfg.head_dim
        self.k = [self.pool[l, 0].view(num_blocks, Hkv, block_size, D) for l in range(cfg.layers)]
        self.v = [self.pool[l, 1].view(num_blocks, Hkv, block_size // 4, D, 4) for l in range(cfg.layers)]

    @staticmethod
    def bytes_per_block(cfg: DecoderConfig, block_size: int) -> int:
        return cfg.layers * 2 * cfg.kv_heads * block_size * cfg.head_dim * 2

    def copy_blocks(self, pairs: torch.Tensor) -> None:
        """Copy-on-write block copies (K12) for every layer, K and V."""
        if pairs.numel():
            ops.kv_block_copy(self.pool.view(self.cfg.layers * 2, self.num_blocks, self.block_elems), pairs)


class _NullCache:
    """Shape-only stand-in for KVCache when no KV is written (encode): one shared 1-block buffer."""

    def __init__(self, cfg: DecoderConfig, device):
        buf = torch.zeros(2, 1, cfg.kv_heads, 16, cfg.head_dim, dtype=torch.bfloat16, device=device)
        self.k = [buf[0]] * cfg.layers
        self.v = [buf[1].view(1, cfg.kv_heads, 4, cfg.head_dim, 4)] * cfg.layers


class LlamaModel:
    # What a subclass is, said by the subclass: the dense decoder on one rank adds its o / down projections into
    # the residual stream itself; the tensor-parallel and MoE subclasses reduce / route them first (False there)
    single_rank_dense = True
    tp_size = 1
    # the activation format of the MXFP4 projections ("e4m3": ``mxfp4_act``, below); a class-level default, so an
    # object that states only its facts (no constructor run) is the bf16-activation model
    act_format = "bf16"

    def __init__(self, cfg: DecoderConfig, device="cuda", dtype=torch.bfloat16, seed: int = 0,
                 weights_path: Optional[str] = None, max_position: Optional[int] = None, fp8_dense: bool = False,
                 fold_norms: bool = True, lora=None, mxfp4: bool = False, mxfp4_act: Optional[str] = None):
        check_decoder(cfg)  # shapes the kernels do not serve are refused here, by arch name
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        check_variant(cfg, tp=self.tp_size > 1, fp8=fp8_dense, mxfp4=mxfp4, adapters=lora is not None,
                      device_type=self.device.type, mxfp4_act=mxfp4_act)
        # The variant, stated once; everything below reads these (and the class's ``single_rank_dense``).
        # "mxfp4" (ops/mxfp4.py): qkv / o / gate|up / down as 4-bit codes with one e8m0 scale per 32, bf16
        # activations; on a CPU device the model holds the dequantised bf16 weights (the same function, through
        # F.linear).  "fp8" (BASELINE config 5): the same projections (a MoE decoder's: attention and experts) in
        # e4m3 with per-channel scales, activations quantised per row; lm_head stays bf16.  The dense decoder's
        # fp8 exists on the GPU only: on a CPU device it stays "bf16"
        # ``mxfp4_act="e4m3"`` (with "mxfp4"; default "bf16": the weight-only model, bit for bit): every GEMM call
        # of at least ops.MXFP4_A8_MIN_ROWS rows runs row-quantised e4m3 activations x the packed weight on the
        # block-scaled MFMA (ops.gemm_mxfp4_a8: no dequantisation, no scratch); calls with fewer rows are the
        # weight-only path unchanged.  Routed by the call's row count alone, never by a timing.  Like the dense
        # fp8 flag it exists on the GPU only: a CPU model accepts it and computes with bf16 activations on the
        # dequantised weights (``act_format`` stays "bf16")
        self.moe = bool(cfg.num_experts)
        self.on_gpu = self.device.type == "cuda"
        self.weight_format = "mxfp4" if mxfp4 else "fp8" if fp8_dense and (self.on_gpu or self.moe) else "bf16"
        if self.moe and self.single_rank_dense:
            raise NotImplementedError("MoE decoders use models.mixtral.MixtralModel")
        if mxfp4 and mxfp4_act == "e4m3" and self.on_gpu:
            self.act_format = "e4m3"
        self.mx_scratch: Optional[torch.Tensor] = None  # bf16, the largest projection (ops.linear_mxfp4)
        self.cos, self.sin = rope_tables(cfg, self.device, max_position)
        if weights_path:
            self._load(weights_path)
        else:
            self._random_init(seed)
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        self.g8_ws = None
        if self.mxfp4 and self.on_gpu and not self._mx_no_scratch():
            # one dequantisation buffer for every projection past 64 rows, allocated here: never inside a capture
            n = max(math.prod(w.shape) for L in self.layers for w in (L.wqkv, L.wo, L.w_gate_up, L.w_down))
            self.mx_scratch = torch.empty(n, dtype=torch.bfloat16, device=self.device)
            torch.cuda.empty_cache()
        if self.on_gpu:
            # the dense layers' GPU layout (after a TP subclass cut its shard: shard_dense_layer reads the plain
            # row order): gate|up interleaved for the SwiGLU epilogues, then the fp8 conversion.  (MXFP4 layers
            # were laid out as they were built, MoE layers in MixtralModel._shard_layer.)
            for L in () if self.moe else self.layers:
                if self.fp8_dense:
                    L.wqkv, L.wo = ops.Fp8Weight(L.wqkv), ops.Fp8Weight(L.wo)
                if _claim_gu_interleave(L):
                    L.w_gate_up = ops.swiglu_interleave(L.w_gate_up)
                if self.fp8_dense:
                    L.w_gate_up, L.w_down = ops.Fp8Weight(L.w_gate_up), ops.Fp8Weight(L.w_down)
            if self.fp8_dense:
                torch.cuda.empty_cache()
            # gemm8p's stream-K workspace, owned by the model (never allocated inside a capture)
            self.g8_ws = ops.new_gemm8p_workspace(self.device)
            blas_tuning.enable()  # offline-tuned library solutions: only with LWC_TUNED_BLAS=1 (off by default)
        # folded RMSNorm (module docstring): the plain dense bf16 decoder on the GPU
        self.norm_folded = False
        self.extra_bytes = 0  # device bytes the folded norms add (a tied lm_head's own copy)
        self.final_norm_weight: Optional[torch.Tensor] = None  # the final norm's weight once lm_head holds it
        self.chain: Optional[ops.NormChain] = None
        self.chain_m: dict = {}  # decode batch M -> the step's chain plan, as a dict (step_plan.ChainPlan.from_dict)
        # LoRA adapters (``lora``: a list of models/lora.py Adapters, laid out here once for this model's weights
        # and device, or a LoraSet): rows of one batch carry different adapters (``lora_ids``).  With unfolded
        # norms: the adapters read the normalised rows
        self.lora = None
        if lora is not None:
            from .lora import LoraSet

            gu_block = self.layers[0].gu_block
            if not (isinstance(lora, LoraSet) and lora.laid_out_for(gu_block, self.device)):
                lora = LoraSet(cfg, lora.adapters if isinstance(lora, LoraSet) else list(lora), gu_block, self.device,
                               dtype)
            self.lora = lora
        self.pinned: dict = {}  # decode batch M -> a fixed step plan (pin_step_plan): nothing is timed at M
        # ``fold_norms=False``: models that never decode through lm_head (the decoder-as-embedder) skip it
        if (fold_norms and self.lora is None and self.on_gpu and self._dense_residual
                and os.environ.get("LWC_NORM_FOLD", "1") != "0"):
            self._fold_norms()

    def _fold_norms(self) -> None:
        """W diag(g) for every projection that reads a normalised row, then g = 1 (the unfolded path computes the
        same function).  One bf16 rounding of each folded weight (exact for the random-init unit norm weights).

        The final norm's weight is folded into lm_head only; :meth:`encode` (hidden states, no lm_head) keeps
        applying it (``final_norm_weight``).  A tied lm_head becomes its own vocab x hidden copy (W_emb diag(g)):
        ~1 GB more at Llama-3-8B shapes, reported by ``extra_bytes``."""
        def fold(w: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
            out = torch.empty_like(w)
            gf = g.float()
            for r in range(0, w.shape[0], 8192):
                out[r:r + 8192] = (w[r:r + 8192].float() * gf).to(w.dtype)
            return out

        for L in self.layers:
            L.wqkv, L.attn_norm = fold(L.wqkv, L.attn_norm), torch.ones_like(L.attn_norm)
            L.w_gate_up, L.mlp_norm = fold(L.w_gate_up, L.mlp_norm), torch.ones_like(L.mlp_norm)
        tied = self.lm_head is self.embed
        self.lm_head = fold(self.lm_head, self.final_norm)  # (a tied embedding table keeps its own copy)
        self.extra_bytes = self.lm_head.numel() * self.lm_head.element_size() if tied else 0
        self.final_norm_weight = self.final_norm  # what encode() applies
        self.final_norm = torch.ones_like(self.final_norm)
        self.norm_folded = True
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ weights
    def _random_init(self, seed: int) -> None:
        cfg, dev, dt = self.cfg, self.device, self.dtype
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        std = 0.02

        def rnd(*shape, s=std):
            return (torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * s).to(dt)

        d, qkv, F_ = cfg.hidden, cfg.qkv_dim, cfg.ffn
        self.embed = rnd(cfg.vocab_size, d)
        self.layers = []
        out_std = std / math.sqrt(2 * cfg.layers)
        for _ in range(cfg.layers):
            self.layers.append(LayerWeights(
                attn_norm=torch.ones(d, device=dev, dtype=dt),
                wqkv=rnd(qkv, d),
                wo=rnd(d, cfg.heads * cfg.head_dim, s=out_std),
                mlp_norm=torch.ones(d, device=dev, dtype=dt),
                w_gate_up=rnd(2 * F_, d),
                w_down=rnd(d, F_, s=out_std),
            ))
            # (drawn for flagged configs only, after the layer's matrices: every other arch draws the sequence
            # it always drew)
            if cfg.qkv_bias:
                self.layers[-1].bqkv = rnd(qkv, s=0.05)
            if cfg.qk_norm:
                def norm_w():  # 1 + 0.3 N(0, 1), in fp32, then one cast
                    return (1.0 + 0.3 * torch.randn(cfg.head_dim, generator=g, device=dev, dtype=torch.float32)).to(dt)

                self.layers[-1].q_norm, self.layers[-1].k_norm = norm_w(), norm_w()
            if self.mxfp4:
                self._quantise_layer(self.layers[-1])
        self.final_norm = torch.ones(d, device=dev, dtype=dt)
        self.lm_head = self.embed if cfg.tie_embeddings else rnd(cfg.vocab_size, d)

    def _quantise_layer(self, L: LayerWeights) -> None:
        """``mxfp4=True``: the layer's four projections become ops.Mxfp4Weight (a bf16 tensor is quantised and
        freed; a pre-quantised one is taken as it is), gate|up after its 32-row SwiGLU interleave — a row
        permutation, so it applies to the codes and scales directly.  Called as each layer is built, so at most
        one layer's bf16 projections are alive.  On a CPU device the layer holds the dequantised bf16 tensors in
        the plain row order."""
        def one(w, interleave=False):
            if isinstance(w, Mxfp4Weight):
                if interleave:
                    w = Mxfp4Weight.from_packed(ops.swiglu_interleave(w.q), ops.swiglu_interleave(w.s))
            else:
                w = Mxfp4Weight(ops.swiglu_interleave(w) if interleave else w)
            return w if self.on_gpu else w.dequant()

        L.wqkv, L.wo, L.w_down = one(L.wqkv), one(L.wo), one(L.w_down)
        L.w_gate_up = one(L.w_gate_up, self.on_gpu and _claim_gu_interleave(L))

    def _load(self, path: str) -> None:
        """Load HF-layout safetensors (model.layers.N.self_attn.q_proj.weight ...) and fuse q|k|v and
        gate|up into the engine's layout.

        ``mxfp4=True``: bf16 projections are quantised layer by layer; a projection stored pre-quantised — uint8
        ``<name>.weight`` [N, K / 2] with uint8 ``<name>.weight_scale`` [N, K / 32] in the format of ops/mxfp4.py
        (``scripts/quantize_mxfp4.py`` writes such files; the project's own convention) — is taken as it is,
        its shapes checked by tensor name."""
        from safetensors.torch import load_file

        files = sorted(Path(path).glob("*.safetensors")) if Path(path).is_dir() else [Path(path)]
        sd = {}
        for f in files:
            sd.update(load_file(str(f), device="cpu"))
        dev, dt = self.device, self.dtype

        def t(name):
            return sd[name].to(device=dev, dtype=dt).contiguous()

        cfg = self.cfg
        D = cfg.head_dim

        def req(name, shape):
            """A tensor a flagged config needs: absent, or of another shape than the config's, is an error
            (a checkpoint of another architecture must not vote with part of its weights dropped)."""
            if name not in sd:
                raise ValueError(f"{path}: {cfg.name} needs {name}, which the checkpoint does not have")
            if tuple(sd[name].shape) != tuple(shape):
                raise ValueError(f"{path}: {name} has shape {tuple(sd[name].shape)}, {cfg.name} expects {tuple(shape)}")
            return t(name)

        def attn_extras(p):
            out = {}
            if cfg.qkv_bias:
                out["bqkv"] = torch.cat([req(p + f"self_attn.{x}_proj.bias", (n * D,)) for x, n in
                                         (("q", cfg.heads), ("k", cfg.kv_heads), ("v", cfg.kv_heads))]).contiguous()
            if cfg.qk_norm:
                out["q_norm"] = req(p + "self_attn.q_norm.weight", (D,))
                out["k_norm"] = req(p + "self_attn.k_norm.weight", (D,))
            return out

        def proj(parts):
            """One projection from its checkpoint tensors ``[(name, N, K)]``, concatenated along N: the bf16
            weight, or an ops.Mxfp4Weight when the parts are stored pre-quantised."""
            packed = [sd[n + ".weight"].dtype == torch.uint8 for n, _, _ in parts]
            if not any(packed):
                return torch.cat([t(n + ".weight") for n, _, _ in parts]).contiguous()
            if not self.mxfp4:
                raise ValueError(f"{path}: {parts[0][0]}.weight is MXFP4-quantised; load it with mxfp4=True")
            if not all(packed):
                raise ValueError(f"{path}: {', '.join(n for n, _, _ in parts)} must all be MXFP4-quantised or none")
            qs, ss = [], []
            for n, N, K in parts:
                for name, shape in ((n + ".weight", (N, K // 2)), (n + ".weight_scale", (N, K // 32))):
                    if name not in sd:
                        raise ValueError(f"{path}: {cfg.name} needs {name}, which the checkpoint does not have")
                    if sd[name].dtype != torch.uint8 or tuple(sd[name].shape) != shape:
                        raise ValueError(f"{path}: {name} is {sd[name].dtype} {tuple(sd[name].shape)}, {cfg.name} "
                                         f"expects uint8 {shape}")
                if bool((sd[n + ".weight_scale"] == 255).any()):
                    raise ValueError(f"{path}: {n}.weight_scale holds the e8m0 byte 255 (NaN)")
                qs.append(sd[n + ".weight"].to(dev))
                ss.append(sd[n + ".weight_scale"].to(dev))
            return Mxfp4Weight.from_packed(torch.cat(qs), torch.cat(ss), parts[0][0])

        d, F_ = cfg.hidden, cfg.ffn
        self.embed = t("model.embed_tokens.weight")
        self.layers = []
        for i in range(self.cfg.layers):
            p = f"model.layers.{i}."
            self.layers.append(LayerWeights(
                **attn_extras(p),
                attn_norm=t(p + "input_layernorm.weight"),
                wqkv=proj([(p + f"self_attn.{x}_proj", n * D, d) for x, n in
                           (("q", cfg.heads), ("k", cfg.kv_heads), ("v", cfg.kv_heads))]),
                wo=proj([(p + "self_attn.o_proj", d, cfg.heads * D)]),
                mlp_norm=t(p + "post_attention_layernorm.weight"),
                w_gate_up=proj([(p + "mlp.gate_proj", F_, d), (p + "mlp.up_proj", F_, d)]),
                w_down=proj([(p + "mlp.down_proj", d, F_)]),
            ))
            if self.mxfp4:
                self._quantise_layer(self.layers[-1])
        self.final_norm = t("model.norm.weight")
        self.lm_head = t("lm_head.weight") if "lm_head.weight" in sd else self.embed

    # ------------------------------------------------------------------ forward
    def _residual_into(self, inp: torch.Tensor, w: torch.Tensor, x_res: torch.Tensor, mode: str) -> None:
        """x_res += inp . w^T, leaving the partial row sums of squares of the new x_res in ``self.chain`` per
        ``mode``: "own32" / "own64" — gemm4w's residual epilogue writes them (RS 2, schedule 32 / 64);
        "sumsq" — the planner's residual GEMM, then one rms_rowsumsq pass; "plain" — no partials (the next
        consumer normalises with the norm kernel)."""
        if mode in step_plan.OWN_VAR:
            ops.gemm4w(inp, w, residual=x_res, out=x_res, chain=self.chain, var=step_plan.OWN_VAR[mode])
            return
        gemm_plan.linear_add_(inp, w, x_res, ws=self.g8_ws)
        if mode == "sumsq":
            ops.rms_rowsumsq(x_res, self.chain)

    def _chain_layers(self, x_res: torch.Tensor, cache: KVCache, positions, slots, attn_fn, rope_q: bool,
                      plan: dict) -> torch.Tensor:
        """Decode layers + lm_head with the folded norms per ``plan`` (a :class:`ChainPlan` dict): at each norm
        point ("attn": qkv, "mlp": gate|up, "final": lm_head) either the consumer scales its rows from the chain's
        partials ("fold") or the norm kernel (weights ones: the norms are in the projections) runs first;
        the producers of folded points leave partials by the plan's live ``o`` / ``down`` mode.  Returns logits."""
        cfg, ch = self.cfg, self.chain
        T = x_res.shape[0]
        Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
        ones, eps = self.final_norm, cfg.rms_eps  # (every norm weight is ones after folding)
        p = ChainPlan.from_dict(plan).live()
        if p.attn:
            ops.rms_rowsumsq(x_res, ch)
        nl = len(self.layers)
        for li, L in enumerate(self.layers):
            if p.attn:
                qkv = ops.gemm4w(x_res, L.wqkv, bn=p.qkv_bn, chain=ch, var=p.qkv_var)
            else:
                qkv = self._proj(ops.rmsnorm(x_res, ones, eps), L.wqkv)
            self._rope_kv_write(qkv, L, positions, cache.k[li], cache.v[li], slots, rope_q)
            attn = attn_fn(qkv, li).reshape(T, Hq * D)
            self._residual_into(attn, L.wo, x_res, p.o)
            if p.mlp:
                act = ops.gemm4w(x_res, L.w_gate_up, swiglu=True, chain=ch, var=p.gu_var)
            else:
                act = gemm_plan.swiglu(ops.rmsnorm(x_res, ones, eps), L.w_gate_up, L.gu_block, ws=self.g8_ws)
            self._residual_into(act, L.w_down, x_res, p.down_mode(last=li + 1 == nl))
        if p.final:
            sk = ops.split_plan(T, self.lm_head.shape[0], cfg.hidden) if p.lm_split else (1, 0)
            return ops.gemm4w(x_res, self.lm_head, chain=ch, var=p.lm_var, splits=sk[0], split_from=sk[1])
        return self._proj(ops.rmsnorm(x_res, ones, eps), self.lm_head)

    def chain_ok(self, M: int) -> bool:
        """Whether a decode step of M rows folds at least one norm (timed faster at M, before capture)."""
        c = self.chain_m.get(M)
        return bool(c) and ChainPlan.from_dict(c).folds and self.chain is not None and M <= self.chain.max_rows

    def _layers(self, x_res: torch.Tensor, cache: KVCache, positions, slots, attn_fn, rope_q: bool = True,
                keep: Optional[torch.Tensor] = None, final_norm: Optional[torch.Tensor] = None,
                lora_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Runs every layer; x_res is the residual stream (updated in place); returns the final
        normalised hidden state.  ``rope_q=False``: q leaves the qkv projection un-rotated and ``attn_fn``
        rotates it (the decode kernels' load-time RoPE).  ``keep`` (row indices): only those rows' final
        states are wanted (a prefill's last tokens, an embedder's pooled token) — the last layer still runs
        qkv / RoPE / the cache write / attention over every row (later tokens' keys and values), then its
        o projection, MLP and the final norm over the kept rows only; returns [len(keep), d].  ``final_norm``:
        the weight of the last norm (default ``self.final_norm``; ones once it is folded into lm_head).
        ``lora_ids`` (int32 per row, -1 = none; models built with ``lora=``): each row's adapter is added to
        every projection it targets, after the base GEMM and in place (:meth:`_lora_add`)."""
        T, Hq, D = x_res.shape[0], self.cfg.heads, self.cfg.head_dim
        # Two seams carry every variant (the rest of the layer is one body):
        # how a projection joins the residual stream — the dense single-rank bf16 layers on the GPU add o / down
        # inside the GEMM (gemm_plan.linear_add_; then the adapters), so the norm that follows only reads x_res;
        # every other variant (fp8, MXFP4, CPU, and the subclasses that reduce the projection across ranks or
        # route it through experts in _attn_out / _mlp) hands the projection's output to the norm kernel, which
        # adds it (``residual=``) — and which norm runs (:meth:`_norm`)
        fused = self._dense_residual and self.on_gpu
        lo = self.lora if lora_ids is not None else None
        if lo is not None and not fused:
            raise RuntimeError("LoRA adapters need the dense fused-residual layer path")
        nl = len(self.layers)

        def add_norm(name, inp, separate, norm_w, feeds):
            if not fused:
                return self._norm(separate(inp, L), norm_w, feeds, residual=x_res)
            gemm_plan.linear_add_(inp, L.wo if name == "o" else L.w_down, x_res, ws=self.g8_ws)
            if lo is not None:
                self._lora_add(x_res, inp, li, name, lora_ids)
            return self._norm(x_res, norm_w, feeds)

        h = self._norm(x_res, self.layers[0].attn_norm, "attn")
        for li, L in enumerate(self.layers):
            last = li + 1 == nl
            qkv = self._proj(h, L.wqkv)
            if lo is not None:
                self._lora_add(qkv, h, li, "qkv", lora_ids)
            self._rope_kv_write(qkv, L, positions, cache.k[li], cache.v[li], slots, rope_q)
            attn = attn_fn(qkv, li)
            if keep is not None and last:
                attn = attn.index_select(keep) if isinstance(attn, ops.MXAct) else \
                    attn.reshape(T, Hq * D).index_select(0, keep)
                x_res = x_res.index_select(0, keep)
                T = x_res.shape[0]
                if lo is not None:
                    lora_ids = lora_ids.index_select(0, keep)
            if not isinstance(attn, ops.MXAct):
                attn = attn.view(T, Hq * D)
            h = add_norm("o", attn, self._attn_out, L.mlp_norm, "mlp")
            if not fused:
                act = h  # _mlp holds gate|up and down
            elif lo is not None and lo.adapts_gate_up:  # the adapters add to the pre-activation: no fused SwiGLU
                gu = self._proj(h, L.w_gate_up)
                self._lora_add(gu, h, li, "gate_up", lora_ids)
                act = ops.silu_mul(gu, block=L.gu_block)
            else:
                act = self._act(h, L)
            if last:  # the final norm feeds the bf16 lm_head / pooling
                nxt, feeds = self.final_norm if final_norm is None else final_norm, "out"
            else:
                nxt, feeds = self.layers[li + 1].attn_norm, "attn"
            h = add_norm("down", act, self._mlp, nxt, feeds)
        return h

    def _norm(self, x, w: torch.Tensor, feeds: str, **kw):
        """RMSNorm of ``x`` (+ ``residual=``, updated in place) for what it ``feeds``: "attn" / "mlp" — fp8
        projections: the norm also emits the per-row e4m3 activation (ops.QAct) in the same pass, so no separate
        quantisation kernel re-reads the normalised rows (the MLP's with its bf16 rows where ``_mlp_reads_bf16``);
        "out" — the bf16 lm_head / pooling, and every norm of the other weight formats: the bf16 kernel."""
        if self.act_format == "e4m3" and feeds != "out":
            # MXFP4 with e4m3 activations: from the W4A8 row threshold on, the consumer (qkv / gate|up) takes the
            # row-quantised activation; below it, the bf16 rows of the weight-only path
            L0 = self.layers[0]
            a8 = self._a8(x.shape[0], L0.wqkv) if feeds == "attn" else \
                self._a8(x.shape[0], L0.w_gate_up, swiglu=L0.gu_block == 32)
            if a8:
                return ops.rmsnorm_quant_fp8(x, w, self.cfg.rms_eps, **kw)
        if self.weight_format != "fp8" or feeds == "out":
            return ops.rmsnorm(x, w, self.cfg.rms_eps, **kw)
        if feeds == "mlp":
            kw["keep_bf16"] = self._mlp_reads_bf16
        return ops.rmsnorm_quant_fp8(x, w, self.cfg.rms_eps, **kw)

    def _rope_kv_write(self, qkv: torch.Tensor, L, positions, k_cache, v_cache, slots, rope_q: bool) -> None:
        """RoPE + the paged KV write of one layer, in place on ``qkv``: the Qwen kernel when the layer carries a
        q|k|v bias or q/k norm weights (added / applied in the same pass, before the rotation), else
        rope_kv_write.  q must leave here biased and normalised also on pure decode steps, where the attention
        kernels rotate it as they load it."""
        cfg = self.cfg
        bias, qn, kn = L.bqkv, L.q_norm, L.k_norm
        if bias is None and qn is None and kn is None:
            ops.rope_kv_write(qkv, positions, self.cos, self.sin, k_cache, v_cache, cfg.heads, cfg.kv_heads,
                              cfg.head_dim, slots=slots, rope_q=rope_q)
        else:
            ops.qknorm_rope_kv_write(qkv, positions, self.cos, self.sin, k_cache, v_cache, cfg.heads, cfg.kv_heads,
                                     cfg.head_dim, slots=slots, rope_q=rope_q, bias=bias, q_weight=qn, k_weight=kn,
                                     eps=cfg.rms_eps)

    def _lora_add(self, y: torch.Tensor, x: torch.Tensor, li: int, proj: str, ids: torch.Tensor) -> None:
        """y[m] += (x[m] . A[ids[m]]^T) . B[ids[m]]^T for layer ``li``'s projection ``proj`` (two launches,
        csrc/kernels/lora.hip); nothing for a projection no adapter of the set targets."""
        A = self.lora.A[li][proj]
        if A is None:
            return
        ops.lora_expand_add_(y, ops.lora_shrink(x, A, ids), self.lora.B[li][proj], ids)

    # whether _mlp reads the bf16 rows of its (fp8-quantised) input too (the MoE router does)
    _mlp_reads_bf16 = False

    def _attn_mx(self) -> bool:
        """Whether the attention kernels (decode cascade, prefill) hand the o projection an MX activation: fp8 o weights on gemm8g
        (head_dim 128, every head one 128-wide K slice); LWC_ATTN_MX=0 keeps bf16 + the row quantisation."""
        return (os.environ.get("LWC_ATTN_MX", "1") != "0" and self.weight_format == "fp8"
                and self.cfg.head_dim == 128 and ops.FP8_GEMM != "blas" and self.layers[0].wo.q.shape[0] % 8 == 0)

    def _a8(self, M: int, w, swiglu: bool = False) -> bool:
        """Whether a GEMM call of ``M`` rows over the MXFP4 weight ``w`` runs e4m3 activations on the block-scaled
        MFMA: the model's ``act_format``, the row threshold and the kernel's shape predicate — nothing timed."""
        if self.act_format != "e4m3" or M < ops.MXFP4_A8_MIN_ROWS or not isinstance(w, Mxfp4Weight):
            return False
        return ops.mxfp4_a8_ok(M, w.shape[0], w.shape[1], swiglu=swiglu)

    def _mx_no_scratch(self) -> bool:
        """Whether no call can reach the dequantise-into-scratch path: every projection of every layer is taken by
        skinny_mxfp4 below ops.MXFP4_A8_MIN_ROWS rows and by the W4A8 kernel from there on."""
        if self.act_format != "e4m3":
            return False
        lo, hi = ops.MXFP4_A8_MIN_ROWS - 1, ops.MXFP4_A8_MIN_ROWS

        def both(w, swiglu=False):
            N, K = w.shape
            return all(ops.skinny_mxfp4_ok(m, N, K, swiglu) for m in (1, lo)) and self._a8(hi, w, swiglu)

        return all(both(L.wqkv) and both(L.wo) and both(L.w_down) and L.gu_block == 32 and both(L.w_gate_up, True)
                   for L in self.layers)

    # the constructor's flags, as the engine and the tests read them
    fp8_dense = property(lambda self: self.weight_format == "fp8" and not self.moe)
    mxfp4 = property(lambda self: self.weight_format == "mxfp4")

    @property
    def _dense_residual(self) -> bool:
        """Whether o / down are plain bf16 projections this rank adds to the residual stream by itself."""
        return self.single_rank_dense and self.weight_format == "bf16"

    def _proj(self, x, w: torch.Tensor) -> torch.Tensor:
        """Dense projection on the per-shape backend (ops/gemm_plan.py: hipBLASLt, gemm4w or gemm8p); e4m3
        weights: row-quantised activations (an ops.QAct from the producing norm, or quantised here) into the
        fp8 GEMM (gemm8g dense or the library, ops.linear_fp8_q)."""
        if isinstance(w, ops.Fp8Weight):
            return ops.linear_fp8(x, w)
        if isinstance(w, Mxfp4Weight):
            if isinstance(x, ops.QAct) or self._a8(x.shape[0], w):  # e4m3 activations x the packed weight
                return ops.linear_mxfp4_a8(x, w)
            if self.mx_scratch is None:  # (_mx_no_scratch: every call below the W4A8 threshold is the weight stream)
                return ops.skinny_mxfp4(x.contiguous(), w)
            # M <= 64: the MXFP4 weight stream; above: dequantise + the bf16 path
            return ops.linear_mxfp4(x, w, self.mx_scratch, ws=self.g8_ws)
        if not self.on_gpu:
            return F.linear(x, w)
        return gemm_plan.linear(x, w, ws=self.g8_ws)

    def _attn_out(self, attn: torch.Tensor, L) -> torch.Tensor:
        """Output projection (row-parallel + all-reduce in tensor-parallel subclasses)."""
        return self._proj(attn, L.wo)

    def _mlp(self, h: torch.Tensor, L) -> torch.Tensor:
        """Dense SwiGLU MLP: gate|up GEMM with SwiGLU (fused in gemm8p's epilogue, or hipBLASLt + K5
        silu_mul), down GEMM.  fp8: gate|up fp8 GEMM, SwiGLU fused with the down projection's row
        quantisation (K11e), down fp8 GEMM."""
        if isinstance(L.w_down, ops.Fp8Weight):
            if ops.dense_mx_ok(h, L.w_gate_up, L.w_down, L.gu_block):
                # large batches (the embedder's prefill): the activation in MX form, no quantisation pass
                aq, amx = ops.linear_fp8_swiglu_mx(h, L.w_gate_up)
                return ops.linear_fp8_mx(aq, amx, L.w_down)
            aq, as_ = ops.linear_fp8_swiglu(h, L.w_gate_up, L.gu_block)
            return ops.linear_fp8_q(aq, as_, L.w_down)
        return self._proj(self._act(h, L), L.w_down)

    def _act(self, h: torch.Tensor, L) -> torch.Tensor:
        """silu(h Wg^T) * (h Wu^T): the gate|up GEMM with its SwiGLU."""
        if isinstance(L.w_gate_up, Mxfp4Weight):
            if isinstance(h, ops.QAct):  # (_norm emitted it: this call runs W4A8)
                return ops.swiglu_mxfp4_a8(h, L.w_gate_up, L.gu_block)
            if self.mx_scratch is None:
                return ops.skinny_mxfp4(h.contiguous(), L.w_gate_up, swiglu=True)
            return ops.swiglu_mxfp4(h, L.w_gate_up, L.gu_block, self.mx_scratch, ws=self.g8_ws)
        if not self.on_gpu:
            return ops.silu_mul(F.linear(h, L.w_gate_up), block=L.gu_block)
        return gemm_plan.swiglu(h, L.w_gate_up, L.gu_block, ws=self.g8_ws)

    def comm_arm(self) -> None:
        """Tensor-parallel subclasses queue the readback of their collective's error word here."""

    def comm_poll(self) -> None:
        """Tensor-parallel subclasses raise here once a failed collective is visible on the host."""

    @property
    def _planned_gemms(self) -> bool:
        """Whether the projections go through ops/gemm_plan.py (the dense bf16 decoder on the GPU)."""
        return self.on_gpu and not self.moe and self.weight_format == "bf16"

    def _chain_unusable(self, M: int) -> Optional[str]:
        """Why a decode step of M rows cannot fold norms, or None when it can; the NormChain is allocated here,
        once for every decode bucket (captured graphs keep its addresses)."""
        if not self._planned_gemms:
            return "this model runs no planned GEMMs"
        if not self.norm_folded:
            return "the model's norms are not folded"
        if self.chain is None:
            self.chain = ops.NormChain(max(M, 8192), self.cfg.hidden, self.cfg.rms_eps, self.device)
        if M > self.chain.max_rows:
            return f"the norm chain holds {self.chain.max_rows} rows"
        return None

    def tune_gemms(self, M: int, bucket: bool = False, lm_head: bool = True, only=None) -> None:
        """Pick the GEMM backend of every decode projection at batch M by timing both (before the
        bucket's hipGraph is captured; see ops/gemm_plan.py).  ``bucket``: M is a row-count bucket of the
        mixed chunked-prefill steps (their M varies step to step); ``lm_head``: tune the vocabulary
        projection too (mixed steps only project the decode rows and completed prompts' last tokens);
        ``only``: the epilogues to tune (e.g. ("swiglu",): the gate|up projection alone)."""
        if M in self.pinned and not bucket and only is None:
            self._apply_pinned(M)
            return
        if not self._planned_gemms:
            return
        cfg, L = self.cfg, self.layers[0]
        if only is not None:
            if "swiglu" in only:
                x = torch.randn(M, cfg.hidden, device=self.device).to(self.dtype)
                gemm_plan.tune(x, L.w_gate_up, "swiglu", L.gu_block, ws=self.g8_ws, bucket=bucket)
            return
        x = torch.randn(M, cfg.hidden, device=self.device).to(self.dtype)
        xa = torch.randn(M, cfg.heads * cfg.head_dim, device=self.device).to(self.dtype)
        xf = torch.randn(M, cfg.ffn, device=self.device).to(self.dtype)
        gemm_plan.tune(x, L.wqkv, ws=self.g8_ws, bucket=bucket)
        epi = "residual" if self._dense_residual else "plain"
        gemm_plan.tune(xa, L.wo, epi, ws=self.g8_ws, bucket=bucket)
        gemm_plan.tune(x, L.w_gate_up, "swiglu", L.gu_block, ws=self.g8_ws, bucket=bucket)
        gemm_plan.tune(xf, L.w_down, epi, ws=self.g8_ws, bucket=bucket)
        if lm_head:
            gemm_plan.tune(x, self.lm_head, ws=self.g8_ws, bucket=bucket)
        if self.norm_folded and not bucket and lm_head:
            self._tune_chain(M, x, xa, xf)

    def pin_step_plan(self, M: int, plan: dict) -> None:
        """Fix the decode step's plan at batch M (the form of :meth:`step_plans`' entries: ``choices`` per
        projection, ``chain`` for the folded norms; ValueError for a plan that does not parse):
        :meth:`tune_gemms` and the engine's in-step A/B then time nothing at M, so every run of the process
        executes the same kernels and computes the same values (timed choices flip between near-equal
        candidates from run to run)."""
        step_plan.check_plan(plan)
        self.pinned[M] = {"choices": dict(plan["choices"]), "chain": dict(plan["chain"]) if plan.get("chain") else None}

    def _apply_pinned(self, M: int) -> None:
        plan = self.pinned[M]
        if not self._planned_gemms:
            raise RuntimeError(f"a decode plan is pinned at batch {M}, but this model runs no planned GEMMs")
        if plan["chain"] is not None and ChainPlan.from_dict(plan["chain"]).folds:
            why = self._chain_unusable(M)
            if why is not None:
                raise RuntimeError(f"the plan pinned at batch {M} folds norms, but {why}")
        self.apply_step_plan(M, plan)

    def _tune_chain(self, M: int, x, xa, xf) -> None:
        """Decode batch M: decide, per norm point, between the norm kernel + the best projection backend and the
        folded norm (the consumer's row-scaled gemm4w, the producer leaving partial row sums of squares by its
        own residual epilogue or by one rms_rowsumsq pass after the planner's GEMM).  Every candidate
        (``step_plan.CHAIN_CANDIDATES``) is timed alone (interleaved rounds, median), the plan is the cheaper
        side at each point and is recorded in ``chain_m`` (``LWC_NORM_CHAIN=0|1`` forces all-unfolded /
        all-folded)."""
        if M in self.chain_m or torch.cuda.is_current_stream_capturing():
            return
        cfg, L = self.cfg, self.layers[0]
        # below 256 rows the chain's 256-row tiles run mostly empty and the weight-streaming cores win every
        # projection: not timed (a serving engine meets many such buckets)
        if (cfg.hidden + 255) // 256 > 16 or M < 256 or self._chain_unusable(M) is not None:
            self.chain_m[M] = ChainPlan.UNFOLDED.as_dict()
            return
        ch, eps = self.chain, cfg.rms_eps
        x_res = x.clone()
        ones = self.final_norm
        ops.rms_rowsumsq(x_res, ch)  # valid partials for the row-scaled candidates
        P0 = ch.P
        w = {"qkv": L.wqkv, "o": L.wo, "gu": L.w_gate_up, "down": L.w_down, "lm": self.lm_head}
        cands = step_plan.CHAIN_CANDIDATES
        lm_sk = ops.split_plan(M, self.lm_head.shape[0], cfg.hidden)  # lm_head's ragged last round, split

        def fold(name, **kw):
            def run():
                ch.P = P0
                ops.gemm4w(x, w[name], chain=ch, **kw)
            return run

        def own(name, inp):  # the producer's own epilogue at both schedules
            def res(var):
                return lambda: ops.gemm4w(inp, w[name], residual=x_res, out=x_res, chain=ch, var=var)
            return {c: res(step_plan.OWN_VAR[f[name]]) for c, f in cands[name].items()}

        runs = {
            "norm": lambda: ops.rmsnorm(x_res, ones, eps),
            "sumsq": lambda: ops.rms_rowsumsq(x_res, ch),
            "qkv": lambda: self._proj(x, L.wqkv),
            "o": lambda: gemm_plan.linear_add_(xa, L.wo, x_res, ws=self.g8_ws), **own("o", xa),
            "gu": lambda: gemm_plan.swiglu(x, L.w_gate_up, L.gu_block, ws=self.g8_ws),
            "down": lambda: gemm_plan.linear_add_(xf, L.w_down, x_res, ws=self.g8_ws), **own("down", xf),
            "lm": lambda: self._proj(x, self.lm_head),
        }
        # the row-scaled consumers at both schedules (VAR 32: block-staged epilogue; 64: wave-local, next tile
        # prefetched), for qkv both tile widths, for lm_head the split tail where there is one
        for pt in ("qkv", "gu", "lm"):
            for c, f in cands[pt].items():
                if f.get("lm_split"):
                    if lm_sk[0] > 1:
                        runs[c] = fold(pt, bn=256, var=f["lm_var"], splits=lm_sk[0], split_from=lm_sk[1])
                else:
                    runs[c] = fold(pt, bn=f.get("qkv_bn", 256), var=f[f"{pt}_var"], swiglu=pt == "gu")
        ts = {k: [] for k in runs}
        for _ in range(3):  # interleaved rounds (one process, one device: matched clocks and caches)
            for k, fn in runs.items():
                ts[k].append(gemm_plan._time(fn, iters=3, rounds=1))
        t = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        ch.P = P0

        def producer(name):  # the cheapest way to leave partials, and its cost over the plain residual GEMM
            # (isolated timings; the engine's in-step A/B of whole captured decode steps then decides between
            # this plan, the all-library one and the all-own one: LlamaModel.step_plans)
            costs = step_plan.producer_costs(name, t)
            best = min(costs, key=costs.get)
            return best, costs[best] - t[name]

        o_mode, o_extra = producer("o")
        d_mode, d_extra = producer("down")
        qk, gk, lk = (step_plan.fastest_candidate(pt, t) for pt in ("qkv", "gu", "lm"))
        # each point: folded (consumer + producer's extra) vs the norm kernel + the consumer's best backend
        attn = t[qk] + d_extra < t["norm"] + t["qkv"]
        mlp = t[gk] + o_extra < t["norm"] + t["gu"]
        final = t[lk] + d_extra < t["norm"] + t["lm"]
        force = os.environ.get("LWC_NORM_CHAIN")
        if force is not None:
            attn = mlp = final = force == "1"
        plan = ChainPlan(attn=attn, mlp=mlp, final=final, **cands["qkv"][qk], **cands["gu"][gk], **cands["lm"][lk],
                         o=o_mode, down=d_mode).as_dict()
        self.chain_m[M] = plan
        key = (M, cfg.hidden, 0, "norm_chain")
        gemm_plan.TIMINGS[key] = t
        gemm_plan._CHOICE[key] = ",".join(f"{k}={v}" for k, v in plan.items())

    # ------------------------------------------------------------------ whole-step plans (engine in-step A/B)
    # (thin wrappers: the planner's recorded state goes in, models/step_plan.py decides)
    def _plan_keys(self, M: int) -> dict:
        cfg = self.cfg
        epi = "residual" if self._dense_residual else "plain"
        return {"qkv": (M, cfg.qkv_dim, cfg.hidden, "plain"), "o": (M, cfg.hidden, cfg.heads * cfg.head_dim, epi),
                "gu": (M, 2 * cfg.ffn, cfg.hidden, "swiglu"), "down": (M, cfg.hidden, cfg.ffn, epi),
                "lm": (M, cfg.vocab_size, cfg.hidden, "plain")}

    def _own_backends(self, M: int) -> dict:
        """Each projection's fastest hand-written backend by the planner's timings at M (None: none timed)."""
        own = {}
        for n, k in self._plan_keys(M).items():
            t = {b: v for b, v in gemm_plan.TIMINGS.get(k, {}).items() if b != "blas" and isinstance(v, float)}
            own[n] = min(t, key=t.get) if t else None
        return own

    def _chain_timings(self, M: int) -> Optional[dict]:
        return gemm_plan.TIMINGS.get((M, self.cfg.hidden, 0, "norm_chain"))

    def step_plans(self, M: int) -> dict:
        """Candidate plans for a decode step of M rows, for the engine's in-step A/B (it captures the decode
        graph under each and times replays: isolated per-GEMM timings misjudge the step's clock and cache
        state, ``profiles/gemm4w_stamps_r5.md``).  ``planner``: the per-shape and norm-chain choices of
        :meth:`tune_gemms`; ``library``: every projection on hipBLASLt, no folded norm; ``own``: every
        projection on its fastest hand-written core with the whole norm chain folded.  {} when nothing was
        tuned at M."""
        keys = self._plan_keys(M)
        if not self.on_gpu or not any(k in gemm_plan._CHOICE for k in keys.values()):
            return {}
        return step_plan.step_plans({n: gemm_plan._CHOICE.get(k) for n, k in keys.items()}, self._own_backends(M),
                                    self.chain_m.get(M), self._chain_timings(M))

    def step_moves(self, M: int, plan: dict) -> list:
        """Single-decision changes of ``plan`` (the engine's coordinate-descent A/B, after the whole-plan
        round): each projection's backend (hipBLASLt <-> its fastest hand-written core) where the norm chain
        does not own it, each norm point folded or not, the consumers' schedule / tile width, the producers'
        mode.  [(label, delta)]: ``with_move(plan, delta)`` applies one."""
        usable = self.chain is not None and M <= self.chain.max_rows
        return step_plan.step_moves(plan, self._own_backends(M), usable, self._chain_timings(M))

    with_move = staticmethod(step_plan.with_move)

    def apply_step_plan(self, M: int, plan: dict) -> None:
        """Make ``plan`` (one of :meth:`step_plans`) the choice of every projection at M (and of the norm chain)."""
        step_plan.check_plan(plan)
        keys = self._plan_keys(M)
        for n, c in plan["choices"].items():
            if c is not None:
                gemm_plan._CHOICE[keys[n]] = c
        if plan.get("chain") is not None:
            self.chain_m[M] = dict(plan["chain"])

    def plan_summary(self, M: int) -> dict:
        """The kernels a decode step of M rows runs, compactly (bench JSON / logs)."""
        backends = {n: gemm_plan._CHOICE.get(k, "blas") for n, k in self._plan_keys(M).items()}
        return step_plan.plan_summary(backends, ChainPlan.from_dict(self.chain_m[M]) if self.chain_ok(M) else None)

    def decode(self, tokens: torch.Tensor, positions: torch.Tensor, slots: torch.Tensor, block_tables: torch.Tensor,
               ctx_lens: torch.Tensor, cache: KVCache, num_splits: int = 1,
               cascade_tiles: Optional[torch.Tensor] = None, lora_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One decode step for B sequences -> logits [B, V] bf16.  All inputs are device tensors
        (int32), so the whole call can be captured in a hipGraph.  Attention: ``cascade_tiles`` [T, 3] —
        the one-launch cascade kernel (shared prompt blocks read once per super-tile; the engine's
        large-batch path); otherwise split-K paged decode."""
        cfg = self.cfg
        x = ops.embedding(self.embed, tokens)
        B = tokens.shape[0]
        # q is rotated inside the attention kernels as they load it (rope_kv_write rotates and caches k
        # only): q's round trip through HBM in rope_kv_write (2/3 of its bytes at GQA 4) is gone.
        # LWC_DECODE_QROPE=0: the previous split (rope_kv_write rotates q in place), an A/B knob
        q_at_load = os.environ.get("LWC_DECODE_QROPE", "1") != "0"
        rope = (self.cos, self.sin, positions) if q_at_load else None
        if cascade_tiles is not None:
            # fp8 o projection (config 5): the attention output leaves the kernel in MX form (ops.MXAct)
            mx = self._attn_mx()

            def attn_fn(qkv, li):
                return ops.paged_decode_cascade(qkv, cache.k[li], cache.v[li], block_tables, ctx_lens, cascade_tiles,
                                                cfg.heads, self.scale, rope=rope, mx=mx)
        else:
            part_o = part_lse = None
            if num_splits > 1:
                part_o = torch.empty(B * cfg.heads * num_splits * cfg.head_dim, dtype=torch.float32, device=x.device)
                part_lse = torch.empty(B * cfg.heads * num_splits, dtype=torch.float32, device=x.device)

            def attn_fn(qkv, li):
                return ops.paged_decode(qkv, cache.k[li], cache.v[li], block_tables, ctx_lens, cfg.heads, self.scale,
                                        num_splits=num_splits, part_o=part_o, part_lse=part_lse, rope=rope)

        if self.chain_ok(B):
            return self._chain_layers(x, cache, positions, slots, attn_fn, not q_at_load, self.chain_m[B])
        h = self._layers(x, cache, positions, slots, attn_fn, rope_q=not q_at_load, lora_ids=lora_ids)
        return self._proj(h, self.lm_head)

    def encode(self, tokens: torch.Tensor, positions: torch.Tensor, cu_seqlens: torch.Tensor,
               max_seqlen: int, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Cache-less causal forward of packed sequences -> final-normed hidden states [T, d] (decoder used
        as an embedder, e.g. e5-mistral: the caller pools the last token).  RoPE runs without a cache
        write (slots=None), attention is the varlen prefill kernel over the fresh k/v."""
        cfg = self.cfg
        Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
        null = _NullCache(cfg, self.device)
        x = ops.embedding(self.embed, tokens)

        mx = self._attn_mx()  # fp8 o projection: the attention epilogue writes its MX operand

        def attn_fn(qkv, li):
            q, k, v = qkv[:, : Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
            if mx:
                return ops.prefill_attention_mx(q, k, v, cu_seqlens, max_seqlen, Hq, Hkv, self.scale, causal=True)
            return ops.prefill_attention(q, k, v, cu_seqlens, max_seqlen, Hq, Hkv, D, self.scale, causal=True)

        # the hidden states themselves are the output: the real final norm weight, also when it is folded
        # into lm_head for decoding
        return self._layers(x, null, positions, None, attn_fn, keep=keep,
                            final_norm=self.final_norm_weight)

    def prefill(self, tokens: torch.Tensor, positions: torch.Tensor, slots: torch.Tensor, cu_seqlens: torch.Tensor,
                max_seqlen: int, last_idx: torch.Tensor, cache: KVCache, ctx: Optional[dict] = None,
                lora_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Prefill packed prompts (cu_seqlens) -> logits of each sequence's last token [nseq, V].

        ``ctx`` (cross-request prefix cache): the packed tokens are only each prompt's UNCACHED tail and
        attention also needs the cached head.  ctx = {k_slots [sum klen] int64: cache slots of every
        position of each prompt (cached + new), cu_k [nseq+1] int32, q_lens, k_lens (host lists)}; per
        layer, after the new rows are written, the whole key range is gathered from the paged cache and
        the varlen kernel runs with queries at the end of each key range."""
        cfg = self.cfg
        Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
        x = ops.embedding(self.embed, tokens)
        mx = self._attn_mx()  # fp8 o projection: the attention epilogue writes its MX operand

        def attn_fn(qkv, li):
            q = qkv[:, : Hq * D]
            if ctx is not None:
                kf, vf = ops.kv_gather(cache.k[li], cache.v[li], ctx["k_slots"])
                return ops.prefill_attention(q, kf, vf, cu_seqlens, max_seqlen, Hq, Hkv, D, self.scale, causal=True,
                                             cu_seqlens_k=ctx["cu_k"], lens=(ctx["q_lens"], ctx["k_lens"]))
            k = qkv[:, Hq * D:(Hq + Hkv) * D]
            v = qkv[:, (Hq + Hkv) * D:]
            if mx:
                return ops.prefill_attention_mx(q, k, v, cu_seqlens, max_seqlen, Hq, Hkv, self.scale, causal=True)
            return ops.prefill_attention(q, k, v, cu_seqlens, max_seqlen, Hq, Hkv, D, self.scale, causal=True)

        # last layer: o / MLP on these rows
        h = self._layers(x, cache, positions, slots, attn_fn, keep=last_idx, lora_ids=lora_ids)
        return F.linear(h, self.lm_head)

    def forward_mixed(self, tokens: torch.Tensor, positions: torch.Tensor, slots: torch.Tensor, cache: KVCache,
                      n_dec: int, dec: Optional[dict], chunk: dict, logit_rows: torch.Tensor,
                      lora_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ONE forward over [n_dec decode rows || prompt-chunk rows] (mixed chunked prefill): every projection
        is one GEMM over both; per layer the decode rows go to the paged decode kernel (``dec``: block_tables,
        ctx_lens and either cascade ``tiles`` or ``splits``) and the chunk rows to the paged-KV prefill kernel
        (``chunk``: cu_q, block_tables, k_lens device tensors, max_q, host lens) — earlier chunks of a prompt
        are read straight from the paged cache.  Returns logits of ``logit_rows`` [R, V]."""
        cfg = self.cfg
        Hq, D = cfg.heads, cfg.head_dim
        x = ops.embedding(self.embed, tokens)
        T = tokens.shape[0]
        part_o = part_lse = None
        splits = 1 if dec is None else int(dec.get("splits", 1))
        if n_dec and "tiles" not in dec and splits > 1:
            part_o = torch.empty(n_dec * Hq * splits * D, dtype=torch.float32, device=x.device)
            part_lse = torch.empty(n_dec * Hq * splits, dtype=torch.float32, device=x.device)

        def attn_fn(qkv, li):
            out = torch.empty(T, Hq * D, dtype=qkv.dtype, device=qkv.device)
            if n_dec:
                o = out[:n_dec].view(n_dec, Hq, D)
                if "tiles" in dec:
                    ops.paged_decode_cascade(qkv[:n_dec], cache.k[li], cache.v[li], dec["block_tables"],
                                             dec["ctx_lens"], dec["tiles"], Hq, self.scale, out=o)
                else:
                    ops.paged_decode(qkv[:n_dec], cache.k[li], cache.v[li], dec["block_tables"], dec["ctx_lens"], Hq,
                                     self.scale, num_splits=splits, out=o, part_o=part_o, part_lse=part_lse)
            ops.prefill_attention_paged(qkv[n_dec:], cache.k[li], cache.v[li], chunk["cu_q"], chunk["block_tables"],
                                        chunk["k_lens"], chunk["max_q"], Hq, self.scale, out=out[n_dec:],
                                        lens=chunk.get("lens") if li == 0 else None)
            return out

        h = self._layers(x, cache, positions, slots, attn_fn, lora_ids=lora_ids)
        return self._proj(h.index_select(0, logit_rows), self.lm_head)
