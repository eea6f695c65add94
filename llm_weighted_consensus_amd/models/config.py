"""Model architecture configs (public shapes, random-init or safetensors weights).

Shapes come from the public model configs named in SURVEY.md §2.3 (not from the reference, which
runs no model): Llama-3-8B, Mixtral-8x7B, Mistral-7B/e5-mistral-7b and the bge-* BERT encoders.
Small variants exist for tests.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional


@dataclass(frozen=True)
class DecoderConfig:
    name: str
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    kv_heads: int
    head_dim: int
    ffn: int
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    max_position: int = 8192
    # llama-3 style rope scaling (factor, low_freq_factor, high_freq_factor, original_max_position)
    rope_scaling: Optional[tuple] = None
    # mixture of experts (Mixtral): experts per layer and experts per token; 0 = dense
    num_experts: int = 0
    experts_per_token: int = 0
    tie_embeddings: bool = False
    bos_token_id: Optional[int] = 1  # None: the tokenizer prepends nothing (Qwen)
    eos_token_id: int = 2
    # Qwen attention block: a bias on the q|k|v projections (Qwen2 / Qwen2.5); an RMSNorm over each q and k
    # head's head_dim values, one weight shared by all heads, before the rotation (Qwen3)
    qkv_bias: bool = False
    qk_norm: bool = False

    @property
    def qkv_dim(self) -> int:
        return (self.heads + 2 * self.kv_heads) * self.head_dim

    def params(self) -> int:
        d, f = self.hidden, self.ffn
        attn = d * self.qkv_dim + self.heads * self.head_dim * d
        attn += (self.qkv_dim if self.qkv_bias else 0) + (2 * self.head_dim if self.qk_norm else 0)
        mlp = 3 * d * f * max(1, self.num_experts) + (d * self.num_experts if self.num_experts else 0)
        emb = self.vocab_size * d * (1 if self.tie_embeddings else 2)
        return self.layers * (attn + mlp + 2 * d) + emb + d


def check_decoder(cfg: DecoderConfig) -> None:
    """Refuse, by name, a decoder shape the kernels do not serve (models call this before building anything).

    Decode attention takes head_dim 64 or 128 and any whole GQA group up to 16.  The fused Qwen attention-block
    pass (bias / per-head QK RMSNorm, csrc/kernels/qknorm.hip) exists for head_dim 128 only."""
    if cfg.head_dim not in (64, 128):
        raise ValueError(f"{cfg.name}: head_dim {cfg.head_dim}: decode attention takes 64 or 128")
    if cfg.kv_heads <= 0 or cfg.heads % cfg.kv_heads or cfg.heads // cfg.kv_heads > 16:
        raise ValueError(f"{cfg.name}: {cfg.heads} heads / {cfg.kv_heads} kv heads: decode attention takes whole "
                         "GQA groups up to 16")
    if cfg.head_dim != 128 and (cfg.qkv_bias or cfg.qk_norm):
        what = " and ".join(n for n, on in (("qkv_bias", cfg.qkv_bias), ("qk_norm", cfg.qk_norm)) if on)
        raise ValueError(f"{cfg.name}: {what} at head_dim {cfg.head_dim}: the Qwen attention block is served at "
                         "head_dim 128 only")


# activation formats of the MXFP4 projections: "bf16" (weight-only) or "e4m3" (W4A8 from ops.MXFP4_A8_MIN_ROWS rows)
MXFP4_ACTS = ("bf16", "e4m3")


# formats of a MoE decoder's expert weights: "bf16" (or e4m3 with "fp8") or "mxfp4" (weight-only, ops.Mxfp4Experts)
EXPERT_WEIGHTS = ("bf16", "mxfp4")


# activation formats of MXFP4 experts: "bf16" (weight-only) or "e4m3" (W4A8 past the weight stream's row limit,
# ops.moe_gemm_mxfp4_a8)
EXPERT_ACTS = ("bf16", "e4m3")


def check_variant(cfg: Optional[DecoderConfig], *, tp: bool = False, fp8: bool = False, mxfp4: bool = False,
                  adapters: bool = False, embedder: bool = False, device_type: Optional[str] = None,
                  who: str = "", mxfp4_act: Optional[str] = None, expert_weights: Optional[str] = None,
                  ep: bool = False, expert_act: Optional[str] = None) -> None:
    """Refuse the decoder variants that do not combine (the model constructors, ``lora.check_model_spec`` and
    the embedding service all call this with the facts they know; ``cfg`` None: an arch not registered).

    MXFP4 weight-only projections (ops/mxfp4.py) and LoRA adapters (models/lora.py) each run on the dense
    single-GPU generation decoder only, not with fp8 weights and not with each other; the adapters on the GPU
    kernels only (``device_type``, where the caller has a device).  ``who`` prefixes the message.

    ``mxfp4_act`` (None: not given): the activation format of the MXFP4 projections, one of ``MXFP4_ACTS`` and only
    together with mxfp4 weights; whatever mxfp4 weights refuse is refused first, in the same words.

    ``expert_weights`` (None: not given): the format of a MoE decoder's expert weights, one of ``EXPERT_WEIGHTS``.
    "mxfp4" (ops.Mxfp4Experts, csrc/kernels/moe_mxfp4.hip) runs on one device (no ``tp``, no ``ep``: expert
    parallelism), not with fp8 weights, adapters or as an embedder; the key is refused on a dense arch.  The dense
    ``mxfp4`` flag stays refused on MoE decoders, in the words it always had.

    ``expert_act`` (None: not given): the activation format of MXFP4 experts, one of ``EXPERT_ACTS`` and only
    together with ``expert_weights`` "mxfp4"; whatever ``expert_weights`` refuses is refused first, in the same
    words."""
    moe = cfg is not None and bool(cfg.num_experts)
    if expert_weights is not None:
        # the experts' format (None: not given): "mxfp4" holds a MoE decoder's expert projections as MXFP4,
        # weight-only, on one device and without fp8 weights or adapters; the key means nothing on a dense arch
        why = None
        if expert_weights not in EXPERT_WEIGHTS:
            why = f"expert_weights {expert_weights!r}: must be one of {', '.join(repr(a) for a in EXPERT_WEIGHTS)}"
        elif embedder and expert_weights == "mxfp4":
            why = "mxfp4 expert weights are served on generation models only"
        elif not moe:
            why = ("expert_weights applies to MoE decoders only"
                   + (f" ({cfg.name} is dense)" if cfg is not None else ""))
        elif expert_weights == "mxfp4":
            if fp8:
                why = "mxfp4 expert weights do not combine with fp8 weights"
            elif tp:
                why = ("mxfp4 expert weights do not combine with "
                       f"{'tp > 1' if who else 'tensor parallelism (tp > 1)'}")
            elif ep:
                why = "mxfp4 expert weights do not combine with expert parallelism (ep > 1)"
            elif adapters:
                why = "mxfp4 expert weights do not combine with LoRA adapters"
        if why is not None:
            raise ValueError(f"{who}: {why}" if who else why)
    if expert_act is not None:
        why = None
        if expert_weights != "mxfp4":
            why = ("\"expert_act\" needs \"expert_weights\": \"mxfp4\"" if who
                   else "expert_act needs expert_weights=\"mxfp4\"")
        elif expert_act not in EXPERT_ACTS:
            why = f"expert_act {expert_act!r}: must be one of {', '.join(repr(a) for a in EXPERT_ACTS)}"
        if why is not None:
            raise ValueError(f"{who}: {why}" if who else why)
    if mxfp4_act is not None and not mxfp4:
        why = "\"mxfp4_act\" needs \"mxfp4\": true" if who else "mxfp4_act needs mxfp4=True"
        raise ValueError(f"{who}: {why}" if who else why)
    for on, what in ((mxfp4, "mxfp4 weights"), (adapters, "LoRA adapters")):
        if not on:
            continue
        why = None
        if embedder:
            why = f"{what} are served on generation models only"
        elif fp8:
            why = f"{what} do not combine with fp8 weights"
        elif tp:
            # (a spec, which has a ``who``, is told by its own key)
            why = f"{what} do not combine with {'tp > 1' if who else 'tensor parallelism (tp > 1)'}"
        elif mxfp4 and adapters:
            why = "mxfp4 weights do not combine with LoRA adapters"
        elif moe:
            why = f"{what} are not supported on MoE decoders ({cfg.name})"
        elif adapters and device_type is not None and device_type != "cuda":
            why = "LoRA adapters run on the GPU kernels only"
        if why is not None:
            raise ValueError(f"{who}: {why}" if who else why)
    if moe and cfg.qk_norm and (tp or embedder):
        # Qwen3-MoE (models/qwen_moe.py): one device, generation only
        why = f"{cfg.name} {'is served as a generation model only' if embedder else 'runs on one device: no tp > 1'}"
        raise ValueError(f"{who}: {why}" if who else why)
    if mxfp4_act is not None and mxfp4_act not in MXFP4_ACTS:
        why = f"mxfp4_act {mxfp4_act!r}: must be one of {', '.join(repr(a) for a in MXFP4_ACTS)}"
        raise ValueError(f"{who}: {why}" if who else why)


@dataclass(frozen=True)
class EncoderConfig:
    name: str
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    ffn: int
    max_position: int = 512
    type_vocab: int = 2
    ln_eps: float = 1e-12
    pooling: str = "cls"  # cls | mean | last

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads


DECODERS = {
    "llama-3-8b": DecoderConfig("llama-3-8b", 128256, 4096, 32, 32, 8, 128, 14336, rope_theta=500000.0,
                                rms_eps=1e-5, max_position=8192, rope_scaling=(8.0, 1.0, 4.0, 8192),
                                bos_token_id=128000, eos_token_id=128001),
    "mistral-7b": DecoderConfig("mistral-7b", 32000, 4096, 32, 32, 8, 128, 14336, rope_theta=10000.0, rms_eps=1e-5,
                                max_position=32768),
    "mixtral-8x7b": DecoderConfig("mixtral-8x7b", 32000, 4096, 32, 32, 8, 128, 14336, rope_theta=1e6, rms_eps=1e-5,
                                  max_position=32768, num_experts=8, experts_per_token=2),
    # e5-mistral-7b-instruct: Mistral-7B decoder used as an embedder (last-token pooling, 4096-d)
    "e5-mistral-7b": DecoderConfig("e5-mistral-7b", 32000, 4096, 32, 32, 8, 128, 14336, rope_theta=10000.0,
                                   rms_eps=1e-5, max_position=32768),
    # Llama-3.2 text models (tied embeddings; 1B: head_dim 64, 3B: a GQA group of 3).  These shapes, and the
    # Qwen ones added with them below, are written from memory of the public config.json files and could not be
    # checked against them when they were added; a checkpoint whose tensors disagree is refused at load.
    "llama-3.2-1b": DecoderConfig("llama-3.2-1b", 128256, 2048, 16, 32, 8, 64, 8192, rope_theta=500000.0,
                                  rms_eps=1e-5, max_position=131072, rope_scaling=(32.0, 1.0, 4.0, 8192),
                                  tie_embeddings=True, bos_token_id=128000, eos_token_id=128001),
    "llama-3.2-3b": DecoderConfig("llama-3.2-3b", 128256, 3072, 28, 24, 8, 128, 8192, rope_theta=500000.0,
                                  rms_eps=1e-5, max_position=131072, rope_scaling=(32.0, 1.0, 4.0, 8192),
                                  tie_embeddings=True, bos_token_id=128000, eos_token_id=128001),
    # tests / smoke: same code paths, tiny sizes
    "llama-hd64-tiny": DecoderConfig("llama-hd64-tiny", 4096, 512, 2, 8, 2, 64, 1024, rope_theta=500000.0,
                                     max_position=2048, bos_token_id=1, eos_token_id=2),
    "llama-g3-tiny": DecoderConfig("llama-g3-tiny", 4096, 512, 2, 6, 2, 128, 1024, rope_theta=500000.0,
                                   max_position=2048, bos_token_id=1, eos_token_id=2),
    "llama-tiny": DecoderConfig("llama-tiny", 4096, 512, 2, 8, 2, 128, 1024, rope_theta=500000.0, max_position=2048,
                                bos_token_id=1, eos_token_id=2),
    "mixtral-tiny": DecoderConfig("mixtral-tiny", 4096, 512, 2, 8, 2, 128, 512, rope_theta=1e6, max_position=2048,
                                  num_experts=4, experts_per_token=2),
}


def _qwen(name: str, vocab: int, hidden: int, layers: int, heads: int, kv_heads: int, ffn: int, tie: bool,
          **flags) -> DecoderConfig:
    return DecoderConfig(name, vocab, hidden, layers, heads, kv_heads, 128, ffn, rope_theta=1e6, rms_eps=1e-6,
                         max_position=32768, tie_embeddings=tie, bos_token_id=None, eos_token_id=151645, **flags)


# Qwen3 (per-head q/k RMSNorm) and Qwen2.5 (q|k|v bias) at head_dim 128, with any GQA group up to 16 (the decode
# attention kernels take groups that do not divide 16: 5, 6 and 7 here).  Qwen2.5-0.5B (head_dim 64 with a
# bias) is not registered: the fused bias / QK-norm pass exists for head_dim 128 only (check_decoder).  The
# 1.5b / 7b / 14b / 32b and qwen3-14b rows are from memory of the public configs (see the Llama-3.2 note above).
DECODERS.update({
    "qwen3-0.6b": _qwen("qwen3-0.6b", 151936, 1024, 28, 16, 8, 3072, True, qk_norm=True),
    "qwen3-4b": _qwen("qwen3-4b", 151936, 2560, 36, 32, 8, 9728, True, qk_norm=True),
    "qwen3-8b": _qwen("qwen3-8b", 151936, 4096, 36, 32, 8, 12288, False, qk_norm=True),
    "qwen3-32b": _qwen("qwen3-32b", 151936, 5120, 64, 64, 8, 25600, False, qk_norm=True),
    "qwen3-14b": _qwen("qwen3-14b", 151936, 5120, 40, 40, 8, 17408, False, qk_norm=True),
    "qwen2.5-1.5b": _qwen("qwen2.5-1.5b", 151936, 1536, 28, 12, 2, 8960, True, qkv_bias=True),
    "qwen2.5-7b": _qwen("qwen2.5-7b", 152064, 3584, 28, 28, 4, 18944, False, qkv_bias=True),
    "qwen2.5-14b": _qwen("qwen2.5-14b", 152064, 5120, 48, 40, 8, 13824, False, qkv_bias=True),
    "qwen2.5-32b": _qwen("qwen2.5-32b", 152064, 5120, 64, 40, 8, 27648, False, qkv_bias=True),
    "qwen2.5-3b": _qwen("qwen2.5-3b", 151936, 2048, 36, 16, 2, 11008, True, qkv_bias=True),
    "qwen2.5-72b": _qwen("qwen2.5-72b", 152064, 8192, 80, 64, 8, 29568, False, qkv_bias=True),
    # tests: the two attention-block variants at llama-tiny sizes
    "qwen3-tiny": replace(_qwen("qwen3-tiny", 4096, 512, 2, 8, 2, 1024, True, qk_norm=True), max_position=2048,
                          eos_token_id=2),
    "qwen2-tiny": replace(_qwen("qwen2-tiny", 4096, 512, 2, 8, 2, 1024, False, qkv_bias=True), max_position=2048,
                          eos_token_id=2),
    # ... and at GQA groups that do not divide 16 (heads * head_dim != hidden, as in Qwen3)
    "qwen2-g7-tiny": replace(_qwen("qwen2-g7-tiny", 4096, 512, 2, 14, 2, 1024, False, qkv_bias=True),
                             max_position=2048, eos_token_id=2),
    "qwen3-g5-tiny": replace(_qwen("qwen3-g5-tiny", 4096, 512, 2, 10, 2, 1024, True, qk_norm=True),
                             max_position=2048, eos_token_id=2),
})

# Qwen3-MoE (models/qwen_moe.py): ``ffn`` is the per-expert moe_intermediate_size; 128 experts, 8 per token, the
# Qwen3 attention block.  qwen3-30b-a3b is from memory of the public config (see the Llama-3.2 note above).  The
# tiny arch keeps 128 experts and top-8 (the wide router's shape) at an ffn of 3 x 128, no power of two, as 768.
DECODERS.update({
    "qwen3-30b-a3b": replace(_qwen("qwen3-30b-a3b", 151936, 2048, 48, 32, 4, 768, False, qk_norm=True),
                             max_position=40960, num_experts=128, experts_per_token=8),
    "qwen3-moe-tiny": replace(_qwen("qwen3-moe-tiny", 4096, 512, 2, 8, 2, 384, False, qk_norm=True),
                              max_position=2048, eos_token_id=2, num_experts=128, experts_per_token=8),
})

ENCODERS = {
    "bge-small-en-v1.5": EncoderConfig("bge-small-en-v1.5", 30522, 384, 12, 12, 1536),
    "bge-base-en-v1.5": EncoderConfig("bge-base-en-v1.5", 30522, 768, 12, 12, 3072),
    "bge-large-en-v1.5": EncoderConfig("bge-large-en-v1.5", 30522, 1024, 24, 16, 4096),
    "bert-tiny": EncoderConfig("bert-tiny", 30522, 256, 2, 4, 1024),
}


def decoder_config(name: str, **overrides) -> DecoderConfig:
    cfg = DECODERS[name]
    return replace(cfg, **overrides) if overrides else cfg


def encoder_config(name: str, **overrides) -> EncoderConfig:
    key = name.split("/")[-1].lower()
    if key.startswith("bge-") and not key.endswith("-v1.5") and key + "-en-v1.5" in ENCODERS:
        key = key + "-en-v1.5"
    cfg = ENCODERS[key]
    return replace(cfg, **overrides) if overrides else cfg
