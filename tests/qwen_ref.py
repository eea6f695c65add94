"""fp32 reference forward of the Qwen decoders: ``torch_ref.llama_forward`` with the q|k|v projection bias
(Qwen2 / Qwen2.5) and the per-head q / k RMSNorm (Qwen3) between the projection and the rotation.  Each of the
two steps can be switched off, to measure what dropping it would cost."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import torch_ref as ref


def qwen_forward(model, tokens, hidden_only=False, use_bias=True, use_qk_norm=True):
    """Full-sequence fp32 forward of a dense models.llama.LlamaModel (single sequence) -> logits [T, V]
    (``hidden_only``: the final normed hidden states [T, d]).  ``final_norm_weight`` is used where the model
    folded its final norm into lm_head."""
    cfg = model.cfg
    T = tokens.shape[0]
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    pos = torch.arange(T, device=tokens.device)
    x = model.embed[tokens.long()].float()
    for L in model.layers:
        h = ref.rmsnorm(x, L.attn_norm, cfg.rms_eps)
        qkv = h @ ref.dense(L.wqkv).t()
        if use_bias and L.bqkv is not None:
            qkv = qkv + L.bqkv.float()
        q = qkv[:, : Hq * D].view(T, Hq, D)
        k = qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
        v = qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)
        if use_qk_norm and L.q_norm is not None:
            q = ref.rmsnorm(q, L.q_norm, cfg.rms_eps)
        if use_qk_norm and L.k_norm is not None:
            k = ref.rmsnorm(k, L.k_norm, cfg.rms_eps)
        q = ref.rope(q, pos, model.cos, model.sin)
        k = ref.rope(k, pos, model.cos, model.sin)
        a = ref.attention(q, k, v, True, 1.0 / math.sqrt(D)).reshape(T, Hq * D)
        x = x + a @ ref.dense(L.wo).t()
        h = ref.rmsnorm(x, L.mlp_norm, cfg.rms_eps)
        gu = h @ ref.dense(L.w_gate_up).t()
        if getattr(L, "gu_block", 0):  # gate/up rows interleaved in blocks (ops.swiglu_interleave)
            gu = gu.view(gu.shape[0], -1, 2, L.gu_block)
            g, u = gu[:, :, 0].reshape(gu.shape[0], -1), gu[:, :, 1].reshape(gu.shape[0], -1)
        else:
            g, u = gu.chunk(2, dim=-1)
        x = x + (F.silu(g) * u) @ ref.dense(L.w_down).t()
    if hidden_only:
        w = getattr(model, "final_norm_weight", None)
        return ref.rmsnorm(x, model.final_norm if w is None else w, cfg.rms_eps)
    return ref.rmsnorm(x, model.final_norm, cfg.rms_eps) @ model.lm_head.float().t()


def row_cosines(a, b):
    """Cosine of each row pair of two [T, n] tensors -> [T]."""
    return F.cosine_similarity(a.float(), b.float(), dim=-1)
