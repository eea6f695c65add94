"""fp32 reference forward of the Qwen3-MoE decoders (models/qwen_moe.py): the attention block of
``qwen_ref.qwen_forward`` (per-head q / k RMSNorm before the rotation) with ``torch_ref.moe_mlp`` as the MLP, and
the MoE MLP evaluated for GIVEN experts and weights, so a comparison does not depend on how a near tie fell."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import torch_ref as ref


def qwen_moe_forward(model, tokens):
    """Full-sequence fp32 forward of a Qwen3MoeModel (single sequence) -> logits [T, V]."""
    cfg = model.cfg
    T = tokens.shape[0]
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    pos = torch.arange(T, device=tokens.device)
    x = model.embed[tokens.long()].float()
    for L in model.layers:
        h = ref.rmsnorm(x, L.attn_norm, cfg.rms_eps)
        qkv = h @ ref.dense(L.wqkv).t()
        q = qkv[:, : Hq * D].view(T, Hq, D)
        k = qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
        v = qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)
        q = ref.rope(ref.rmsnorm(q, L.q_norm, cfg.rms_eps), pos, model.cos, model.sin)
        k = ref.rope(ref.rmsnorm(k, L.k_norm, cfg.rms_eps), pos, model.cos, model.sin)
        a = ref.attention(q, k, v, True, 1.0 / math.sqrt(D)).reshape(T, Hq * D)
        x = x + a @ ref.dense(L.wo).t()
        x = x + ref.moe_mlp(model, L, ref.rmsnorm(x, L.mlp_norm, cfg.rms_eps))
    return ref.rmsnorm(x, model.final_norm, cfg.rms_eps) @ model.lm_head.float().t()


def moe_mlp_given(L, h, ids, w):
    """``torch_ref.moe_mlp`` for given experts ids [T, k] and weights w [T, k] (fp32, expert by expert)."""
    h = h.float()
    out = torch.zeros_like(h)
    ids = ids.long()
    for e in ids.unique().tolist():
        t, j = (ids == e).nonzero(as_tuple=True)
        w13 = L.w13[e].float() * (L.s13[e].unsqueeze(-1) if L.s13 is not None else 1.0)
        w2 = L.w2[e].float() * (L.s2[e].unsqueeze(-1) if L.s2 is not None else 1.0)
        gu = h[t] @ w13.t()
        if getattr(L, "gu_block", 0):
            gu = gu.view(gu.shape[0], -1, 2, L.gu_block)
            g, u = gu[:, :, 0].reshape(gu.shape[0], -1), gu[:, :, 1].reshape(gu.shape[0], -1)
        else:
            g, u = gu.chunk(2, dim=-1)
        out.index_add_(0, t, w[t, j].float().unsqueeze(-1) * ((F.silu(g) * u) @ w2.t()))
    return out
