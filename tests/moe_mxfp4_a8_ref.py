"""Oracles of the MoE decoders with MXFP4 experts and e4m3 activations (``expert_act="e4m3"``): the fp32 MoE MLP of
the dequantised experts with its input rows and its SwiGLU output row-quantised to e4m3 (``quant_rows``: what
``ops.moe_swiglu_mxfp4_a8`` / ``ops.moe_linear_mxfp4_a8`` read), for given experts (``moe_mlp_given_a8``) and
inside the full-sequence fp32 forward of a dequantised twin (``a8_forward``)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import rowwise_probes as rp
from tests import torch_ref as ref


def quant_rows(x: torch.Tensor) -> torch.Tensor:
    """What the expert GEMM reads, as fp32: the rows rounded to bf16, then ``ops.quant_fp8_rows`` as
    tests/rowwise_probes.py pins it — scale s = fp32 max(amax, 1e-12) / 448, codes RNE_e4m3(fp32(v) * fp32(1 / s)) —
    computed on the CPU as the probes do: a GPU tensor divided by the scalar 448 is multiplied by its reciprocal,
    which moves s by an ulp in about half the rows.  ``mxfp4_a8_ref.quant_rows`` with the quantiser's own arithmetic:
    a bf16 value times 448 over a bf16 amax lands on an e4m3 midpoint often enough to show, and there the last bit
    of the scaled value decides the code."""
    if x.numel() == 0:
        return x.float()
    xb = x.to(torch.bfloat16).float().cpu()
    s = rp.scale_ref(xb)
    q = rp.e4m3_codes(xb, s).view(torch.float8_e4m3fn).float()
    return (q * s.view(-1, 1)).to(x.device)


def _ffn(L, e, x, quant):
    """Expert e's fp32 FFN on rows x; ``quant``: x and the SwiGLU output go through ``quant_rows``."""
    gu = (quant_rows(x) if quant else x) @ L.w13[e].float().t()
    if getattr(L, "gu_block", 0):
        gu = gu.view(gu.shape[0], -1, 2, L.gu_block)
        g, u = gu[:, :, 0].reshape(gu.shape[0], -1), gu[:, :, 1].reshape(gu.shape[0], -1)
    else:
        g, u = gu.chunk(2, dim=-1)
    act = F.silu(g) * u
    return (quant_rows(act) if quant else act) @ L.w2[e].float().t()


def moe_mlp_given_a8(L, h, ids, w, rows=None):
    """``qwen_moe_ref.moe_mlp_given`` (experts ids [T, k], weights w [T, k], fp32, expert by expert) on a layer
    holding the dequantised experts, with the e4m3 row quantisation on the token rows ``rows`` ([T] bool; None: all):
    the rows of a step that took the W4A8 kernel."""
    h = h.float()
    T = h.shape[0]
    rows = torch.ones(T, dtype=torch.bool, device=h.device) if rows is None else rows
    out = torch.zeros_like(h)
    ids = ids.long()
    for e in ids.unique().tolist():
        t, j = (ids == e).nonzero(as_tuple=True)
        y = torch.where(rows[t].view(-1, 1), _ffn(L, e, h[t], True), _ffn(L, e, h[t], False))
        out.index_add_(0, t, w[t, j].float().unsqueeze(-1) * y)
    return out


def a8_forward(model, tokens, body_rows=None, tail_rows=None):
    """Full-sequence fp32 forward (one sequence) of a dequantised twin of a MixtralModel / Qwen3MoeModel -> logits
    [T, V]: ``torch_ref.llama_forward`` / ``qwen_moe_ref.qwen_moe_forward`` with the router's fp32 top-k and
    ``moe_mlp_given_a8`` as the MLP.  ``body_rows`` [T] bool: the token rows quantised in every layer but the last;
    ``tail_rows``: in the LAST layer, where a prefill keeps one row per sequence, so that layer's step has fewer routed
    rows and may take another route than the layers before it.  None: every row."""
    cfg = model.cfg
    T = tokens.shape[0]
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    k = model.full_cfg.experts_per_token
    pos = torch.arange(T, device=tokens.device)
    x = model.embed[tokens.long()].float()
    for li, L in enumerate(model.layers):
        rows = tail_rows if li + 1 == len(model.layers) else body_rows
        h = ref.rmsnorm(x, L.attn_norm, cfg.rms_eps)
        qkv = h @ ref.dense(L.wqkv).t()
        q = qkv[:, : Hq * D].view(T, Hq, D)
        kk = qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
        v = qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)
        if L.q_norm is not None:
            q = ref.rmsnorm(q, L.q_norm, cfg.rms_eps)
        if L.k_norm is not None:
            kk = ref.rmsnorm(kk, L.k_norm, cfg.rms_eps)
        q = ref.rope(q, pos, model.cos, model.sin)
        kk = ref.rope(kk, pos, model.cos, model.sin)
        a = ref.attention(q, kk, v, True, 1.0 / math.sqrt(D)).reshape(T, Hq * D)
        x = x + a @ ref.dense(L.wo).t()
        h = ref.rmsnorm(x, L.mlp_norm, cfg.rms_eps)
        top, ids = (h @ L.router.float().t()).topk(k, dim=-1)
        x = x + moe_mlp_given_a8(L, h, ids, top.softmax(-1), rows)
    return ref.rmsnorm(x, model.final_norm, cfg.rms_eps) @ model.lm_head.float().t()
