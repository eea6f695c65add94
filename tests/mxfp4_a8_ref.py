"""Oracles of the MXFP4 decoder with e4m3 activations (``mxfp4_act="e4m3"``): the fp32 forward of the dequantised
twin with the inputs of qkv, o, gate|up and down row-quantised to e4m3 exactly where the model's GEMM call has at
least ``ops.MXFP4_A8_MIN_ROWS`` rows (``a8_forward``), next to the unquantised ``qwen_ref.qwen_forward``."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import torch_ref as ref


def quant_rows(x: torch.Tensor) -> torch.Tensor:
    """What the projection reads: the rows rounded to bf16, then per-row e4m3 (scale amax / 448), as fp32."""
    xb = x.to(torch.bfloat16).float()
    s = xb.abs().amax(-1, keepdim=True).clamp(min=1e-12) / 448.0
    return (xb / s).to(torch.float8_e4m3fn).float() * s


def a8_forward(model, tokens, body_rows: torch.Tensor, tail_rows: torch.Tensor):
    """``qwen_ref.qwen_forward``'s body (fp32, full sequence, one sequence) on a dequantised twin -> logits [T, V],
    with the e4m3 row quantisation of the GEMM inputs on the rows whose GEMM call had at least 65 rows:

    ``body_rows`` [T] bool: the rows quantised in front of every layer's qkv and of o / gate|up / down in every
    layer but the last; ``tail_rows`` [T] bool: the rows quantised in front of the LAST layer's o / gate|up / down
    — a prefill keeps one row per sequence there (``keep``), so those calls stay below the threshold while a
    decode step of 65 rows or more quantises them too."""
    cfg = model.cfg
    T = tokens.shape[0]
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    pos = torch.arange(T, device=tokens.device)
    x = model.embed[tokens.long()].float()

    def q(h, rows):
        return torch.where(rows.view(-1, 1), quant_rows(h), h)

    for li, L in enumerate(model.layers):
        rows = tail_rows if li + 1 == len(model.layers) else body_rows
        h = q(ref.rmsnorm(x, L.attn_norm, cfg.rms_eps), body_rows)
        qkv = h @ ref.dense(L.wqkv).t()
        if L.bqkv is not None:
            qkv = qkv + L.bqkv.float()
        qh = qkv[:, : Hq * D].view(T, Hq, D)
        k = qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
        v = qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)
        if L.q_norm is not None:
            qh = ref.rmsnorm(qh, L.q_norm, cfg.rms_eps)
        if L.k_norm is not None:
            k = ref.rmsnorm(k, L.k_norm, cfg.rms_eps)
        qh = ref.rope(qh, pos, model.cos, model.sin)
        k = ref.rope(k, pos, model.cos, model.sin)
        a = ref.attention(qh, k, v, True, 1.0 / math.sqrt(D)).reshape(T, Hq * D)
        x = x + q(a, rows) @ ref.dense(L.wo).t()
        h = q(ref.rmsnorm(x, L.mlp_norm, cfg.rms_eps), rows)
        gu = h @ ref.dense(L.w_gate_up).t()
        if getattr(L, "gu_block", 0):  # gate/up rows interleaved in blocks (ops.swiglu_interleave)
            gu = gu.view(gu.shape[0], -1, 2, L.gu_block)
            g, u = gu[:, :, 0].reshape(gu.shape[0], -1), gu[:, :, 1].reshape(gu.shape[0], -1)
        else:
            g, u = gu.chunk(2, dim=-1)
        x = x + q(F.silu(g) * u, rows) @ ref.dense(L.w_down).t()
    return ref.rmsnorm(x, model.final_norm, cfg.rms_eps) @ model.lm_head.float().t()
