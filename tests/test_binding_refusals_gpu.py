"""Operand refusals of the extension's bindings (csrc/kernels/bindings.cpp).

A binding hands a kernel nothing but pointers that came out of its operand checks: a tensor of another dtype, a
host tensor, or a strided view read through a flat pointer is refused with a message that names the binding and
the operand.  Every case here makes the smallest call the binding's shape checks allow, shows that it is
accepted, swaps ONE operand for a bad one and expects the refusal; a refused call launches nothing.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32, I32, I64, U8, FP8 = (torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.uint8,
                              torch.float8_e4m3fn)


def _K():
    from llm_weighted_consensus_amd import ops

    return ops.kernels()


def _strided(t):
    """The same shape and values as a [::2] view over twice the rows: what a flat pointer would misread."""
    v = t.repeat_interleave(2, 0)[::2]
    assert v.shape == t.shape and not v.is_contiguous()
    return v


# what is wrong with the one bad operand
SPOIL = {"cpu": lambda t: t.cpu(), "strided": _strided, "short": lambda t: t[:1], "int32": lambda t: t.to(I32),
         "int64": lambda t: t.to(I64), "bf16": lambda t: t.to(BF), "float64": lambda t: t.to(torch.float64)}


def _sample(dev):
    B, V = 2, 64
    z = lambda dt: torch.zeros(B, dtype=dt, device=dev)
    rows = torch.arange(B, dtype=I32, device=dev)
    return dict(logits=torch.zeros(B, V, dtype=BF, device=dev), temperature=z(F32) + 1, top_p=z(F32) + 1, top_k=z(I32),
                min_p=z(F32), top_a=z(F32), freq_pen=z(F32), pres_pen=z(F32), rep_pen=z(F32) + 1,
                counts=torch.zeros(B, V, dtype=torch.int16, device=dev), count_rows=rows.clone(),
                bias=torch.zeros(B, V, dtype=F32, device=dev), bias_rows=rows.clone(),
                mask=torch.full((B, V // 32), -1, dtype=I32, device=dev), mask_rows=rows.clone(),
                seeds=z(I64) + 7, offsets=z(I64), num_logprobs=0, out_token=z(I32), out_logprob=z(F32),
                out_topk_ids=torch.zeros(B, 1, dtype=I32, device=dev), out_topk_lp=torch.zeros(B, 1, dtype=F32, device=dev),
                mask_logprobs=False, need_logprob=True)


def _decode(dev, cascade):
    B, NB, BS, D = 2, 2, 16, 64    # one block of 16 tokens per sequence, Hq = Hkv = 1
    a = dict(q=torch.zeros(B, D, dtype=BF, device=dev), k_cache=torch.zeros(NB, 1, BS, D, dtype=BF, device=dev),
             v_cache=torch.zeros(NB, 1, BS // 4, D, 4, dtype=BF, device=dev),
             block_tables=torch.tensor([[0, 0], [1, 0]], dtype=I32, device=dev),
             ctx_lens=torch.ones(B, dtype=I32, device=dev))
    out = torch.zeros(B, 1, D, dtype=BF, device=dev)
    if cascade:
        return dict(a, tiles=torch.tensor([[0, B, 0]], dtype=I32, device=dev), out=out, Hq=1, scale=1.0,
                    rope_cos=None, rope_sin=None, positions=None, out8=None, mx=None)
    return dict(a, out=out, part_o=None, part_lse=None, num_splits=1, scale=1.0, rope_cos=None, rope_sin=None,
                positions=None)


def _prefill(dev, kind):
    T, D = 4, 128                   # two sequences of two tokens, Hq = Hkv = 1
    q = torch.zeros(T, D, dtype=BF, device=dev)
    cu = torch.tensor([0, 2, 4], dtype=I32, device=dev)
    if kind == "plain":
        return dict(q=q, k=q.clone(), v=q.clone(), out=torch.zeros(T, D, dtype=BF, device=dev), cu_seqlens=cu,
                    max_seqlen=2, Hq=1, Hkv=1, D=D, scale=1.0, causal=True, cu_seqlens_k=cu.clone())
    if kind == "mx":
        return dict(q=q, k=q.clone(), v=q.clone(), out8=torch.zeros(T, D, dtype=U8, device=dev),
                    mx=torch.zeros(1, T, 4, dtype=U8, device=dev), cu_seqlens=cu, max_seqlen=2, Hq=1, Hkv=1, scale=1.0,
                    causal=True)
    return dict(q=q, k_cache=torch.zeros(2, 1, 16, D, dtype=BF, device=dev),
                v_cache=torch.zeros(2, 1, 4, D, 4, dtype=BF, device=dev), out=torch.zeros(T, D, dtype=BF, device=dev),
                cu_seqlens=cu, block_tables=torch.tensor([[0, 0], [1, 0]], dtype=I32, device=dev),
                k_lens=torch.tensor([2, 2], dtype=I32, device=dev), max_seqlen=2, Hq=1, scale=1.0)


def _quant(dev, kind):
    rows = 2
    scale = torch.zeros(rows, dtype=F32, device=dev)
    if kind == "rows":
        return dict(x=torch.ones(rows, 64, dtype=BF, device=dev), q=torch.zeros(rows, 64, dtype=FP8, device=dev), scale=scale)
    if kind == "silu":
        return dict(gu=torch.ones(rows, 128, dtype=BF, device=dev), q=torch.zeros(rows, 64, dtype=FP8, device=dev),
                    scale=scale, block=0)
    d = 2048
    return dict(x=torch.ones(rows, d, dtype=BF, device=dev), residual=None, w=torch.ones(d, dtype=BF, device=dev),
                out=None, q=torch.zeros(rows, d, dtype=FP8, device=dev), scale=scale, eps=1e-5)


def _grouped(dev, g8):
    # fp8, two groups of two rows; max_slots = 0 m-tiles: the launcher returns before its kernel, the binding has
    # checked every operand by then
    rows, G, N, K = 4, 2, 16, 128
    A = torch.zeros(rows, K, dtype=FP8, device=dev)
    W = torch.zeros(G, N, K, dtype=FP8, device=dev)
    C = torch.zeros(rows, N, dtype=BF, device=dev)
    row_off = torch.tensor([0, 2, 4], dtype=I32, device=dev)
    a_rows = torch.arange(rows, dtype=I32, device=dev)
    a_scale = torch.ones(rows, dtype=F32, device=dev)
    w_scale = torch.ones(G, N, dtype=F32, device=dev)
    if g8:
        return dict(A=A, W=W, C=C, row_off=row_off, max_slots=0, a_rows=a_rows, a_scale=a_scale, w_scale=w_scale,
                    mode=0, a_mx=None, mx_out=None)
    return dict(A=A, W=W, C=C, row_off=row_off, max_slots=0, a_scale=a_scale, w_scale=w_scale,
                bias=torch.zeros(G, N, dtype=BF, device=dev), a_rows=a_rows, splits=1)


def _route(dev, router):
    T, E, k, d = 4, 8, 2, 64
    outs = dict(topk_ids=torch.zeros(T * k, dtype=I32, device=dev), topk_w=torch.zeros(T * k, dtype=F32, device=dev),
                row_off=torch.zeros(E + 1, dtype=I32, device=dev), src_row=torch.zeros(T * k, dtype=I32, device=dev),
                inv=torch.zeros(T * k, dtype=I32, device=dev))
    if router:
        return dict(h=torch.ones(T, d, dtype=BF, device=dev), router=torch.ones(E, d, dtype=BF, device=dev), k=k, **outs,
                    logits=torch.zeros(T, E, dtype=BF, device=dev))
    return dict(logits=torch.zeros(T, E, dtype=BF, device=dev), k=k, **outs)


def _ep(dev, which):
    W, El, C, d = 1, 2, 2, 8        # one rank, two experts, one row each; 16-byte rows, 32-byte slots with the scale
    x = torch.ones(2, d, dtype=BF, device=dev)
    row_off = torch.tensor([0, 1, 2], dtype=I32, device=dev)
    if which == "pack":
        return dict(x=x, xs=torch.ones(2, dtype=F32, device=dev), src=torch.tensor([1, 0], dtype=I32, device=dev),
                    row_off=row_off, W=W, El=El, C=C, send=torch.zeros(W, (C + 1) * 32, dtype=U8, device=dev))
    if which == "unpack":
        return dict(recv=torch.zeros(W, (C + 1) * 32, dtype=U8, device=dev), W=W, El=El, C=C, x_local=torch.zeros_like(x),
                    s_local=torch.zeros(2, dtype=F32, device=dev), map=torch.zeros(W * C, dtype=I32, device=dev),
                    row_off_local=torch.zeros(El + 1, dtype=I32, device=dev))
    if which == "back":
        return dict(y_local=x, map=torch.tensor([1, 0], dtype=I32, device=dev), W=W, C=C, back=torch.zeros_like(x))
    return dict(ret=x, row_off=row_off, inv=torch.tensor([0, 1], dtype=I32, device=dev),
                w=torch.ones(2, dtype=F32, device=dev), El=El, C=C, k=1, out=torch.zeros_like(x))


def _embedding(dev):
    return dict(table=torch.ones(4, 8, dtype=BF, device=dev), ids=torch.tensor([3, 0], dtype=I32, device=dev),
                out=torch.zeros(2, 8, dtype=BF, device=dev))


def _kv_gather(dev):
    n, NB, BS, D = 2, 2, 16, 64     # one token of each block, Hkv = 1
    return dict(kc=torch.zeros(NB, 1, BS, D, dtype=BF, device=dev), vc=torch.zeros(NB, 1, BS // 4, D, 4, dtype=BF, device=dev),
                slots=torch.tensor([0, 17], dtype=I64, device=dev), ko=torch.zeros(n, D, dtype=BF, device=dev),
                vo=torch.zeros(n, D, dtype=BF, device=dev))


def _norm(dev, layer):
    d = 64
    x = torch.ones(2, d, dtype=BF, device=dev)
    w = torch.ones(d, dtype=BF, device=dev)
    if layer:
        return dict(x=x, residual=None, g=w, b=w.clone(), out=torch.zeros_like(x), eps=1e-5, pre_bias=None)
    return dict(x=x, residual=None, w=w, out=torch.zeros_like(x), eps=1e-5)


def _collective(dev, a2a):
    """An empty payload: the launcher returns before its kernel, so no peer region is needed; the operands are
    checked all the same."""
    err = torch.zeros(1, dtype=I32, device=dev)
    if a2a:
        return dict(bases=[0], me=0, send=torch.zeros(1, 0, dtype=U8, device=dev), recv=torch.zeros(1, 0, dtype=U8, device=dev),
                    cap=4096, err=err, blocks=1, spin_limit=1)
    x = torch.zeros(0, dtype=BF, device=dev)
    return dict(bases=[0], me=0, x=x, out=x.clone(), cap=4096, err=err, blocks=1, spin_limit=1)


# binding -> (the name its messages carry, the good arguments in the binding's order)
GOOD = {
    "sample": ("sample", _sample),
    "paged_decode": ("paged_decode", lambda dev: _decode(dev, False)),
    "paged_decode_cascade": ("paged_decode_cascade", lambda dev: _decode(dev, True)),
    "prefill_attention": ("prefill_attention", lambda dev: _prefill(dev, "plain")),
    "prefill_attention_mx": ("prefill_attention_mx", lambda dev: _prefill(dev, "mx")),
    "prefill_attention_paged": ("prefill_attention_paged", lambda dev: _prefill(dev, "paged")),
    "quant_fp8_rows": ("quant_fp8_rows", lambda dev: _quant(dev, "rows")),
    "silu_mul_quant_fp8": ("silu_mul_quant_fp8", lambda dev: _quant(dev, "silu")),
    "rmsnorm_quant_fp8": ("rmsnorm_quant_fp8", lambda dev: _quant(dev, "norm")),
    "grouped_gemm": ("grouped_gemm", lambda dev: _grouped(dev, False)),
    "gemm8g_fp8": ("gemm8g", lambda dev: _grouped(dev, True)),
    "moe_route": ("moe_route", lambda dev: _route(dev, False)),
    "moe_router": ("moe_router", lambda dev: _route(dev, True)),
    "ep_pack": ("ep_pack", lambda dev: _ep(dev, "pack")),
    "ep_unpack": ("ep_unpack", lambda dev: _ep(dev, "unpack")),
    "ep_back": ("ep_back", lambda dev: _ep(dev, "back")),
    "ep_combine": ("ep_combine", lambda dev: _ep(dev, "combine")),
    "embedding": ("embedding", _embedding),
    "kv_gather": ("kv_gather", _kv_gather),
    "rmsnorm": ("rmsnorm", lambda dev: _norm(dev, False)),
    "layernorm": ("layernorm", lambda dev: _norm(dev, True)),
    "allreduce": ("allreduce", lambda dev: _collective(dev, False)),
    "alltoall": ("alltoall", lambda dev: _collective(dev, True)),
}

# (binding, operand, what is wrong with it): one case per gap the operand vocabulary closed
CASES = [
    # the eight operands sample took through an unchecked pointer cast
    ("sample", "freq_pen", "int32"), ("sample", "pres_pen", "cpu"), ("sample", "rep_pen", "strided"),
    ("sample", "count_rows", "int64"), ("sample", "bias", "bf16"), ("sample", "bias_rows", "cpu"),
    ("sample", "mask", "int64"), ("sample", "mask_rows", "strided"),
    # its per-row tables: device, contiguity, one entry per row
    ("sample", "top_k", "cpu"), ("sample", "top_k", "strided"), ("sample", "top_k", "short"),
    ("sample", "seeds", "cpu"), ("sample", "seeds", "strided"), ("sample", "seeds", "short"),
    ("sample", "offsets", "cpu"), ("sample", "offsets", "strided"), ("sample", "offsets", "short"),
    ("sample", "temperature", "cpu"), ("sample", "min_p", "strided"),
    ("sample", "out_token", "cpu"), ("sample", "out_logprob", "strided"),
    # decode attention
    ("paged_decode", "k_cache", "strided"), ("paged_decode", "block_tables", "cpu"), ("paged_decode", "ctx_lens", "cpu"),
    ("paged_decode_cascade", "k_cache", "strided"), ("paged_decode_cascade", "block_tables", "cpu"),
    ("paged_decode_cascade", "ctx_lens", "cpu"), ("paged_decode_cascade", "tiles", "cpu"),
    # prefill attention
    ("prefill_attention", "cu_seqlens", "cpu"), ("prefill_attention", "cu_seqlens", "strided"),
    ("prefill_attention", "cu_seqlens_k", "cpu"), ("prefill_attention", "cu_seqlens_k", "strided"),
    ("prefill_attention_mx", "cu_seqlens", "cpu"), ("prefill_attention_mx", "cu_seqlens", "strided"),
    ("prefill_attention_paged", "cu_seqlens", "cpu"), ("prefill_attention_paged", "cu_seqlens", "strided"),
    ("prefill_attention_paged", "k_lens", "cpu"), ("prefill_attention_paged", "block_tables", "cpu"),
    # the fp8 row quantisers
    ("quant_fp8_rows", "q", "cpu"), ("quant_fp8_rows", "scale", "cpu"), ("quant_fp8_rows", "scale", "strided"),
    ("silu_mul_quant_fp8", "q", "cpu"), ("silu_mul_quant_fp8", "scale", "cpu"), ("silu_mul_quant_fp8", "scale", "strided"),
    ("rmsnorm_quant_fp8", "q", "cpu"), ("rmsnorm_quant_fp8", "scale", "cpu"),
    # grouped GEMMs
    ("grouped_gemm", "row_off", "cpu"), ("grouped_gemm", "a_rows", "cpu"), ("grouped_gemm", "a_scale", "cpu"),
    ("grouped_gemm", "w_scale", "cpu"), ("grouped_gemm", "a_scale", "strided"), ("grouped_gemm", "w_scale", "strided"),
    ("grouped_gemm", "bias", "strided"),
    ("gemm8g_fp8", "row_off", "cpu"), ("gemm8g_fp8", "a_rows", "cpu"), ("gemm8g_fp8", "a_scale", "cpu"),
    ("gemm8g_fp8", "w_scale", "cpu"),
    # MoE routing
    ("moe_route", "topk_w", "cpu"), ("moe_router", "topk_w", "cpu"), ("moe_router", "logits", "cpu"),
    ("moe_router", "logits", "strided"),
    # expert-parallel exchange
    ("ep_pack", "xs", "float64"), ("ep_pack", "xs", "cpu"), ("ep_pack", "src", "cpu"), ("ep_pack", "row_off", "cpu"),
    ("ep_pack", "row_off", "strided"),
    ("ep_unpack", "x_local", "cpu"), ("ep_unpack", "s_local", "cpu"), ("ep_unpack", "map", "cpu"),
    ("ep_unpack", "row_off_local", "cpu"),
    ("ep_back", "back", "cpu"), ("ep_back", "map", "cpu"), ("ep_back", "map", "strided"),
    ("ep_combine", "row_off", "cpu"), ("ep_combine", "inv", "cpu"), ("ep_combine", "inv", "strided"), ("ep_combine", "w", "cpu"),
    ("ep_combine", "w", "strided"),
    # embedding ids, gathered slots, norm weights
    ("embedding", "ids", "strided"), ("embedding", "ids", "cpu"), ("kv_gather", "slots", "cpu"),
    ("rmsnorm", "w", "strided"), ("layernorm", "g", "strided"), ("layernorm", "b", "strided"),
    # the collectives' error word
    ("allreduce", "err", "cpu"), ("alltoall", "err", "cpu"),
]


@pytest.mark.parametrize("binding,operand,how", CASES, ids=["-".join(c) for c in CASES])
def test_bad_operand_is_refused_by_name(gpu, binding, operand, how):
    who, good = GOOD[binding]
    fn = getattr(_K(), binding)
    args = good(gpu)
    fn(*args.values())                                         # the call is fine as it stands
    args[operand] = SPOIL[how](args[operand])
    with pytest.raises(RuntimeError) as e:
        fn(*args.values())
    assert f"{who}: " in str(e.value) and operand in str(e.value), str(e.value)
    torch.cuda.synchronize()


def test_prefill_attention_refuses_k_and_v_of_different_rows(gpu):
    """Without cu_seqlens_k too: v is read at k's row indices."""
    a = _prefill(gpu, "plain")
    a["cu_seqlens_k"] = None
    _K().prefill_attention(*a.values())
    a["v"] = a["v"][:3]
    with pytest.raises(RuntimeError, match="prefill_attention: k/v row mismatch"):
        _K().prefill_attention(*a.values())
    torch.cuda.synchronize()


@pytest.mark.parametrize("binding,M,N,good_K", [("gemm4w", 256, 256, 128), ("skinny_gemm", 4, 16, 2048)])
def test_gemm_operand_errors_name_their_binding(gpu, binding, M, N, good_K):
    """The MFMA GEMM cores share their operand checks, and each refusal carries the name of the binding that was
    called: K = 96 is no multiple of 64."""
    def call(K):
        A = torch.zeros(M, K, dtype=BF, device=gpu)
        W = torch.zeros(N, K, dtype=BF, device=gpu)
        C = torch.zeros(M, N, dtype=BF, device=gpu)
        if binding == "gemm4w":
            _K().gemm4w(A, W, C, None, 0, 256, None, 0, 0, 0.0, 0, 0, 1, 0, None, None)
        else:
            _K().skinny_gemm(A, W, C, None, 0)

    call(good_K)
    with pytest.raises(RuntimeError) as e:
        call(96)
    assert f"{binding}: " in str(e.value) and "K % 64" in str(e.value) and "gemm8p" not in str(e.value), str(e.value)
    torch.cuda.synchronize()
