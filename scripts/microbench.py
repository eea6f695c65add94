#!/usr/bin/env python3
"""Micro-benchmarks of the decode hot path on one MI355X: the Llama-3-8B projection GEMMs at decode
batch sizes (hipBLASLt default vs TunableOp-tuned), paged decode attention, the fused sampler and the
small fused kernels.  Prints one line per case: time, TFLOP/s, GB/s."""
import argparse
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def gemms(dev, Ms, tuned):
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336),
              "lm_head": (128256, 4096)}
    for M in Ms:
        for name, (N, K) in shapes.items():
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
            us = timeit(lambda: F.linear(x, w), iters=20)
            fl = 2 * M * N * K / (us * 1e-6) / 1e12
            gb = (N * K * 2 + M * K * 2 + M * N * 2) / (us * 1e-6) / 1e9
            print(f"gemm{'-tuned' if tuned else ''} M={M:4d} {name:8s} N={N:6d} K={K:5d}: {us:8.1f} us "
                  f"{fl:7.1f} TF/s {gb:7.0f} GB/s", flush=True)


def gemm_layouts(dev, Ms):
    """Same products through different operand layouts: hipBLASLt picks different kernels."""
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}
    for M in Ms:
        for name, (N, K) in shapes.items():
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
            wt = w.t().contiguous()
            xt = x.t().contiguous()
            cases = {
                "NT  x@w^T": lambda: F.linear(x, w),
                "NN  x@wt": lambda: torch.mm(x, wt),
                "sw  w@x^T": lambda: torch.mm(w, xt),
                "sw2 w@xT(view)": lambda: torch.mm(w, x.t()),
            }
            for cname, fn in cases.items():
                us = timeit(fn, iters=20)
                fl = 2 * M * N * K / (us * 1e-6) / 1e12
                print(f"layout M={M:4d} {name:8s} {cname:16s}: {us:8.1f} us {fl:7.1f} TF/s", flush=True)
    for n in (4096, 8192):
        a = torch.randn(n, n, device=dev).to(torch.bfloat16)
        b = torch.randn(n, n, device=dev).to(torch.bfloat16)
        us = timeit(lambda: torch.mm(a, b), iters=10)
        print(f"square {n}: {us:8.1f} us {2 * n ** 3 / (us * 1e-6) / 1e12:7.1f} TF/s", flush=True)


def gemm_backends(dev, Ms):
    """The decode GEMM shapes through each BLAS backend torch can dispatch to on ROCm."""
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336),
              "lm_head": (128256, 4096)}
    for lib in ("cublaslt", "cublas", "ck"):
        try:
            torch.backends.cuda.preferred_blas_library(lib)
        except Exception as e:  # noqa: BLE001
            print(f"backend {lib}: unavailable ({e})", flush=True)
            continue
        for M in Ms:
            for name, (N, K) in shapes.items():
                x = torch.randn(M, K, device=dev).to(torch.bfloat16)
                w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
                try:
                    us = timeit(lambda: F.linear(x, w), iters=20)
                except Exception as e:  # noqa: BLE001
                    print(f"backend {lib} M={M} {name}: failed ({type(e).__name__})", flush=True)
                    continue
                fl = 2 * M * N * K / (us * 1e-6) / 1e12
                print(f"backend {lib:8s} M={M:4d} {name:8s}: {us:8.1f} us {fl:7.1f} TF/s", flush=True)
    torch.backends.cuda.preferred_blas_library("cublaslt")


def grouped(dev):
    """Hand-written grouped MFMA GEMM (K6g) vs hipBLASLt on plain shapes, and the MoE decode shape."""
    from llm_weighted_consensus_amd import ops

    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336),
              "lm_head": (128256, 4096)}
    for M in (1024, 3072):
        for name, (N, K) in shapes.items():
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
            off = torch.tensor([0, M], dtype=torch.int32, device=dev)
            t_h = timeit(lambda: F.linear(x, w), iters=20)
            t_g = timeit(lambda: ops.grouped_gemm(x, w.unsqueeze(0), off), iters=20)
            xq = x.to(torch.float8_e4m3fn)
            wq = w.unsqueeze(0).to(torch.float8_e4m3fn)
            sa = torch.ones(M, device=dev)
            sw = torch.ones(1, N, device=dev)
            t_8 = timeit(lambda: ops.grouped_gemm(xq, wq, off, a_scale=sa, w_scale=sw), iters=20)
            t_2 = timeit(lambda: ops.gemm8p(x, w), iters=20)
            err = (ops.gemm8p(x, w).float() - F.linear(x, w).float()).abs().max().item()
            fl = 2 * M * N * K / 1e12
            print(f"ggemm M={M:4d} {name:8s}: hipblaslt {t_h:7.1f} us ({fl / t_h * 1e6:6.0f} TF/s)  "
                  f"gemm8p {t_2:7.1f} us ({fl / t_2 * 1e6:6.0f}, err {err:.3g})  "
                  f"grouped-bf16 {t_g:7.1f} us ({fl / t_g * 1e6:6.0f})  grouped-fp8 {t_8:7.1f} us ({fl / t_8 * 1e6:6.0f})",
                  flush=True)
    # Mixtral decode MoE: T tokens x top-2 over 8 experts, d=4096, ffn=14336 (gate_up fused 28672)
    E, d, f = 8, 4096, 14336
    w13 = (torch.randn(E, 2 * f, d, device=dev) * 0.02).to(torch.bfloat16)
    for T in (256, 1024):
        rows = 2 * T
        sizes = torch.full((E,), rows // E, dtype=torch.int64)
        off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
        x = torch.randn(rows, d, device=dev).to(torch.bfloat16)
        t = timeit(lambda: ops.grouped_gemm(x, w13, off), iters=10)
        fl = 2 * rows * 2 * f * d / 1e12
        print(f"ggemm moe gate_up T={T}: {t:7.1f} us ({fl / t * 1e6:6.0f} TF/s)", flush=True)


def gemm8p_study(dev, Ms):
    """8-phase 256x256 GEMM (csrc/kernels/gemm8p.hip) vs hipBLASLt, interleaved
    rounds in one process (median of 3), random operands; plus the fused SwiGLU epilogue against
    hipBLASLt gate_up + silu_mul."""
    from llm_weighted_consensus_amd import ops

    shapes = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336),
              "lm_head": (128256, 4096)}
    cases = [(M, name, N, K) for M in Ms for name, (N, K) in shapes.items()]
    cases += [(4096, "sq4096", 4096, 4096), (8192, "sq8192", 8192, 8192)]
    for M, name, N, K in cases:
        x = (torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16)
        w = ((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
        o = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        fns = {"hipblaslt": lambda: torch.matmul(x, w.t(), out=o), "gemm8p": lambda: ops.gemm8p(x, w, out=o)}
        ref = F.linear(x, w).float()
        err = (ops.gemm8p(x, w).float() - ref).abs().max().item()
        res = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                res[k].append(timeit(fn, iters=10 if M * N * K > 1e11 else 30))
        fl = 2 * M * N * K / 1e12
        line = "  ".join(f"{k} {sorted(v)[1]:8.1f} us ({fl / sorted(v)[1] * 1e6:5.0f})" for k, v in res.items())
        print(f"g8 M={M:5d} {name:8s}: {line}  err {err:.3g}", flush=True)
    for M in Ms:
        N, K = 28672, 4096
        x = (torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16)
        w = ((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
        wi = ops.swiglu_interleave(w)
        gu = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        h = torch.empty(M, N // 2, dtype=torch.bfloat16, device=dev)

        def unfused():
            torch.matmul(x, w.t(), out=gu)
            ops.silu_mul(gu, out=h)

        ref = F.silu(F.linear(x, w).float()[:, :N // 2]) * F.linear(x, w).float()[:, N // 2:]
        err = (ops.gemm8p(x, wi, swiglu=True).float() - ref).abs().max().item()
        ta, tb = [], []
        for _ in range(3):
            ta.append(timeit(unfused, iters=10))
            tb.append(timeit(lambda: ops.gemm8p(x, wi, out=h, swiglu=True), iters=10))
        print(f"g8 swiglu M={M:5d}: hipblaslt+silu_mul {sorted(ta)[1]:8.1f} us  gemm8p-fused {sorted(tb)[1]:8.1f} us"
              f"  err {err:.3g}", flush=True)


def gemm8p_ab(dev):
    """A/B of gemm8p knobs (env LWC_G8_*, read at launch) in interleaved rounds, median of 5."""
    from llm_weighted_consensus_amd import ops

    variants = [v.split(":") for v in os.environ.get("G8_VARIANTS", "GM=1:STAGGER=1,GM=4:STAGGER=1,GM=8:STAGGER=1,"
                                                     "GM=4:STAGGER=0").split(",")]
    shapes = [(4096, 4096, 4096, False), (3072, 28672, 4096, True), (3072, 6144, 4096, False),
              (3072, 4096, 14336, False), (3072, 4096, 4096, False), (3072, 128256, 4096, False),
              (8192, 8192, 8192, False)]
    for M, N, K, sw in shapes:
        x = (torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16)
        w = ((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
        if sw:
            w = ops.swiglu_interleave(w)
        res = {",".join(v): [] for v in variants}
        for _ in range(5):
            for v in variants:
                for kv in v:
                    k, val = kv.split("=")
                    os.environ["LWC_G8_" + k] = val
                res[",".join(v)].append(timeit(lambda: ops.gemm8p(x, w, swiglu=sw), iters=10))
        fl = 2 * M * N * K / 1e12
        line = "  ".join(f"[{k}] {sorted(t)[2]:7.1f} us ({fl / sorted(t)[2] * 1e6:5.0f})" for k, t in res.items())
        print(f"g8ab {M}x{N}x{K}{' swiglu' if sw else ''}: {line}", flush=True)
    for k in ("LWC_G8_GM", "LWC_G8_STAGGER"):
        os.environ.pop(k, None)


def gemm4w_ab(dev):
    """hipBLASLt vs gemm8p vs gemm4w (bn 256 / 192) on the headline's decode shapes (M = 4096), prefill and
    encoder shapes; interleaved rounds in one process, median of 5, random [-1, 1) operands."""
    import torch.nn.functional as F

    from llm_weighted_consensus_amd import ops

    shapes = [(4096, 6144, 4096, "plain"), (4096, 4096, 4096, "res"), (4096, 28672, 4096, "swiglu"),
              (4096, 4096, 14336, "res"), (4096, 128256, 4096, "plain"), (16384, 6144, 4096, "plain"),
              (65536, 3072, 1024, "bias"), (65536, 4096, 1024, "gelu"), (65536, 1024, 4096, "bias"),
              (8192, 8192, 8192, "plain")]
    only = os.environ.get("G4_SHAPES")
    if only:
        shapes = [shapes[int(i)] for i in only.split(",")]
    ws = ops.new_gemm8p_workspace(dev)
    for M, N, K, epi in shapes:
        x = (torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16)
        w = ((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
        b = (torch.rand(N, device=dev) - 0.5).to(torch.bfloat16)
        acc = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
        # gemm4w at both schedules (32: block-staged epilogue, 64: wave-local epilogue + next-tile prefetch;
        # G4_VARS selects) and both tile widths
        vars_ = [int(v) for v in os.environ.get("G4_VARS", "32,64").split(",")]
        gms = [int(v) for v in os.environ.get("G4_GMS", "0").split(",")]  # 0: the kernel's choice by shape
        vg = [(v, gm) for v in vars_ for gm in gms]

        def nm(p, v, gm):
            return f"{p}v{v}" + (f"g{gm}" if len(gms) > 1 else "")
        no_g8 = os.environ.get("G4_NO_G8") == "1"
        if epi == "swiglu":
            wi = ops.swiglu_interleave(w)
            runs = {"blas": lambda: ops.silu_mul(F.linear(x, wi), block=32),
                    "g8": lambda: ops.gemm8p(x, wi, swiglu=True, ws=ws)}
            runs.update({nm("g4", v, gm): (lambda v=v, gm=gm: ops.gemm4w(x, wi, swiglu=True, var=v, gm=gm)) for v, gm in vg})
        elif epi == "res":
            runs = {"blas": lambda: acc.addmm_(x, w.t()), "g8": lambda: ops.gemm8p(x, w, residual=acc, out=acc, ws=ws)}
            runs.update({nm("g4", v, gm): (lambda v=v, gm=gm: ops.gemm4w(x, w, residual=acc, out=acc, var=v, gm=gm))
                         for v, gm in vg})
        elif epi in ("bias", "gelu"):
            g = epi == "gelu"
            runs = {"blas": (lambda: torch._addmm_activation(b, x, w.t(), use_gelu=True)) if g
                    else (lambda: F.linear(x, w, b)),
                    "g8": lambda: ops.gemm8p(x, w, bias=b, gelu=g, ws=ws)}
            runs.update({nm("g4", v, gm): (lambda v=v, gm=gm: ops.gemm4w(x, w, bias=b, gelu=g, var=v, gm=gm))
                         for v, gm in vg})
        else:
            runs = {"blas": lambda: F.linear(x, w), "g8": lambda: ops.gemm8p(x, w, ws=ws)}
            runs.update({nm("g4", v, gm): (lambda v=v, gm=gm: ops.gemm4w(x, w, var=v, gm=gm)) for v, gm in vg})
            runs.update({nm("g4n192", v, gm): (lambda v=v, gm=gm: ops.gemm4w(x, w, bn=192, var=v, gm=gm))
                         for v, gm in vg})
        if no_g8:
            runs.pop("g8", None)
        res = {k: [] for k in runs}
        for _ in range(5):
            for k, fn in runs.items():
                res[k].append(timeit(fn, iters=10, warm=2))
        fl = 2 * M * N * K / 1e12
        line = "  ".join(f"{k} {sorted(t)[2]:8.1f} us ({fl / sorted(t)[2] * 1e6:5.0f})" for k, t in res.items())
        print(f"g4ab {M}x{N}x{K} {epi}: {line}", flush=True)
        del x, w, acc


def attention(dev):
    from llm_weighted_consensus_amd import ops

    Hq, Hkv, D, BS = 32, 8, 128, 16
    for B, ctx_len in [(256, 320), (512, 320), (64, 2048), (8, 4096)]:
        nb = (ctx_len + BS - 1) // BS
        NB = B * nb + 8
        kc = torch.randn(NB, Hkv, BS, D, device=dev).to(torch.bfloat16)
        vc = torch.randn(NB, Hkv, BS // 4, D, 4, device=dev).to(torch.bfloat16)
        bt = torch.arange(B * nb, device=dev, dtype=torch.int32).view(B, nb)
        ctx = torch.full((B,), ctx_len, device=dev, dtype=torch.int32)
        q = torch.randn(B, (Hq + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
        for splits in (1, 2, 4, 8):
            us = timeit(lambda: ops.paged_decode(q, kc, vc, bt, ctx, Hq, 1 / math.sqrt(D), num_splits=splits))
            gb = B * ctx_len * Hkv * D * 2 * 2 / (us * 1e-6) / 1e9
            print(f"paged_decode B={B:4d} ctx={ctx_len:5d} splits={splits}: {us:8.1f} us {gb:7.0f} GB/s", flush=True)


def attention_prefix(dev):
    """The bench's decode attention: R groups of N candidates sharing a 256-token prompt, suffix of
    `gen` tokens each — prefix (cascade) pass + suffix pass vs plain, both kernel paths."""
    from llm_weighted_consensus_amd import ops

    Hq, Hkv, D, BS = 32, 8, 128, 16
    cases = [(16, 64, 16, 64), (48, 64, 16, 64), (48, 64, 16, 120), (64, 64, 16, 64)]
    if os.environ.get("MICRO_PREFIX_QUICK"):
        cases = [(48, 64, 16, 64), (64, 64, 16, 64)]
    for (R, N, P, gen) in cases:
        B = R * N
        sblk = (gen + 1 + BS - 1) // BS
        NB = R * P + B * sblk + 8
        kc = torch.randn(NB, Hkv, BS, D, device=dev).to(torch.bfloat16)
        vc = torch.randn(NB, Hkv, BS // 4, D, 4, device=dev).to(torch.bfloat16)
        width = P + sblk
        bt = torch.zeros(B, width, dtype=torch.int32)
        for r in range(R):
            bt[r * N:(r + 1) * N, :P] = torch.arange(r * P, (r + 1) * P, dtype=torch.int32)
        bt[:, P:] = (R * P + torch.arange(B * sblk, dtype=torch.int32)).view(B, sblk)
        bt = bt.to(dev)
        ctx = torch.full((B,), P * BS + gen + 1, device=dev, dtype=torch.int32)
        q = torch.randn(B, (Hq + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
        per = 16 // (Hq // Hkv)
        sc = 1 / math.sqrt(D)
        for path, thr in (() if os.environ.get("MICRO_PREFIX_QUICK") else (("wg4", 1 << 30), ("wave", 0))):
            old = ops.set_decode_wave_min_items(thr)
            t_plain = timeit(lambda: ops.paged_decode(q, kc, vc, bt, ctx, Hq, sc))
            ops.set_decode_wave_min_items(old)
            print(f"plain decode R={R} N={N} P={P * BS} gen={gen} [{path}]: {t_plain:7.1f} us", flush=True)
        from llm_weighted_consensus_amd.engine.engine import cascade_table_size, cascade_tiles
        import numpy as np

        per_t = ops.cascade_rows_per_tile(Hq // Hkv)
        ct = np.zeros((cascade_table_size(B, per_t), 3), dtype=np.int32)
        nt = cascade_tiles([(r * N, N, P) for r in range(R)], per_t, ct)
        ct_exact = torch.from_numpy(ct[:nt].copy()).to(dev)
        ct = torch.from_numpy(ct).to(dev)
        t_exact = timeit(lambda: ops.paged_decode_cascade(q, kc, vc, bt, ctx, ct_exact, Hq, sc))
        print(f"  cascade exact grid ({nt} tiles): {t_exact:7.1f} us", flush=True)
        t_c = timeit(lambda: ops.paged_decode_cascade(q, kc, vc, bt, ctx, ct, Hq, sc))
        for pairs in os.environ.get("CASCADE_PAIRS", "").split(","):
            if pairs:
                os.environ["LWC_CASCADE_PAIRS"] = pairs
                tp_ = [timeit(lambda: ops.paged_decode_cascade(q, kc, vc, bt, ctx, ct, Hq, sc)) for _ in range(3)]
                print(f"  cascade LDS pairs={pairs}: {sorted(tp_)[1]:7.1f} us", flush=True)
        os.environ.pop("LWC_CASCADE_PAIRS", None)
        ref_o = ops.paged_decode(q, kc, vc, bt, ctx, Hq, sc)
        got = ops.paged_decode_cascade(q, kc, vc, bt, ctx, ct, Hq, sc)
        err = (got.float() - ref_o.float()).abs().max().item()
        print(f"cascade-decode R={R} N={N} P={P * BS} gen={gen}: {t_c:7.1f} us  (max|diff| vs plain {err:.3g})",
              flush=True)
        # decomposition: prefix only (ctx = prompt), suffix only (own blocks moved to the front, no prefix)
        ctx_p = torch.full((B,), P * BS, device=dev, dtype=torch.int32)
        t_p = timeit(lambda: ops.paged_decode_cascade(q, kc, vc, bt, ctx_p, ct, Hq, sc))
        bt_s = torch.zeros_like(bt)
        bt_s[:, :sblk] = bt[:, P:]
        ctx_s = torch.full((B,), gen + 1, device=dev, dtype=torch.int32)
        ct_s = np.zeros((cascade_table_size(B, per_t), 3), dtype=np.int32)
        cascade_tiles([(0, B, 0)], per_t, ct_s)
        ct_s = torch.from_numpy(ct_s).to(dev)
        t_s = timeit(lambda: ops.paged_decode_cascade(q, kc, vc, bt_s, ctx_s, ct_s, Hq, sc))
        ctx_f = torch.full((B,), P * BS + gen + 1, device=dev, dtype=torch.int32)
        t_f = timeit(lambda: ops.paged_decode_cascade(q, kc, vc, bt, ctx_f, ct_s, Hq, sc))
        print(f"  cascade parts: prefix-only {t_p:7.1f} us  suffix-only {t_s:7.1f} us  "
              f"no-sharing full ctx {t_f:7.1f} us", flush=True)


def decode_shapes(dev):
    """One cascade decode attention layer at head_dim 64 and 128 (Hkv 8, G 4): B = 4096 sequences in 64 groups of
    64 candidates, a 128-token shared prompt and 64 generated tokens each.  The two shapes alternate inside one
    run (5 rounds of 50 launches each, median); bytes are what the algorithm needs: the prompt's K and V once
    per (super-tile, KV head), every sequence's own K and V, q in and the output out."""
    import numpy as np

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.engine.engine import cascade_table_size, cascade_tiles

    Hkv, G, BS, R, N, P, gen = 8, 4, 16, 64, 64, 8, 64
    Hq, B, sblk = Hkv * G, R * N, gen // BS
    per_t = ops.cascade_rows_per_tile(G)
    ct = np.zeros((cascade_table_size(B, per_t), 3), dtype=np.int32)
    nt = cascade_tiles([(r * N, N, P) for r in range(R)], per_t, ct)
    ct = torch.from_numpy(ct).to(dev)
    bt = torch.zeros(B, P + sblk, dtype=torch.int32)
    for r in range(R):
        bt[r * N:(r + 1) * N, :P] = torch.arange(r * P, (r + 1) * P, dtype=torch.int32)
    bt[:, P:] = (R * P + torch.arange(B * sblk, dtype=torch.int32)).view(B, sblk)
    bt = bt.to(dev)
    ctx = torch.full((B,), P * BS + gen, device=dev, dtype=torch.int32)
    runs, nbytes = {}, {}
    for D in (64, 128):
        NB = R * P + B * sblk + 8
        kc = torch.randn(NB, Hkv, BS, D, device=dev).to(torch.bfloat16)
        vc = torch.randn(NB, Hkv, BS // 4, D, 4, device=dev).to(torch.bfloat16)
        q = torch.randn(B, (Hq + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
        out = torch.empty(B, Hq, D, device=dev, dtype=torch.bfloat16)
        runs[D] = (lambda q=q, kc=kc, vc=vc, out=out, D=D:
                   ops.paged_decode_cascade(q, kc, vc, bt, ctx, ct, Hq, 1 / math.sqrt(D), out=out))
        nbytes[D] = 2 * 2 * D * Hkv * (nt * P * BS + B * gen) + 2 * 2 * B * Hq * D
        got = runs[D]().float()
        ref_o = ops.paged_decode(q, kc, vc, bt, ctx, Hq, 1 / math.sqrt(D)).float()
        print(f"decode-shapes D={D}: max|cascade - plain| {(got - ref_o).abs().max().item():.3g}", flush=True)
    times = {D: [] for D in runs}
    for _ in range(5):
        for D in runs:
            times[D].append(timeit(runs[D]))
    for D in runs:
        t = sorted(times[D])
        print(f"decode-shapes cascade Hkv={Hkv} G={G} D={D} B={B} prompt={P * BS} gen={gen} ({nt} tiles): "
              f"median {t[2]:7.1f} us (min {t[0]:.1f}, max {t[4]:.1f}), {nbytes[D] / 1e6:.1f} MB needed, "
              f"{nbytes[D] / t[2] / 1e6:.2f} TB/s", flush=True)


def prefill_attn(dev):
    """Chunk-prefill attention: queries = the last q rows of a k-key range, keys contiguous (cached-prefix
    path, after kv_gather) vs paged (block tables, the mixed chunked-prefill path); + the gather itself."""
    from llm_weighted_consensus_amd import ops

    Hq, Hkv, D, BS = 32, 8, 128, 16
    sc = 1 / math.sqrt(D)
    for n, ql, kl in [(1, 512, 512), (1, 512, 2048), (1, 512, 4096), (4, 256, 512), (1, 2048, 2048)]:
        nbs = -(-kl // BS)
        NB = n * nbs + 8
        kc = torch.randn(NB, Hkv, BS, D, device=dev).to(torch.bfloat16)
        vc = torch.randn(NB, Hkv, BS // 4, D, 4, device=dev).to(torch.bfloat16)
        W = 2 * -(-kl // 32)
        bt = torch.zeros(n, W, dtype=torch.int32)
        perm = torch.randperm(NB - 8, dtype=torch.int32)
        for i in range(n):
            bt[i, :nbs] = perm[i * nbs:(i + 1) * nbs]
        bt = bt.to(dev)
        q = torch.randn(n * ql, (Hq + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
        cu_q = torch.arange(n + 1, device=dev, dtype=torch.int32) * ql
        cu_k = torch.arange(n + 1, device=dev, dtype=torch.int32) * kl
        k_lens = torch.full((n,), kl, device=dev, dtype=torch.int32)
        toks = torch.arange(kl, device=dev)
        slots = torch.cat([bt[i, toks // BS].long() * BS + toks % BS for i in range(n)])
        kf, vf = ops.kv_gather(kc, vc, slots)
        t_g = timeit(lambda: ops.kv_gather(kc, vc, slots))
        t_c = timeit(lambda: ops.prefill_attention(q[:, : Hq * D], kf, vf, cu_q, ql, Hq, Hkv, D, sc, True,
                                                   cu_seqlens_k=cu_k, lens=([ql] * n, [kl] * n)))
        t_p = timeit(lambda: ops.prefill_attention_paged(q, kc, vc, cu_q, bt, k_lens, ql, Hq, sc))
        fl = n * 4 * Hq * D * ql * (kl - ql / 2) / 1e12
        print(f"pfattn {n} x q{ql} k{kl}: gather {t_g:7.1f} us  contiguous {t_c:7.1f} us ({fl / t_c * 1e6:4.0f} TF/s)  "
              f"paged {t_p:7.1f} us ({fl / t_p * 1e6:4.0f} TF/s)", flush=True)


def bandwidth(dev):
    """HBM calibration: streaming read (sum), copy (read + write), and 4 KiB-segment gathers in random order
    (the decode attention's access pattern) — bytes moved / time."""
    n = 1 << 30  # 2 GiB of bf16
    x = torch.empty(n, dtype=torch.bfloat16, device=dev).normal_()
    y = torch.empty_like(x)
    us = timeit(lambda: x.sum(), iters=10)
    print(f"bw read (sum)          : {2 * n / us / 1e3:7.0f} GB/s", flush=True)
    us = timeit(lambda: x.view(-1, 4096).amax(dim=1), iters=10)
    print(f"bw read (row amax)     : {2 * n / us / 1e3:7.0f} GB/s", flush=True)
    us = timeit(lambda: y.copy_(x), iters=10)
    print(f"bw copy (r + w)        : {4 * n / us / 1e3:7.0f} GB/s", flush=True)
    seg = x.view(-1, 2048)  # 4 KiB rows
    idx = torch.randperm(seg.shape[0], device=dev)[: seg.shape[0] // 2]
    us = timeit(lambda: seg.index_select(0, idx), iters=10)
    print(f"bw 4KiB gather (r + w) : {2 * idx.numel() * 4096 / us / 1e3:7.0f} GB/s", flush=True)
    lg = torch.randn(4096, 128256, device=dev).to(torch.bfloat16)
    us = timeit(lambda: lg.amax(dim=1), iters=10)
    print(f"logits [4096, 128256] row amax: {us:7.1f} us ({lg.numel() * 2 / us / 1e3:5.0f} GB/s)", flush=True)
    us = timeit(lambda: torch.softmax(lg, dim=1), iters=5)
    print(f"logits [4096, 128256] softmax (r + w): {us:7.1f} us", flush=True)


def moe_decode(dev):
    """Mixtral decode MoE at the config-5 batch: fp8 experts, T tokens x top-2 over 8 experts, balanced and
    router-driven (uneven) segments; time and the expert-weight bytes streamed per second."""
    from llm_weighted_consensus_amd import ops

    E, d, f = 8, 4096, 14336
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = (torch.randn(E, 2 * f, d, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    w2 = (torch.randn(E, d, f, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    q13, s13 = ops.quant_fp8_weight(w13)
    q2, s2 = ops.quant_fp8_weight(w2)
    del w13, w2
    router = (torch.randn(E, d, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    for T in [int(t) for t in os.environ.get("MICRO_MOE_T", "512,2048").split(",")]:
        rows = 2 * T
        h = torch.randn(T, d, device=dev, generator=g).to(torch.bfloat16)
        _ids, _w, off_r, src, _inv = ops.moe_route(torch.nn.functional.linear(h, router), 2)
        sizes = torch.full((E,), rows // E, dtype=torch.int64)
        off_b = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
        hq, hs = ops.quant_fp8_rows(h)
        act = torch.randn(rows, f, device=dev, generator=g).to(torch.bfloat16)
        aq, as_ = ops.quant_fp8_rows(act)
        for label, off in (("balanced", off_b), ("routed", off_r)):
            t13 = timeit(lambda: ops.grouped_gemm(hq, q13, off, a_rows=src, rows=rows, a_scale=hs, w_scale=s13), iters=20)
            t2 = timeit(lambda: ops.grouped_gemm(aq, q2, off, a_scale=as_, w_scale=s2), iters=20)
            mx = int((off[1:] - off[:-1]).max())
            print(f"moe fp8 T={T:5d} {label:8s} (max rows/expert {mx:4d}): w13 {t13:7.1f} us "
                  f"({q13.numel() / t13 / 1e3:5.0f} GB/s of weights)  w2 {t2:7.1f} us ({q2.numel() / t2 / 1e3:5.0f} GB/s)",
                  flush=True)


def sampler(dev):
    from llm_weighted_consensus_amd import ops

    V = 128256
    for B in (512, 4096):
        logits = (torch.randn(B, V, device=dev) * 2).to(torch.bfloat16)
        f = lambda v: torch.full((B,), float(v), device=dev)
        seeds = torch.arange(B, device=dev, dtype=torch.int64)
        offs = torch.zeros(B, device=dev, dtype=torch.int64)
        tk = torch.zeros(B, dtype=torch.int32, device=dev)
        for label, tp, K, T in [("greedy", 1.0, 0, 0.0), ("temp", 1.0, 0, 0.8), ("top_p", 0.95, 0, 0.8),
                                ("top_p+lp20", 0.95, 20, 0.8)]:
            us = timeit(lambda: ops.sample(logits, f(T), f(tp), tk, f(0), f(0), seeds, offs, num_logprobs=K),
                        iters=20)
            print(f"sample B={B} {label:10s}: {us:8.1f} us  {B * V * 2 / (us * 1e-6) / 1e9:7.0f} GB/s", flush=True)


def small(dev):
    from llm_weighted_consensus_amd import ops

    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache, rope_tables

    cfg = decoder_config("llama-3-8b")
    cos, sin = rope_tables(cfg, dev, 4096)
    for T in (512, 3072, 4096):
        cache = KVCache(cfg, T + 64, 16, dev)
        qkv = torch.randn(T, cfg.qkv_dim, device=dev).to(torch.bfloat16)
        pos = torch.randint(0, 4000, (T,), device=dev, dtype=torch.int32)
        slots = (torch.randperm(T, device=dev).to(torch.int32) * 16 + 5)
        us = timeit(lambda: ops.rope_kv_write(qkv, pos, cos, sin, cache.k[0], cache.v[0], 32, 8, 128, slots=slots))
        us_k = timeit(lambda: ops.rope_kv_write(qkv, pos, cos, sin, cache.k[0], cache.v[0], 32, 8, 128, slots=slots,
                                                rope_q=False))
        print(f"rope_kv_write T={T}: {us:6.1f} us   k only (q rotated in the decode kernels): {us_k:6.1f} us",
              flush=True)
    for T in (512, 3072):
        x = torch.randn(T, 4096, device=dev).to(torch.bfloat16)
        r = torch.randn(T, 4096, device=dev).to(torch.bfloat16)
        w = torch.ones(4096, device=dev, dtype=torch.bfloat16)
        us = timeit(lambda: ops.rmsnorm(x, w, 1e-5, residual=r))
        print(f"rmsnorm+res T={T}: {us:6.1f} us", flush=True)
        gu = torch.randn(T, 2 * 14336, device=dev).to(torch.bfloat16)
        us = timeit(lambda: ops.silu_mul(gu))
        print(f"silu_mul T={T}: {us:6.1f} us", flush=True)


def encoder_gemms(dev):
    """The encoders' small-K projections (config 2 bge-base: d = 768, FFN 3072; bge-large: 1024 / 4096) at
    ENC_M tokens: hipBLASLt (bias / bias+GELU epilogue) vs gemm8p, gemm4w (VAR 32) and gemm4w VAR 64 (next
    tile's prologue under the epilogue, polynomial GELU), g4p192 its 256 x 192 tiles.  Median of 5 interleaved
    rounds."""
    import torch.nn.functional as F

    from llm_weighted_consensus_amd import ops

    M = int(os.environ.get("ENC_M", "524288"))  # config 2: 64 requests x 64 candidates x 128 tokens
    d = int(os.environ.get("ENC_D", "768"))
    shapes = [(3 * d, d, False), (d, d, False), (4 * d, d, True), (d, 4 * d, False)]
    for N, K, gelu in shapes:
        x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16)
        b = (torch.randn(N, device=dev) * 0.1).to(torch.bfloat16)
        runs = {
            "blas": (lambda: torch._addmm_activation(b, x, w.t(), use_gelu=True)) if gelu else (lambda: F.linear(x, w, b)),
            # (gemm8p addresses A through one 32-bit buffer range: no A of 2 GiB or more)
            **({"g8": lambda: ops.gemm8p(x, w, bias=b, gelu=gelu)} if x.numel() * 2 < (1 << 31) else {}),
            "g4": lambda: ops.gemm4w(x, w, bias=b, gelu=gelu),
            "g4p": lambda: ops.gemm4w(x, w, bias=b, gelu=gelu, var=64),
            "g4p192": lambda: ops.gemm4w(x, w, bias=b, gelu=gelu, var=64, bn=192),
        }
        res = {k: [] for k in runs}
        for _ in range(5):
            for k, fn in runs.items():
                res[k].append(timeit(fn, iters=5, warm=1))
        line = "  ".join(f"{k} {sorted(t)[2]:8.1f}" for k, t in res.items())
        print(f"enc M={M} {N}x{K}{' gelu' if gelu else ''}: {line} us", flush=True)
        del x, w


def skinny_ab(dev):
    """Decode-sized projections (serving decode buckets): hipBLASLt vs the skinny weight-stream GEMM
    (skinny.hip) for Llama-3-8B's projections, plain and residual, median of 5 interleaved rounds; TB/s = W
    bytes / time."""
    import torch.nn.functional as F

    from llm_weighted_consensus_amd import ops

    shapes = [(6144, 4096, False), (4096, 4096, True), (28672, 4096, False), (4096, 14336, True),
              (128256, 4096, False)]  # (28672: gate|up with SwiGLU)
    for M in [int(m) for m in os.environ.get("SKINNY_M", "2,8,16,32,64").split(",")]:
        for N, K, res in shapes:
            x = ((torch.rand(M, K, device=dev) * 2 - 1)).to(torch.bfloat16)
            # rotate over enough weight copies to exceed the 256 MB last-level cache (a decode step streams
            # 32 layers of different weights)
            nw = max(1, min(16, (768 << 20) // (N * K * 2)))
            ws = [((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16) for _ in range(nw)]
            it = [0]

            def nxt():
                it[0] = (it[0] + 1) % nw
                return ws[it[0]]
            acc = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
            if res:
                runs = {"blas": lambda: acc.addmm_(x, nxt().t()),
                        "gv": lambda: ops.skinny_gemm(x, nxt(), residual=acc, out=acc)}
            elif N == 28672:  # gate|up: library + silu_mul vs the skinny SwiGLU epilogue
                runs = {"blas": lambda: ops.silu_mul(F.linear(x, nxt()), block=32),
                        "gv": lambda: ops.skinny_gemm(x, nxt(), swiglu=True)}
            else:
                runs = {"blas": lambda: F.linear(x, nxt()), "gv": lambda: ops.skinny_gemm(x, nxt())}
            t = {k: [] for k in runs}
            for _ in range(5):
                for k, fn in runs.items():
                    t[k].append(timeit(fn, iters=20, warm=3))
            gb = N * K * 2 / 1e12
            line = "  ".join(f"{k} {sorted(v)[2]:7.1f} us ({gb / sorted(v)[2] * 1e6:4.1f} TB/s)" for k, v in t.items())
            print(f"skinny M={M} {N}x{K}{' res' if res else ''}: {line}", flush=True)
            del x, ws, acc


def _rand_mx(dev, N, K):  # timing only: any codes, scales near 2^-6
    from llm_weighted_consensus_amd import ops

    q = torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8)
    s = torch.randint(117, 125, (N, K // 32), device=dev, dtype=torch.uint8)
    return ops.Mxfp4Weight.from_packed(q, s)


def _rotating(items):
    it = [0]

    def nxt():
        it[0] = (it[0] + 1) % len(items)
        return items[it[0]]
    return nxt


def _graph_medians(runs, iters, rounds=7):
    """us per call: each arm captured as one graph of ``iters`` calls (the serving decode step is a captured
    graph: eager launches of kernels this short time the host, not the device), replays interleaved."""
    graphs = {}
    for k, fn in runs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(iters):
                fn()
        graphs[k].replay()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            t[k].append(s.elapsed_time(e) / iters * 1e3)
    return {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def _decode_step_ms(model, cfg, dev, B):
    """Median ms of one captured decode step of B rows at position 32 (23 replays, the first 3 dropped)."""
    from llm_weighted_consensus_amd.models.llama import KVCache

    i32 = dict(dtype=torch.int32, device=dev)
    pos = 32
    cache = KVCache(cfg, 3 * B, 16, dev)
    bt = torch.arange(3 * B, **i32).view(B, 3)
    positions, ctx = torch.full((B,), pos, **i32), torch.full((B,), pos + 1, **i32)
    slots = (bt[:, 2] * 16).contiguous()
    tokens = torch.randint(0, cfg.vocab_size, (B,), device=dev).int()
    model.tune_gemms(B)

    def fwd():
        return model.decode(tokens, positions, slots, bt, ctx, cache, num_splits=1)

    for _ in range(2):
        fwd()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fwd()
    ts = []
    for _ in range(23):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ts = sorted(ts[3:])
    return ts[len(ts) // 2], ts[0], ts[-1]


def mxfp4a8_ab(dev):
    """MXFP4 weights with e4m3 activations (ops.gemm_mxfp4_a8, profiles/mxfp4_a8.md) at the Llama-3-8B shapes, arms
    interleaved in one process, median of 7 rounds, weights rotated over more copies than the last-level cache holds:
    (a) per projection and M in {33, 48, 64, 128, 512, 2048, 4096} (MX_M overrides): the W4A8 kernel — for o and
        down with the activation's quant_fp8_rows pass, which no norm fuses (the kernel alone is printed too); qkv
        and gate|up read the fused norm's QAct —, the parent path ops.linear_mxfp4 / swiglu_mxfp4 (weight stream up
        to 64 rows, dequantise + the planner's bf16 GEMM above), the planner's bf16 GEMM on a bf16 weight, and
        gemm8g_dense on an Fp8Weight of the same shape;
    (b) one llama-3-8b random-weight decode step (captured graph) at B in {128, 4096} (MX_B overrides):
        bf16 / mxfp4 / mxfp4 + e4m3.
    MX_PARTS=a,b selects the parts."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from llm_weighted_consensus_amd.ops import gemm_plan

    parts = os.environ.get("MX_PARTS", "a,b").split(",")
    shapes = [("qkv", 6144, 4096, False, True), ("o", 4096, 4096, False, False),
              ("gate_up", 28672, 4096, True, True), ("down", 4096, 14336, False, False)]  # (.., swiglu, norm-fused)
    Ms = [int(m) for m in os.environ.get("MX_M", "33,48,64,128,512,2048,4096").split(",")]
    for name, N, K, sw, fused in shapes if "a" in parts else []:
        nw = max(2, min(16, (768 << 20) // (N * K * 2)))
        wb = _rotating([((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16) for _ in range(nw)])
        w8 = _rotating([ops.Fp8Weight(wb()) for _ in range(2 * nw)])
        wm = _rotating([_rand_mx(dev, N, K) for _ in range(4 * nw)])
        scratch = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
        for M in Ms:
            x = (torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16)
            xq, xs = ops.quant_fp8_rows(x)
            gemm_plan.tune(x, wb(), "swiglu" if sw else "plain", 32 if sw else 0)  # parent and bf16 arms run its choice
            runs = {"a8 kernel": lambda: ops.gemm_mxfp4_a8(xq, xs, wm(), swiglu=sw),
                    "fp8": lambda: ops.gemm8g_dense(xq, xs, w8(), swiglu=sw)}
            if not fused:
                runs["a8"] = lambda: ops.linear_mxfp4_a8(x, wm())
            if sw:
                runs["parent"] = lambda: ops.swiglu_mxfp4(x, wm(), 32, scratch)
                runs["bf16"] = lambda: gemm_plan.swiglu(x, wb(), 32)
            else:
                runs["parent"] = lambda: ops.linear_mxfp4(x, wm(), scratch)
                runs["bf16"] = lambda: gemm_plan.linear(x, wb())
            t = _graph_medians(runs, 20 if M <= 128 else 6 if M <= 512 else 3)
            a8 = t["a8 kernel" if fused else "a8"]
            tf = 2.0 * M * N * K / a8 / 1e6
            print(f"mxfp4a8 (a) {name} {N}x{K} M={M}: a8 {a8:8.1f} us ({tf:6.0f} TF/s"
                  f"{'' if fused else ', kernel alone %.1f us' % t['a8 kernel']})  parent {t['parent']:8.1f} us  "
                  f"bf16[{gemm_plan.choice(M, N, K, 'swiglu' if sw else 'plain')}] {t['bf16']:8.1f} us  "
                  f"fp8 g8g {t['fp8']:8.1f} us  a8/parent {a8 / t['parent']:.2f}x"
                  f"{'  SLOWER than parent' if a8 > t['parent'] else ''}", flush=True)
        del wb, w8, wm, scratch
        torch.cuda.empty_cache()
    if "b" not in parts:
        return
    cfg = decoder_config("llama-3-8b")
    for label, kw in (("bf16", {}), ("mxfp4", {"mxfp4": True}), ("mxfp4+e4m3", {"mxfp4": True, "mxfp4_act": "e4m3"})):
        torch.cuda.empty_cache()
        model = LlamaModel(cfg, device=dev, seed=0, max_position=256, **kw)
        torch.cuda.synchronize()
        print(f"mxfp4a8 (b) llama-3-8b [{label}]: {torch.cuda.memory_allocated(dev) / 2 ** 30:.1f} GiB allocated, "
              f"scratch {0 if model.mx_scratch is None else model.mx_scratch.nbytes >> 20} MiB", flush=True)
        for B in [int(b) for b in os.environ.get("MX_B", "128,4096").split(",")]:
            med, lo, hi = _decode_step_ms(model, cfg, dev, B)
            print(f"mxfp4a8 (b) llama-3-8b [{label}] decode step B={B}: median {med:.3f} ms (min {lo:.3f}, "
                  f"max {hi:.3f})", flush=True)
        del model
        torch.cuda.empty_cache()


def mxfp4_ab(dev):
    """MXFP4 weight-only projections at the Llama-3-8B shapes (profiles/mxfp4.md), arms interleaved in one
    process, median of 7 rounds, weights rotated over more copies than the last-level cache holds:
    (a) M <= 64: skinny_mxfp4 vs ops.skinny_gemm on a bf16 weight vs the planner's bf16 choice, us and weight GB/s
        (each arm's own weight bytes);
    (b) M > 64: dequantise + GEMM (ops.linear_mxfp4 / swiglu_mxfp4) vs the GEMM alone, and the dequantisation alone;
    (c) one llama-3-8b random-weight decode step (captured graph) at B in {1, 16, 64}, bf16 vs mxfp4, with the KV
        blocks LLMEngine's sizing rule (kv_memory_fraction 0.85 of the free memory) gives each.
    MX_PARTS=a,b,c selects the parts."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache, LlamaModel
    from llm_weighted_consensus_amd.ops import gemm_plan

    parts = os.environ.get("MX_PARTS", "a,b,c").split(",")
    shapes = [("qkv", 6144, 4096, False), ("o", 4096, 4096, False), ("gate_up", 28672, 4096, True),
              ("down", 4096, 14336, False)]

    for name, N, K, sw in shapes:
        if not ({"a", "b"} & set(parts)):
            break
        nw = max(2, min(16, (768 << 20) // (N * K * 2)))
        wb = _rotating([((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16) for _ in range(nw)])
        wm = _rotating([_rand_mx(dev, N, K) for _ in range(4 * nw)])  # (a quarter of the bytes each)
        scratch = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
        mxb, bfb = N * K * (0.5 + 1 / 32), N * K * 2.0
        for M in ([int(m) for m in os.environ.get("MX_M", "1,8,16,32,64").split(",")] if "a" in parts else []):
            x = (torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16)
            gemm_plan.tune(x, wb(), "swiglu" if sw else "plain", 32 if sw else 0)
            if sw:
                runs = {"mxfp4": lambda: ops.skinny_mxfp4(x, wm(), swiglu=True),
                        "gv": lambda: ops.skinny_gemm(x, wb(), swiglu=True),
                        "planner": lambda: gemm_plan.swiglu(x, wb(), 32)}
            else:
                runs = {"mxfp4": lambda: ops.skinny_mxfp4(x, wm()), "gv": lambda: ops.skinny_gemm(x, wb()),
                        "planner": lambda: gemm_plan.linear(x, wb())}
            t = _graph_medians(runs, 20)
            ch = gemm_plan.choice(M, N, K, "swiglu" if sw else "plain")
            print(f"mxfp4 (a) {name} {N}x{K} M={M}: mxfp4 {t['mxfp4']:7.1f} us ({mxb / t['mxfp4'] / 1e3:6.0f} GB/s)  "
                  f"gv {t['gv']:7.1f} us ({bfb / t['gv'] / 1e3:6.0f} GB/s)  planner[{ch}] {t['planner']:7.1f} us "
                  f"({bfb / t['planner'] / 1e3:6.0f} GB/s)  gv/mxfp4 {t['gv'] / t['mxfp4']:.2f}x", flush=True)
        for M in ([128, 512, 2048] if "b" in parts else []):
            x = (torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16)
            gemm_plan.tune(x, wb(), "swiglu" if sw else "plain", 32 if sw else 0)  # both arms run its choice
            if sw:
                runs = {"dq+gemm": lambda: ops.swiglu_mxfp4(x, wm(), 32, scratch),
                        "gemm": lambda: gemm_plan.swiglu(x, wb(), 32)}
            else:
                runs = {"dq+gemm": lambda: ops.linear_mxfp4(x, wm(), scratch), "gemm": lambda: gemm_plan.linear(x, wb())}
            runs["dq"] = lambda: ops.mxfp4_dequant(wm(), scratch.view(N, K))
            t = _graph_medians(runs, 10)
            print(f"mxfp4 (b) {name} {N}x{K} M={M}: dequant+gemm {t['dq+gemm']:7.1f} us  gemm {t['gemm']:7.1f} us  "
                  f"dequant alone {t['dq']:6.1f} us ({(mxb + bfb) / t['dq'] / 1e3:5.0f} GB/s read+written)  "
                  f"+{(t['dq+gemm'] / t['gemm'] - 1) * 100:.0f} %", flush=True)
        del wb, wm, scratch
        torch.cuda.empty_cache()
    if "c" not in parts:
        return
    cfg = decoder_config("llama-3-8b")
    i32 = dict(dtype=torch.int32, device=dev)
    for label, kw in (("bf16", {}), ("mxfp4", {"mxfp4": True})):
        torch.cuda.empty_cache()
        model = LlamaModel(cfg, device=dev, seed=0, max_position=256, **kw)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(dev)
        blocks = int(free * 0.85) // KVCache.bytes_per_block(cfg, 16)
        print(f"mxfp4 (c) llama-3-8b [{label}]: {torch.cuda.memory_allocated(dev) / 2 ** 30:.1f} GiB allocated, "
              f"{free / 2 ** 30:.1f} GiB free -> {blocks} KV blocks of 16 tokens", flush=True)
        for B in (1, 16, 64):
            pos = 32
            cache = KVCache(cfg, 3 * B, 16, dev)
            bt = torch.arange(3 * B, **i32).view(B, 3)
            positions, ctx = torch.full((B,), pos, **i32), torch.full((B,), pos + 1, **i32)
            slots = (bt[:, 2] * 16).contiguous()
            tokens = torch.randint(0, cfg.vocab_size, (B,), device=dev).int()
            model.tune_gemms(B)

            def fwd():
                return model.decode(tokens, positions, slots, bt, ctx, cache, num_splits=1)

            for _ in range(2):
                fwd()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fwd()
            ts = []
            for _ in range(23):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                g.replay()
                e.record()
                e.synchronize()
                ts.append(s.elapsed_time(e))
            ts = sorted(ts[3:])
            print(f"mxfp4 (c) llama-3-8b [{label}] decode step B={B}: median {ts[len(ts) // 2]:.3f} ms "
                  f"(min {ts[0]:.3f}, max {ts[-1]:.3f})", flush=True)
            del g, cache
        del model
        torch.cuda.empty_cache()


def serve_shapes(dev):
    """Llama-3-8B projections at the serving path's mixed chunked-prefill row counts (2048 prompt rows + the
    decode rows): every backend the planner times, median of 5 interleaved rounds (SERVE_M overrides)."""
    import torch.nn.functional as F

    from llm_weighted_consensus_amd import ops

    d, Fd, QKV = 4096, 14336, 6144
    r = lambda *s: ((torch.rand(*s, device=dev) * 2 - 1) / s[-1] ** 0.5).to(torch.bfloat16)  # noqa: E731
    wqkv, wo, wgu, wd = r(QKV, d), r(d, d), ops.swiglu_interleave(r(2 * Fd, d)), r(d, Fd)
    for M in [int(m) for m in os.environ.get("SERVE_M", "512,1024,2048,2304,2560,3072").split(",")]:
        x, xa, xf = r(M, d) * 8, r(M, d) * 8, r(M, Fd) * 8
        acc = torch.zeros(M, d, device=dev, dtype=torch.bfloat16)
        runs = {
            "qkv blas": lambda: F.linear(x, wqkv), "qkv g4": lambda: ops.gemm4w(x, wqkv),
            "qkv g4n192": lambda: ops.gemm4w(x, wqkv, bn=192), "qkv g8": lambda: ops.gemm8p(x, wqkv),
            "o blas": lambda: acc.addmm_(xa, wo.t()), "o g4": lambda: ops.gemm4w(xa, wo, residual=acc, out=acc),
            "o g8": lambda: ops.gemm8p(xa, wo, residual=acc, out=acc),
            "gu blas+silu": lambda: ops.silu_mul(F.linear(x, wgu), block=32),
            "gu g4": lambda: ops.gemm4w(x, wgu, swiglu=True), "gu g4p": lambda: ops.gemm4w(x, wgu, swiglu=True, var=64),
            "gu g8": lambda: ops.gemm8p(x, wgu, swiglu=True),
            "down blas": lambda: acc.addmm_(xf, wd.t()), "down g4": lambda: ops.gemm4w(xf, wd, residual=acc, out=acc),
            "down g8": lambda: ops.gemm8p(xf, wd, residual=acc, out=acc),
        }
        # split-K (VAR 64) where ops.split_plan splits the call or its ragged tail
        for k, (w, K, kw) in {"qkv": (wqkv, d, {}), "o": (wo, d, {"residual": acc, "out": acc}),
                              "gu": (wgu, d, {"swiglu": True}), "down": (wd, Fd, {"residual": acc, "out": acc})}.items():
            S, f = ops.split_plan(M, w.shape[0], K)
            if S > 1:
                a_ = xf if k == "down" else (xa if k == "o" else x)
                runs[f"{k} g4s{S}@{f}"] = (lambda a_=a_, w=w, kw=kw, S=S, f=f:
                                           ops.gemm4w(a_, w, var=64, splits=S, split_from=f, **kw))
            # SERVE_SPLITS: forced whole-call splits (any S: uneven K shares) for qkv / o / down
            for S in [int(v) for v in os.environ.get("SERVE_SPLITS", "").split(",") if v]:
                if k != "gu" and (K // 64) // 2 >= S:
                    a_ = xf if k == "down" else (xa if k == "o" else x)
                    runs[f"{k} g4s{S}"] = (lambda a_=a_, w=w, kw=kw, S=S:
                                           ops.gemm4w(a_, w, var=64, splits=S, split_from=0, **kw))
        if os.environ.get("SERVE_ONLY"):  # e.g. "o ,down ": arms whose name starts with one of these
            pre = tuple(os.environ["SERVE_ONLY"].split(","))
            runs = {k: v for k, v in runs.items() if k.startswith(pre)}
        res = {k: [] for k in runs}
        for _ in range(5):
            for k, fn in runs.items():
                res[k].append(timeit(fn, iters=10, warm=2))
        for k, t in res.items():
            print(f"serve M={M} {k}: {sorted(t)[2]:8.1f} us", flush=True)


def g48_ab(dev):
    """Dense fp8: gemm8g (dense mode) vs hipBLASLt's row-scaled fp8 GEMM at config 5's shapes (median of 5
    interleaved rounds; G48_SHAPES picks a subset).  (The 4-wave gemm4w8 arm was removed in round 6: 3-13 %
    behind gemm8g, profiles/fp8_4wave_r5.md, and its accumulators rotated through in-flight copies.)"""
    from llm_weighted_consensus_amd import ops

    shapes = [(4096, 6144, 4096), (4096, 4096, 4096), (4096, 4096, 14336), (16384, 6144, 4096), (8192, 4096, 14336),
              (65536, 6144, 4096)]
    only = os.environ.get("G48_SHAPES")
    if only:
        shapes = [shapes[int(i)] for i in only.split(",")]
    for M, N, K in shapes:
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        xq, xs = ops.quant_fp8_rows(x)
        del x
        w = ops.Fp8Weight((torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16))
        runs = {"blas": lambda: ops._fp8_blas(xq, xs, w), "g8g": lambda: ops.gemm8g_dense(xq, xs, w)}
        res = {k: [] for k in runs}
        for _ in range(5):
            for k, fn in runs.items():
                res[k].append(timeit(fn, iters=5, warm=1))
        fl = 2 * M * N * K / 1e12
        line = "  ".join(f"{k} {sorted(t)[2]:8.1f} us ({fl / sorted(t)[2] * 1e6:5.0f})" for k, t in res.items())
        print(f"g48 {M}x{N}x{K}: {line}", flush=True)
        del xq, xs, w


def route_ab(dev):
    """Config-5 MoE plumbing at the decode batch (T = 4096 tokens, Mixtral d = 4096, 8 experts, top-2):
    the router projection + route (unfused: F.linear then moe_route) vs the fused moe_router kernel, and
    the other small per-layer kernels around the experts.  Median of 5 interleaved rounds."""
    import torch.nn.functional as F

    from llm_weighted_consensus_amd import ops

    T, d, E = int(os.environ.get("ROUTE_T", "4096")), 4096, 8
    h = torch.randn(T, d, device=dev).to(torch.bfloat16)
    r = torch.randn(T, d, device=dev).to(torch.bfloat16)
    router = (torch.randn(E, d, device=dev) * 0.05).to(torch.bfloat16)
    ones = torch.ones(d, device=dev, dtype=torch.bfloat16)
    lg = F.linear(h, router)
    _ids, w, _ro, _src, inv = ops.moe_route(lg, 2)
    Y = torch.randn(2 * T, d, device=dev).to(torch.bfloat16)
    runs = {
        "router F.linear": lambda: F.linear(h, router),
        "moe_route (logits)": lambda: ops.moe_route(lg, 2),
        "unfused (linear + route)": lambda: ops.moe_route(F.linear(h, router), 2),
        "fused moe_router": lambda: ops.moe_router(h, router, 2),
        "rmsnorm+res+q (bf16 kept)": lambda: ops.rmsnorm_quant_fp8(h, ones, 1e-5, residual=r, keep_bf16=True),
        "rmsnorm+res": lambda: ops.rmsnorm(h, ones, 1e-5, residual=r),
        "quant_fp8_rows": lambda: ops.quant_fp8_rows(h),
        "moe_combine": lambda: ops.moe_combine(Y, inv, w, 2),
    }
    res = {k: [] for k in runs}
    for _ in range(5):
        for k, fn in runs.items():
            res[k].append(timeit(fn, iters=20, warm=3))
    for k, t in res.items():
        print(f"route T={T} {k}: {sorted(t)[2]:8.1f} us", flush=True)


def chain_ab(dev):
    """Folded-RMSNorm decode chain at the headline's decode batch (Llama-3-8B shapes, M = 4096; random
    operands): per projection the unfolded backends (hipBLASLt / gemm4w, + the norm kernel) vs the row-scaled
    gemm4w modes, then one whole layer + lm_head both ways.  Interleaved rounds, median of 5."""
    import torch.nn.functional as F

    from llm_weighted_consensus_amd import ops

    M, d, Fd, V, QKV = int(os.environ.get("CHAIN_M", "4096")), 4096, 14336, 128256, 6144
    r = lambda *s: ((torch.rand(*s, device=dev) * 2 - 1) / s[-1] ** 0.5).to(torch.bfloat16)  # noqa: E731
    x = (torch.rand(M, d, device=dev) * 2 - 1).to(torch.bfloat16)
    xa, xf = r(M, d) * 8, r(M, Fd) * 8
    wqkv, wo, wgu, wd, wl = r(QKV, d), r(d, d), ops.swiglu_interleave(r(2 * Fd, d)), r(d, Fd), r(V, d)
    ones = torch.ones(d, device=dev, dtype=torch.bfloat16)
    ch = ops.NormChain(M, d, 1e-5, dev)
    acc = x.clone()
    ops.rms_rowsumsq(acc, ch)
    runs = {
        "rmsnorm": lambda: ops.rmsnorm(acc, ones, 1e-5),
        "rowsumsq": lambda: ops.rms_rowsumsq(acc, ch),
        "qkv blas": lambda: F.linear(x, wqkv),
        "qkv g4n192": lambda: ops.gemm4w(x, wqkv, bn=192),
        "qkv g4n192 rs": lambda: ops.gemm4w(x, wqkv, bn=192, chain=ch),
        "qkv g4 rs": lambda: ops.gemm4w(x, wqkv, chain=ch),
        "o blas res": lambda: acc.addmm_(xa, wo.t()),
        "o g4 res": lambda: ops.gemm4w(xa, wo, residual=acc, out=acc),
        "o g4 res+ss": lambda: ops.gemm4w(xa, wo, residual=acc, out=acc, chain=ch),
        "o g4 res+ss v64": lambda: ops.gemm4w(xa, wo, residual=acc, out=acc, chain=ch, var=64),
        "gu g4": lambda: ops.gemm4w(x, wgu, swiglu=True),
        "gu g4 rs": lambda: ops.gemm4w(x, wgu, swiglu=True, chain=ch),
        "down blas res": lambda: acc.addmm_(xf, wd.t()),
        "down g4 res": lambda: ops.gemm4w(xf, wd, residual=acc, out=acc),
        "down g4 res+ss": lambda: ops.gemm4w(xf, wd, residual=acc, out=acc, chain=ch),
        "down g4 res+ss v64": lambda: ops.gemm4w(xf, wd, residual=acc, out=acc, chain=ch, var=64),
        "lm blas": lambda: F.linear(x, wl),
        "lm g4": lambda: ops.gemm4w(x, wl),
        "lm g4 v64": lambda: ops.gemm4w(x, wl, var=64),
        "lm g4 rs": lambda: ops.gemm4w(x, wl, chain=ch),
    }
    res = {k: [] for k in runs}
    for _ in range(5):
        for k, fn in runs.items():
            res[k].append(timeit(fn, iters=10, warm=2))
    for k, t in res.items():
        print(f"chain {M} {k}: {sorted(t)[2]:8.1f} us", flush=True)
    med = {k: sorted(t)[2] for k, t in res.items()}
    base = (2 * med["rmsnorm"] + min(med["qkv blas"], med["qkv g4n192"]) + med["o blas res"] + med["gu g4"]
            + med["down blas res"])
    chain = (med["qkv g4n192 rs"] + min(med["o g4 res+ss"], med["o g4 res+ss v64"]) + med["gu g4 rs"]
             + min(med["down g4 res+ss"], med["down g4 res+ss v64"]))
    print(f"chain {M} per layer: unfolded {base:.1f} us, chain {chain:.1f} us; lm_head: unfolded "
          f"{med['rmsnorm'] + med['lm blas']:.1f}, chain {med['lm g4 rs']:.1f}", flush=True)


def lora_kernels(dev):
    """Batched LoRA (lora.hip) on the Llama-3-8B projections at M = 4096 / 2048 rows and adapter ranks 16 / 64
    (the fused q|k|v call runs 3 rank slots, gate|up 2): shrink and expand-add on a 4-adapter batch in
    request-sized runs of 64 rows, and on a batch with no adapter at all (every id -1: what a configured but
    unused adapter set costs per launch), next to the base projection from the same run, both as the model runs
    it (the planner's backend, ops/gemm_plan.py, tuned here: qkv and the gate|up pre-activation plain, o and
    down with the residual add in the GEMM) and through hipBLASLt alone (``F.linear``).  Bytes
    each kernel must move: shrink reads X [M, K]; expand-add reads and writes Y [M, N].  Inputs rotate over
    enough copies to exceed the 256 MB last-level cache; medians of 5 interleaved rounds."""
    import torch.nn.functional as F

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.ops import gemm_plan

    ws = ops.new_gemm8p_workspace(dev)
    projs = [("qkv", 6144, 4096, 3), ("o", 4096, 4096, 1), ("gate_up", 28672, 4096, 2), ("down", 4096, 14336, 1)]
    n_ad = 4
    print("| proj | M | rank (R) | planner GEMM us | hipBLASLt us | shrink us | X MB | TB/s | expand us | Y r+w MB | TB/s | "
          "shrink -1 us | expand -1 us |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for M in [int(m) for m in os.environ.get("LORA_M", "4096,2048").split(",")]:
        ids = ((torch.arange(M, device=dev) // 64) % n_ad).to(torch.int32)
        none = torch.full((M,), -1, dtype=torch.int32, device=dev)
        for name, N, K, slots in projs:
            w = ((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
            nx = max(2, min(8, -(-(512 << 20) // (M * K * 2))))
            ny = max(2, min(8, -(-(512 << 20) // (M * N * 2))))
            xs = [(torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16) for _ in range(nx)]
            ys = [(torch.rand(M, N, device=dev) * 2 - 1).to(torch.bfloat16) for _ in range(ny)]
            it = [0]

            def nxt(pool):
                it[0] += 1
                return pool[it[0] % len(pool)]

            res = name in ("o", "down")
            choice = gemm_plan.tune(xs[0], w, "residual" if res else "plain", ws=ws)
            if res:
                def planner():
                    return gemm_plan.linear_add_(nxt(xs), w, nxt(ys), ws=ws)
            else:
                def planner():
                    return gemm_plan.linear(nxt(xs), w, ws=ws)

            for rank in (16, 64):
                R = rank * slots
                A = ((torch.rand(n_ad, R, K, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
                B = ((torch.rand(n_ad, N, R, device=dev) * 2 - 1) / R ** 0.5).to(torch.bfloat16)
                T = torch.zeros(M, R, device=dev, dtype=torch.bfloat16)
                runs = {"plan": planner, "base": lambda: F.linear(nxt(xs), w),
                        "shrink": lambda: ops.lora_shrink(nxt(xs), A, ids, out=T),
                        "expand": lambda: ops.lora_expand_add_(nxt(ys), T, B, ids),
                        "shrink0": lambda: ops.lora_shrink(nxt(xs), A, none, out=T),
                        "expand0": lambda: ops.lora_expand_add_(nxt(ys), T, B, none)}
                t = {k: [] for k in runs}
                for _ in range(5):
                    for k, fn in runs.items():
                        t[k].append(timeit(fn, iters=10, warm=2))
                m = {k: sorted(v)[2] for k, v in t.items()}
                xb, yb = M * K * 2, 2 * M * N * 2
                print(f"| {name} | {M} | {rank} ({R}) | {m['plan']:.1f} ({choice}) | {m['base']:.1f} | {m['shrink']:.1f} | {xb / 1e6:.1f} | "
                      f"{xb / m['shrink'] / 1e6:.2f} | {m['expand']:.1f} | {yb / 1e6:.1f} | {yb / m['expand'] / 1e6:.2f} | "
                      f"{m['shrink0']:.1f} | {m['expand0']:.1f} |", flush=True)
                del A, B, T
            del w, xs, ys


def lora_step(dev):
    """One llama-3-8b decode step at B = 4096 (every sequence at position 32, captured in a graph, median of 20
    replays) on three models built one after the other in this process: the plain model (norms folded, the
    planner's chain), the plain model with unfolded norms, and a model with 4 rank-16 adapters on all seven
    targets whose rows all carry id -1 — the price of having adapters configured but unused."""
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache, LlamaModel
    from llm_weighted_consensus_amd.models.lora import random_adapter

    cfg = decoder_config("llama-3-8b")
    B, pos = int(os.environ.get("LORA_STEP_B", "4096")), 32
    i32 = dict(dtype=torch.int32, device=dev)
    cache = KVCache(cfg, 3 * B, 16, dev)
    bt = torch.arange(3 * B, **i32).view(B, 3)
    tokens = torch.randint(0, cfg.vocab_size, (B,), device=dev).int()
    positions = torch.full((B,), pos, **i32)
    slots = (bt[:, 2] * 16).contiguous()
    ctx = torch.full((B,), pos + 1, **i32)
    none = torch.full((B,), -1, **i32)
    res = {}
    for label in ("plain", "plain unfolded norms", "adapters configured, all rows -1"):
        kw = {}
        if label.startswith("adapters"):
            kw["lora"] = [random_adapter(f"a{i}", cfg, i, rank=16) for i in range(4)]
        elif "unfolded" in label:
            kw["fold_norms"] = False
        model = LlamaModel(cfg, device=dev, seed=0, max_position=256, **kw)
        model.tune_gemms(B)
        dk = {"lora_ids": none} if model.lora is not None else {}

        def fwd():
            return model.decode(tokens, positions, slots, bt, ctx, cache, num_splits=1, **dk)

        for _ in range(2):
            fwd()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fwd()
        ts = []
        for _ in range(23):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
        ts = sorted(ts[3:])
        res[label] = ts[len(ts) // 2]
        print(f"decode step B={B} [{label}]: median {res[label]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}) "
              f"chain={model.chain_ok(B)} plan={model.plan_summary(B)}", flush=True)
        del g, model
        torch.cuda.empty_cache()
    base = res["plain"]
    for k, v in res.items():
        print(f"  {k}: {v:.3f} ms  ({(v / base - 1) * 100:+.2f} % vs plain)")


def qknorm(dev):
    """qknorm_rope_kv_write (q|k|v bias, per-head q / k RMSNorm, RoPE, KV write) beside rope_kv_write at Llama-3-8B
    head counts (32 / 8 / 128), T = 4096 and 64, both rope_q modes: interleaved rounds, median, and the bytes each
    call has to move (from the shapes) over that time.  Then one decode layer at B = 4096 — (3-layer step - 1-layer
    step) / 2 of graph replays, norms unfolded — for llama-3-8b, qwen3-8b and qwen3-8b's shapes without the q / k
    norm (the same GEMMs on rope_kv_write)."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import KVCache, LlamaModel, rope_tables

    cfg = decoder_config("llama-3-8b")
    Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
    cos, sin = rope_tables(cfg, dev, 4096)
    bf = torch.bfloat16
    bias = (0.05 * torch.randn(cfg.qkv_dim, device=dev)).to(bf)
    qw, kw = [(1 + 0.3 * torch.randn(D, device=dev)).to(bf) for _ in range(2)]
    feats = {"norms": dict(q_weight=qw, k_weight=kw), "bias": dict(bias=bias),
             "both": dict(bias=bias, q_weight=qw, k_weight=kw)}

    def nbytes(T, rope_q, q_work, v_back):
        q, kv = T * Hq * D * 2, T * Hkv * D * 2
        rd = kv + kv + (q if q_work else 0) + T * D * 4  # k, v, q; one cos + sin row per token
        wr = kv + kv + (q if q_work else 0) + ((kv + (kv if v_back else 0)) if rope_q else 0)  # caches, q, k / v back
        return rd + wr

    for T in (4096, 64):
        cache = KVCache(decoder_config("llama-3-8b", layers=1), T + 64, 16, dev)
        qkv0 = torch.randn(T, cfg.qkv_dim, device=dev).to(bf)
        qkv = qkv0.clone()
        pos = torch.randint(0, 4000, (T,), device=dev, dtype=torch.int32)
        slots = (torch.randperm(T, device=dev).to(torch.int32) * 16 + 5)
        args = (qkv, pos, cos, sin, cache.k[0], cache.v[0], Hq, Hkv, D)
        runs = {}
        for rope_q in (True, False):
            m = "q+k" if rope_q else "k only"
            runs[f"rope_kv_write [{m}]"] = (lambda r=rope_q: ops.rope_kv_write(*args, slots=slots, rope_q=r),
                                            nbytes(T, rope_q, rope_q, False))
            for name, kwargs in feats.items():
                runs[f"qknorm {name} [{m}]"] = (
                    lambda r=rope_q, k=kwargs: ops.qknorm_rope_kv_write(*args, slots=slots, rope_q=r, eps=1e-6, **k),
                    nbytes(T, rope_q, True, "bias" in kwargs))
        ts = {k: [] for k in runs}
        for _ in range(7):  # (in place on qkv: refreshed each round so the norms never see a drifted row)
            for k, (fn, _) in runs.items():
                qkv.copy_(qkv0)
                ts[k].append(timeit(fn, iters=20, warm=3))
        for k, (_, nb) in runs.items():
            v = sorted(ts[k])
            us = v[len(v) // 2]
            print(f"T={T:5d} {k:32s}: {us:7.1f} us (min {v[0]:.1f}, max {v[-1]:.1f})  {nb / 1e6:7.1f} MB  "
                  f"{nb / (us * 1e-6) / 1e12:5.2f} TB/s", flush=True)
        del cache

    B, pos = int(os.environ.get("QKNORM_STEP_B", "4096")), 32
    i32 = dict(dtype=torch.int32, device=dev)
    bt = torch.arange(3 * B, **i32).view(B, 3)
    positions, ctx = torch.full((B,), pos, **i32), torch.full((B,), pos + 1, **i32)
    slots = (bt[:, 2] * 16).contiguous()
    res = {}
    for label, arch, over in (("llama-3-8b", "llama-3-8b", {}), ("qwen3-8b", "qwen3-8b", {}),
                              ("qwen3-8b shapes, no q/k norm", "qwen3-8b", {"qk_norm": False})):
        step = {}
        for nl in (1, 3):
            c = decoder_config(arch, layers=nl, **over)
            cache = KVCache(c, 3 * B, 16, dev)
            model = LlamaModel(c, device=dev, seed=0, max_position=256, fold_norms=False)
            model.tune_gemms(B)
            tokens = torch.randint(0, c.vocab_size, (B,), device=dev).int()

            def fwd():
                return model.decode(tokens, positions, slots, bt, ctx, cache, num_splits=1)

            for _ in range(2):
                fwd()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fwd()
            ts = []
            for _ in range(23):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                g.replay()
                e.record()
                e.synchronize()
                ts.append(s.elapsed_time(e))
            ts = sorted(ts[3:])
            step[nl] = ts[len(ts) // 2]
            print(f"decode step B={B} [{label}, {nl} layer(s)]: median {step[nl]:.3f} ms (min {ts[0]:.3f}, "
                  f"max {ts[-1]:.3f}) plan={model.plan_summary(B)}", flush=True)
            del g, model, cache
            torch.cuda.empty_cache()
        res[label] = (step[3] - step[1]) / 2
    for k, v in res.items():
        print(f"  one decode layer B={B} [{k}]: {v * 1e3:.1f} us")


def qwen_moe(dev):
    """Qwen3-MoE (profiles/qwen_moe.md): the wide router against a torch composition, one decode step of the
    qwen3-30b-a3b shapes at 4 layers with its parts, and the whole-model cosines of qwen3-moe-tiny against the fp32
    oracle of tests/qwen_moe_ref.py.  Arms interleaved in one process, medians of 7 rounds of captured graphs."""
    import sys
    from pathlib import Path

    import torch.nn.functional as F

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    out = Path(os.environ.get("QWENMOE_OUT", Path(__file__).resolve().parent.parent / "profiles" / "qwen_moe.md"))
    d, E, k = 2048, 128, 8
    lines = ["# Qwen3-MoE: the wide router and one decode step (`python scripts/microbench.py qwenmoe`)", "",
             f"MI355X, torch {torch.__version__}.  Arms interleaved in one process, median of 7 rounds; every arm is a "
             "captured graph of 20 calls (a decode step is a captured graph: eager launches this short time the host).",
             "", "## Router: `moe_router_wide` vs a torch composition (d = 2048, E = 128, k = 8)", "",
             "torch: `F.linear` -> `topk` -> `softmax` -> stable `argsort` of the flat ids (the dispatch permutation).",
             "unfused: `F.linear` -> `moe_route_wide` (the library GEMM, then the same top-k and permutation).",
             "", "| T | moe_router_wide us | unfused us | torch us | wide / torch | wide / unfused |", "|---|---|---|---|---|---|"]
    router = (torch.randn(E, d, device=dev) * 0.1).to(torch.bfloat16)
    for T in (1, 64, 512, 4096):
        h = torch.randn(T, d, device=dev).to(torch.bfloat16)

        def torch_route():
            top, ids = F.linear(h, router).float().topk(k, dim=-1)
            return ids, top.softmax(-1), torch.argsort(ids.flatten(), stable=True)

        t = _graph_medians({"wide": lambda: ops.moe_router_wide(h, router, k), "torch": torch_route,
                            "unfused": lambda: ops.moe_route_wide(F.linear(h, router), k)}, 20)
        cells = [f"**{r:.2f} (slower)**" if r > 1 else f"{r:.2f}" for r in (t["wide"] / t["torch"], t["wide"] / t["unfused"])]
        lines.append(f"| {T} | {t['wide']:.1f} | {t['unfused']:.1f} | {t['torch']:.1f} | {cells[0]} | {cells[1]} |")
        print(lines[-1], flush=True)

    lines += ["", "## One decode step, qwen3-30b-a3b shapes at 4 layers (context 32, captured graph)", "",
              "route: `ops.route`; expert FFN: row quantisation (fp8), the two grouped GEMMs with the SwiGLU between "
              "them, `moe_combine`; lm_head: the 151936 x 2048 projection timed alone; the rest (norms, qkv / o "
              "projections, QK-norm + RoPE + KV write, decode attention, embedding) is the remainder.", "",
              "| weights | B | step ms | route | expert FFN | lm_head | attention block + rest | expert FFN us / layer "
              "| expert weight GB/s |", "|---|---|---|---|---|---|---|---|---|"]
    cfg = decoder_config("qwen3-30b-a3b", layers=4)
    for fp8 in (False, True):
        model = Qwen3MoeModel(cfg, device=dev, seed=0, max_position=128, fp8=fp8)
        L = model.layers[0]
        wbytes = 3 * cfg.hidden * cfg.ffn * E * (1 if fp8 else 2)
        for B in (64, 512, 4096):
            step = _decode_step_ms(model, cfg, dev, B)[0]
            x = torch.randn(B, cfg.hidden, device=dev).to(torch.bfloat16)
            t = _graph_medians({"route": lambda: ops.route(x, L.router, k), "mlp": lambda: model._mlp(x, L),
                                "head": lambda: model._proj(x, model.lm_head)}, 10)
            ffn = t["mlp"] - t["route"]
            route_s, ffn_s, head_s = (cfg.layers * t["route"] / 1e3 / step, cfg.layers * ffn / 1e3 / step,
                                      t["head"] / 1e3 / step)
            lines.append(f"| {'fp8' if fp8 else 'bf16'} | {B} | {step:.3f} | {route_s:.1%} | {ffn_s:.1%} | {head_s:.1%} | "
                         f"{1 - route_s - ffn_s - head_s:.1%} | {ffn:.0f} | {wbytes / ffn / 1e3:.0f} |")
            print(lines[-1], flush=True)
        del model, L
        torch.cuda.empty_cache()
    lines += ["", "At B = 64 a step routes 512 rows to 128 experts: about 4 rows per expert, each in a 128-row tile of "
              "the grouped GEMM (256 in gemm8g), so 97 % of the MFMA rows are padding while every expert's weights are "
              "streamed once.  The last column is what that costs: the expert weights of a layer divided by the expert "
              "FFN time, to hold against the ~5 TB/s a weight-streaming kernel reaches.  The lead, not built here: a "
              "16- or 32-row tail tile in the grouped GEMM, or a weight-stream (skinny) kernel per expert for "
              "segments of a few rows."]

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from tests.test_qwen_moe_gpu import _model, _model_cosines

    lines += ["", "## Whole model against the fp32 oracle (qwen3-moe-tiny)", "",
              "Largest 1 - cos over the prefill's last-token logits (37 tokens) and 7 decode steps; the bounds of "
              "tests/test_qwen_moe_gpu.py are 1 - 4 x the largest value of a row, within [0.99, Mixtral's bound].", "",
              "| weights | seed 2 | seed 3 | seed 4 |", "|---|---|---|---|"]
    for fp8 in (False, True):
        worst = []
        for seed in (2, 3, 4):
            m = _model(dev, fp8, seed)
            worst.append(1 - min(_model_cosines(m, dev)))
            del m
        lines.append(f"| {'fp8' if fp8 else 'bf16'} | " + " | ".join(f"{v:.3g}" for v in worst) + " |")
        print(lines[-1], flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("wrote", out)


def moe_mxfp4_ab(dev):
    """MoE experts in MXFP4 (profiles/moe_mxfp4.md).  (a) the expert FFN of one layer (gate|up + SwiGLU + down, rows
    routed by ``ops.route`` on N(0, 1) tokens) at the qwen3-30b-a3b and mixtral-8x7b expert shapes: bf16 experts,
    fp8 experts, the MXFP4 grouped weight stream and the MXFP4 dequantise path; (b) one qwen3-30b-a3b decode step at
    4 layers, bf16 vs ``expert_weights="mxfp4"``; (c) GiB allocated after the load.  Arms interleaved in one
    process, medians of 7 rounds of captured graphs; the MXFP4 stacks rotate over 3 copies where one would fit the
    last-level cache."""
    from pathlib import Path
    from types import SimpleNamespace

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel, MoELayerWeights
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    out = Path(os.environ.get("MOEMXFP4_OUT", Path(__file__).resolve().parent.parent / "profiles" / "moe_mxfp4.md"))
    Ts = [int(t) for t in os.environ.get("MOEMXFP4_T", "1,16,64,128,256,512,4096").split(",")]
    lines = ["# MoE experts in MXFP4: the grouped weight stream (`python scripts/microbench.py moemxfp4`)", "",
             f"MI355X, torch {torch.__version__}.  Arms interleaved in one process, median of 7 rounds; every arm is a "
             "captured graph of several calls.", "",
             "## (a) Expert FFN of one layer: gate|up + SwiGLU + down", "",
             "Rows are the (token, slot) pairs `ops.route` makes of T N(0, 1) tokens and a random router.  bf16: "
             "`grouped_gemm`, `silu_mul`, `grouped_gemm`; fp8: the model's fp8 branch on rows quantised outside the "
             "timing; stream: `moe_skinny_mxfp4` twice; dequant: `mxfp4_dequant` of each stack into the scratch, then "
             "the bf16 arm.  GB/s: the bytes of the active experts' weights in the arm's format over the time.", "",
             "| shapes | T | rows / expert | active | bf16 us (GB/s) | fp8 us (GB/s) | stream us (GB/s) | dequant us (GB/s) "
             "| stream / dequant | stream / bf16 |", "|---|---|---|---|---|---|---|---|---|---|"]
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, std=0.02):
        return (torch.randn(*shape, device=dev, generator=g) * std).to(torch.bfloat16)

    def rand_stack(E, N, K):  # timing only: any codes, scales near 2^-6
        st = ops.Mxfp4Experts.__new__(ops.Mxfp4Experts)
        st.q = torch.randint(0, 256, (E, N, K // 2), device=dev, dtype=torch.uint8)
        st.s = torch.randint(117, 125, (E, N, K // 32), device=dev, dtype=torch.uint8)
        st.shape = (E, N, K)
        return st

    crossover = {}
    for arch in ("qwen3-30b-a3b", "mixtral-8x7b"):
        cfg = decoder_config(arch)
        d, F_, E, k = cfg.hidden, cfg.ffn, cfg.num_experts, cfg.experts_per_token
        w13 = torch.stack([ops.swiglu_interleave(rnd(2 * F_, d)) for _ in range(E)])
        w2 = rnd(E, d, F_)
        q13, s13 = ops.quant_fp8_weight(w13)
        q2, s2 = ops.quant_fp8_weight(w2)
        copies = 3 if E * 3 * F_ * d * 17 // 32 < (512 << 20) else 1
        mx = _rotating([(rand_stack(E, 2 * F_, d), rand_stack(E, d, F_)) for _ in range(copies)])
        scratch = torch.empty(E * 2 * F_ * d, dtype=torch.bfloat16, device=dev)
        router = rnd(E, d, std=0.1)
        me = SimpleNamespace(fp8=True, moe_scratch=scratch)
        L8 = MoELayerWeights(None, None, None, None, router, q13, q2, s13, s2, 32)
        per_expert = 3 * F_ * d
        for T in Ts:
            h = torch.randn(T, d, device=dev, generator=g).to(torch.bfloat16)
            _, _, row_off, src, _ = ops.route(h, router, k)
            rows = T * k
            active = int((row_off.diff() > 0).sum())
            hq, hs = ops.quant_fp8_rows(h)

            def bf16():
                gu = ops.grouped_gemm(h, w13, row_off, a_rows=src, rows=rows)
                return ops.grouped_gemm(ops.silu_mul(gu, block=32), w2, row_off)

            def mxfp4(path):
                a, b = mx()
                act = ops.moe_swiglu_mxfp4(h, a, row_off, src, rows, scratch, path=path)
                return ops.moe_linear_mxfp4(act, b, row_off, scratch, path=path)

            t = _graph_medians({"bf16": bf16,
                                "fp8": lambda: MixtralModel._experts(me, hq, row_off, L8, hs, a_rows=src, rows=rows),
                                "stream": lambda: mxfp4("stream"), "dequant": lambda: mxfp4("dequant")},
                               10 if rows <= 1024 else 3)
            gbs = {a: active * per_expert * b / t[a] / 1e3 for a, b in
                   (("bf16", 2), ("fp8", 1), ("stream", 17 / 32), ("dequant", 17 / 32))}
            r1, r2 = t["stream"] / t["dequant"], t["stream"] / t["bf16"]
            cells = [f"**{r:.2f} (slower)**" if r > 1 else f"{r:.2f}" for r in (r1, r2)]
            lines.append(f"| {arch} | {T} | {rows / E:.2f} | {active} / {E} | "
                         + " | ".join(f"{t[a]:.1f} ({gbs[a]:.0f})" for a in ("bf16", "fp8", "stream", "dequant"))
                         + f" | {cells[0]} | {cells[1]} |")
            print(lines[-1], flush=True)
            crossover.setdefault(arch, []).append((rows / E, r1))
        del w13, w2, q13, q2, s13, s2, mx, scratch, L8, me
        torch.cuda.empty_cache()
    lines += ["", "Crossover (largest measured rows / expert at which the stream path is still no slower than the "
              "dequantise path): " + "; ".join(
                  f"{a}: {max([r for r, x in v if x <= 1] or [0]):.2f}" for a, v in crossover.items()) + "."]

    lines += ["", "## (b) One decode step, qwen3-30b-a3b shapes at 4 layers (context 32, captured graph)", "",
              "| experts | B | step ms | vs bf16 |", "|---|---|---|---|"]
    cfg = decoder_config("qwen3-30b-a3b", layers=4)
    gib, base = {}, {}
    for fmt in ("bf16", "mxfp4"):
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated(dev)
        model = Qwen3MoeModel(cfg, device=dev, seed=0, max_position=128, expert_weights=fmt)
        torch.cuda.synchronize()
        gib[fmt] = (torch.cuda.memory_allocated(dev) - before) / 2 ** 30
        for B in (64, 512, 4096):
            step = _decode_step_ms(model, cfg, dev, B)[0]
            base.setdefault(B, step)
            r = step / base[B]
            lines.append(f"| {fmt} | {B} | {step:.3f} | " + (f"**{r:.2f} (slower)**" if r > 1 else f"{r:.2f}") + " |")
            print(lines[-1], flush=True)
        del model
    lines += ["", "## (c) GiB allocated after the load (qwen3-30b-a3b shapes at 4 layers, scratch included)", "",
              "| experts | GiB |", "|---|---|"] + [f"| {f} | {v:.2f} |" for f, v in gib.items()]
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("wrote", out)


def moe_mxfp4_a8_ab(dev):
    """MoE experts in MXFP4 with e4m3 activations (profiles/moe_mxfp4_a8.md).  (a) the expert FFN of one layer at the
    eight shapes of the README's MXFP4-experts table: W4A8 (``quant_fp8_rows`` of the T token rows, the gathered
    gate|up + SwiGLU, ``quant_fp8_rows`` of its output, down: both quantisation passes inside the timing), the parent's
    path at that row count (the weight stream up to ``MOE_MXFP4_STREAM_AVG_ROWS`` rows per expert, the dequantise
    path above), bf16 experts and fp8 experts; (b) one qwen3-30b-a3b decode step at 4 layers with bf16 experts, with
    MXFP4 experts and with ``expert_act="e4m3"`` on top; (c) GiB allocated after the load.  Arms interleaved in one
    process, medians of 7 rounds of captured graphs; the MXFP4 stacks rotate over 3 copies where one would fit the
    last-level cache."""
    from pathlib import Path
    from types import SimpleNamespace

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel, MoELayerWeights
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    out = Path(os.environ.get("MOEMXFP4A8_OUT",
                              Path(__file__).resolve().parent.parent / "profiles" / "moe_mxfp4_a8.md"))
    shapes = {"qwen3-30b-a3b": (1, 64, 512, 4096), "mixtral-8x7b": (16, 128, 256, 512)}
    lines = ["# MoE experts in MXFP4 with e4m3 activations: the grouped W4A8 kernel "
             "(`python scripts/microbench.py moemxfp4a8`)", "",
             f"MI355X, torch {torch.__version__}.  Arms interleaved in one process, median of 7 rounds; every arm is a "
             "captured graph of several calls.", "",
             "## (a) Expert FFN of one layer: gate|up + SwiGLU + down", "",
             "Rows are the (token, slot) pairs `ops.route` makes of T N(0, 1) tokens and a random router.  W4A8: "
             "`quant_fp8_rows` of the T token rows, `moe_gemm_mxfp4_a8` with the gather and the SwiGLU epilogue, "
             "`quant_fp8_rows` of its output, `moe_gemm_mxfp4_a8` (both quantisation passes are timed).  parent: what "
             "a model without `expert_act` runs at that row count, the weight stream (`moe_skinny_mxfp4` twice) up to "
             f"{ops.MOE_MXFP4_STREAM_AVG_ROWS} rows per expert on average, above it the dequantise path "
             "(`mxfp4_dequant` of each stack, then the bf16 arm).  bf16: `grouped_gemm`, `silu_mul`, `grouped_gemm`; "
             "fp8: the model's fp8 branch on rows quantised outside the timing.  routed: whether a model with "
             "`\"expert_act\": \"e4m3\"` takes the W4A8 kernel at that row count.", "",
             "| shapes | T | rows / expert | active | routed | W4A8 us | parent us (path) | bf16 us | fp8 us | "
             "W4A8 / parent | W4A8 / bf16 | W4A8 / fp8 |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, std=0.02):
        return (torch.randn(*shape, device=dev, generator=g) * std).to(torch.bfloat16)

    def rand_stack(E, N, K):  # timing only: any codes, scales near 2^-6
        st = ops.Mxfp4Experts.__new__(ops.Mxfp4Experts)
        st.q = torch.randint(0, 256, (E, N, K // 2), device=dev, dtype=torch.uint8)
        st.s = torch.randint(117, 125, (E, N, K // 32), device=dev, dtype=torch.uint8)
        st.shape = (E, N, K)
        return st

    def mark(r):
        return f"**{r:.2f} (slower)**" if r > 1 else f"{r:.2f}"

    for arch, Ts in shapes.items():
        cfg = decoder_config(arch)
        d, F_, E, k = cfg.hidden, cfg.ffn, cfg.num_experts, cfg.experts_per_token
        w13 = torch.stack([ops.swiglu_interleave(rnd(2 * F_, d)) for _ in range(E)])
        w2 = rnd(E, d, F_)
        q13, s13 = ops.quant_fp8_weight(w13)
        q2, s2 = ops.quant_fp8_weight(w2)
        copies = 3 if E * 3 * F_ * d * 17 // 32 < (512 << 20) else 1
        mx = _rotating([(rand_stack(E, 2 * F_, d), rand_stack(E, d, F_)) for _ in range(copies)])
        scratch = torch.empty(E * 2 * F_ * d, dtype=torch.bfloat16, device=dev)
        router = rnd(E, d, std=0.1)
        me = SimpleNamespace(fp8=True, moe_scratch=scratch)
        L8 = MoELayerWeights(None, None, None, None, router, q13, q2, s13, s2, 32)
        for T in Ts:
            h = torch.randn(T, d, device=dev, generator=g).to(torch.bfloat16)
            _, _, row_off, src, _ = ops.route(h, router, k)
            rows = T * k
            active = int((row_off.diff() > 0).sum())
            hq, hs = ops.quant_fp8_rows(h)
            path = "stream" if rows <= ops.MOE_MXFP4_STREAM_AVG_ROWS * E else "dequant"

            def bf16():
                gu = ops.grouped_gemm(h, w13, row_off, a_rows=src, rows=rows)
                return ops.grouped_gemm(ops.silu_mul(gu, block=32), w2, row_off)

            def parent():
                a, b = mx()
                act = ops.moe_swiglu_mxfp4(h, a, row_off, src, rows, scratch, path=path)
                return ops.moe_linear_mxfp4(act, b, row_off, scratch, path=path)

            def a8():
                a, b = mx()
                act = ops.moe_swiglu_mxfp4_a8(h, a, row_off, src, rows)
                return ops.moe_linear_mxfp4_a8(act, b, row_off)

            t = _graph_medians({"a8": a8, "parent": parent, "bf16": bf16,
                                "fp8": lambda: MixtralModel._experts(me, hq, row_off, L8, hs, a_rows=src, rows=rows)},
                               10 if rows <= 1024 else 3)
            routed = "yes" if ops.moe_mxfp4_a8_route(rows, E, True) == "a8" else "no"
            lines.append(f"| {arch} | {T} | {rows / E:.2f} | {active} / {E} | {routed} | {t['a8']:.1f} | "
                         f"{t['parent']:.1f} ({path}) | {t['bf16']:.1f} | {t['fp8']:.1f} | "
                         + " | ".join(mark(t["a8"] / t[a]) for a in ("parent", "bf16", "fp8")) + " |")
            print(lines[-1], flush=True)
        del w13, w2, q13, q2, s13, s2, mx, scratch, L8, me
        torch.cuda.empty_cache()

    lines += ["", "## (b) One decode step, qwen3-30b-a3b shapes at 4 layers (context 32, captured graph)", "",
              "| experts | B | step ms | vs bf16 | vs mxfp4 |", "|---|---|---|---|---|"]
    cfg = decoder_config("qwen3-30b-a3b", layers=4)
    gib, steps = {}, {}
    for name, kw in (("bf16", {}), ("mxfp4", {"expert_weights": "mxfp4"}),
                     ("mxfp4 + e4m3", {"expert_weights": "mxfp4", "expert_act": "e4m3"})):
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated(dev)
        model = Qwen3MoeModel(cfg, device=dev, seed=0, max_position=128, **kw)
        torch.cuda.synchronize()
        gib[name] = (torch.cuda.memory_allocated(dev) - before) / 2 ** 30
        for B in (64, 512, 4096):
            steps[name, B] = step = _decode_step_ms(model, cfg, dev, B)[0]
            lines.append(f"| {name} | {B} | {step:.3f} | {mark(step / steps['bf16', B])} | "
                         + (mark(step / steps["mxfp4", B]) if ("mxfp4", B) in steps else "") + " |")
            print(lines[-1], flush=True)
        del model
    lines += ["", "## (c) GiB allocated after the load (qwen3-30b-a3b shapes at 4 layers; the dequantisation scratch, "
              "0.75 GiB, is what `expert_act` drops)", "",
              "| experts | GiB |", "|---|---|"] + [f"| {f} | {v:.2f} |" for f, v in gib.items()]
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["gemm", "attn", "sample", "small"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if "gemm" in a.what:
        gemms(dev, [int(m) for m in os.environ.get("MICRO_M", "256,512").split(",")], tuned=os.environ.get("PYTORCH_TUNABLEOP_ENABLED") == "1")
    if "backends" in a.what:
        gemm_backends(dev, [1024, 1536])
    if "grouped" in a.what:
        grouped(dev)
    if "g4ab" in a.what:
        gemm4w_ab(dev)
    if "chain" in a.what:
        chain_ab(dev)
    if "route" in a.what:
        route_ab(dev)
    if "enc" in a.what:
        encoder_gemms(dev)
    if "serve" in a.what:
        serve_shapes(dev)
    if "skinny" in a.what:
        skinny_ab(dev)
    if "mxfp4" in a.what:
        mxfp4_ab(dev)
    if "mxfp4a8" in a.what:
        mxfp4a8_ab(dev)
    if "lora" in a.what:
        lora_kernels(dev)
    if "lorastep" in a.what:
        lora_step(dev)
    if "qknorm" in a.what:
        qknorm(dev)
    if "qwenmoe" in a.what:
        qwen_moe(dev)
    if "moemxfp4" in a.what:
        moe_mxfp4_ab(dev)
    if "moemxfp4a8" in a.what:
        moe_mxfp4_a8_ab(dev)
    if "g48" in a.what:
        g48_ab(dev)
    if "g8ab" in a.what:
        gemm8p_ab(dev)
    if "g8" in a.what:
        gemm8p_study(dev, [int(m) for m in os.environ.get("MICRO_M", "3072,1024").split(",")])
    if "layout" in a.what:
        gemm_layouts(dev, [int(m) for m in os.environ.get("MICRO_M", "512,1024").split(",")])
    if "attn" in a.what:
        attention(dev)
    if "bw" in a.what:
        bandwidth(dev)
    if "pfattn" in a.what:
        prefill_attn(dev)
    if "prefix" in a.what:
        attention_prefix(dev)
    if "decode_shapes" in a.what:
        decode_shapes(dev)
    if "sample" in a.what:
        sampler(dev)
    if "moe" in a.what:
        moe_decode(dev)
    if "small" in a.what:
        small(dev)


if __name__ == "__main__":
    main()
