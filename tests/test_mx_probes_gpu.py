"""The kernels that exchange activations in MX form (e4m3 rows + one e8m0 scale byte per 32 values) under exact
probes (tests/mx_probes.py): three writers, the planes between them, and the reader.

The relative Frobenius bounds of tests/test_kernels_gpu.py (4e-2 / 5e-2 over a whole tensor) accept a scale byte
stored for the wrong row or block, a wrong rounding mode of the e4m3 conversion, a scale one binade off at the 0.875
threshold, and cannot see a store past the rows of a plane.  Here:

  bitwise   prefill twin law    prefill_attention_mx quantises the bf16 tile prefill_attention stores: its bytes
                                are mx_quant_ref of that kernel's output on the same operands.
            SwiGLU twin law     gemm8g mode 2 quantises the bf16 tile mode 1 stores, dense and grouped, with and
                                without the row gather, and through ops.linear_fp8_swiglu_mx in row blocks.
            cascade, exact rows one-hot rows whose softmax is a single key (a 271-nat spike: every other weight is
                                0 in fp32) over V made of the edge-block table, and flat rows over integer V
                                whose context is a power of two: the fp32 value the epilogue quantises is exact.
            reader              one live block per 128-slice under scale bytes that tell rows, slices and blocks
                                apart, and all blocks live under one byte per slice: every partial sum is exact
                                in fp32, so the bf16 output is the RNE code of the exact product.
            chain               attention writer -> MXAct.index_select -> ops.linear_fp8 on spike rows.
  bounded   cascade, other rows the epilogue quantises fp32 o / l, the bf16 twin rounds it: per element
                                |deq - out| <= max(|out| 2^-4, 2^(e - 10)) (1 + 2^-8) + 2^-8 |out|, and the byte
                                is that of mx_quant_ref(out) unless the block maximum sits within 2^-8 of the
                                0.875 threshold or of a power of two (at most 5 % of the blocks).

The edge-block table (maxima 0, 7, 7.5, 8, 448, 480, 2^-126, 2^-120, 2^100 in every quarter of the block, the other
lanes on e4m3 ties, in the subnormal range, of both signs) reaches the quantisers through V (attention) and through
a saturated gate (SwiGLU: gate = 64, silu(64) = 64 in fp32, act = 64 * up).  Every output sits in a cage of
sentinel bytes, row stride above the row, planes with more rows than the batch, and every case is launched twice.
tests/test_mx_probes.py shows on the CPU which family rejects which broken kernel.

What the probes found on an MI355X: both twin laws hold bit for bit as read from the kernel source, the exact
cascade rows, both reader families and the chain are bitwise, and no sentinel is touched; no kernel needed a fix.
Two claims are narrower than first planned.  The upper clamp of the scale exponent cannot be reached from fp32 (the
largest finite value gives byte 247), so the "large" class is a plain 2^100.  The saturated-gate SwiGLU family
cannot emit the 2^-126 class, nor elements below 2^-120: ``up`` = act / 64 would be a subnormal fp32 number; the
lower clamp is reached there by a block maximum of 2^-120, and the 2^-126 class by the attention writers.  Where a
test asks whether a table block "appears", -0 counts as 0: a zero lane of V[at] takes the sign of the e^-30 leak
of the other keys (the twin law itself stays bitwise, sign of zero included)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import attn_probes as ap
from tests import gemm_probes as gp
from tests import mx_probes as mp

pytestmark = pytest.mark.gpu

BS, D = 16, 128
SCALE = 1 / math.sqrt(D)
_cases = {}


def _case(key, build):
    if key not in _cases:
        _cases[key] = build()
    return _cases[key]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


# ---------------------------------------------------------------------------------------------------------
# 1  prefill twin law

LENS = [1, 15, 16, 17, 63, 64, 65, 130]


def _prefill_edge_v(Hkv):
    """V [T, Hkv * 128] of table blocks: one class per (sequence, 32-column block), so that the e^-30 leak of a
    spike row comes from keys of its own magnitude; the position walks with the key."""
    grid = mp.edge_grid()
    ncls = grid.shape[0]
    rows = []
    for si, L in enumerate(LENS):
        t = torch.arange(L)[:, None]
        cb = torch.arange(4 * Hkv)[None, :]
        rows.append(grid[(cb + si) % ncls, (t + cb) % 6].reshape(L, Hkv * D))
    return torch.cat(rows).to(torch.bfloat16)


def _twin_prefill(gpu, q, k, v, cu, Hq, Hkv, causal, what):
    from llm_weighted_consensus_amd import ops

    T = q.shape[0]
    out = ops.prefill_attention(q, k, v, cu, max(LENS), Hq, Hkv, D, SCALE, causal)
    wq, ws = mp.mx_quant_ref(out.float().cpu())
    qc, pc = mp.ByteCage(T, Hq * D, gpu, pad=32), mp.PlaneCage(Hq, T, gpu, extra=5)
    for it in range(2):
        qc.poison(), pc.poison()
        ops.kernels().prefill_attention_mx(q, k, v, qc.view, pc.buf, cu, max(LENS), Hq, Hkv, SCALE, causal)
        torch.cuda.synchronize()
        mp.check(qc, pc, wq, ws, f"{what} launch {it}")
    return qc.view.cpu(), mp.from_plane(pc.buf, T).cpu()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (4, 4)])
def test_prefill_mx_is_the_quantised_bf16_twin(gpu, Hq, Hkv, causal):
    """prefill_attention_mx quantises the bf16-rounded output tile it stages in LDS, the tile prefill_attention
    stores: e4m3 bytes and scale bytes are bitwise mx_quant_ref(prefill_attention(...)) on the q / k / v slices of
    one qkv row, lengths across the 16-row wave and 64-query workgroup edges, out8 with a row stride of Hq * 128
    + 32 bytes and a plane of T + 5 rows in sentinels that must survive, two launches.  Once on random inputs;
    once with the score programmes of attn_probes.prefill_programmes over V made of the edge-block table, where
    every block of the table must appear among the emitted blocks (spike rows emit V[at])."""
    from tests.test_attention_probes_gpu import _build_prefill

    T = sum(LENS)
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32, device=gpu)
    torch.manual_seed(3)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=gpu).to(torch.bfloat16)
    q, k, v = qkv[:, : Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    _twin_prefill(gpu, q, k, v, cu, Hq, Hkv, causal, "prefill random")

    c = _case(("mx prefill", causal, Hq, Hkv), lambda: _build_prefill(LENS, LENS, Hq, Hkv, D, causal)(gpu))
    assert c.stats["spikes"] > 0
    qkv = torch.cat([c.q, c.k, _prefill_edge_v(Hkv).to(gpu)], 1)
    q, k, v = qkv[:, : Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    got_q, got_sc = _twin_prefill(gpu, q, k, v, cu, Hq, Hkv, causal, "prefill edge blocks")
    names, table = mp.edge_table()
    assert mp.missing_edge_blocks(got_q, got_sc, names, table) == []


# ---------------------------------------------------------------------------------------------------------
# 2  SwiGLU twin law

SIZES = [300, 0, 17, 129, 128]


def _interleave(W, w_s):
    from llm_weighted_consensus_amd import ops

    return ops.swiglu_interleave(W), ops.swiglu_interleave(w_s.view(-1, 1)).view(-1)


def _swiglu_dense_case(M, N, K, kind, gpu):
    """-> A (poisoned), a_s, W [1, N, K] (poisoned, interleaved), w_s [N], activations or None."""
    def build():
        if kind == "random":
            from tests.test_gemm_probes_gpu import _fp8_case

            A, a_s, w, _ = _fp8_case(M, N, K, gpu, swiglu=True)
            return A, a_s.float().contiguous(), w.q.view(1, N, K), w.s.reshape(-1).contiguous(), None
        A, W, w_s, x = mp.saturated_gate_operands(M, N // 2, K)
        Wi, wsi = _interleave(W, w_s)
        return (gp.poison_a(A, gpu), torch.ones(M, device=gpu), gp.poison_w(Wi.to(mp.E4M3).view(1, N, K), gpu),
                wsi.contiguous().to(gpu), x)
    return _case(("swiglu dense", M, N, K, kind), build)


def _twin_swiglu(gpu, launch, rows, F, N, what, act=None):
    """``launch(C, mode, mx_out)``: mode 1 into a bf16 cage, then mode 2 twice into byte cages; the bytes must be
    mx_quant_ref of the mode 1 output (``act``: which must be these activations exactly)."""
    cage = gp.Cage(rows, F, gpu)
    launch(cage.view, 1, None)
    torch.cuda.synchronize()
    assert cage.outside_touched() == 0
    out1 = cage.view.float().cpu()
    assert bool(torch.isfinite(out1).all()), what
    if act is not None:
        assert torch.equal(gp.bits(cage.view.cpu()), gp.bits(act.to(torch.bfloat16))), f"{what}: the gate is not saturated"
    wq, ws = mp.mx_quant_ref(out1)
    qc, pc = mp.ByteCage(rows, F, gpu), mp.PlaneCage(N // 256, rows, gpu)
    for it in range(2):
        qc.poison(), pc.poison()
        launch(qc.f8, 2, pc.buf)
        torch.cuda.synchronize()
        mp.check(qc, pc, wq, ws, f"{what} launch {it}")
    return wq, ws


@pytest.mark.parametrize("kind", ["random", "saturated"])
@pytest.mark.parametrize("M", [1, 255, 513])
def test_swiglu_mx_dense_is_the_quantised_bf16_twin(gpu, M, kind):
    """gemm8g mode 2 (SwiGLU epilogue, MX output) quantises the bf16 tile mode 1 stores: bitwise mx_quant_ref of
    the mode 1 output, C with ldc = F + 16 bytes and a plane of M + 7 rows in sentinels.  random: the exact
    operands of the one-step SwiGLU probe.  saturated: gate = 64 exactly and up set through power-of-two channel
    scales so that the activations ARE the edge-block table (mode 1 must store them exactly), one class per
    column block; from 6 rows on every block of the table is emitted."""
    from llm_weighted_consensus_amd import ops

    N, K = 512, 256
    A, a_s, W, w_s, act = _swiglu_dense_case(M, N, K, kind, gpu)
    wq, ws = _twin_swiglu(gpu, lambda C, mode, mx: ops.kernels().gemm8g_fp8(A, W, C, None, -(-M // 256), None, a_s, w_s,
                                                                            mode, None, mx),
                          M, N // 2, N, f"swiglu dense {kind} M={M}", act)
    if kind == "saturated" and M >= 6:
        names, table = mp.edge_table(mp.SATURATED_MIN)
        assert mp.missing_edge_blocks(wq, ws, names, table) == []


def _swiglu_grouped_case(kind, gather, gpu):
    def build():
        G, N, K = len(SIZES), 512, 256
        F, rows = N // 2, sum(SIZES)
        gen = torch.Generator().manual_seed(29 + gather)
        if kind == "random":
            A, _, a_s, _ = gp.fp8_operands(rows, 8, K, gen)
            W, _, w_s, _ = gp.fp8_operands(G * N, 8, K, gen)
            a_s = a_s.clamp(0.5, 1.0)
            W, w_s = W.float().view(G, N, K), w_s.view(G, N).clone()
            w_s[:, :F] = 2.0 ** -max(0, (K // 8 - 1).bit_length())     # |gate| <= 4 K / (K / 8) = 32
            act = None
        else:
            parts = [mp.saturated_gate_operands(n, F, K, shift=g) for g, n in enumerate(SIZES)]
            A = torch.cat([p[0].float() for p in parts]).to(mp.E4M3)
            W, w_s = torch.stack([p[1] for p in parts]), torch.stack([p[2] for p in parts])
            a_s, act = torch.ones(rows), torch.cat([p[3] for p in parts])
        pairs = [_interleave(W[g], w_s[g]) for g in range(G)]
        Wi = torch.stack([p[0] for p in pairs]).to(mp.E4M3)
        wsi = torch.stack([p[1] for p in pairs]).contiguous()
        a_rows = None
        if gather:                                   # A's rows scattered over rows + 37; the unused ones are NaN
            rows_a = rows + 37
            a_rows = torch.randperm(rows_a, generator=gen)[:rows]
            Af = torch.full((rows_a, K), mp.SENTINEL8, dtype=torch.uint8)
            Af[a_rows] = A.view(torch.uint8)
            sf = torch.full((rows_a,), float("nan"))
            sf[a_rows] = a_s
            A, a_s, a_rows = Af.view(mp.E4M3), sf, a_rows.to(torch.int32).to(gpu)
        off = torch.tensor([0] + list(np.cumsum(SIZES)), dtype=torch.int32, device=gpu)
        return gp.poison_a(A, gpu), a_s.float().to(gpu), gp.poison_w(Wi, gpu), wsi.float().to(gpu), off, a_rows, act
    return _case(("swiglu grouped", kind, gather), build)


@pytest.mark.parametrize("kind", ["random", "saturated"])
@pytest.mark.parametrize("gather", [False, True])
def test_swiglu_mx_grouped_is_the_quantised_bf16_twin(gpu, gather, kind):
    """The grouped call: groups of 300, 0, 17, 129 and 128 rows (a partial tile, an empty group, less than a wave
    row, one row past 128, exactly 128), with and without the A-row gather (unused A rows and scales NaN).  The
    saturated family turns the classes of the edge table by one column block per group."""
    from llm_weighted_consensus_amd import ops

    G, N, rows = len(SIZES), 512, sum(SIZES)
    A, a_s, W, w_s, off, a_rows, act = _swiglu_grouped_case(kind, gather, gpu)
    wq, ws = _twin_swiglu(gpu, lambda C, mode, mx: ops.kernels().gemm8g_fp8(A, W, C, off, -(-rows // 256) + G, a_rows,
                                                                            a_s, w_s, mode, None, mx),
                          rows, N // 2, N, f"swiglu grouped {kind} gather={gather}", act)
    if kind == "saturated":
        names, table = mp.edge_table(mp.SATURATED_MIN)
        assert mp.missing_edge_blocks(wq, ws, names, table) == []


def test_swiglu_mx_in_row_blocks(gpu, monkeypatch):
    """ops.linear_fp8_swiglu_mx with the span of one launch shrunk to 256 rows: three launches, each given the
    plane as a row-range view mx[:, r0:r1].  Bytes and planes stay bitwise the quantised mode 1 output."""
    from llm_weighted_consensus_amd import ops

    M, N, K = 513, 512, 256
    A, a_s, W, w_s, _ = _swiglu_dense_case(M, N, K, "random", gpu)
    w = ops.Fp8Weight.__new__(ops.Fp8Weight)
    w.q, w.s, w.shape = W.view(N, K), w_s.view(1, -1), (N, K)
    out1 = ops.gemm8g_dense(A, a_s, w, swiglu=True)
    wq, ws = mp.mx_quant_ref(out1.float().cpu())
    monkeypatch.setattr(ops, "G8G_SPAN", 256 * A.stride(0) + 1)
    assert len(ops._row_blocks(M, A.stride(0))) == 3
    q, mx = ops.linear_fp8_swiglu_mx(ops.QAct(None, A, a_s), w)
    assert torch.equal(_bytes(q).cpu(), wq) and torch.equal(mp.from_plane(mx).cpu(), ws)


# ---------------------------------------------------------------------------------------------------------
# 3  cascade decode

CASCADE_PROGS = ("first_own", "key0", "flat", "bg", "last_prefix", "last", "stair")
# suffix lengths per prefix length (keys): the first one makes the context a power of two
SUFFIXES = {0: [16, 1, 33], 32: [32, 1, 17, 15], 80: [48, 1, 16, 33], 304: [208, 17, 1]}


def _column(kind, pctx, L, t, gen):
    """fp32 K column values at key positions t for a one-hot row of programme ``kind`` (context L, prefix pctx)."""
    nat = 1.0 / (ap.AMP * SCALE)
    if kind == "flat":
        return torch.zeros(t.numel())
    if kind == "stair":
        return ap.k_column(ap.Prog("stair", anchor=pctx), t, SCALE, gen)
    vals = torch.randn(t.numel(), generator=gen) * nat
    at = _spike_at(kind, pctx, L)
    if at is not None:
        vals[t == at] = mp.TALL_K
    return vals


def _spike_at(kind, pctx, L):
    return {"first_own": pctx, "key0": 0, "last_prefix": max(pctx - 1, 0), "last": L - 1}.get(kind)


def _chain_v(shape_t, gen):
    """V [n, Hkv, 128] in {+-1, +-2} * 2^c with one c per (key, KV head): the four blocks of a head share their
    maximum 2^(c + 1), so their scale bytes are equal and q = +-128 / +-256 exactly."""
    n, Hkv = shape_t
    v = gp._signs((n, Hkv, D), gen) * torch.randint(1, 3, (n, Hkv, D), generator=gen).float()
    v[:, :, ::32] = 2.0 * gp._signs((n, Hkv, 4), gen)
    c = torch.randint(-3, 4, (n, Hkv, 1), generator=gen).float()
    return v * torch.exp2(c)


def _build_cascade(G, chain, gpu):
    def build():
        from llm_weighted_consensus_amd import ops
        from llm_weighted_consensus_amd.engine.engine import cascade_tiles
        from tests.test_attention_probes_gpu import _nan_cache, _store

        gen = torch.Generator().manual_seed(70 + G + 100 * chain)
        Hkv = 2
        Hq, dims = Hkv * G, ap.probe_dims(D)
        per = ops.cascade_rows_per_tile(G)
        assert per * G == D
        # (count, prefix blocks): a group over two super-tiles, an odd prefix, an empty prefix, a prefix of more
        # than one 16-block LDS chunk
        groups = [(per + 3, 2), (4, 5), (3, 0), (3, 19)]
        progs = ("first_own", "key0", "last_prefix", "last") if chain else CASCADE_PROGS
        B = sum(c for c, _ in groups)
        width = 34
        names, table = mp.edge_table()
        kinds_v = ("chain",) if chain else ("edge", "int", "rand")
        NB = 1 + sum(p + c * -(-max(SUFFIXES[p * BS]) // BS) for c, p in groups)
        kc, _ = _nan_cache(NB, Hkv, D)
        vcs = [torch.full((NB, Hkv, BS // 4, D, 4), float("nan"), dtype=torch.bfloat16) for _ in kinds_v]
        bt = torch.zeros(B, width, dtype=torch.int32)
        ctx = torch.zeros(B, dtype=torch.int32)
        q = torch.randn(B, (Hq + 2 * Hkv) * D, generator=gen)
        q[:, : Hq * D] = 0

        def values(n, t0, salt):
            if chain:
                return [_chain_v((n, Hkv), gen).to(torch.bfloat16)]
            t = torch.arange(t0, t0 + n)[:, None, None]
            idx = (5 * t + 4 * torch.arange(Hkv)[None, :, None] + torch.arange(4)[None, None, :] + salt) % len(names)
            return [table[idx].reshape(n, Hkv, D).to(torch.bfloat16), ap.int_values((n, Hkv, D), gen),
                    torch.randn(n, Hkv, D, generator=gen).to(torch.bfloat16)]

        nxt, b, runs = 1, 0, []
        kind_of = {}
        claim = torch.zeros(B, Hq, D, dtype=torch.float64)      # the exact value of the exact rows, first V
        claim_i = torch.zeros(B, Hq, D, dtype=torch.float64)    # and over the integer V
        spike = torch.zeros(B, Hq, dtype=torch.bool)
        flat2 = torch.zeros(B, Hq, dtype=torch.bool)
        for gi, (count, pblk) in enumerate(groups):
            pctx = pblk * BS
            shared = list(range(nxt, nxt + pblk))
            nxt += pblk
            kp = torch.randn(pctx, Hkv, D, generator=gen)
            for kvh in range(Hkv):
                for ci in range(D if pblk else 0):
                    kp[:, kvh, dims[ci]] = _column(progs[(ci + kvh) % len(progs)], pctx, 1 << 30, torch.arange(pctx), gen)
            kp = kp.to(torch.bfloat16)
            vps = values(pctx, 0, 5 * gi)
            if pblk:
                _store(kc, vcs, shared, 0, kp, vps)
            suf = SUFFIXES[pctx]
            for sg in range(count):
                L = pctx + suf[(sg + gi) % len(suf)]
                nb = -(-L // BS)
                blocks = shared + list(range(nxt, nxt + nb - pblk))
                nxt += nb - pblk
                bt[b, :nb] = torch.tensor(blocks, dtype=torch.int32)
                ctx[b] = L
                ko = torch.randn(L - pctx, Hkv, D, generator=gen)
                for kvh in range(Hkv):
                    for h in range(G):
                        ci = (sg * G + h) % D
                        kind = progs[(ci + kvh) % len(progs)]
                        ko[:, kvh, dims[ci]] = _column(kind, pctx, L, torch.arange(pctx, L), gen)
                        q[b, (kvh * G + h) * D + dims[ci]] = ap.AMP
                        kind_of[b, kvh * G + h] = (kind, dims[ci])
                ko = ko.to(torch.bfloat16)
                vos = values(L - pctx, pctx, 3 * b)
                _store(kc, vcs, blocks, pctx, ko, vos)
                keys = torch.cat([kp, ko]).double()
                vals = [torch.cat([vp, vo]).double() for vp, vo in zip(vps, vos)]
                for hq in range(Hq):
                    kind, col = kind_of[b, hq]
                    kvh = hq // G
                    at = _spike_at(kind, pctx, L)
                    pow2 = L & (L - 1) == 0
                    if at is None and not (kind == "flat" and pow2 and not chain):
                        continue
                    w = torch.softmax(ap.AMP * keys[:, kvh, col] * SCALE, 0)       # the fp64 reference of the row
                    spike[b, hq], flat2[b, hq] = at is not None, at is None
                    for vv, cl in zip(vals[:2], (claim, claim_i)):
                        if at is None and cl is claim:
                            continue                                  # flat rows are exact over integer V only
                        cl[b, hq] = vv[at, kvh] if at is not None else vv[:, kvh].mean(0)
                        # premise: the reference is the claimed value to 2^-26 relative (2^-149 absolute: below fp32)
                        err = (w @ vv[:, kvh] - cl[b, hq]).abs() - 2.0 ** -149
                        rel = float((err / cl[b, hq].abs().clamp_min(2.0 ** -149)).max())
                        assert rel <= 2.0 ** -26, (b, hq, kind, rel)
                b += 1
            runs.append((b - count, count, pblk))
        assert nxt <= NB and b == B
        if not chain:                    # the spike rows emit every block of the table
            eq, es = mp.mx_quant_ref(claim.float())
            assert mp.missing_edge_blocks(eq[spike], es[spike], names, table) == []
        tiles_np = np.zeros((-(-B // per) + len(groups) + 2, 3), dtype=np.int32)
        nt = cascade_tiles(runs, per, tiles_np)
        assert nt > len(groups)       # the first group spans two super-tiles
        return SimpleNamespace(B=B, Hq=Hq, q=q.to(torch.bfloat16).to(gpu), kc=kc.to(gpu), vcs=[v.to(gpu) for v in vcs],
                               bt=bt.to(gpu), ctx=ctx.to(gpu), tiles=torch.from_numpy(tiles_np).to(gpu),
                               claim=claim, claim_i=claim_i, spike=spike, flat2=flat2)
    return _case(("mx cascade", G, chain), build)


def _cascade_mx(gpu, c, vc, qc, pc):
    from llm_weighted_consensus_amd import ops

    qc.poison(), pc.poison()
    ops.kernels().paged_decode_cascade(c.q, c.kc, vc, c.bt, c.ctx, c.tiles, None, c.Hq, SCALE, None, None, None,
                                       qc.buf.view(mp.E4M3), pc.buf)
    torch.cuda.synchronize()
    assert qc.outside() == [] and pc.outside() == [], (qc.outside(), pc.outside())
    return qc.view.cpu(), mp.from_plane(pc.buf, c.B).cpu()


@pytest.mark.parametrize("G", [1, 4, 8])
def test_cascade_mx_exact_rows_and_bounded_rows(gpu, G):
    """Cascade decode with out8 / mx: a group over two super-tiles (2-block prefix), an odd prefix (5 blocks), an
    empty prefix and a 19-block prefix (chunked pass), out8 with 8 rows and the plane with 3 rows of sentinels
    behind the batch.  The epilogue quantises fp32 o / l, so its bytes are determined only where that value is
    exact:
      (a) spike rows (271 nats: every other key's weight is 0 in fp32) over V made of the edge-block table, and
          over integer V, are bitwise mx_quant_ref(V[at]), and flat rows whose context is a power of two, over
          integer V, are bitwise mx_quant_ref(mean); the builder asserts that the fp64 reference of each such row
          is its claimed value.
      (b) every other row of the integer-V launch and every row of an N(0, 1)-V launch against the bf16 output of
          the same call without mx: mx_probes.bounded_violations (the bound and its one exemption are derived
          there); exempt blocks must stay below 5 % of the compared ones.  The spike rows over integer V are
          held to (a), not (b): their maxima are mostly 8, a power of two, which (b) would exempt.
    Observed on an MI355X, exempt share of the compared blocks (integer V / N(0, 1) V): G = 1 2.93 % / 2.39 %,
    G = 4 3.15 % / 2.92 %, G = 8 4.33 % / 1.83 %; no byte disagreed outside the window and no element left the
    bound.  The share is printed on every run."""
    from llm_weighted_consensus_amd import ops

    c = _build_cascade(G, False, gpu)
    assert int(c.spike.sum()) > 0 and int(c.flat2.sum()) > 0
    B, Hq = c.B, c.Hq
    qc, pc = mp.ByteCage(B, Hq * D, gpu, pad=0), mp.PlaneCage(Hq, B, gpu, extra=3)
    claim = c.claim.float().reshape(B, Hq * D)
    wq, ws = mp.mx_quant_ref(claim)
    # (a) spike rows over the edge table; every block of the table is emitted
    for it in range(2):
        _cascade_mx(gpu, c, c.vcs[0], qc, pc)
        mp.check(qc, pc, wq, ws, f"cascade G={G} spike rows launch {it}", where=c.spike)
    got_q, got_sc = qc.view.cpu().view(B, Hq, D)[c.spike], mp.from_plane(pc.buf, B).cpu().view(B, Hq, 4)[c.spike]
    names, table = mp.edge_table()
    assert mp.missing_edge_blocks(got_q, got_sc, names, table) == []
    # (a) over integer V: the spike rows again (V[at]) and the flat rows of power-of-two contexts (the mean);
    # (b) every other row of that launch, and every row of the N(0, 1) launch
    exact_i = c.spike | c.flat2
    wq, ws = mp.mx_quant_ref(c.claim_i.float().reshape(B, Hq * D))
    for vi, what, where in ((1, "integer V", ~exact_i), (2, "random V", torch.ones_like(exact_i))):
        got_q, got_sc = _cascade_mx(gpu, c, c.vcs[vi], qc, pc)
        if vi == 1:
            mp.check(qc, pc, wq, ws, f"cascade G={G} exact rows over integer V", where=exact_i)
        out = ops.paged_decode_cascade(c.q, c.kc, c.vcs[vi], c.bt, c.ctx, c.tiles, Hq, SCALE)
        v, share = mp.bounded_violations(got_q, got_sc, out.float().cpu().reshape(B, Hq * D),
                                         where.repeat_interleave(4, dim=1))
        print(f"MX cascade G={G} {what}: {int(where.sum()) * 4} blocks compared, exempt {100 * share:.2f} %")
        assert not v and share <= 0.05, (what, v, share)


# ---------------------------------------------------------------------------------------------------------
# 4, 5  the reader: gemm8g with a_mx

N_OUT = 264


def _reader_case(rows, K, all_live, groups, gpu):
    def build():
        gen = torch.Generator().manual_seed(rows + K + all_live)
        A, sc = mp.scale_walk(rows, K, gen, all_live)
        assert mp.exact_in_fp32(A, sc)
        G = groups or 1
        _, W, _, w_s = gp.fp8_operands(8, G * N_OUT, K, gen)
        W, w_s = W.view(G, N_OUT, K), w_s.view(G, N_OUT)
        want = torch.zeros(rows, N_OUT, dtype=torch.float64)
        o = [0] + [int(v) for v in np.cumsum(SIZES)] if groups else [0, rows]
        for g in range(G):
            sl = slice(o[g], o[g + 1])
            want[sl] = mp.mx_product(A[sl], sc[sl], W[g], w_s[g])
        plane = mp.slice_plane(sc, K, s_rows=rows + 7, fill=200).to(gpu)     # 2^73 behind the rows
        return gp.poison_a(A, gpu), plane, gp.poison_w(W, gpu), w_s.contiguous().to(gpu), want.to(gpu)
    return _case(("reader", rows, K, all_live, groups), build)


def _weight(W, w_s):
    from llm_weighted_consensus_amd import ops

    w = ops.Fp8Weight.__new__(ops.Fp8Weight)
    w.q, w.s, w.shape = W.view(W.shape[-2], W.shape[-1]), w_s.view(1, -1), tuple(W.shape[-2:])
    return w


@pytest.mark.parametrize("all_live", [False, True])
@pytest.mark.parametrize("K", [128, 1024])
@pytest.mark.parametrize("M", [1, 255, 513])
def test_reader_dense_is_bitwise(gpu, M, K, all_live):
    """gemm8g with a_mx, dense.  all_live False: one live block per (row, 128-slice), chosen by a hash of both,
    A in {+-1, +-2}, the dead blocks zero under bytes of 110..144 that differ from the live one and from each
    other — a scale taken from the wrong row, slice or block changes the output by a power of two.  True: the
    four blocks of a slice share a byte that differs between slices and rows (spread 2^10).  W in {+-1, +-2}
    with power-of-two channel scales: the bf16 output is bitwise the RNE code of the exact product, in a cage,
    over two launches, and through ops.linear_fp8_mx.  Blocks of one slice under different scales are not
    asserted bitwise: how the MFMA aligns them is not documented (the relative test stays)."""
    from llm_weighted_consensus_amd import ops

    A, plane, W, w_s, want = _reader_case(M, K, all_live, 0, gpu)
    cage = gp.Cage(M, N_OUT, gpu)
    for it in range(2):
        cage.poison()
        ops.kernels().gemm8g_fp8(A, W, cage.view, None, -(-M // 256), None, None, w_s.view(-1), 0, plane, None)
        torch.cuda.synchronize()
        gp.check(cage, want, "bitwise", f"reader dense M={M} K={K} all_live={all_live} launch {it}")
    out = ops.linear_fp8_mx(A, plane, _weight(W, w_s))
    assert not bool(gp.bitwise(out, want).any())


@pytest.mark.parametrize("all_live", [False, True])
@pytest.mark.parametrize("K", [128, 1024])
def test_reader_grouped_is_bitwise(gpu, K, all_live):
    """The same through ops.grouped_gemm(..., a_mx=) over groups of 300, 0, 17, 129 and 128 rows."""
    from llm_weighted_consensus_amd import ops

    rows = sum(SIZES)
    A, plane, W, w_s, want = _reader_case(rows, K, all_live, len(SIZES), gpu)
    off = torch.tensor([0] + list(np.cumsum(SIZES)), dtype=torch.int32, device=gpu)
    cage = gp.Cage(rows, N_OUT, gpu)
    for it in range(2):
        cage.poison()
        ops.grouped_gemm(A, W, off, out=cage.view, w_scale=w_s, a_mx=plane)
        torch.cuda.synchronize()
        gp.check(cage, want, "bitwise", f"reader grouped K={K} all_live={all_live} launch {it}")


# ---------------------------------------------------------------------------------------------------------
# 6  plane views


def test_reader_takes_plane_views(gpu, monkeypatch):
    """The plane as row-range views a_mx[:, r0:r1] of a plane with more rows than the batch (ops.linear_fp8_mx
    with the span of a launch shrunk to 256 rows), and MXAct.index_select with a permuted row list: both bitwise
    the whole-plane call on the selected rows."""
    from llm_weighted_consensus_amd import ops

    M, K = 513, 1024
    A, plane, W, w_s, want = _reader_case(M, K, False, 0, gpu)
    w = _weight(W, w_s)
    whole = ops.linear_fp8_mx(A, plane, w)
    assert not bool(gp.bitwise(whole, want).any())
    monkeypatch.setattr(ops, "G8G_SPAN", 256 * A.stride(0) + 1)
    assert len(ops._row_blocks(M, A.stride(0))) == 3
    assert torch.equal(ops.linear_fp8_mx(A, plane, w), whole)
    monkeypatch.undo()
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5)).to(gpu)
    act = ops.MXAct(A, plane).index_select(perm)
    assert act.mx.shape == (K // 128, M, 4) and act.mx.is_contiguous()
    assert torch.equal(ops.linear_fp8(act, w), whole[perm])
    some = perm[:77]
    assert torch.equal(ops.linear_fp8(ops.MXAct(A, plane).index_select(some), w), whole[some])


# ---------------------------------------------------------------------------------------------------------
# 7  chain


def _chain_weight(K, gpu):
    def build():
        gen = torch.Generator().manual_seed(K)
        _, W, _, w_s = gp.fp8_operands(8, N_OUT, K, gen)
        return _weight(gp.poison_w(W, gpu), w_s.to(gpu)), W.float().double(), w_s.double()
    return _case(("chain weight", K), build)


def _chain_check(act, vat, w, Wd, wsd, keep, what):
    """act: the writer's MXAct; vat [rows, K] fp64: V[at] of every row.  The MX bytes are the quantised V[at],
    which they represent exactly, and linear_fp8 of the kept rows is bitwise rne(V[at] . W^T * w_scale)."""
    from llm_weighted_consensus_amd import ops

    wq, ws = mp.mx_quant_ref(vat.float())
    assert torch.equal(mp.dequant(wq, ws), vat), what
    assert torch.equal(_bytes(act.q).cpu(), wq) and torch.equal(mp.from_plane(act.mx).cpu(), ws), what
    blocks = ws.view(ws.shape[0], -1, 4)
    assert bool((blocks == blocks[..., :1]).all()) and len(ws.unique()) > 3
    out = ops.linear_fp8(act.index_select(keep), w)
    want = (vat[keep.cpu()] @ Wd.t()) * wsd[None, :]
    bad = gp.bitwise(out.cpu(), want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (4, 4)])
def test_chain_prefill_to_projection(gpu, Hq, Hkv, causal):
    """ops.prefill_attention_mx -> MXAct.index_select -> ops.linear_fp8.  Every (row, head) is a one-hot spike
    row on a key it can see, V is {+-1, +-2} * 2^c with one c per (key, KV head), so the attention output is
    V[at], its four blocks per head share a scale byte, and the projection by W in {+-1, +-2} with power-of-two
    channel scales is exact in fp32: bitwise rne(V[at] . W^T * w_scale), N = 264."""
    from llm_weighted_consensus_amd import ops

    def build():
        gen = torch.Generator().manual_seed(11 * Hq + causal)
        dims, G = ap.probe_dims(D), Hq // Hkv
        qs, ks, vs, vat = [], [], [], []
        for L in LENS:
            P = sorted(p for p in {0, 15, 16, 31, 32, 63, 64, L - 1} if p < L)
            k = torch.randn(L, Hkv, D, generator=gen)
            for kvh in range(Hkv):
                for j, p in enumerate(P):
                    k[:, kvh, dims[(11 * j + kvh) % D]] = ap.k_column(ap.Prog("spike", at=p), torch.arange(L), SCALE, gen)
            v = _chain_v((L, Hkv), gen)
            q = torch.zeros(L, Hq, D)
            va = torch.zeros(L, Hq, D, dtype=torch.float64)
            for r in range(L):
                vis = [j for j, p in enumerate(P) if p <= r or not causal]
                for hq in range(Hq):
                    j = vis[(r + 3 * hq) % len(vis)]
                    q[r, hq, dims[(11 * j + hq // G) % D]] = ap.AMP
                    va[r, hq] = v[P[j], hq // G].double()
            qs.append(q.view(L, -1)), ks.append(k.view(L, -1)), vs.append(v.view(L, -1)), vat.append(va.view(L, -1))
        qkv = torch.cat([torch.cat(qs), torch.cat(ks), torch.cat(vs)], 1).to(torch.bfloat16).to(gpu)
        return qkv, torch.cat(vat)
    qkv, vat = _case(("chain prefill", Hq, Hkv, causal), build)
    T = qkv.shape[0]
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32, device=gpu)
    q, k, v = qkv[:, : Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    act = ops.prefill_attention_mx(q, k, v, cu, max(LENS), Hq, Hkv, SCALE, causal)
    w, Wd, wsd = _chain_weight(Hq * D, gpu)
    keep = torch.randperm(T, generator=torch.Generator().manual_seed(1))[: T // 2].to(gpu)
    _chain_check(act, vat, w, Wd, wsd, keep, f"chain prefill Hq={Hq} causal={causal}")


@pytest.mark.parametrize("G", [2, 4])
def test_chain_cascade_to_projection(gpu, G):
    """ops.paged_decode_cascade(..., mx=True) -> MXAct.index_select -> ops.linear_fp8 on the cascade groups of the
    test above with every row a 271-nat spike row (first own key, key 0, last prefix key, last key)."""
    from llm_weighted_consensus_amd import ops

    c = _build_cascade(G, True, gpu)
    assert bool(c.spike.all())
    act = ops.paged_decode_cascade(c.q, c.kc, c.vcs[0], c.bt, c.ctx, c.tiles, c.Hq, SCALE, mx=True)
    w, Wd, wsd = _chain_weight(c.Hq * D, gpu)
    keep = torch.randperm(c.B, generator=torch.Generator().manual_seed(2)).to(gpu)
    _chain_check(act, c.claim.reshape(c.B, -1), w, Wd, wsd, keep, f"chain cascade G={G}")


# ---------------------------------------------------------------------------------------------------------
# 8  refusals


def test_mx_calls_that_must_be_refused(gpu):
    """Refused by the binding or the launcher before anything is written (the caged outputs keep their
    sentinels): mode 2 with N % 256 != 0, a plane with fewer rows than C, ldc % 16 != 0, a_mx with a_rows or with
    mode 1, cascade out8 without mx, and head_dim 64 with mx."""
    from llm_weighted_consensus_amd import ops

    K8 = ops.kernels()
    M, K = 40, 128
    gen = torch.Generator().manual_seed(0)

    def operands(N):
        A, W, a_s, w_s = gp.fp8_operands(M, N, K, gen)
        return A.to(gpu), W.view(1, N, K).to(gpu), a_s.to(gpu), w_s.to(gpu)

    def untouched(*cages):
        torch.cuda.synchronize()
        assert all(c.outside() == [] and bool((c.buf == c.buf.view(-1)[0]).all()) for c in cages)

    A, W, a_s, w_s = operands(320)
    qc, pc = mp.ByteCage(M, 160, gpu), mp.PlaneCage(1, M, gpu)
    with pytest.raises(RuntimeError):                      # N % 256 != 0
        K8.gemm8g_fp8(A, W, qc.f8, None, 1, None, a_s, w_s, 2, None, pc.buf)
    untouched(qc, pc)
    A, W, a_s, w_s = operands(512)
    qc, pc = mp.ByteCage(M, 256, gpu), mp.PlaneCage(2, M, gpu)
    with pytest.raises(RuntimeError):                      # s_rows < rows
        K8.gemm8g_fp8(A, W, qc.f8, None, 1, None, a_s, w_s, 2, None, pc.buf[:, :M - 1].contiguous())
    with pytest.raises(RuntimeError):                      # a row-range view shorter than C
        K8.gemm8g_fp8(A, W, qc.f8, None, 1, None, a_s, w_s, 2, None, pc.buf[:, :M - 1])
    untouched(qc, pc)
    odd = torch.full((M + 8, 256 + 8), mp.SENTINEL8, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError):                      # ldc % 16 != 0
        K8.gemm8g_fp8(A, W, odd.view(mp.E4M3)[:M, :256], None, 1, None, a_s, w_s, 2, None, pc.buf)
    torch.cuda.synchronize()
    assert bool((odd == mp.SENTINEL8).all())
    untouched(pc)
    plane = torch.full((1, M, 4), 127, dtype=torch.uint8, device=gpu)
    rows_i = torch.arange(M, dtype=torch.int32, device=gpu)
    cage = gp.Cage(M, 512, gpu)
    with pytest.raises(RuntimeError):                      # a_mx with a_rows
        K8.gemm8g_fp8(A, W, cage.view, None, 1, rows_i, None, w_s, 0, plane, None)
    half = gp.Cage(M, 256, gpu)
    with pytest.raises(RuntimeError):                      # a_mx with mode 1
        K8.gemm8g_fp8(A, W, half.view, None, 1, None, None, w_s, 1, plane, None)
    torch.cuda.synchronize()
    for c in (cage, half):
        assert c.outside_touched() == 0 and bool((gp.bits(c.view) == gp.SENTINEL).all())

    # cascade: out8 without mx; head_dim 64 with out8 and mx
    for Dh in (128, 64):
        B, Hq, Hkv = 2, 4, 2
        kc = torch.zeros(3, Hkv, BS, Dh, dtype=torch.bfloat16, device=gpu)
        vc = torch.zeros(3, Hkv, BS // 4, Dh, 4, dtype=torch.bfloat16, device=gpu)
        q = torch.zeros(B, (Hq + 2 * Hkv) * Dh, dtype=torch.bfloat16, device=gpu)
        bt = torch.tensor([[1, 0], [2, 0]], dtype=torch.int32, device=gpu)
        ctx = torch.ones(B, dtype=torch.int32, device=gpu)
        tiles = torch.tensor([[0, 2, 0]], dtype=torch.int32, device=gpu)
        qc, pc = mp.ByteCage(B, Hq * Dh, gpu, pad=0), mp.PlaneCage(Hq * Dh // 128, B, gpu)
        with pytest.raises(RuntimeError):
            K8.paged_decode_cascade(q, kc, vc, bt, ctx, tiles, None, Hq, 1.0, None, None, None, qc.buf.view(mp.E4M3),
                                    None if Dh == 128 else pc.buf)
        untouched(qc, pc)
    with pytest.raises(ValueError):
        ops.paged_decode_cascade(q, kc, vc, bt, ctx, tiles, Hq, 1.0, mx=True)
