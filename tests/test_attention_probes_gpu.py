"""Attention kernels under structured inputs (tests/attn_probes.py) against the fp32 reference.

The random inputs of tests/test_kernels_gpu.py never rescale a non-empty softmax accumulator and cannot see
one wrong key in a long context.  Here every query row is one-hot, so a K column programmes its scores:
staircases that force the lazy rescale at every tile, spikes on every edge key, flat rows whose exact output
is mean(V), and background rows that must not move when a neighbour rescales — mixed inside every 16-row
MFMA tile.  tests/test_attention_probes.py shows on the CPU that these comparisons reject a dropped, doubled
or leaked key, a skipped O rescale and an alpha taken from the wrong row.

Every case is built once on the host, its reference computed once and shared by the parametrisations that
run it.  Each case runs its kernel twice: with V ~ N(0, 1) every row is held to the suite's attention bound
(atol = rtol = 2e-2); with small integer V the flat rows are held to rtol = 2^-8, atol = 0.  No load-time
RoPE (it would rotate the one-hot rows); the whole cache outside the contexts is NaN."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import attn_probes as ap
from tests import torch_ref as ref

pytestmark = pytest.mark.gpu

BS = 16
_cases = {}


def _case(key, build, gpu):
    if key not in _cases:
        _cases[key] = build(gpu)
    return _cases[key]


@pytest.fixture(params=["wg4", "wave"])
def decode_path(request, gpu):
    """Both plain-decode kernels: 4 waves per sequence, and one wave per (sequence, split)."""
    from llm_weighted_consensus_amd import ops

    old = ops.set_decode_wave_min_items(1 << 30 if request.param == "wg4" else 0)
    yield request.param
    ops.set_decode_wave_min_items(old)


def _nan_cache(NB, Hkv, D):
    nan = float("nan")
    return (torch.full((NB, Hkv, BS, D), nan, dtype=torch.bfloat16),
            [torch.full((NB, Hkv, BS // 4, D, 4), nan, dtype=torch.bfloat16) for _ in range(2)])


def _store(kc, vcs, blocks, t0, k, vs):
    """Write keys k [n, Hkv, D] and each values tensor of vs at key positions t0.. of a sequence whose
    logical blocks are ``blocks`` (physical ids): K token-major, V 4-token interleaved."""
    t = torch.arange(t0, t0 + k.shape[0])
    blk, off = torch.as_tensor(blocks, dtype=torch.long)[t // BS], t % BS
    kc[blk, :, off, :] = k
    for vc, v in zip(vcs, vs):
        vc[blk, :, off // 4, :, off % 4] = v


def _paged_ref(q, kc, vc, bt_row, L, causal, scale):
    """torch_ref.attention of query rows q [n, Hq, D] on the L keys the block table addresses."""
    from llm_weighted_consensus_amd import ops

    toks = torch.arange(L, device=kc.device)
    blk = bt_row[toks // BS].long()
    return ref.attention(q, kc[blk, :, toks % BS, :], ops.v_gather(vc, blk, toks % BS), causal, scale)


def _check(out, want, out_i, want_i, flat, what):
    """All rows at the suite's bound (V ~ N(0, 1)); flat rows of the integer-V run at one bf16 rounding."""
    assert flat.any() and not flat.all()
    ap.assert_close(out.float(), want, ap.ATOL, ap.RTOL, what)
    ap.assert_close(out_i.float()[flat], want_i[flat], 0.0, ap.FLAT_RTOL, what + " (flat rows, integer V)")


def _row_conditions(prog, s, orders, scale, stats):
    """Preconditions of one row from the reference's own scores s [L] (visible keys only): a visible spike
    holds >= 0.999 of the weight; a staircase forces the rescale branch, on a non-empty accumulator, at every
    tile boundary its slope promises, for each processing order in ``orders``."""
    if prog.kind == "spike" and 0 <= prog.at < s.numel():
        assert ap.key_weight(s, prog.at) >= 0.999, prog
        stats["spikes"] += 1
    if prog.kind == "stair":
        for name, tiles in orders:
            n = ap.forced_rescales(s, tiles)
            assert n == ap.stair_rises(tiles, scale, prog.slope), (prog, tiles)
            stats[name] = stats.get(name, 0) + n


# ---------------------------------------------------------------------------------------------------------
# ops.paged_decode

# 449 = 29 blocks: with 3 splits a wave of the 4-wave kernel still gets two pairs (pairs 0 and 4 of 5)
CTX = [1, 16, 17, 32, 33, 49, 200, 257, 449]


def _build_decode(G, splits):
    def build(gpu):
        gen = torch.Generator().manual_seed(100 * G + splits)
        Hkv, D = 2, 128
        Hq, scale, dims = Hkv * G, 1 / math.sqrt(128), ap.probe_dims(128)
        seqs = []
        for L in CTX:  # enough sequences per context for every programme to appear
            progs = ap.decode_programmes(L, splits)
            seqs += [(L, rep, progs) for rep in range(-(-len(progs) // Hq))]
        B, width = len(seqs), -(-max(CTX) // BS) + 1
        NB = 1 + sum(-(-L // BS) for L, _, _ in seqs)  # block 0 stays NaN: padding table entries point at it
        kc, (vc, vci) = _nan_cache(NB, Hkv, D)
        perm = 1 + torch.randperm(NB - 1, generator=gen)
        bt = torch.zeros(B, width, dtype=torch.int32)
        q = torch.randn(B, (Hq + 2 * Hkv) * D, generator=gen)
        q[:, : Hq * D] = 0
        flat = torch.zeros(B, Hq, dtype=torch.bool)
        stats, used = {"spikes": 0}, 0
        for b, (L, rep, progs) in enumerate(seqs):
            nb = -(-L // BS)
            bt[b, :nb] = perm[used:used + nb].to(torch.int32)
            used += nb
            k = torch.randn(L, Hkv, D, generator=gen)
            t = torch.arange(L)
            rows = []
            for kvh in range(Hkv):
                wave = []
                for h in range(G):
                    pi = ((rep * Hkv + kvh) * G + h) % len(progs)
                    col = dims[(7 * h + 3 * kvh + b) % D]  # distinct over the heads of a KV head
                    k[:, kvh, col] = ap.k_column(progs[pi], t, scale, gen)
                    q[b, (kvh * G + h) * D + col] = ap.AMP
                    flat[b, kvh * G + h] = progs[pi].kind == "flat"
                    rows.append((kvh, h, progs[pi]))
                    wave.append(pi)
                assert len(set(wave)) == min(G, len(progs))  # rows of one wave: different programmes
            k = k.to(torch.bfloat16)
            v = torch.randn(L, Hkv, D, generator=gen).to(torch.bfloat16)
            vi = ap.nonzero_prefix_sums(ap.int_values((L, Hkv, D), gen))
            _store(kc, (vc, vci), bt[b, :nb].tolist(), 0, k, (v, vi))
            qb = q[b, : Hq * D].view(Hq, D).to(torch.bfloat16)
            orders = [(path + str(i), st) for path in ("wg4", "wave")
                      for i, st in enumerate(ap.decode_tiles(L, splits, path))]
            for kvh, h, prog in rows:
                s = ap.scores_nats(qb[kvh * G + h][None], k[:, kvh], scale)[0]
                _row_conditions(prog, s, orders, scale, stats)
        c = SimpleNamespace(Hq=Hq, scale=scale, splits=splits, flat=flat.to(gpu), stats=stats,
                            q=q.to(torch.bfloat16).to(gpu), kc=kc.to(gpu), vc=vc.to(gpu), vci=vci.to(gpu),
                            bt=bt.to(gpu), ctx=torch.tensor([L for L, _, _ in seqs], dtype=torch.int32, device=gpu))
        qh = c.q[:, : Hq * D].view(B, 1, Hq, D)
        c.want = torch.cat([_paged_ref(qh[b], c.kc, c.vc, c.bt[b], L, False, scale)
                            for b, (L, _, _) in enumerate(seqs)])
        c.want_i = torch.cat([_paged_ref(qh[b], c.kc, c.vci, c.bt[b], L, False, scale)
                              for b, (L, _, _) in enumerate(seqs)])
        return c
    return build


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("G", [1, 4, 8])
def test_paged_decode_probes(gpu, G, splits, decode_path):
    """Plain decode, both kernels, contexts {1, 16, 17, 32, 33, 49, 200, 257, 449}: pairs with and without a
    B block, a B block of one key, odd and even blocks per split (pairs starting on odd blocks), empty splits.
    Each wave's G rows carry different programmes: staircase (every pair of every wave / split rescales a
    live accumulator, and consecutive splits differ by tens of log2 units in lse — the reduce kernel's
    weighting), flat, background, and a spike on each of keys {0, 15, 16, 31, 32, L-2, L-1} and on the first
    and last key of every split range.  Flat rows: the wg4 combine weighs with exp2f(0) = 1 exactly; the
    split-K reduce goes through log2f / exp2f of the key counts, ~1e-6 relative (times the cancellation among
    the split means, < 200 here), which stays inside 2^-8 next to the one bf16 rounding of 2^-9."""
    from llm_weighted_consensus_amd import ops

    c = _case(("decode", G, splits), _build_decode(G, splits), gpu)
    # preconditions, from the reference's scores: live-accumulator rescales in the states of THIS path
    assert sum(n for name, n in c.stats.items() if name.startswith(decode_path)) > 0 and c.stats["spikes"] > 0
    out = ops.paged_decode(c.q, c.kc, c.vc, c.bt, c.ctx, c.Hq, c.scale, num_splits=splits)
    out_i = ops.paged_decode(c.q, c.kc, c.vci, c.bt, c.ctx, c.Hq, c.scale, num_splits=splits)
    _check(out, c.want, out_i, c.want_i, c.flat, f"paged_decode {decode_path} G={G} splits={splits}")


# ---------------------------------------------------------------------------------------------------------
# ops.paged_decode_cascade

SUFFIX = [1, 15, 16, 17, 33]


def _build_cascade(G):
    def build(gpu):
        from llm_weighted_consensus_amd import ops
        from llm_weighted_consensus_amd.engine.engine import cascade_tiles

        gen = torch.Generator().manual_seed(40 + G)
        Hkv, D = 2, 128
        Hq, scale, dims = Hkv * G, 1 / math.sqrt(128), ap.probe_dims(128)
        per, spw = ops.cascade_rows_per_tile(G), 16 // G
        assert per * G == D  # a super-tile's rows of one KV head: one K column each
        # (count, prefix blocks): larger than a super-tile; an odd prefix (last prefix pair without a B block);
        # plain rows; a prefix of more than one 16-block LDS chunk (chunk edge between keys 255 and 256)
        groups = [(per + 9, 2), (7, 5), (3, 0), (5, 19)]
        B = sum(c for c, _ in groups)
        width = 24
        NB = 1 + sum(p + c * 3 for c, p in groups)
        kc, (vc, vci) = _nan_cache(NB, Hkv, D)
        bt = torch.zeros(B, width, dtype=torch.int32)
        ctx = torch.zeros(B, dtype=torch.int32)
        q = torch.randn(B, (Hq + 2 * Hkv) * D, generator=gen)
        q[:, : Hq * D] = 0
        flat = torch.zeros(B, Hq, dtype=torch.bool)
        nxt, b, runs, keys, rowprog = 1, 0, [], {}, {}
        for gi, (count, pblk) in enumerate(groups):
            progs = ap.cascade_programmes(pblk)
            assert len(progs) % 2 == 1
            pctx = pblk * BS
            shared = list(range(nxt, nxt + pblk))
            nxt += pblk
            kp = torch.randn(pctx, Hkv, D, generator=gen)
            for kvh in range(Hkv):  # the shared part of all 128 row programmes
                for ci in range(D if pblk else 0):
                    p = progs[(ci + kvh) % len(progs)]
                    p = p(1 << 30) if callable(p) else p
                    kp[:, kvh, dims[ci]] = ap.k_column(p, torch.arange(pctx), scale, gen)
            kp = kp.to(torch.bfloat16)
            vp = torch.randn(pctx, Hkv, D, generator=gen).to(torch.bfloat16)
            vpi = ap.nonzero_prefix_sums(ap.int_values((pctx, Hkv, D), gen))
            if pblk:
                _store(kc, (vc, vci), shared, 0, kp, (vp, vpi))
            for sg in range(count):
                L = pctx + SUFFIX[(sg + gi) % len(SUFFIX)]
                nb = -(-L // BS)
                blocks = shared + list(range(nxt, nxt + nb - pblk))
                nxt += nb - pblk
                bt[b, :nb] = torch.tensor(blocks, dtype=torch.int32)
                ctx[b] = L
                ko = torch.randn(L - pctx, Hkv, D, generator=gen)
                for kvh in range(Hkv):
                    for h in range(G):
                        ci = (sg * G + h) % D  # the row's place in its super-tile
                        pi = (ci + kvh) % len(progs)
                        p = progs[pi](L) if callable(progs[pi]) else progs[pi]
                        ko[:, kvh, dims[ci]] = ap.k_column(p, torch.arange(pctx, L), scale, gen)
                        q[b, (kvh * G + h) * D + dims[ci]] = ap.AMP
                        flat[b, kvh * G + h] = p.kind == "flat"
                        rowprog[b, kvh, h] = (pi, p)
                ko = ko.to(torch.bfloat16)
                vo = torch.randn(L - pctx, Hkv, D, generator=gen).to(torch.bfloat16)
                voi = ap.nonzero_prefix_sums(ap.int_values((L - pctx, Hkv, D), gen), vpi.float().sum(0))
                _store(kc, (vc, vci), blocks, pctx, ko, (vo, voi))
                keys[b] = torch.cat([kp, ko])
                b += 1
            runs.append((b - count, count, pblk))
        assert nxt <= NB
        tiles_np = np.zeros((-(-B // per) + len(groups) + 2, 3), dtype=np.int32)
        nt = cascade_tiles(runs, per, tiles_np)
        assert nt >= len(groups)
        # preconditions per wave, in the order the kernel attends that wave's keys
        qb = q.to(torch.bfloat16)
        stats = {"spikes": 0}
        for r0, nseq, pb in tiles_np[:nt].tolist():
            for w0 in range(r0, r0 + nseq, spw):
                wave = list(range(w0, min(w0 + spw, r0 + nseq)))
                ctxs = [int(ctx[i]) for i in wave]
                name = "chunked" if pb > 16 else "interleaved" if pb else "plain"
                for kvh in range(Hkv):
                    mine = [tuple(rowprog[i, kvh, h][0] for h in range(G)) for i in wave]
                    # sequences of one wave: different programmes (G = 1: as many as there are)
                    assert len(set(mine)) == min(len(wave), len(ap.cascade_programmes(pb)))
                    for j, i in enumerate(wave):
                        order = ap.cascade_row_tiles(pb, ctxs, j)
                        for h in range(G):
                            s = ap.scores_nats(qb[i, (kvh * G + h) * D:][None, :D], keys[i][:, kvh], scale)[0]
                            _row_conditions(rowprog[i, kvh, h][1], s, [(name, order)], scale, stats)
        c = SimpleNamespace(Hq=Hq, scale=scale, flat=flat.to(gpu), stats=stats, q=qb.to(gpu), kc=kc.to(gpu),
                            vc=vc.to(gpu), vci=vci.to(gpu), bt=bt.to(gpu), ctx=ctx.to(gpu),
                            tiles=torch.from_numpy(tiles_np).to(gpu))
        qh = c.q[:, : Hq * D].view(B, 1, Hq, D)
        c.want = torch.cat([_paged_ref(qh[i], c.kc, c.vc, c.bt[i], int(ctx[i]), False, scale) for i in range(B)])
        c.want_i = torch.cat([_paged_ref(qh[i], c.kc, c.vci, c.bt[i], int(ctx[i]), False, scale) for i in range(B)])
        return c
    return build


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_paged_decode_cascade_probes(gpu, G):
    """Cascade decode: a group larger than a super-tile (2-block prefix), an odd prefix (5 blocks), plain
    rows, and a 19-block prefix (chunked pass; chunk edge at keys 255 / 256); suffixes of {1, 15, 16, 17, 33}
    keys.  Every (sequence, head) row of a super-tile has its own K column, so rows differ INSIDE the shared
    prefix and the 16/G sequences of a wave run different programmes: while one sequence's suffix is walked
    (row_on) and its staircase rescales, its neighbours' rows must not move.  Spikes sit on prefix keys 0 and
    pctx - 1, on the first own key pctx, on L - 1 and on 255 / 256; the rising staircase crosses the
    prefix / suffix boundary (forced rescales in the chunked pass), a falling one makes the first prefix pair
    of the interleaved pass tower over the suffix pair accumulated before it.  Flat rows are exact: the
    prefix and suffix states merge in registers with alpha = 1."""
    from llm_weighted_consensus_amd import ops

    c = _case(("cascade", G), _build_cascade(G), gpu)
    assert c.stats["chunked"] > 0 and c.stats["interleaved"] > 0 and c.stats["spikes"] > 0
    out = ops.paged_decode_cascade(c.q, c.kc, c.vc, c.bt, c.ctx, c.tiles, c.Hq, c.scale)
    out_i = ops.paged_decode_cascade(c.q, c.kc, c.vci, c.bt, c.ctx, c.tiles, c.Hq, c.scale)
    _check(out, c.want, out_i, c.want_i, c.flat, f"paged_decode_cascade G={G}")


# ---------------------------------------------------------------------------------------------------------
# ops.prefill_attention (keys = queries, and cu_seqlens_k) and ops.prefill_attention_paged


def _build_prefill(ql, kl, Hq, Hkv, D, causal, paged=False):
    def build(gpu):
        gen = torch.Generator().manual_seed(7 * Hq + D + len(ql) + 2 * causal)
        scale, dims, G = 1 / math.sqrt(D), ap.probe_dims(D), Hq // Hkv
        q = torch.zeros(sum(ql), Hq * D)
        flat = torch.zeros(sum(ql), Hq, dtype=torch.bool)
        ks, vs, vis, conds = [], [], [], []
        q0 = 0
        for a, n in zip(ql, kl):
            qoff = n - a
            progs = ap.prefill_programmes(n, qoff)
            k = torch.randn(n, Hkv, D, generator=gen)
            col = lambda pi, kvh: dims[(11 * pi + kvh) % D]  # noqa: E731  (distinct over pi < D)
            for kvh in range(Hkv):
                for pi, p in enumerate(progs):
                    k[:, kvh, col(pi, kvh)] = ap.k_column(p, torch.arange(n), scale, gen)
            for r in range(a):  # query token r, head hq: consecutive tokens and heads take different programmes
                for hq in range(Hq):
                    pi = (r + 3 * hq) % len(progs)
                    q[q0 + r, hq * D + col(pi, hq // G)] = ap.AMP
                    flat[q0 + r, hq] = progs[pi].kind == "flat"
                    conds.append((len(ks), q0 + r, hq, progs[pi], r + qoff + 1 if causal else n))
            ks.append(k.to(torch.bfloat16))
            vs.append(torch.randn(n, Hkv, D, generator=gen).to(torch.bfloat16))
            vis.append(ap.nonzero_prefix_sums(ap.int_values((n, Hkv, D), gen)))
            q0 += a
        qb = q.to(torch.bfloat16)
        stats = {"spikes": 0}
        for i, row, hq, prog, nvis in conds:
            if prog.kind in ("spike", "stair"):
                s = ap.scores_nats(qb[row, hq * D:][None, :D], ks[i][:nvis, hq // G], scale)[0]
                _row_conditions(prog, s, [("tiles", ap.tiles_of(nvis))], scale, stats)
        c = SimpleNamespace(scale=scale, flat=flat.to(gpu), stats=stats, q=qb.to(gpu),
                            cu_q=torch.tensor([0] + list(np.cumsum(ql)), dtype=torch.int32, device=gpu),
                            cu_k=torch.tensor([0] + list(np.cumsum(kl)), dtype=torch.int32, device=gpu))
        want, want_i = [], []
        q0 = 0
        for i, a in enumerate(ql):
            qi = c.q[q0:q0 + a].view(a, Hq, D)
            want.append(ref.attention(qi, ks[i].to(gpu), vs[i].to(gpu), causal, scale))
            want_i.append(ref.attention(qi, ks[i].to(gpu), vis[i].to(gpu), causal, scale))
            q0 += a
        c.want, c.want_i = torch.cat(want), torch.cat(want_i)
        if not paged:
            c.k = torch.cat(ks).view(-1, Hkv * D).to(gpu)
            c.v, c.vi = (torch.cat(x).view(-1, Hkv * D).to(gpu) for x in (vs, vis))
            return c
        W = 2 * -(-max(kl) // 32)
        NB = 1 + sum(-(-n // BS) for n in kl)
        kc, (vc, vci) = _nan_cache(NB, Hkv, D)
        perm = 1 + torch.randperm(NB - 1, generator=gen)
        bt = torch.zeros(len(kl), W, dtype=torch.int32)
        used = 0
        for i, n in enumerate(kl):
            nb = -(-n // BS)
            bt[i, :nb] = perm[used:used + nb].to(torch.int32)
            used += nb
            _store(kc, (vc, vci), bt[i, :nb].tolist(), 0, ks[i], (vs[i], vis[i]))
        qkv = torch.randn(sum(ql), (Hq + 2 * Hkv) * D, generator=gen).to(torch.bfloat16)
        qkv[:, : Hq * D] = qb
        c.q, c.kc, c.vc, c.vci, c.bt = qkv.to(gpu), kc.to(gpu), vc.to(gpu), vci.to(gpu), bt.to(gpu)
        c.k_lens = torch.tensor(kl, dtype=torch.int32, device=gpu)
        return c
    return build


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (4, 4)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_prefill_attention_probes(gpu, causal, D, Hq, Hkv):
    """Prefill, keys = queries, lengths {1, 17, 64, 65, 100, 130} (across the 16-query wave and 64-query
    workgroup edges).  The 16 query tokens of a wave pick different K columns: under the causal staircase each
    row hangs on its diagonal key and key i + 1 would outweigh the whole row (the mask, and the unmasked
    interior-tile shortcut); every full tile rescales a live accumulator; flat rows are the exact running
    means of V; spikes sit on keys 0, 31 / 32, 63 / 64 and L - 1, inside and between the waves' query ranges."""
    from llm_weighted_consensus_amd import ops

    lens = [1, 17, 64, 65, 100, 130]
    c = _case(("prefill", causal, D, Hq, Hkv), _build_prefill(lens, lens, Hq, Hkv, D, causal), gpu)
    assert c.stats["tiles"] > 0 and c.stats["spikes"] > 0
    out = ops.prefill_attention(c.q, c.k, c.v, c.cu_q, max(lens), Hq, Hkv, D, c.scale, causal)
    out_i = ops.prefill_attention(c.q, c.k, c.vi, c.cu_q, max(lens), Hq, Hkv, D, c.scale, causal)
    _check(out.view(-1, Hq, D), c.want, out_i.view(-1, Hq, D), c.want_i, c.flat,
           f"prefill_attention causal={causal} D={D} Hq={Hq}")


QL, KL = [1, 17, 64, 70, 32, 5], [33, 17, 200, 118, 32, 300]


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 2), (64, 4, 4)])
def test_prefill_attention_key_ranges_probes(gpu, D, Hq, Hkv):
    """Cached-prefix prefill (cu_seqlens_k): the queries are the last rows of a longer key range.  Staircase
    and flat rows as above, with the causal offset; spikes on key 0, on the first query's own key kl - ql
    (the last key it may see) and the tile / workgroup edges counted from it, and on the last key."""
    from llm_weighted_consensus_amd import ops

    ql, kl = QL[:4], KL[:4]
    c = _case(("ranges", D, Hq, Hkv), _build_prefill(ql, kl, Hq, Hkv, D, True), gpu)
    assert c.stats["tiles"] > 0 and c.stats["spikes"] > 0
    run = lambda v: ops.prefill_attention(c.q, c.k, v, c.cu_q, max(ql), Hq, Hkv, D, c.scale, True,  # noqa: E731
                                          cu_seqlens_k=c.cu_k, lens=(ql, kl)).view(-1, Hq, D)
    _check(run(c.v), c.want, run(c.vi), c.want_i, c.flat, f"prefill_attention key ranges D={D}")


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (4, 4)])
def test_prefill_attention_paged_probes(gpu, Hq, Hkv):
    """Chunked prefill out of the paged cache (scattered blocks, everything outside the key ranges NaN), q a
    strided view of the qkv rows: the same programmes and spike positions as the key-range test."""
    from llm_weighted_consensus_amd import ops

    D = 128
    c = _case(("paged", Hq, Hkv), _build_prefill(QL, KL, Hq, Hkv, D, True, paged=True), gpu)
    assert c.stats["tiles"] > 0 and c.stats["spikes"] > 0
    run = lambda vc: ops.prefill_attention_paged(c.q, c.kc, vc, c.cu_q, c.bt, c.k_lens, max(QL), Hq,  # noqa: E731
                                                 c.scale, lens=(QL, KL)).view(-1, Hq, D)
    _check(run(c.vc), c.want, run(c.vci), c.want_i, c.flat, f"prefill_attention_paged Hq={Hq}")
