"""Decode attention at head_dim 64 and at GQA groups that do not divide 16, against the fp32 reference.

Same oracles and bounds as tests/test_kernels_gpu.py and tests/test_attention_probes_gpu.py
(``torch_ref.attention`` on the bf16 tensors the kernel gets; atol = rtol = 2e-2; flat rows with integer V at
rtol = 2^-8), at the shapes those files never ran: (head_dim, group) in {(64, 1), (64, 4), (64, 7), (64, 8),
(128, 3), (128, 5), (128, 6), (128, 7)}, always with 2 KV heads.  Every cache slot past a context is NaN, K and V:
at head_dim 64 a (block, head) segment is 2 KiB, and a buffer resource left at the 4 KiB of head_dim 128 would let
the lanes of out-of-context tokens read the next head's segment (or the NaN tail) instead of zeros.

Every case is built once, its reference computed once and shared by the parametrisations that run it."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import attn_probes as ap
from tests import torch_ref as ref

pytestmark = pytest.mark.gpu

BS, HKV = 16, 2
SHAPES = [(64, 1), (64, 4), (64, 7), (64, 8), (128, 3), (128, 5), (128, 6), (128, 7)]
PROBE_SHAPES = [(64, 4), (128, 7)]
_cases = {}


def _case(key, build, dev):
    if key not in _cases:
        _cases[key] = build(dev)
    return _cases[key]


@pytest.fixture(params=["wg4", "wave"])
def decode_path(request, gpu):
    """Both plain-decode kernels: 4 waves per sequence, and one wave per (sequence, split)."""
    from llm_weighted_consensus_amd import ops

    old = ops.set_decode_wave_min_items(1 << 30 if request.param == "wg4" else 0)
    yield request.param
    ops.set_decode_wave_min_items(old)


def rows_per_tile(G):
    """Sequences per cascade super-tile: 8 waves of floor(16 / G) (checked against the extension on the GPU)."""
    return 8 * (16 // G)


def _bf(*shape, gen):
    return torch.randn(*shape, generator=gen).to(torch.bfloat16)


def _rope(D, B, dev, gen):
    """(cos, sin, positions) for the load-time RoPE at head_dim D: q arrives un-rotated."""
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import rope_tables

    cos, sin = rope_tables(decoder_config("llama-tiny", head_dim=D), dev, 512)
    assert cos.shape == (512, D // 2)
    return cos, sin, torch.randint(0, 500, (B,), generator=gen, dtype=torch.int32).to(dev)


def _q_ref(q_full, b, Hq, D, rope):
    q = q_full[b, : Hq * D].view(1, Hq, D)
    if rope is None:
        return q
    cos, sin, pos = rope
    return ref.rope(q, pos[b:b + 1], cos, sin).to(torch.bfloat16)


def _poison_tails(kc, vc, bt, ctx):
    """NaN in every slot of a sequence's last block at or past its context, K and V."""
    for b in range(bt.shape[0]):
        L = int(ctx[b])
        if L % BS:
            last = int(bt[b, (L - 1) // BS])
            kc[last, :, L % BS:, :] = float("nan")
            for t in range(L % BS, BS):
                vc[last, :, t // 4, :, t % 4] = float("nan")


def _reference(c, D, Hq, rows=None):
    """torch_ref.attention of every sequence (or of ``rows``) on the keys its block table addresses."""
    from llm_weighted_consensus_amd import ops

    out = {}
    for b in (range(c.q.shape[0]) if rows is None else rows):
        L = int(c.ctx[b])
        toks = torch.arange(L, device=c.q.device)
        blk = c.bt[b, toks // BS].long()
        out[b] = ref.attention(_q_ref(c.q, b, Hq, D, c.rope), c.kc[blk, :, toks % BS, :],
                               ops.v_gather(c.vc, blk, toks % BS), False, 1 / math.sqrt(D))[0]
    return out


def _close(a, b, what):
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    err = (a - b).abs()
    assert (err <= ap.ATOL + ap.RTOL * b.abs()).all(), f"{what}: max err {err.max().item():.4g}"


# ---------------------------------------------------------------------------------------------------------
# 1. plain decode, random inputs

CTX = [1, 15, 16, 77, 200]


def build_decode(D, G, rope):
    def build(dev):
        gen = torch.Generator().manual_seed(1000 + 10 * D + G)
        Hq, B, width, NB = HKV * G, len(CTX), 16, 64
        # unused blocks stay NaN too: padding table entries point at block 0, which no sequence owns
        kc = torch.full((NB, HKV, BS, D), float("nan"), dtype=torch.bfloat16)
        vc = torch.full((NB, HKV, BS // 4, D, 4), float("nan"), dtype=torch.bfloat16)
        perm = 1 + torch.randperm(NB - 1, generator=gen)
        bt = torch.zeros(B, width, dtype=torch.int32)
        used = 0
        for b, L in enumerate(CTX):
            nb = -(-L // BS)
            bt[b, :nb] = perm[used:used + nb].to(torch.int32)
            kc[bt[b, :nb].long()] = _bf(nb, HKV, BS, D, gen=gen)
            vc[bt[b, :nb].long()] = _bf(nb, HKV, BS // 4, D, 4, gen=gen)
            used += nb
        ctx = torch.tensor(CTX, dtype=torch.int32)
        _poison_tails(kc, vc, bt, ctx)
        c = SimpleNamespace(q=_bf(B, (Hq + 2 * HKV) * D, gen=gen).to(dev), kc=kc.to(dev), vc=vc.to(dev),
                            bt=bt.to(dev), ctx=ctx.to(dev), rope=_rope(D, B, dev, gen) if rope else None)
        c.want = _reference(c, D, Hq)
        return c
    return build


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D,G", SHAPES)
def test_paged_decode_shapes(gpu, D, G, splits, decode_path, rope):
    """Contexts {1, 15, 16, 77, 200}: a single key, a block one short of full, a full block, an odd number of
    blocks (a last pair without a B block), and with 3 splits ranges that start on odd blocks and an empty one."""
    from llm_weighted_consensus_amd import ops

    c = _case(("decode", D, G, rope), build_decode(D, G, rope), gpu)
    out = ops.paged_decode(c.q, c.kc, c.vc, c.bt, c.ctx, HKV * G, 1 / math.sqrt(D), num_splits=splits, rope=c.rope)
    assert out.shape == (len(CTX), HKV * G, D)
    for b in range(len(CTX)):
        _close(out[b], c.want[b], f"paged_decode {decode_path} D={D} G={G} splits={splits} seq {b}")


# ---------------------------------------------------------------------------------------------------------
# 2. cascade, random inputs


def build_cascade(D, G, rope):
    def build(dev):
        from llm_weighted_consensus_amd.engine.engine import cascade_tiles

        gen = torch.Generator().manual_seed(2000 + 10 * D + G)
        Hq, per = HKV * G, rows_per_tile(G)
        # (count, prefix blocks): a group larger than one super-tile, an odd prefix (a last prefix pair without a
        # B block), a singleton, a group with an empty prefix (plain), a short group with an odd prefix, and a
        # prompt of 19 blocks > 16: more than one LDS chunk, the chunked pass
        groups = [(per + 9, 2), (7, 5), (1, 4), (3, 0), (3, 3), (5, 19)]
        B, width = sum(n for n, _ in groups), 24
        bt = torch.zeros(B, width, dtype=torch.int32)
        ctx = torch.zeros(B, dtype=torch.int32)
        nxt, row, runs = 1, 0, []
        for n, pblk in groups:
            shared = torch.arange(nxt, nxt + pblk, dtype=torch.int32)
            nxt += pblk
            for _ in range(n):
                L = pblk * BS + int(torch.randint(1, (width - pblk) * BS, (1,), generator=gen))
                nb = -(-L // BS)
                bt[row, :pblk] = shared
                bt[row, pblk:nb] = torch.arange(nxt, nxt + nb - pblk, dtype=torch.int32)
                nxt += nb - pblk
                ctx[row] = L
                row += 1
            runs.append((row - n, n, pblk))
        NB = nxt + 1
        kc, vc = _bf(NB, HKV, BS, D, gen=gen), _bf(NB, HKV, BS // 4, D, 4, gen=gen)
        kc[0], vc[0], kc[NB - 1], vc[NB - 1] = (float("nan"),) * 4  # blocks no table entry of a context names
        _poison_tails(kc, vc, bt, ctx)
        tiles_np = np.zeros((-(-B // per) + len(groups) + 2, 3), dtype=np.int32)
        nt = cascade_tiles(runs, per, tiles_np)
        assert nt >= len(groups) and (tiles_np[:nt, 1] <= per).all()
        assert any(p > 16 for _, _, p in tiles_np[:nt].tolist())  # the chunked pass runs
        c = SimpleNamespace(q=_bf(B, (Hq + 2 * HKV) * D, gen=gen).to(dev), kc=kc.to(dev), vc=vc.to(dev),
                            bt=bt.to(dev), ctx=ctx.to(dev), tiles=torch.from_numpy(tiles_np).to(dev), B=B,
                            rope=_rope(D, B, dev, gen) if rope else None)
        c.want = torch.stack([w for _, w in sorted(_reference(c, D, Hq).items())])
        return c
    return build


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("D,G", SHAPES)
def test_paged_decode_cascade_shapes(gpu, D, G, rope):
    """The one-launch cascade kernel over groups that span several super-tiles of floor(16 / G) * 8 sequences
    (40 at G = 3, 24 at 5, 16 at 6 and 7: the last 16 mod G MFMA rows of every wave idle), odd prefix block
    counts, plain rows and a 19-block prompt.  head_dim 128: the MX output too, against the bf16 output as
    tests/test_kernels_gpu.py checks it.  head_dim 64: the MX output is refused before any launch."""
    from llm_weighted_consensus_amd import ops

    assert ops.cascade_rows_per_tile(G) == rows_per_tile(G)
    c = _case(("cascade", D, G, rope), build_cascade(D, G, rope), gpu)
    Hq, B, scale = HKV * G, c.B, 1 / math.sqrt(D)
    out = ops.paged_decode_cascade(c.q, c.kc, c.vc, c.bt, c.ctx, c.tiles, Hq, scale, rope=c.rope)
    assert out.shape == (B, Hq, D) and torch.isfinite(out.float()).all()
    _close(out, c.want, f"paged_decode_cascade D={D} G={G}")
    if D != 128:
        with pytest.raises(ValueError, match=f"head_dim {D}"):
            ops.paged_decode_cascade(c.q, c.kc, c.vc, c.bt, c.ctx, c.tiles, Hq, scale, rope=c.rope, mx=True)
        return
    a = ops.paged_decode_cascade(c.q, c.kc, c.vc, c.bt, c.ctx, c.tiles, Hq, scale, rope=c.rope, mx=True)
    assert a.q.shape == (B, Hq * D) and a.mx.shape == (Hq * D // 128, B, 4)
    dims = torch.arange(Hq * D, device=gpu)
    deq = a.q.float() * torch.exp2(a.mx.float() - 127.0)[dims // 128, :, (dims % 128) // 32].t()
    want = out.float().reshape(B, -1)
    assert ((deq - want).norm() / want.norm()).item() < 4e-2
    bmax = a.q.float().abs().view(B, -1, 32).amax(-1)
    assert (bmax[bmax > 0] >= 224).all()


# ---------------------------------------------------------------------------------------------------------
# 3. cascade, short super-tile


@pytest.mark.parametrize("D,G", PROBE_SHAPES)
def test_paged_decode_cascade_short_tile(gpu, D, G):
    """B = per + 1: the last super-tile holds one sequence, so seven of its waves own none and the eighth has
    G real rows (7 of 16 at G = 7).  The waves without a sequence must read no query row past the batch and write
    nothing: q is the first B rows of a larger buffer whose other rows are NaN, and the output rows behind the
    batch keep their NaN fill.  Compared with the reference on the first and last row of the full super-tile
    and on the row of the short one."""
    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.engine.engine import cascade_tiles

    gen = torch.Generator().manual_seed(3000 + D + G)
    Hq, per = HKV * G, ops.cascade_rows_per_tile(G)
    B, pblk, width = per + 1, 3, 6
    NB = pblk + B * (width - pblk) + 2
    bt = torch.zeros(B, width, dtype=torch.int32)
    ctx = torch.zeros(B, dtype=torch.int32)
    nxt = pblk
    for b in range(B):
        L = pblk * BS + 5 + b % 30
        nb = -(-L // BS)
        bt[b, :pblk] = torch.arange(pblk, dtype=torch.int32)
        bt[b, pblk:nb] = torch.arange(nxt, nxt + nb - pblk, dtype=torch.int32)
        nxt += nb - pblk
        ctx[b] = L
    kc, vc = _bf(NB, HKV, BS, D, gen=gen), _bf(NB, HKV, BS // 4, D, 4, gen=gen)
    _poison_tails(kc, vc, bt, ctx)
    tiles_np = np.zeros((-(-B // per) + 3, 3), dtype=np.int32)
    cascade_tiles([(0, B, pblk)], per, tiles_np)
    assert tiles_np[1].tolist() == [per, 1, pblk]  # the short last super-tile: one sequence, seven idle waves
    stride = (Hq + 2 * HKV) * D
    buf = torch.full((B + 2 * per, stride), float("nan"), dtype=torch.bfloat16)
    buf[:B] = _bf(B, stride, gen=gen)
    buf = buf.to(gpu)
    c = SimpleNamespace(q=buf[:B], kc=kc.to(gpu), vc=vc.to(gpu), bt=bt.to(gpu), ctx=ctx.to(gpu), rope=None)
    obuf = torch.full((B + per, Hq, D), float("nan"), dtype=torch.bfloat16, device=gpu)
    out = ops.paged_decode_cascade(c.q, c.kc, c.vc, c.bt, c.ctx, torch.from_numpy(tiles_np).to(gpu), Hq,
                                   1 / math.sqrt(D), out=obuf[:B])
    assert torch.isfinite(out.float()).all() and torch.isnan(obuf[B:].float()).all()
    for b, want in _reference(c, D, Hq, rows=(0, per - 1, per)).items():
        _close(out[b], want, f"short tile D={D} G={G} seq {b}")


# ---------------------------------------------------------------------------------------------------------
# 4. structured probes (tests/attn_probes.py)


def _nan_cache(NB, D):
    nan = float("nan")
    return (torch.full((NB, HKV, BS, D), nan, dtype=torch.bfloat16),
            [torch.full((NB, HKV, BS // 4, D, 4), nan, dtype=torch.bfloat16) for _ in range(2)])


def _store(kc, vcs, blocks, t0, k, vs):
    """Write keys k [n, Hkv, D] and each values tensor of vs at key positions t0.. of a sequence whose logical
    blocks are ``blocks`` (physical ids): K token-major, V 4-token interleaved."""
    t = torch.arange(t0, t0 + k.shape[0])
    blk, off = torch.as_tensor(blocks, dtype=torch.long)[t // BS], t % BS
    kc[blk, :, off, :] = k
    for vc, v in zip(vcs, vs):
        vc[blk, :, off // 4, :, off % 4] = v


def _paged_ref(q, kc, vc, bt_row, L, scale):
    from llm_weighted_consensus_amd import ops

    toks = torch.arange(L, device=kc.device)
    blk = bt_row[toks // BS].long()
    return ref.attention(q, kc[blk, :, toks % BS, :], ops.v_gather(vc, blk, toks % BS), False, scale)


def _row_conditions(prog, s, orders, scale, stats):
    """Preconditions of one row from the reference's own scores s [L]: a visible spike holds >= 0.999 of the
    weight; a staircase forces the rescale branch, on a non-empty accumulator, at every tile boundary its slope
    promises, for each processing order in ``orders``."""
    if prog.kind == "spike" and 0 <= prog.at < s.numel():
        assert ap.key_weight(s, prog.at) >= 0.999, prog
        stats["spikes"] += 1
    if prog.kind == "stair":
        for name, tiles in orders:
            n = ap.forced_rescales(s, tiles)
            assert n == ap.stair_rises(tiles, scale, prog.slope), (prog, tiles)
            stats[name] = stats.get(name, 0) + n


def _check(out, want, out_i, want_i, flat, what):
    """All rows at the suite's bound (V ~ N(0, 1)); flat rows of the integer-V run at one bf16 rounding."""
    assert flat.any() and not flat.all()
    ap.assert_close(out.float(), want, ap.ATOL, ap.RTOL, what)
    ap.assert_close(out_i.float()[flat], want_i[flat], 0.0, ap.FLAT_RTOL, what + " (flat rows, integer V)")


# 449 = 29 blocks: with 3 splits a wave of the 4-wave kernel still gets two pairs (pairs 0 and 4 of 5)
PROBE_CTX = [1, 16, 17, 33, 200, 449]


def build_decode_probes(D, G, splits):
    def build(dev):
        gen = torch.Generator().manual_seed(100 * G + splits + D)
        Hq, scale, dims = HKV * G, 1 / math.sqrt(D), ap.probe_dims(D)
        seqs = []
        for L in PROBE_CTX:  # enough sequences per context for every programme to appear
            progs = ap.decode_programmes(L, splits)
            seqs += [(L, rep, progs) for rep in range(-(-len(progs) // Hq))]
        B, width = len(seqs), -(-max(PROBE_CTX) // BS) + 1
        NB = 1 + sum(-(-L // BS) for L, _, _ in seqs)  # block 0 stays NaN: padding table entries point at it
        kc, (vc, vci) = _nan_cache(NB, D)
        perm = 1 + torch.randperm(NB - 1, generator=gen)
        bt = torch.zeros(B, width, dtype=torch.int32)
        q = torch.randn(B, (Hq + 2 * HKV) * D, generator=gen)
        q[:, : Hq * D] = 0
        flat = torch.zeros(B, Hq, dtype=torch.bool)
        stats, used = {"spikes": 0}, 0
        for b, (L, rep, progs) in enumerate(seqs):
            nb = -(-L // BS)
            bt[b, :nb] = perm[used:used + nb].to(torch.int32)
            used += nb
            k = torch.randn(L, HKV, D, generator=gen)
            t = torch.arange(L)
            rows = []
            for kvh in range(HKV):
                wave, cols = [], []
                for h in range(G):
                    pi = ((rep * HKV + kvh) * G + h) % len(progs)
                    col = dims[(7 * h + 3 * kvh + b) % D]
                    k[:, kvh, col] = ap.k_column(progs[pi], t, scale, gen)
                    q[b, (kvh * G + h) * D + col] = ap.AMP
                    flat[b, kvh * G + h] = progs[pi].kind == "flat"
                    rows.append((kvh, h, progs[pi]))
                    wave.append(pi)
                    cols.append(col)
                assert len(set(cols)) == G  # the rows of one wave: a K column each ...
                assert len(set(wave)) == min(G, len(progs))  # ... and different programmes
            k = k.to(torch.bfloat16)
            v = torch.randn(L, HKV, D, generator=gen).to(torch.bfloat16)
            vi = ap.nonzero_prefix_sums(ap.int_values((L, HKV, D), gen))
            _store(kc, (vc, vci), bt[b, :nb].tolist(), 0, k, (v, vi))
            qb = q[b, : Hq * D].view(Hq, D).to(torch.bfloat16)
            orders = [(path + str(i), st) for path in ("wg4", "wave")
                      for i, st in enumerate(ap.decode_tiles(L, splits, path))]
            for kvh, h, prog in rows:
                s = ap.scores_nats(qb[kvh * G + h][None], k[:, kvh], scale)[0]
                _row_conditions(prog, s, orders, scale, stats)
        c = SimpleNamespace(Hq=Hq, scale=scale, flat=flat.to(dev), stats=stats, q=q.to(torch.bfloat16).to(dev),
                            kc=kc.to(dev), vc=vc.to(dev), vci=vci.to(dev), bt=bt.to(dev),
                            ctx=torch.tensor([L for L, _, _ in seqs], dtype=torch.int32, device=dev))
        qh = c.q[:, : Hq * D].view(B, 1, Hq, D)
        c.want = torch.cat([_paged_ref(qh[b], c.kc, c.vc, c.bt[b], L, scale) for b, (L, _, _) in enumerate(seqs)])
        c.want_i = torch.cat([_paged_ref(qh[b], c.kc, c.vci, c.bt[b], L, scale) for b, (L, _, _) in enumerate(seqs)])
        return c
    return build


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D,G", PROBE_SHAPES)
def test_paged_decode_shape_probes(gpu, D, G, splits, decode_path):
    """tests/test_attention_probes_gpu.py test_paged_decode_probes at (64, 4) and (128, 7): staircases that
    rescale a live accumulator at every pair of every wave / split (0.5 nats per key at head_dim 64), spikes on
    the block, pair, context and split edges, flat rows (exact means of integer V) and background rows, mixed
    among the G rows of a wave.  At G = 7 the staircase of one head must leave its six neighbours and the nine
    idle MFMA rows alone; at head_dim 64 a key read from the wrong half of a 256 B line would move a spike."""
    from llm_weighted_consensus_amd import ops

    c = _case(("decode-probes", D, G, splits), build_decode_probes(D, G, splits), gpu)
    assert sum(n for name, n in c.stats.items() if name.startswith(decode_path)) > 0 and c.stats["spikes"] > 0
    out = ops.paged_decode(c.q, c.kc, c.vc, c.bt, c.ctx, c.Hq, c.scale, num_splits=splits)
    out_i = ops.paged_decode(c.q, c.kc, c.vci, c.bt, c.ctx, c.Hq, c.scale, num_splits=splits)
    _check(out, c.want, out_i, c.want_i, c.flat, f"paged_decode {decode_path} D={D} G={G} splits={splits}")


SUFFIX = [1, 15, 16, 17, 33]


def build_cascade_probes(D, G):
    def build(dev):
        from llm_weighted_consensus_amd.engine.engine import cascade_tiles

        gen = torch.Generator().manual_seed(40 + G + D)
        Hq, scale, dims = HKV * G, 1 / math.sqrt(D), ap.probe_dims(D)
        per, spw = rows_per_tile(G), 16 // G
        # Sequence sg of a group takes the G consecutive K columns from (G + 1) sg, modulo M: the spw sequences of
        # a wave span spw (G + 1) <= M columns, so the rows of one wave have a column each, while rows of
        # different waves may share one (a super-tile at (64, 4) has 128 rows per KV head and 64 columns) and then
        # share its prefix programme.  Column c runs programme (c + kvh) mod 7 or 9 (cascade_programmes), and M is
        # a multiple of both, so that also holds where the columns wrap; the stride G + 1 (not G) is a unit modulo
        # 7 and 9 for G = 4 and 7, which keeps the sequences of a wave on different programme tuples.
        M = 63 * (D // 64)
        column = lambda sg, h: ((G + 1) * sg + h) % M  # noqa: E731
        assert spw * (G + 1) <= M <= D
        # (count, prefix blocks): larger than a super-tile; an odd prefix (last prefix pair without a B block);
        # plain rows; a prefix of more than one 16-block LDS chunk (chunk edge between keys 255 and 256)
        groups = [(per + 9, 2), (7, 5), (3, 0), (5, 19)]
        B = sum(n for n, _ in groups)
        width = 24
        NB = 1 + sum(p + n * 3 for n, p in groups)
        kc, (vc, vci) = _nan_cache(NB, D)
        bt = torch.zeros(B, width, dtype=torch.int32)
        ctx = torch.zeros(B, dtype=torch.int32)
        q = torch.randn(B, (Hq + 2 * HKV) * D, generator=gen)
        q[:, : Hq * D] = 0
        flat = torch.zeros(B, Hq, dtype=torch.bool)
        nxt, b, runs, keys, rowprog, rowcol = 1, 0, [], {}, {}, {}
        for gi, (count, pblk) in enumerate(groups):
            progs = ap.cascade_programmes(pblk)
            assert len(progs) % 2 == 1
            pctx = pblk * BS
            shared = list(range(nxt, nxt + pblk))
            nxt += pblk
            kp = torch.randn(pctx, HKV, D, generator=gen)
            for kvh in range(HKV):  # the shared part of all D column programmes
                for ci in range(D if pblk else 0):
                    p = progs[(ci + kvh) % len(progs)]
                    p = p(1 << 30) if callable(p) else p
                    kp[:, kvh, dims[ci]] = ap.k_column(p, torch.arange(pctx), scale, gen)
            kp = kp.to(torch.bfloat16)
            vp = torch.randn(pctx, HKV, D, generator=gen).to(torch.bfloat16)
            vpi = ap.nonzero_prefix_sums(ap.int_values((pctx, HKV, D), gen))
            if pblk:
                _store(kc, (vc, vci), shared, 0, kp, (vp, vpi))
            for sg in range(count):
                L = pctx + SUFFIX[(sg + gi) % len(SUFFIX)]
                nb = -(-L // BS)
                blocks = shared + list(range(nxt, nxt + nb - pblk))
                nxt += nb - pblk
                bt[b, :nb] = torch.tensor(blocks, dtype=torch.int32)
                ctx[b] = L
                ko = torch.randn(L - pctx, HKV, D, generator=gen)
                for kvh in range(HKV):
                    for h in range(G):
                        ci = column(sg, h)
                        pi = (ci + kvh) % len(progs)
                        p = progs[pi](L) if callable(progs[pi]) else progs[pi]
                        ko[:, kvh, dims[ci]] = ap.k_column(p, torch.arange(pctx, L), scale, gen)
                        q[b, (kvh * G + h) * D + dims[ci]] = ap.AMP
                        flat[b, kvh * G + h] = p.kind == "flat"
                        rowprog[b, kvh, h] = (pi, p)
                        rowcol[b, kvh, h] = ci
                ko = ko.to(torch.bfloat16)
                vo = torch.randn(L - pctx, HKV, D, generator=gen).to(torch.bfloat16)
                voi = ap.nonzero_prefix_sums(ap.int_values((L - pctx, HKV, D), gen), vpi.float().sum(0))
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
                for kvh in range(HKV):
                    cols = [rowcol[i, kvh, h] for i in wave for h in range(G)]
                    assert len(set(cols)) == len(cols)  # one wave's rows of a KV head: a K column each
                    mine = [tuple(rowprog[i, kvh, h][0] for h in range(G)) for i in wave]
                    assert len(set(mine)) == min(len(wave), len(ap.cascade_programmes(pb)))
                    for j, i in enumerate(wave):
                        order = ap.cascade_row_tiles(pb, ctxs, j)
                        for h in range(G):
                            s = ap.scores_nats(qb[i, (kvh * G + h) * D:][None, :D], keys[i][:, kvh], scale)[0]
                            _row_conditions(rowprog[i, kvh, h][1], s, [(name, order)], scale, stats)
        c = SimpleNamespace(Hq=Hq, scale=scale, flat=flat.to(dev), stats=stats, q=qb.to(dev), kc=kc.to(dev),
                            vc=vc.to(dev), vci=vci.to(dev), bt=bt.to(dev), ctx=ctx.to(dev),
                            tiles=torch.from_numpy(tiles_np).to(dev))
        qh = c.q[:, : Hq * D].view(B, 1, Hq, D)
        c.want = torch.cat([_paged_ref(qh[i], c.kc, c.vc, c.bt[i], int(ctx[i]), scale) for i in range(B)])
        c.want_i = torch.cat([_paged_ref(qh[i], c.kc, c.vci, c.bt[i], int(ctx[i]), scale) for i in range(B)])
        return c
    return build


@pytest.mark.parametrize("D,G", PROBE_SHAPES)
def test_paged_decode_cascade_shape_probes(gpu, D, G):
    """tests/test_attention_probes_gpu.py test_paged_decode_cascade_probes at (64, 4) and (128, 7).  Rows differ
    INSIDE the shared prefix (a K column each within a wave), so the swizzled LDS image of the prefix is read at
    every (row, 16 B chunk) with a different expected score: a chunk fetched from the wrong place moves a spike
    or a staircase.  At G = 7 a wave carries two sequences on rows 0-6 and 7-13; while one sequence's suffix is
    walked (row_on) and its staircase rescales, the other's rows and rows 14-15 must not move."""
    from llm_weighted_consensus_amd import ops

    c = _case(("cascade-probes", D, G), build_cascade_probes(D, G), gpu)
    assert c.stats["chunked"] > 0 and c.stats["interleaved"] > 0 and c.stats["spikes"] > 0
    out = ops.paged_decode_cascade(c.q, c.kc, c.vc, c.bt, c.ctx, c.tiles, c.Hq, c.scale)
    out_i = ops.paged_decode_cascade(c.q, c.kc, c.vci, c.bt, c.ctx, c.tiles, c.Hq, c.scale)
    _check(out, c.want, out_i, c.want_i, c.flat, f"paged_decode_cascade D={D} G={G}")


# ---------------------------------------------------------------------------------------------------------
# 5. refusals


@pytest.mark.parametrize("D,G,msg", [(96, 4, "head_dim 96"), (128, 32, "64 heads / 2 kv heads")])
def test_unserved_shapes_are_refused_with_the_shape_named(gpu, D, G, msg):
    from llm_weighted_consensus_amd import ops

    Hq, B = HKV * G, 2
    kc = torch.zeros(4, HKV, BS, D, dtype=torch.bfloat16, device=gpu)
    vc = torch.zeros(4, HKV, BS // 4, D, 4, dtype=torch.bfloat16, device=gpu)
    q = torch.zeros(B, (Hq + 2 * HKV) * D, dtype=torch.bfloat16, device=gpu)
    bt = torch.zeros(B, 2, dtype=torch.int32, device=gpu)
    ctx = torch.ones(B, dtype=torch.int32, device=gpu)
    tiles = torch.tensor([[0, B, 0]], dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match=msg):
        ops.paged_decode(q, kc, vc, bt, ctx, Hq, 1.0)
    with pytest.raises(ValueError, match=msg):
        ops.paged_decode_cascade(q, kc, vc, bt, ctx, tiles, Hq, 1.0)
    # the extension's own entry points refuse them too (no launch): callers that bypass ops
    out = torch.zeros(B, Hq, D, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(RuntimeError, match=msg):
        ops.kernels().paged_decode(q, kc, vc, bt, ctx, out, None, None, 1, 1.0, None, None, None)
    with pytest.raises(RuntimeError, match=msg):
        ops.kernels().paged_decode_cascade(q, kc, vc, bt, ctx, tiles, out, Hq, 1.0, None, None, None, None, None)
    assert not bool(out.any())


# ---------------------------------------------------------------------------------------------------------
# 6. graph capture


def test_cascade_head_dim_64_in_a_captured_graph(gpu):
    """One captured and replayed paged_decode_cascade call at (64, 4), its tile table padded with nseq = 0 entries
    as the engine pads a bucket's, equals the eager call bit for bit."""
    from llm_weighted_consensus_amd import ops

    D, G = 64, 4
    c = _case(("cascade", D, G, True), build_cascade(D, G, True), gpu)
    Hq, scale = HKV * G, 1 / math.sqrt(D)
    tiles = torch.cat([c.tiles, torch.zeros(5, 3, dtype=torch.int32, device=gpu)])
    assert int((tiles[:, 1] == 0).sum()) >= 5
    want = ops.paged_decode_cascade(c.q, c.kc, c.vc, c.bt, c.ctx, c.tiles, Hq, scale, rope=c.rope)
    out = torch.zeros_like(want)

    def run():
        ops.paged_decode_cascade(c.q, c.kc, c.vc, c.bt, c.ctx, tiles, Hq, scale, out=out, rope=c.rope)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert bool(out.any()) and torch.equal(out.view(torch.int16), want.view(torch.int16))
