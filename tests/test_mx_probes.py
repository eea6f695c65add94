"""What the comparisons of tests/test_mx_probes_gpu.py accept and reject, shown on the CPU.  The host quantiser
gives the documented bytes, the plane helpers invert each other, the element bound holds, the premises of the
exact cascade rows and of the saturated-gate SwiGLU family hold, and each wrong reference is rejected by the
named probe family:

  writer    threshold >= instead of >                 edge: maxima 7 and 448 (mantissa exactly 0.875)
            no bump (the maximum saturates)           edge: maxima 7.5 and 480; random
            e4m3 conversion towards zero              edge: the ties and roundings of SCALED; random
            amax over 8 / 16 values                   edge: the maximum in lanes 31, 12, 20, 27 (8) / 31, 20, 27 (16)
            scale stored at block 3 - b               edge rows (column blocks of different classes); random
            plane laid out [rows, P, 4]               edge rows; random
            row r takes the scale of row r + 1        random rows times 2^(r % 5)
            plane row qr instead of s0 + qr           prefill: any batch of more than one sequence
            a row stored past the end                 the cages (every family)
  consumer  scale of block b ^ 1                      walk (one live block per slice, dead bytes all different)
            scale of row r ^ 16                       walk and shared (bytes differ between rows)"""
import math

import pytest
import torch

from tests import attn_probes as ap
from tests import gemm_probes as gp
from tests import mx_probes as mp


def _random(rows, cols, seed=0, stairs=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    if stairs:
        x = x * torch.exp2((torch.arange(rows) % 5).float())[:, None]
    return x.to(torch.bfloat16).float()


def _cages(rows, cols):
    return mp.ByteCage(rows, cols), mp.PlaneCage(cols // 128, rows)


def _accepts(x, **mut):
    rows, cols = x.shape
    qc, pc = _cages(rows, cols)
    mp.write(qc, pc, x, **mut)
    wq, ws = mp.mx_quant_ref(x)
    return mp.violations(qc, pc, wq, ws)


def test_quantiser_bytes_of_the_documented_maxima():
    x = torch.zeros(5, 32)
    x[1, 0], x[2, 31], x[3, 5], x[4, 9] = 7.0, -7.5, 2.0 ** -126, 2.0 ** -120
    q, sc = mp.mx_quant_ref(x)
    assert sc[:, 0].tolist() == [118, 121, 122, 0, 0]
    qv = mp.q_values(q)
    assert [float(qv[1, 0]), float(qv[2, 31]), float(qv[3, 5]), float(qv[4, 9])] == [448.0, -240.0, 2.0, 128.0]
    assert not torch.isnan(qv).any()
    # fp32's largest value: byte 247, the upper clamp is out of reach
    assert int(mp.mx_quant_ref(torch.full((1, 32), 3.4028234e38))[1]) == 247


def test_every_live_block_peaks_in_the_top_binade_and_a_half():
    names, table = mp.edge_table()
    for x in (table, _random(64, 256), _random(64, 256, 1) * 1e-30, _random(64, 256, 2) * 1e30):
        q, sc = mp.mx_quant_ref(x)
        peak = mp.q_values(q).abs().view(x.shape[0], -1, 32).amax(-1)
        live = x.view(x.shape[0], -1, 32).abs().amax(-1) > 0
        tight = live & (sc > 0)    # byte 0 is the lower clamp: the block's values are too small for any scale
        assert bool(((peak[tight] >= 224) & (peak[tight] <= 448)).all())
        assert bool((sc[~live] == mp.ZERO_BYTE).all())
        assert not torch.isnan(mp.q_values(q)).any()


def test_the_cast_is_the_format_written_out():
    """torch's float -> float8_e4m3fn cast equals round-to-nearest-even written from the format, on every scaled
    edge value, on both sides of every tie, and on random data."""
    t = torch.tensor(mp.SCALED + (448.0, 240.0, 256.0, 0.0146484375))
    g = torch.Generator().manual_seed(3)
    x = torch.cat([t, -t, torch.rand(4096, generator=g) * 448, torch.rand(4096, generator=g) * 0.03])
    for v in (x, torch.nextafter(x, torch.zeros(())), torch.nextafter(x, torch.full((), 1e9))):
        assert torch.equal(v.to(mp.E4M3).float().double(), mp.e4m3_rne(v))
    want = {432.0: 448.0, 400.0: 384.0, 8.5: 8.0, 9.5: 10.0, 1.0625: 1.0, 101.0: 104.0, 99.0: 96.0,
            3 * 2.0 ** -10: 2.0 ** -8, 5 * 2.0 ** -10: 2.0 ** -8, 2.0 ** -10: 0.0, 7.5 * 2.0 ** -9: 2.0 ** -6}
    for a, b in want.items():
        assert float(torch.tensor(a).to(mp.E4M3).float()) == b, a


def test_edge_table_covers_the_issue():
    names, table = mp.edge_table()
    assert {n for n, _ in names} == {n for n, _ in mp.CLASSES}
    q, sc = mp.mx_quant_ref(table)
    by = {n: int(s) for (n, _), s in zip(names, sc[:, 0])}
    assert by == {"zero": 118, "m7": 121, "m7.5": 122, "m8": 122, "m448": 127, "m480": 128, "tiny": 0, "clamp": 0,
                  "large": 219}
    for (n, pos), row in zip(names, table):
        if n != "zero":
            assert int(row.abs().argmax()) == pos and (row.abs() == row.abs().max()).sum() == 1
    assert {pos for _, pos in names} == set(mp.POSITIONS) and {p // 8 for p in mp.POSITIONS} == {0, 1, 2, 3}
    assert bool((table > 0).any()) and bool((table < 0).any())
    # the rows meet ties, the subnormal range and both signs after scaling
    scaled = torch.ldexp(table.double(), -(sc.int() - 127))
    assert 432.0 in scaled and -432.0 in scaled and 2.0 ** -9 in scaled.abs() and 3 * 2.0 ** -10 in scaled.abs()
    assert mp.missing_edge_blocks(q, sc, names, table) == []
    assert mp.missing_edge_blocks(q[1:], sc[1:], names, table) == [names[0]]


def test_plane_round_trip():
    g = torch.Generator().manual_seed(0)
    sc = torch.randint(0, 255, (37, 32), dtype=torch.uint8, generator=g)
    assert torch.equal(mp.from_plane(mp.to_plane(sc)), sc)
    assert torch.equal(mp.from_plane(mp.head_plane(sc, 8, s_rows=44), 37), sc)
    pl = mp.slice_plane(sc, 1024, s_rows=40)
    assert pl.shape == (8, 40, 4) and bool((pl[:, 37:] == mp.PLANE_SENTINEL).all())
    # block b of slice s of row r sits at [s, r, b]
    assert int(pl[3, 5, 2]) == int(sc[5, 3 * 4 + 2])
    plane = torch.randint(0, 255, (8, 37, 4), dtype=torch.uint8, generator=g)
    assert torch.equal(mp.to_plane(mp.from_plane(plane)), plane)


@pytest.mark.parametrize("scale", [1.0, 1e-20, 1e20, 2.0 ** -120])
def test_element_bound_holds(scale):
    x = _random(128, 512, 5) * scale
    q, sc = mp.mx_quant_ref(x)
    err = (mp.dequant(q, sc) - x.double()).abs()
    assert bool((err <= mp.element_bound(x, sc.int() - 127)).all())
    names, table = mp.edge_table()
    q, sc = mp.mx_quant_ref(table)
    assert bool(((mp.dequant(q, sc) - table.double()).abs() <= mp.element_bound(table, sc.int() - 127)).all())


# ---------------------------------------------------------------------------------------------------------
# wrong writers


def _edge():
    return mp.edge_rows(36, 16)


@pytest.mark.parametrize("mutant,families", [
    (dict(threshold="ge"), ["edge"]),
    (dict(bump=False), ["edge", "random"]),
    (dict(trunc=True), ["edge", "random"]),
    (dict(span=8), ["edge", "random"]),
    (dict(span=16), ["edge", "random"]),
    (dict(flip_blocks=True), ["edge", "random"]),
    (dict(transposed=True), ["edge", "random"]),
    (dict(neighbour_row=True), ["stairs"]),
    (dict(past_rows=1), ["edge", "random"]),
])
def test_wrong_writers_are_rejected(mutant, families):
    data = {"edge": _edge(), "random": _random(36, 512), "stairs": _random(36, 512, 7, stairs=True)}
    for f in families:
        assert _accepts(data[f]) == []
        assert _accepts(data[f], **mutant), (mutant, f)


def test_named_edge_blocks_catch_the_quantiser_mutants():
    names, table = mp.edge_table()
    q, sc = mp.mx_quant_ref(table)

    def caught(**mut):
        q2, s2 = mp.mx_quant_ref(table, **mut)
        return {n for n, a, b, c, d in zip(names, q, q2, sc, s2) if not (torch.equal(a, b) and torch.equal(c, d))}

    assert {n for n, _ in caught(threshold="ge")} == {"m7", "m448"}
    assert {n for n, _ in caught(bump=False)} == {"m7.5", "m480"}
    assert {n for n, _ in caught(trunc=True)} >= {"m7", "m7.5", "m8", "m448", "m480", "large"}
    # maxima 7 and 448 scale to 448, in one binade with the 432 and 400 of the other lanes: a partial amax shows
    # there only when it misses those too; the other classes show it at every position it leaves out
    sure = ("m7.5", "m8", "m480", "large", "tiny")
    assert caught(span=8) >= {(n, p) for n, p in names if n in sure and p >= 8}
    assert caught(span=16) >= {(n, p) for n, p in names if n in sure and p >= 16}
    assert {n for n, _ in caught(span=8)} >= {"m7", "m448"}


def test_sequence_local_plane_rows_are_rejected():
    """A prefill batch of two sequences: the second one's rows stored at plane rows qr instead of s0 + qr."""
    x = _random(20, 512, 9, stairs=True)
    qc, pc = _cages(20, 512)
    mp.write(qc, pc, x[:7])
    mp.write(qc, pc, x[7:], row0=7, plane_row0=0)
    wq, ws = mp.mx_quant_ref(x)
    v = mp.violations(qc, pc, wq, ws)
    assert v and "scale bytes differ" in v[0]
    qc, pc = _cages(20, 512)
    mp.write(qc, pc, x[:7])
    mp.write(qc, pc, x[7:], row0=7)
    assert mp.violations(qc, pc, wq, ws) == []


def test_check_names_the_first_difference_and_the_sentinels():
    x = _edge()
    qc, pc = _cages(36, 512)
    mp.write(qc, pc, x)
    wq, ws = mp.mx_quant_ref(x)
    qc.view[5, 77] ^= 1
    pc.buf[2, 9, 3] += 1
    qc.buf[36, 3] = 0
    qc.buf[4, 512] = 0
    pc.buf[1, 36, 0] = 0
    v = " ".join(mp.violations(qc, pc, wq, ws))
    assert "row 5 column 77" in v and "row 9 block 11 (plane 2)" in v and "(4, 512)" in v and "(36, 3)" in v
    assert "(1, 36, 0)" in v


# ---------------------------------------------------------------------------------------------------------
# consumer


@pytest.mark.parametrize("all_live", [False, True])
@pytest.mark.parametrize("K", [128, 1024])
def test_consumer_families(K, all_live):
    g = torch.Generator().manual_seed(K)
    rows, N = 300, 264
    A, sc = mp.scale_walk(rows, K, g, all_live)
    _, W, _, w_s = gp.fp8_operands(8, N, K, g)
    assert mp.exact_in_fp32(A, sc) and 110 <= int(sc.min()) and int(sc.max()) <= 144
    live = A.float().view(rows, K // 128, 4, 32).abs().amax(-1) > 0
    assert bool((live.sum(-1) == (4 if all_live else 1)).all())
    blocks = sc.view(rows, K // 128, 4)
    if all_live:
        assert bool((blocks == blocks[..., :1]).all())
        assert int(blocks[:, :, 0].int().amax(1).sub(blocks[:, :, 0].int().amin(1)).max()) <= 10
    else:
        # the four bytes of a slice differ, and so do rows r and r ^ 16, r + 1
        assert all(len(set(b.tolist())) == 4 for b in blocks.reshape(-1, 4))
    want = gp.rne(mp.mx_product(A, sc, W, w_s))
    bad_row = gp.rne(mp.mx_product(A, sc, W, w_s, row_xor=16))
    assert float(gp.bitwise(bad_row, want).float().mean()) > 0.5
    bad_blk = gp.rne(mp.mx_product(A, sc, W, w_s, block_xor=1))
    if all_live:
        assert not bool(gp.bitwise(bad_blk, want).any())   # blocks share a byte: this family cannot see it
    else:
        assert float(gp.bitwise(bad_blk, want).float().mean()) > 0.5
    # the exact product is a bf16-representable sum in fp32: fp32 accumulation in slice order reproduces it
    a = A.float() * torch.exp2(sc.float() - 127.0).repeat_interleave(32, dim=1)
    acc = torch.zeros(rows, N)
    for s in range(K // 128):
        acc = acc + a[:, 128 * s:128 * s + 128] @ W.float()[:, 128 * s:128 * s + 128].t()
    assert torch.equal((acc * w_s[None, :]).double(), mp.mx_product(A, sc, W, w_s))


# ---------------------------------------------------------------------------------------------------------
# premises


def test_saturated_gate_operands_give_the_edge_table():
    rows, F, K = 13, 256, 256
    for shift in (0, 3):
        A, W, w_s, x = mp.saturated_gate_operands(rows, F, K, shift)
        acc = A.float() @ W.t()                                  # fp32: every product and sum exact
        y = acc * w_s[None, :]
        assert torch.equal(y[:, :F], torch.full((rows, F), 64.0))
        silu = y[:, :F] * (1.0 / (1.0 + torch.exp(-y[:, :F])))   # the kernel's form, in fp32
        assert torch.equal(silu, y[:, :F])
        act = silu * y[:, F:]
        assert torch.equal(act, x) and torch.equal(x.to(torch.bfloat16).float(), x)
        assert bool((y[:, F:][y[:, F:] != 0].abs() >= 2.0 ** -126).all()) and bool((w_s >= 2.0 ** -126).all())
    names, table = mp.edge_table(mp.SATURATED_MIN)
    q, sc = mp.mx_quant_ref(mp.edge_rows(rows, F // 32, mp.SATURATED_MIN))
    assert mp.missing_edge_blocks(q, sc, names, table) == [] and len({n for n, _ in names}) == 8


def test_spike_rows_are_exact_under_the_kernels_recurrence():
    """A spike row over integer V returns V[at] with l == 1.0 under the tiled fp32 recurrence (30 nats, the
    longest context of the GPU test), whatever tile the spike sits in; a 271-nat spike (K = 192 in the one-hot
    column) leaves no other key any weight at all, so V may mix magnitudes: the row is V[at] over the edge table."""
    g = torch.Generator().manual_seed(1)
    L, scale = 400, 1 / math.sqrt(128)
    vi = ap.int_values((L, 128), g)
    names, table = mp.edge_table()
    ve = table[(7 * torch.arange(L)[:, None] + torch.arange(4)[None, :]) % len(names)].reshape(L, 128).bfloat16()
    nat = 1.0 / (ap.AMP * scale)
    for at in (0, 31, 32, 255, 256, 399):
        s = torch.randn(3, L, generator=g)
        s[1, at] = ap.SPIKE_NATS
        s[2, at] = mp.TALL_K / nat
        o, l = ap.emulate(s, vi, state=True)
        assert float(l[1]) == 1.0 and torch.equal(o[1], vi[at].float())
        assert not torch.equal(o[0], vi[at].float())
        o, l = ap.emulate(s, ve, state=True)
        assert float(l[2]) == 1.0 and torch.equal(o[2], ve[at].float())
        q, sc = mp.mx_quant_ref(o[2][None])
        wq, ws = mp.mx_quant_ref(ve[at].float()[None])
        assert torch.equal(q, wq) and torch.equal(sc, ws)


def test_bounded_rule_accepts_an_fp32_quantiser_and_rejects_a_wrong_row():
    """The cascade rule: bytes quantised from fp32 values are accepted against their bf16 rounding, with a few per
    cent of the blocks exempt; a scale taken from the neighbouring row, or truncation, is not."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(300, 1024, generator=g) * torch.exp2((torch.arange(300) % 5).float())[:, None]
    out = x.to(torch.bfloat16).float()
    q, sc = mp.mx_quant_ref(x)
    v, share = mp.bounded_violations(q, sc, out)
    assert v == [] and 0 < share <= 0.05, (v, share)
    assert mp.bounded_violations(q, torch.cat([sc[1:], sc[-1:]]), out)[0]
    assert mp.bounded_violations(*mp.mx_quant_ref(x, bump=False), out)[0]
    assert mp.bounded_violations(*mp.mx_quant_ref(x, span=8), out)[0]


def test_flat_rows_of_power_of_two_contexts_are_exact():
    g = torch.Generator().manual_seed(2)
    for L in (1, 16, 64, 128, 512):
        v = ap.int_values((L, 128), g)
        o, l = ap.emulate(torch.zeros(1, L), v, state=True)
        assert float(l[0]) == L and torch.equal(o[0].double(), v.double().mean(0))
