"""What the comparisons of tests/test_mxw_probes_gpu.py accept and reject, shown on the CPU.  The reference of
tests/mxw_probes.py equals the host function on all 16 x 255 (code, byte) pairs, the premises of the bitwise dense
claim hold at every shape the GPU tests launch, and each wrong reader is rejected by the named family while the
reader written from the kernels passes all of them:

  range     nibbles swapped; the scale of block b ^ 1; byte 0 read as the float 0.0 (``s << 23``); bf16 subnormal
            results flushed; overflow saturated to the largest finite bf16; code 8 stored as +0
  dense     a wave's odd last batch added twice / left out; the second K tile computed from the first's registers;
            one k contribution dropped; a wave's partial rounded to bf16 before the cross-wave sum
  segments  a row of a 33-row segment stored one m-tile further; a segment read with the next expert's weights; the
            gather index taken as the identity
  swiglu    gate and up swapped; the up tile 16 columns off; silu as a ratio that is inf / inf at a saturated
            negative gate"""
import pytest
import torch

from llm_weighted_consensus_amd.ops import mxfp4 as host
from tests import gemm_probes as gp
from tests import mxw_probes as wp


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------
# the reference and the format


def test_reference_is_the_host_function_on_all_4080_pairs():
    q, s = wp.pair_weight()
    assert q.shape == (255, 16) and int(s.max()) == 254
    host.check_mxfp4(q, s)
    law = host.dequant_mxfp4(q, s)
    mine = gp.rne(wp.values(wp.unpack(q), s))
    assert law.shape == (255, 32) and torch.equal(gp.bits(law), gp.bits(mine))
    assert torch.equal(gp.bits(mine[:, :16]), gp.bits(mine[:, 16:]))
    assert torch.equal(wp.pack(wp.unpack(q)), q)


def test_which_pairs_are_subnormal_negative_zero_or_not_finite():
    v = gp.rne(wp.pair_values())
    # byte 0 with codes 1 and 2: the bf16 subnormals 2^-128 and 2^-127; code 8 is -0 under every byte
    assert (int(gp.bits(v)[0, 1]), int(gp.bits(v)[0, 2])) == (0x0020, 0x0040)
    assert bool((gp.bits(v)[:, 8] == -0x8000).all()) and bool((gp.bits(v)[:, 0] == 0).all())
    sub = (v.float().abs() < 2.0 ** -126) & (v.float() != 0)
    # below 2^-126: +-0.5, 1, 1.5 under byte 0 and +-0.5 under byte 1
    assert sorted({int(b) for b, _ in sub.nonzero().tolist()}) == [0, 1]
    assert sub[0].nonzero().view(-1).tolist() == [1, 2, 3, 9, 10, 11] and sub[1].nonzero().view(-1).tolist() == [1, 9]
    # what overflows bf16 follows from the format: 2^128 and above, that is 4 and 6 under byte 253 and 2, 3, 4, 6
    # under byte 254, with either sign
    bad = wp.nonfinite_pairs()
    assert {b for _, b in bad} == {253, 254}
    assert sorted(c for c, b in bad if b == 253) == [6, 7, 14, 15]
    assert sorted(c for c, b in bad if b == 254) == [4, 5, 6, 7, 12, 13, 14, 15]
    assert float(v[254, 7]) == float("inf") and float(v[254, 15]) == float("-inf")


def test_range_weight_holds_every_pair_and_its_finite_form_only_finite_ones():
    full, fin = wp.range_weight("full"), wp.range_weight("finite")
    assert full.q.shape == (256, 128) and full.s.shape == (256, 8)
    host.check_mxfp4(full.q, full.s)
    host.check_mxfp4(fin.q, fin.s)
    assert torch.equal(full.s, fin.s) and full.s[:255, 0].tolist() == list(range(255))
    blocks = full.codes.view(256, 8, 32)
    assert bool((torch.sort(blocks, dim=-1).values == torch.arange(32) // 2).all())   # all 16 codes twice
    assert not torch.equal(blocks[0, 0], blocks[0, 1]) and not torch.equal(blocks[0, 0], blocks[1, 0])
    pairs = {(int(c), int(b)) for c, b in zip(full.codes.view(-1), full.s.repeat_interleave(32, 1).view(-1))}
    assert len(pairs) == 16 * 255
    assert not bool(torch.isfinite(gp.rne(full.W).float()).all())
    assert bool(torch.isfinite(gp.rne(fin.W).float()).all())
    changed = (full.codes != fin.codes).view(256, 8, 32).any(-1)
    assert bool((changed == (full.s >= 253)).all())
    # the probed k show every code of every block
    ks = torch.tensor(wp.range_ks())
    assert len(set(ks.tolist())) == 128
    for b in range(8):
        assert set(full.codes[7, ks[ks // 32 == b]].tolist()) == set(range(16))


# ---------------------------------------------------------------------------------------------------------
# range


def _range_rejects(mutant, variant="full"):
    rw = wp.range_weight(variant)
    return bool(gp.bitwise(wp.read_weight(rw.q, rw.s, mutant), gp.rne(rw.W)).any())


def test_range_accepts_the_reader_and_is_the_host_law():
    for variant in ("full", "finite"):
        assert not _range_rejects(None, variant)
        rw = wp.range_weight(variant)
        assert torch.equal(gp.bits(host.dequant_mxfp4(rw.q, rw.s)), gp.bits(gp.rne(rw.W)))


@pytest.mark.parametrize("mutant", ["nibbles", "block", "byte0", "flush", "saturate", "plus_zero"])
def test_range_rejects(mutant):
    assert _range_rejects(mutant)
    if mutant != "saturate":   # the GEMMs' weight has no overflowing pair to saturate
        assert _range_rejects(mutant, "finite")


def test_range_one_hot_rows_see_the_same_mutants_through_a_gemm():
    """The one-hot product of the GPU test: out[m, n] = RNE(W[n, k_m] * a_scale[m]).  Under the row scales the
    subnormal results move (2^-128 * 2^-2 is still a bf16) and the top bytes overflow to inf, which the comparison
    admits where the reference has it."""
    rw = wp.range_weight("finite")
    ks = wp.range_ks()
    a = wp.a_scales(128)
    want = wp.one_hot_law(rw.W, ks, a)
    f = want.float()
    assert bool(torch.isinf(f).any()) and int(((f.abs() < 2.0 ** -126) & (f != 0)).sum()) > 0
    assert not bool((gp.bits(want) == -0x8000).any())      # a GEMM's zero is +0 (one_hot_law)
    cage = gp.Cage(128, 256)
    # the sign of a zero weight is the dequantiser's to show: through a GEMM code 8 stored as +0 is no mutant
    for mutant, rejected in ((None, False), ("nibbles", True), ("block", True), ("byte0", True), ("flush", True),
                             ("plus_zero", False)):
        w = wp.read_weight(rw.q, rw.s, mutant).double()
        cage.view.copy_(wp.one_hot_law(w, ks, a))
        v = wp.bit_violations(cage, want, ks, rw.s)
        assert bool(v) == rejected, (mutant, v)
        if mutant == "byte0":
            assert "byte 0)" in v[0], v
    cage.buf[128, 0] = 1.0
    assert any("sentinels" in x for x in wp.bit_violations(cage, want))


# ---------------------------------------------------------------------------------------------------------
# dense


@pytest.mark.parametrize("N,K", wp.SKINNY_SHAPES)
def test_dense_premises_hold_at_every_weight_stream_shape(N, K):
    d = wp.dense_case(N, K, max(wp.SKINNY_M))
    assert d.A.shape[0] == 72 and d.headroom < 2 ** 24, d.headroom
    assert d.exact_share >= 0.9, d.exact_share


@pytest.mark.parametrize("N,K", wp.A8_SHAPES)
def test_dense_premises_hold_at_every_w4a8_shape(N, K):
    d = wp.dense_case(N, K, max(wp.A8_M))
    assert d.A.shape[0] == 265 and d.headroom < 2 ** 24, d.headroom
    assert d.exact_share >= 0.9, d.exact_share
    # the power-of-two row scales move the exponent only
    assert torch.equal(gp.rne(d.acc * 4.0).float(), d.want.float() * 4.0)


def test_dense_operands_are_what_the_issue_describes():
    d = wp.dense_case(48, 384, 64)
    A = d.A
    assert torch.equal(A.to(torch.bfloat16).float(), A) and torch.equal(A.to(torch.float8_e4m3fn).float(), A)
    assert bool((A.view(72, -1, 8).abs().sum(-1) == 1).all())                 # one k of every 8
    for s in range(wp.SHIFTS):                                                # a one-row launch per shift: every k
        assert bool((A[s:s + 8].abs().sum(0) == 1).all())
    assert set(d.codes.view(-1).tolist()) == set(range(16))
    assert sorted(set(d.s[:, 0].tolist())) == list(range(121, 134)) and bool((d.s == d.s[:, :1]).all())
    host.check_mxfp4(d.q, d.s)
    assert torch.equal(host.dequant_mxfp4(d.q, d.s).double(), d.W)


def test_dense_accepts_the_readers():
    for N, K in ((48, 384), (64, 1152)):
        d = wp.dense_case(N, K, 64)
        assert not bool(gp.bitwise(gp.rne(wp.read_stream(d.A, d.W)), d.want).any())
        assert not bool(gp.bitwise(gp.rne(wp.read_tiles(d.A, d.W)), d.want).any())
        assert not bool(gp.bitwise(gp.rne(wp.read_stream(d.A.float(), d.W.float())), d.want).any())


@pytest.mark.parametrize("mutant", ["twice", "dropped"])
@pytest.mark.parametrize("N,K", [(48, 384), (64, 1152)])
def test_dense_rejects_a_wrong_weight_stream(N, K, mutant):
    """K = 384: waves 2, 5 and 7 hold one batch; K = 1152: waves 0 to 6.  One row (the MT = 1 launch with its two-batch
    register sets) is enough to see it."""
    d = wp.dense_case(N, K, 64)
    assert any(wp.wave_batches(K, w)[1] % 2 for w in range(8))
    for rows in (slice(0, 1), slice(0, 64)):
        got = gp.rne(wp.read_stream(d.A[rows], d.W, mutant))
        assert bool(gp.bitwise(got, d.want[rows]).any()), rows


@pytest.mark.parametrize("N,K", wp.WIDE_SHAPES)
def test_dense_rejects_a_partial_that_went_through_bf16_on_wide_rows(N, K):
    """The +-1 rows do not see it (their partials are bf16 numbers), which is why the weight-stream kernels also run
    on rows whose odd groups hold +-2^-5.  Those rows keep the bitwise premise (``headroom``); their sums are no
    bf16 numbers, so the ``exact_share`` claim is the plain rows' alone."""
    plain, wide = wp.dense_case(N, K, 64), wp.dense_case(N, K, 64, wide=True)
    assert wide.headroom < 2 ** 24 and wide.exact_share < 0.5
    assert torch.equal(wide.A.to(torch.bfloat16).float(), wide.A)
    assert torch.equal(wide.A.to(torch.float8_e4m3fn).float(), wide.A)
    assert not bool(gp.bitwise(gp.rne(wp.read_stream(wide.A, wide.W)), wide.want).any())
    assert not bool(gp.bitwise(gp.rne(wp.read_stream(plain.A, plain.W, "bf16_partial")), plain.want).any())
    for rows in (slice(0, 1), slice(0, 64)):
        got = gp.rne(wp.read_stream(wide.A[rows], wide.W, "bf16_partial"))
        assert float(gp.bitwise(got, wide.want[rows]).double().mean()) > 0.25, rows


def test_dense_rejects_a_stale_second_tile_and_a_dropped_k():
    d = wp.dense_case(144, 256, 257)
    assert bool(gp.bitwise(gp.rne(wp.read_tiles(d.A, d.W, stale=True)), d.want).any())
    # one k left out of one 16 x 16 block: the rows whose +-1 sits at that k change, wherever the weight is not 0
    for k, r0, c0 in ((0, 0, 0), (255, 128, 128), (131, 249, 16)):
        got = gp.rne(gp.drop_k(d.acc, d.A, d.W, k, r0, c0))
        hit = (d.A[r0:r0 + 16, k] != 0)[:, None] & (d.W[c0:c0 + 16, k] != 0)[None, :]
        assert bool(hit.any())
        changed = gp.bitwise(got, d.want)[r0:r0 + 16, c0:c0 + 16]
        exact = (d.want.double() == d.acc)[r0:r0 + 16, c0:c0 + 16]
        assert bool((changed | ~hit | ~exact).all()) and bool((changed & hit).any())


# ---------------------------------------------------------------------------------------------------------
# segments


def test_segments_are_what_the_issue_describes():
    sg = wp.segments(64, 384, _gen(3))
    assert sg.lens == (33, 48, 0, 49, 63, 1, 64, 17, 80) and sg.rows == 355 and sg.row_off.tolist()[-1] == 355
    assert len(set(sg.a_rows.tolist())) < sg.rows and int(sg.a_rows.max()) < sg.A.shape[0]
    assert torch.equal(sg.A_em, sg.A[sg.a_rows.long()])
    assert all(not torch.equal(sg.q[e], sg.q[e + 1]) for e in range(8))
    for e in range(9):
        host.check_mxfp4(sg.q[e], sg.s[e])
        assert torch.equal(host.dequant_mxfp4(sg.q[e], sg.s[e]).double(), sg.W[e])


def test_segments_accept_the_reader_and_reject_the_three_mutants():
    sg = wp.segments(64, 384, _gen(3))
    want = gp.rne(sg.acc)
    cage = gp.Cage(sg.rows, 64)
    ro = sg.row_off.tolist()
    per_row = torch.cat([gp.rne(wp.read_stream(sg.A_em[ro[e]:ro[e + 1]], sg.W[e])) for e in range(9)])
    assert not gp.violations(wp.write_segments(cage.poison(), per_row, sg.row_off), want, "bitwise")
    # expert 0 has 33 rows: its third m-tile holds one row, a fourth is wholly past the end
    v = gp.violations(wp.write_segments(cage.poison(), per_row, sg.row_off, tile_further=0), want, "bitwise")
    assert v and "first at [48," in v[0], v
    # expert 1 has 48 rows: three full m-tiles, and the fourth lands in expert 3's rows (expert 2 is empty)
    v = gp.violations(wp.write_segments(cage.poison(), per_row, sg.row_off, tile_further=1), want, "bitwise")
    assert v and "first at [96," in v[0], v
    for wrong in (dict(shift_expert=1), dict(identity_gather=True)):
        got = gp.rne(wp.segment_product(sg, **wrong))
        bad = gp.bitwise(got, want)
        assert all(bool(bad[ro[e]:ro[e + 1]].any()) for e in range(9) if ro[e + 1] > ro[e] + 1), wrong


def test_swiglu_segments_are_bitwise_material():
    sg = wp.segments(128, 384, _gen(4), swiglu_=True)
    assert sg.gate.shape == (355, 64)
    zero, pos, neg = sg.gate == 0, sg.gate >= wp.SAT_POS, sg.gate <= wp.SAT_NEG
    assert bool((zero | pos | neg).all()) and min(int(zero.sum()), int(pos.sum()), int(neg.sum())) > 1000
    got = wp.epilogue(sg.gate, sg.up)
    assert not wp.swiglu_violations(got, sg.gate, sg.up)
    wrong = wp.segment_product(sg, shift_expert=1)
    assert wp.swiglu_violations(wp.epilogue(wrong[:, :64], wrong[:, 64:]), sg.gate, sg.up)


# ---------------------------------------------------------------------------------------------------------
# swiglu


def _sw():
    return wp.swiglu(40, 96, 384, _gen(5))


def test_swiglu_operands_are_what_the_issue_describes():
    sw = _sw()
    assert sw.q.shape == (192, 192) and sw.s.shape == (192, 12)
    host.check_mxfp4(sw.q, sw.s)
    assert torch.equal(sw.A.to(torch.float8_e4m3fn).float(), sw.A)
    # the interleaved weight is the [gate; up] one, 32 rows at a time
    dq = host.dequant_mxfp4(sw.q, sw.s).double().view(3, 2, 32, 384)
    assert torch.equal(dq[:, 0].reshape(96, 384), sw.W[:96]) and torch.equal(dq[:, 1].reshape(96, 384), sw.W[96:])
    g = sw.gate
    for c, ok in ((0, g == 0), (1, (g != 0) & (g.abs() <= 8)), (2, (g.abs() == 96) | (g.abs() == 200))):
        assert bool(ok[:, sw.cls == c].all()) and int((sw.cls == c).sum()) == 32
    sat = g[:, sw.cls == 2]
    assert {float(v) for v in sat.unique()} == {96.0, -96.0, 200.0, -200.0}
    for v in (96.0, -96.0, 200.0, -200.0):   # ups of both signs under every saturated gate
        u = sw.up[g == v]
        assert bool((u > 0).any()) and bool((u < 0).any())
    # every sum is a small integer times a power of two: exact in fp32, and gate * up as well
    gu = torch.cat([sw.gate, sw.up], 1)
    assert torch.equal(gu.float().double(), gu) and torch.equal((sw.gate * sw.up).float().double(), sw.gate * sw.up)
    assert float((sw.A.abs().double() @ sw.W.abs().t()).max()) / 2.0 ** -4 < 2 ** 24


def test_the_saturated_premise():
    """1 + exp(-g) is 1 in fp32 from g = 17 up (the premise of tests/mx_probes.py at g = 64), so silu(g) = g;
    exp(-g) is inf in fp32 from g = -89 down, where x * rcp(inf) is a zero."""
    one = torch.ones((), dtype=torch.float32)
    for g in (wp.SAT_POS, 64.0, 96.0, 200.0):
        assert float(one + torch.exp(torch.tensor(-g))) == 1.0
    assert float(one + torch.exp(torch.tensor(-16.0))) > 1.0
    assert float(torch.exp(torch.tensor(-wp.SAT_NEG))) == float("inf")
    assert float(torch.exp(torch.tensor(88.0))) < float("inf")


@pytest.mark.parametrize("mutant,rejected", [(None, False), ("swapped", True), ("up_off", True), ("ratio", True)])
def test_swiglu_accepts_the_epilogue_and_rejects_the_mutants(mutant, rejected):
    sw = _sw()
    got = wp.epilogue(sw.gate, sw.up, mutant)
    v = wp.swiglu_violations(got, sw.gate, sw.up)
    assert bool(v) == rejected, v
    if mutant == "ratio":   # nothing but the NaN of the saturated negative gates
        assert len(v) == 2 and "non-finite" in v[0] and "negative saturated" in v[1], v
        assert bool((torch.isnan(got.float()) == (sw.gate <= wp.SAT_NEG)).all())
