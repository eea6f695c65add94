"""The attention probes of tests/attn_probes.py would notice the failures they target (CPU only).

For every programme at the key counts the GPU tests use, an honest emulation of the kernels' arithmetic
(log2 domain, 32-key tiles, lazy rescale, bf16 P, bf16 output) passes the comparison the GPU tests make, and
each targeted mutation — a dropped, doubled or leaked key, a skipped O rescale, an alpha taken from the
wrong row — is rejected by it.  The last tests record why the probes exist: with the random inputs of the
older attention tests, the suite's bound cannot see one wrong key in a long context."""
import functools
import math

import pytest
import torch

from tests import attn_probes as ap
from tests import torch_ref as ref

# every context / key-range length of tests/test_attention_probes_gpu.py
LENGTHS = [1, 16, 17, 32, 33, 49, 64, 65, 100, 118, 130, 200, 257, 300, 449]


@functools.lru_cache(maxsize=None)
def _wave(L, D=128, splits=3, seed=0):
    """A 16-row wave with mixed programmes over L visible keys plus one key past the end (masked); built
    once per shape and shared (no test writes to it)."""
    gen = torch.Generator().manual_seed(seed + L)
    progs = ap.decode_programmes(L, splits)[:16]
    scale = 1 / math.sqrt(D)
    q, k = ap.build_wave(progs, L + 1, D, scale, gen)
    s_all = ap.scores_nats(q, k, scale)
    s = s_all.clone()
    s[:, L] = -math.inf
    v = torch.randn(L + 1, D, generator=gen).to(torch.bfloat16)
    vi = ap.nonzero_prefix_sums(ap.int_values((L + 1, D), gen))
    return progs, s, s_all, v, vi, (q, k)


def _rows(progs, kind):
    return [r for r, p in enumerate(progs) if p.kind == kind]


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("L", LENGTHS)
def test_honest_emulation_is_accepted(L, D):
    progs, s, _, v, vi, (q, k) = _wave(L, D)
    want = ap.softmax_out(s, v)
    assert ap.accepted(ap.emulate(s, v), want)
    flat = _rows(progs, "flat")
    assert ap.accepted(ap.emulate(s, vi)[flat], ap.softmax_out(s, vi)[flat], 0.0, ap.FLAT_RTOL)
    # the oracle of the GPU tests (rows as the heads of one query token) agrees with the fp64 one used here
    o = ref.attention(q.view(1, -1, D), k[:L].view(L, 1, D), v[:L].view(L, 1, D), False, 1 / math.sqrt(D))[0]
    assert ap.accepted(o, want, 1e-4, 1e-4)


@pytest.mark.parametrize("L", LENGTHS)
def test_preconditions_hold(L):
    """What the GPU tests assert from the reference's scores: a spike holds >= 0.999 of its row's weight and
    the staircase forces a rescale at every 32-key boundary, for every way the decode kernels tile a context."""
    progs, s, _, _, _, _ = _wave(L)
    for r, p in enumerate(progs):
        if p.kind == "spike":
            assert ap.key_weight(s[r, :L], p.at) >= 0.999
    stair = _rows(progs, "stair")[0]
    sc = 1 / math.sqrt(128)
    assert ap.forced_rescales(s[stair], ap.tiles_of(L)) == ap.stair_rises(ap.tiles_of(L), sc)
    assert ap.stair_rises(ap.tiles_of(L), sc) == (L - 1) // 32 - (0 < L % 32 < 16 and L > 32)  # 16 keys clear 8
    assert ap.forced_rescales(s[_rows(progs, "flat")[0]], ap.tiles_of(L)) == 0
    for splits in (1, 2, 3):
        for path in ("wg4", "wave"):
            states = ap.decode_tiles(L, splits, path)
            assert sorted(t for st in states for t in st) == [t for e in _split_ranges(L, splits) for t in e]
            for st in states:
                assert ap.forced_rescales(s[stair], st) == ap.stair_rises(st, sc)


def _split_ranges(L, splits):
    nblk = -(-L // 16)
    per = -(-nblk // splits)
    return [ap.tiles_of(min(16 * min(nblk, sp * per + per), L), 16 * sp * per) for sp in range(splits)]


@pytest.mark.parametrize("L", LENGTHS)
def test_wrong_keys_are_rejected(L):
    """A dropped, doubled or leaked key moves the probed rows out of the bound, at every length."""
    progs, s, s_all, v, vi, _ = _wave(L)
    want, want_i = ap.softmax_out(s, v), ap.softmax_out(s, vi)
    stair, flat = _rows(progs, "stair"), _rows(progs, "flat")
    mutants = [dict(leak=True)] + ([dict(drop=L - 1), dict(double=L - 1)] if L >= 2 else [])
    for mu in mutants:
        src = s_all if mu.get("leak") else s
        kw = {k_: v_ for k_, v_ in mu.items() if k_ != "leak"}
        assert not ap.accepted(ap.softmax_out(src, v, **kw)[stair], want[stair]), mu
        assert not ap.accepted(ap.softmax_out(src, vi, **kw)[flat], want_i[flat], 0.0, ap.FLAT_RTOL), mu
    if L >= 2:
        for r, p in enumerate(progs):
            if p.kind == "spike":
                assert not ap.accepted(ap.softmax_out(s, v, drop=p.at)[[r]], want[[r]]), p
    # the flat rows see EVERY key, not only the last: any one dropped or doubled
    for p in sorted({0, L // 2, L - 1}):
        if L >= 2:
            assert not ap.accepted(ap.softmax_out(s, vi, drop=p)[flat], want_i[flat], 0.0, ap.FLAT_RTOL)
            assert not ap.accepted(ap.softmax_out(s, vi, double=p)[flat], want_i[flat], 0.0, ap.FLAT_RTOL)


@pytest.mark.parametrize("L", [n for n in LENGTHS if n > ap.TILE])
def test_broken_rescale_is_rejected(L):
    """More than one tile: an O that is not rescaled, or rescaled by a neighbour's alpha, is rejected — on
    the rows that rescale and on the control rows next to them."""
    progs, s, _, v, vi, _ = _wave(L)
    want = ap.softmax_out(s, v)
    stair, flat, bg = _rows(progs, "stair"), _rows(progs, "flat"), _rows(progs, "bg")
    late = [r for r, p in enumerate(progs) if p.kind == "spike" and p.at >= ap.TILE]
    skipped = ap.emulate(s, v, skip_o_rescale=True)
    assert not ap.accepted(skipped[stair], want[stair])
    for r in late:
        assert not ap.accepted(skipped[[r]], want[[r]]), progs[r]
    assert ap.accepted(skipped[flat], want[flat])  # alpha = 1 always: the flat row has nothing to rescale
    shifted = ap.emulate(s, v, alpha_shift=1)
    assert not ap.accepted(shifted[flat], want[flat])  # the flat row sits below the staircase row
    assert not ap.accepted(ap.emulate(s, vi, alpha_shift=1)[flat], ap.softmax_out(s, vi)[flat], 0.0, ap.FLAT_RTOL)
    assert not ap.accepted(ap.emulate(s, v, alpha_shift=2)[bg], want[bg])  # the control row, two below it
    assert not ap.accepted(ap.emulate(s, v, alpha_shift=-1), want)


@pytest.mark.parametrize("D", [128, 64])
def test_causal_wave_leak_is_rejected(D):
    """A prefill wave (16 consecutive query tokens, causal): the honest emulation passes; admitting key i + 1
    is rejected on every staircase and flat row."""
    L, i0 = 130, 96
    gen = torch.Generator().manual_seed(7)
    scale = 1 / math.sqrt(D)
    progs = ap.prefill_programmes(L, 0)
    rows = [progs[(i + 3) % len(progs)] for i in range(i0, i0 + 16)]
    q, k = ap.build_wave(progs, L, D, scale, gen)
    pick = [progs.index(p) for p in rows]
    s_all = ap.scores_nats(q[pick], k, scale)
    t, i = torch.arange(L)[None, :], torch.arange(i0, i0 + 16)[:, None]
    s = s_all.masked_fill(t > i, -math.inf)
    leak = s_all.masked_fill(t > i + 1, -math.inf)
    v, vi = torch.randn(L, D, generator=gen).to(torch.bfloat16), ap.nonzero_prefix_sums(ap.int_values((L, D), gen))
    want, want_i = ap.softmax_out(s, v), ap.softmax_out(s, vi)
    assert ap.accepted(ap.emulate(s, v), want)
    flat, stair = _rows(rows, "flat"), _rows(rows, "stair")
    assert flat and stair
    assert ap.accepted(ap.emulate(s, vi)[flat], want_i[flat], 0.0, ap.FLAT_RTOL)
    for r in stair:
        assert not ap.accepted(ap.softmax_out(leak, v)[[r]], want[[r]])
        assert ap.forced_rescales(s[r], ap.tiles_of(L)) == ap.stair_rises(ap.tiles_of(i0 + r + 1), scale) >= 2
    for r in flat:
        assert not ap.accepted(ap.softmax_out(leak, vi)[[r]], want_i[[r]], 0.0, ap.FLAT_RTOL)
    assert not ap.accepted(ap.emulate(s, v, skip_o_rescale=True)[stair], want[stair])


def test_cascade_order_falls_and_rises():
    """One-chunk cascade: prefix pairs are attended between suffix pairs, so a staircase row's tile maxima
    fall and rise.  The order covers every key once; the honest emulation in that order passes and a skipped
    rescale is rejected.  A longer prefix is walked front to back."""
    pblk, ctxs = 5, [80 + 33, 80 + 17, 80 + 1, 80 + 16]
    for j, L in enumerate(ctxs):
        order = ap.cascade_row_tiles(pblk, ctxs, j)
        assert sorted(order) == ap.tiles_of(80) + ap.tiles_of(L, 80)
    order = ap.cascade_row_tiles(pblk, ctxs, 0)
    assert order[0] == (80, 112) and order[1] == (0, 32) and order[2] == (112, 113)
    assert ap.cascade_row_tiles(19, [304 + 33], 0) == ap.tiles_of(304) + ap.tiles_of(337, 304)
    gen = torch.Generator().manual_seed(3)
    L, D, scale = ctxs[0], 128, 1 / math.sqrt(128)
    progs = [p(L) if callable(p) else p for p in ap.cascade_programmes(pblk)]
    q, k = ap.build_wave(progs, L, D, scale, gen)
    s, v = ap.scores_nats(q, k, scale), torch.randn(L, D, generator=gen).to(torch.bfloat16)
    want = ap.softmax_out(s, v)
    up, down = [r for r, p in enumerate(progs) if p.kind == "stair" and p.slope == 1], [len(progs) - 1]
    assert progs[down[0]].slope == -1
    assert ap.forced_rescales(s[up[0]], order) == ap.stair_rises(order, scale) == 0
    assert ap.forced_rescales(s[down[0]], order) == ap.stair_rises(order, scale, -1) == 1
    assert ap.accepted(ap.emulate(s, v, order), want)
    assert not ap.accepted(ap.emulate(s, v, order, skip_o_rescale=True)[down], want[down])
    assert not ap.accepted(ap.emulate(s, v, order, alpha_shift=1), want)
    # the falling staircase hangs on key 0: the first prefix key dropped or doubled is rejected
    assert not ap.accepted(ap.softmax_out(s, v, drop=0)[down], want[down])
    assert not ap.accepted(ap.softmax_out(s, v, double=0)[down], want[down])


@pytest.mark.parametrize("L", [200, 300])
def test_random_inputs_cannot_see_one_key_in_a_long_context(L):
    """The older attention tests draw q, k, v ~ N(0, 1) and compare at atol = rtol = 2e-2.  As a fact about
    that reference and that bound: dropping (or doubling) the last key moves a row by about w |v| with w =
    e^s / (1.65 L) the key's weight, and the largest |v| of 128 dims is about 2.7, so the bound notices only
    if e^s > 0.0075 * 1.65 * L — a score 0.9 sigma above average at L = 200, 1.3 at L = 300.  Most rows do not
    notice (at L = 33 most do).  The structured rows above are what sees such a key."""
    def blind(n):
        gen = torch.Generator().manual_seed(n)
        D, scale = 128, 1 / math.sqrt(128)
        q, k, v = (torch.randn(r, D, generator=gen).to(torch.bfloat16) for r in (256, n, n))
        s = ap.scores_nats(q, k, scale)
        want = ap.softmax_out(s, v)
        return [1 - ap.violations(ap.softmax_out(s, v, **kw), want, ap.ATOL, ap.RTOL).any(1).float().mean().item()
                for kw in (dict(drop=n - 1), dict(double=n - 1))]

    assert min(blind(L)) > 0.5
    assert max(blind(33)) < 0.5
