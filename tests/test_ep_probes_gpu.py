"""The expert-parallel exchange kernels (ep_pack, ep_unpack, ep_back, ep_combine of csrc/kernels/ep.hip) under the
exact inputs and the byte-for-byte oracle of tests/ep_probes.py: one process plays all W ranks on one device, the
all-to-all is tensor indexing.  The two-process test of tests/test_alltoall_gpu.py stays what it was: one comparison
of a final output at W = 2, El = 4, k = 2, d = 256, C = 128.

  stages     every case of ep_probes.CASES ((W, El) from (1, 1) to (8, 8), k = 1, 2, 8, bf16 rows of 8, 264, 2056 and
             e4m3 rows of 16, 4112 columns with scales, d_out = d or 264, C = max R, max R + 3, 1; random,
             single-expert, starved, holed and idle-rank routings): each kernel's output compared on its own with
             the oracle, bit for bit, the message naming kernel, rank, chunk, slot and byte; each kernel run twice
             into fresh cages whose contents must be identical; the unspecified bytes refilled with the NaN sentinel
             before the next kernel.
  combine    the exact, fine, one-hot (bitwise) and random (one_step_cond, COMBINE_ERR) families of
             tests/select_probes.py on returned chunks whose unused slots hold NaN.
  routed     ops.moe_route feeds the four kernels at (2, 4), k = 2; the output equals ops.moe_combine of the oracle's
             expert outputs bit for bit.
  poisoned   ep_unpack on received chunks whose last source is all-ones, has one count of -1, counts summing to C + 1,
             or counts {2^31 - 1, 2^31 - 1, 2, 0}: that source absent, the others where the oracle puts them, its
             slots of ep_back zero.  The pads around x_local, s_local and map are C + W El rows and the unsanitised
             emulation is first shown to stay inside them.
  refusals   W = 9, W El = 65, row_bytes % 16 != 0, RB < row_bytes + 4 with scales, ep_combine with k = 9, d % 8 != 0,
             E % El != 0: each raises and leaves its output cage untouched.

Every output sits in a PadCage whose sentinel rows must survive.  tests/test_ep_probes.py shows on the CPU what
these comparisons reject.  The tests print what they measured (pytest -s).

Observed on an MI355X: every comparison held bit for bit, the random combine family included (no output off plain
one_step); an idle rank's empty x, src, inv and w are accepted by the bindings as they are.  The file's 30 cases ran
in 2 s."""
import pytest
import torch

from tests import ep_probes as ep
from tests import select_probes as sp
from tests.ep_probes import BF, F32, I32, U8, Case, PadCage, bits, bitwise

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn


def _K():
    from llm_weighted_consensus_amd import ops
    return ops.kernels()


def _twice(what, run):
    """Run ``run()`` (which returns the cages it wrote) twice; the second set must equal the first, pads included."""
    a, b = run(), run()
    for i, (p, q) in enumerate(zip(a, b)):
        assert p.same_as(q), f"{what}: output {i} differs between two identical launches"
        assert p.touched() == 0, f"{what}: {p.touched()} sentinels around output {i} overwritten"
    return a


def _rows_dev(c: Case, rk, gpu):
    x = rk.x.to(gpu)
    return (x.view(FP8) if c.fp8 else x), (rk.xs.to(gpu) if c.fp8 else None)


def _pack(gpu, c: Case, r, rk):
    x, xs = _rows_dev(c, rk, gpu)

    def run():
        cage = PadCage(c.W, (c.C + 1) * c.RB, gpu, U8)
        _K().ep_pack(x, xs, rk.src.to(gpu), rk.row_off.to(gpu), c.W, c.El, c.C, cage.view)
        return [cage]

    cage = _twice(f"ep_pack {c.name} rank {r}", run)[0]
    msg = ep.first_byte("ep_pack", r, cage.view, rk.o["send"], rk.o["send_mask"], c.C + 1, c.RB, True)
    assert msg is None, f"{c.name}: {msg}"
    return cage.view


def _unpack(gpu, W, El, C, RB, rb, fp8, r, recv, o, what, pad=16):
    cols = rb if fp8 else rb // 2

    def run():
        cages = [PadCage(W * C, cols, gpu, U8 if fp8 else BF, pad), PadCage(W * C, 1, gpu, I32, pad),
                 PadCage(El + 1, 1, gpu, I32)] + ([PadCage(W * C, 1, gpu, F32, pad)] if fp8 else [])
        _K().ep_unpack(recv, W, El, C, cages[0].view, cages[3].flat if fp8 else None, cages[1].flat, cages[2].flat)
        return cages

    cages = _twice(f"ep_unpack {what} rank {r}", run)
    xc, mc, rc = cages[:3]
    n = int(o["n"])
    for msg in (ep.ints_message("ep_unpack", r, "row_off_local", rc.flat, o["row_off_local"]),
                ep.ints_message("ep_unpack", r, "map", mc.flat, o["map"], C),
                ep.rows_message("ep_unpack", r, xc.view, o["x_local"], n, o, C),
                ep.ints_message("ep_unpack", r, "s_local", cages[3].flat[:n], o["s_local"][:n]) if fp8 else None):
        assert msg is None, f"{what}: {msg}"
    ep.fill_unspecified_rows(xc.view, cages[3].flat if fp8 else None, n, fp8)
    return xc.view, (cages[3].flat if fp8 else None), mc.flat, rc.flat


def _back(gpu, W, C, r, y_local, rmap, want, what):
    d_out = y_local.shape[1]

    def run():
        cage = PadCage(W * C, d_out, gpu, BF)
        _K().ep_back(y_local, rmap, W, C, cage.view)
        return [cage]

    cage = _twice(f"ep_back {what} rank {r}", run)[0]
    msg = ep.first_byte("ep_back", r, cage.view, want, None, C, 2 * d_out, False)
    assert msg is None, f"{what}: {msg}"
    assert cage.unwritten() == 0, f"ep_back {what} rank {r}: {cage.unwritten()} outputs never written"
    return cage.view


def _combine(gpu, c: Case, r, rk, ret, w):
    T = w.shape[0]
    dev = [t.to(gpu) for t in (rk.row_off, rk.inv, w.reshape(-1).contiguous())]

    def run():
        cage = PadCage(T, c.d_out, gpu, BF)
        _K().ep_combine(ret, dev[0], dev[1], dev[2], c.El, c.C, c.k, cage.view)
        return [cage]

    cage = _twice(f"ep_combine {c.name} rank {r}", run)[0]
    assert cage.unwritten() == 0, f"ep_combine {c.name} rank {r}: {cage.unwritten()} outputs never written"
    return cage.view


def _out_message(c, r, got, want) -> str:
    bad = bitwise(got.cpu(), want)
    if not bool(bad.any()):
        return ""
    t, col = (int(v) for v in bad.nonzero()[0])
    return (f"{c.name}: ep_combine rank {r}: {int(bad.sum())} of {bad.numel()} outputs differ, first out[{t}, {col}]: "
            f"got {float(got[t, col]):.8g} want {float(ep.rne(want)[t, col]):.8g}")


def _chain(gpu, c: Case, ranks, check_out=True):
    """The whole exchange for all ranks, every stage held to the oracle; returns the outputs per rank."""
    W, C = c.W, c.C
    send = [_pack(gpu, c, r, rk) for r, rk in enumerate(ranks)]
    backs = []
    for r, recv in enumerate(ep.exchange(send, W)):
        o = ranks[r].o
        ep.fill_unspecified_send(recv, o["recv_mask"], c.fp8)
        x_local, s_local, rmap, rol = _unpack(gpu, W, c.El, C, c.RB, c.row_bytes, c.fp8, r, recv, o, c.name)
        mine = {"x_local": x_local.cpu().contiguous().view(U8).view(W * C, c.row_bytes),
                "s_local": s_local.cpu() if c.fp8 else None, "row_off_local": rol.cpu()}
        y_local = ep.oracle_experts(c, r, mine).to(gpu)      # the NaN sentinel in every row past the segments
        backs.append(_back(gpu, W, C, r, y_local, rmap, o["back"], c.name))
    outs = []
    for r, ret in enumerate(ep.exchange([b.view(W, -1) for b in backs], W)):
        rk = ranks[r]
        out = _combine(gpu, c, r, rk, ret.view(W * C, c.d_out).contiguous(), rk.w)
        if check_out:
            assert not _out_message(c, r, out, rk.o["out"]), _out_message(c, r, out, rk.o["out"])
        outs.append(out)
    return outs


@pytest.mark.parametrize("name", [c.name for c in ep.CASES])
def test_exchange_stages(gpu, name):
    c = ep.CASE[name]
    _chain(gpu, c, ep.oracle(c, ep.inputs(c)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ep.COMBINE_CASES)
def test_combine_families(gpu, name):
    c = ep.CASE[name]
    ranks = ep.inputs(c)
    for kind in ("exact", "fine", "onehot", "random"):
        well = total = 0.0
        for r, rk in enumerate(ranks):
            T = rk.x.shape[0]
            if T == 0:
                continue
            Y, w = ep.combine_inputs(kind, T, c.k, c.d_out, ep._gen(c), rows=rk.src.numel())
            ret = ep.ret_from_sorted(Y, rk.row_off, c.W, c.El, c.C)
            want, mag = ep.combine_want(Y, rk.inv, w, c.k)
            out = _combine(gpu, c, r, rk, ret.to(gpu), w).cpu()
            if kind == "random":
                bad, share = ep.one_step_cond(out, want, mag, ep.COMBINE_ERR)
                well, total = well + share * want.numel(), total + want.numel()
                print(f"\n[ep] combine random {name} rank {r}: {int(bad.sum())} of {bad.numel()} off one_step_cond, "
                      f"{int(sp.one_step(out, want).sum())} off plain one_step, worst {int(sp.steps(out, want).max())}")
            else:
                bad = bitwise(out, want)
            assert not bool(bad.any()), (f"ep_combine {kind} {name} rank {r}: {int(bad.sum())} of {bad.numel()} "
                                         f"outputs fail, first at {[int(v) for v in bad.nonzero()[0]]}")
        assert kind != "random" or well / total >= 0.95, f"{name}: only {well / total:.4f} well conditioned"


def test_routed_chain(gpu):
    """moe_route -> pack -> unpack -> experts -> back -> combine equals moe_combine of the expert outputs."""
    from llm_weighted_consensus_amd import ops

    c = ep.CHAIN
    routed = []
    for r, T in enumerate(c.T):
        logits = sp.route_logits(T, c.E, c.k, torch.Generator().manual_seed(5 + r)).to(gpu)
        routed.append(ops.moe_route(logits, c.k))
    ranks = ep.inputs(c, ids=[ids.cpu().long() for ids, *_ in routed])
    for rk, (ids, w, row_off, src, inv) in zip(ranks, routed):
        rk.row_off, rk.src, rk.inv, rk.w = row_off.cpu(), src.cpu(), inv.cpu(), w.cpu()
        assert torch.equal(rk.inv.long().sort().values, torch.arange(ids.numel()))
    assert c.C >= max(rk.src.numel() for rk in ranks)
    outs = _chain(gpu, c, ep.oracle(c, ranks), check_out=False)
    for r, (rk, out, (ids, w, row_off, src, inv)) in enumerate(zip(ranks, outs, routed)):
        Y = ep.sorted_expert_outputs(c, rk).to(gpu)
        want = ops.moe_combine(Y, inv, w, c.k)
        assert not _out_message(c, r, out, want.cpu()), _out_message(c, r, out, want.cpu())


@pytest.mark.parametrize("geo", ep.POISON_GEOS, ids=lambda g: f"w{g[0]}e{g[1]}d{g[2]}{'fp8' if g[3] else 'bf16'}")
@pytest.mark.parametrize("kind", ep.POISONS)
def test_unpack_poisoned_headers(gpu, kind, geo):
    W, El, d, fp8 = geo
    recv, C, RB, rb, bad = ep.poisoned_recv(W, El, d, fp8, kind)
    pad = ep.poison_pad(W, El, C)
    # the guard is exercised, not relied on: the emulation without it keeps every index inside the pads
    trace, scratch = [], [torch.zeros(W * C, rb, dtype=U8), torch.zeros(W * C), torch.zeros(W * C, dtype=I32),
                          torch.zeros(El + 1, dtype=I32)]
    ep.emul_unpack(recv, W, El, C, RB, rb, fp8, *scratch, sanitise=False, trace=trace)
    assert pad >= C + W * El and all(-pad <= row < W * C + pad for _, row in trace)
    o = ep.oracle_unpack(recv, W, El, C, RB, rb, fp8)
    assert bool((o["map"][bad * C:(bad + 1) * C] == -1).all()) and int(o["n"]) > 0
    what = f"poisoned {kind}"
    x_local, s_local, rmap, rol = _unpack(gpu, W, El, C, RB, rb, fp8, 0, recv.to(gpu), o, what, pad)
    y = torch.empty(W * C, 8, dtype=BF)
    bits(y).fill_(ep.SENTINEL)
    y[:int(o["n"])] = ep.distinct((int(o["n"]), 8))
    back = _back(gpu, W, C, 0, y.to(gpu), rmap, ep.oracle_back(y, o["map"], W, C), what)
    assert bool((bits(back)[bad * C:(bad + 1) * C] == 0).all()), f"{what}: the poisoned source's slots are not zero"
    torch.cuda.synchronize()


def test_refusals_write_nothing(gpu):
    K = _K()

    def refused(what, cage, call):
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        assert cage.touched() == 0 and cage.unwritten() == cage.view.numel(), f"{what}: refused but wrote"

    def pack(W, El, C, d, RB, scales=False, dtype=BF):
        x = torch.zeros(4, d, dtype=dtype, device=gpu)
        xs = torch.ones(4, device=gpu) if scales else None
        cage = PadCage(W, (C + 1) * RB, gpu, U8)
        row_off = torch.zeros(W * El + 1, dtype=I32, device=gpu)
        return cage, lambda: K.ep_pack(x, xs, None, row_off, W, El, C, cage.view)

    def unpack(W, El, C, d, RB, scales=False):
        recv = torch.zeros(W, (C + 1) * RB, dtype=U8, device=gpu)
        cage = PadCage(W * C, d, gpu, U8 if scales else BF)
        s = torch.zeros(W * C, device=gpu) if scales else None
        m, rol = torch.zeros(W * C, dtype=I32, device=gpu), torch.zeros(El + 1, dtype=I32, device=gpu)
        return cage, lambda: K.ep_unpack(recv, W, El, C, cage.view, s, m, rol)

    refused("pack W = 9", *pack(9, 1, 2, 8, 16))
    refused("pack W El = 65", *pack(5, 13, 2, 32, 64))
    refused("pack row_bytes = 8", *pack(2, 2, 2, 4, 16))
    refused("pack RB < row_bytes + 4 with scales", *pack(2, 2, 2, 16, 16, True, FP8))
    refused("unpack W = 9", *unpack(9, 1, 2, 8, 16))
    refused("unpack W El = 65", *unpack(5, 13, 2, 32, 64))
    refused("unpack RB < row_bytes + 4 with scales", *unpack(2, 2, 2, 16, 16, True))

    def combine(k, d, E, El, C=4, T=3):
        ret = torch.zeros((E // El) * C, d, dtype=BF, device=gpu)
        cage = PadCage(T, d, gpu, BF)
        row_off = torch.zeros(E + 1, dtype=I32, device=gpu)
        inv, w = torch.zeros(T * k, dtype=I32, device=gpu), torch.zeros(T * k, device=gpu)
        return cage, lambda: K.ep_combine(ret, row_off, inv, w, El, C, k, cage.view)

    refused("combine k = 9", *combine(9, 16, 8, 4))
    refused("combine d = 12", *combine(2, 12, 8, 4))
    refused("combine E % El != 0", *combine(2, 16, 8, 3))
