"""Packed host/device formats of the engine's sampler staging, and nothing else: the pinned upload ring, the
int32 segment layout of a staging buffer, the per-row sampler columns with the batch value built from them, and
the sampler's packed output format.  Usable on a CPU device (host memory is pinned only for a GPU target)."""
from __future__ import annotations

import threading
from collections import deque
from dataclasses import dataclass
from typing import Deque, Dict, List, Optional, Sequence as Seq, Tuple

import numpy as np
import torch


class _PinnedRing:
    """Pinned host staging for the engine's per-step uploads: one pinned arena used as a ring.  An upload
    copies into the next free region and issues a non-blocking copy from it; a region is written again only
    after the event recorded behind its upload completed (oldest first, the ring's own order).  A fresh
    ``pin_memory()`` per upload cost ~250 us of host time each (~15 per mixed step; serve_load cProfile)."""

    def __init__(self, nbytes: int = 32 << 20):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.n, self.head = nbytes, 0
        self.live: Deque[Tuple[int, int, "torch.cuda.Event"]] = deque()

    def upload(self, t: torch.Tensor, dev) -> torch.Tensor:
        nb = t.numel() * t.element_size()
        size = (nb + 255) & ~255
        if size > self.n // 4:
            return t.pin_memory().to(dev, non_blocking=True)
        if self.head + size > self.n:
            self.head = 0
        start, end = self.head, self.head + size
        while self.live and self.live[0][0] < end and start < self.live[0][1]:
            self.live.popleft()[2].synchronize()  # (regions are handed out in order: the oldest overlaps first)
        self.head = end
        dst = self.buf[start:start + nb].view(t.dtype).view(t.shape)
        dst.copy_(t)
        out = dst.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.live.append((start, end, ev))
        if len(self.live) > 4096:  # bounded bookkeeping: retire the oldest
            self.live.popleft()[2].synchronize()
        return out


_RINGS = threading.local()


def _h2d(x, dtype, dev) -> torch.Tensor:
    """Host list / array -> device through pinned memory, non-blocking: a pageable upload synchronises
    the stream, i.e. would hold the host until every queued kernel (a decode step in flight) finished.
    Staged through this thread's pinned ring (one per engine thread and device)."""
    t = (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else torch.tensor(x)).to(dtype)
    dev = torch.device(dev)
    if dev.type != "cuda":
        return t.to(dev)
    rings = getattr(_RINGS, "by_dev", None)
    if rings is None:
        rings = _RINGS.by_dev = {}
    ring = rings.get(dev)
    if ring is None:
        ring = rings[dev] = _PinnedRing()
    return ring.upload(t.contiguous(), dev)


class PackedLayout:
    """Named segments of one int32 buffer.  ``segs``: (name, shape, numpy dtype), shape an int or a tuple of
    elements of that dtype.  Every segment starts 8-byte aligned (an even int32 index: int64 views)."""

    def __init__(self, segs: Seq[Tuple[str, object, object]]):
        self.segs: Dict[str, Tuple[int, int, np.dtype, object]] = {}  # name -> (start, end, dtype, shape)
        o = 0
        for name, shape, dt in segs:
            dt = np.dtype(dt)
            o += o & 1
            n = int(np.prod(shape)) * dt.itemsize // 4
            self.segs[name] = (o, o + n, dt, shape)
            o += n
        self.size = o + (o & 1)

    def views(self, buf) -> dict:
        """Typed, shaped views by name over ``buf``: int32, numpy or torch, at least ``size`` long."""
        return {name: buf[a:b].view(getattr(torch, dt.name) if isinstance(buf, torch.Tensor) else dt).reshape(shape)
                for name, (a, b, dt, shape) in self.segs.items()}


# The sampler's per-row columns: (name, dtype, fill of padded rows, how to read it from a sequence).
COLUMNS = (
    ("temperature", np.float32, 1.0, lambda s: s.params.temperature),
    ("top_p", np.float32, 1.0, lambda s: s.params.top_p),
    ("min_p", np.float32, 0, lambda s: s.params.min_p),
    ("top_a", np.float32, 0, lambda s: s.params.top_a),
    ("freq_pen", np.float32, 0, lambda s: s.params.frequency_penalty),
    ("pres_pen", np.float32, 0, lambda s: s.params.presence_penalty),
    ("rep_pen", np.float32, 1.0, lambda s: s.params.repetition_penalty),
    ("top_k", np.int32, 0, lambda s: s.params.top_k),
    ("count_rows", np.int32, -1, lambda s: s.count_row),
    ("bias_rows", np.int32, -1, lambda s: s.group.bias_row),
    ("lora_ids", np.int32, -1, lambda s: s.group.adapter_id),  # padding rows: no adapter
    ("seeds", np.int64, 0, lambda s: s.seed),
)


def row_segments(rows: int) -> List[Tuple[str, int, object]]:
    """Layout segments of the sampler inputs of ``rows`` rows: every column plus the Philox offsets."""
    return [(name, rows, dt) for name, dt, _, _ in COLUMNS] + [("offsets", rows, np.int64)]


@dataclass(frozen=True)
class SamplerBatch:
    """The sampler inputs of a list of sequences: one array of length n per column, and the batch's flags."""
    cols: Dict[str, np.ndarray]
    n: int
    K: int          # top logprobs to report (the largest request's)
    need_lp: bool   # some row reads its token's logprob
    any_pen: bool
    any_bias: bool

    @classmethod
    def of(cls, seqs) -> "SamplerBatch":
        ps = [s.params for s in seqs]
        return cls({name: np.array([get(s) for s in seqs], dtype=dt) for name, dt, _, get in COLUMNS}, len(seqs),
                   max((p.top_logprobs for p in ps), default=0), any(p.logprobs for p in ps),
                   any(p.uses_penalties for p in ps), any(s.group.bias_row >= 0 for s in seqs))

    def write(self, h: dict) -> None:
        """Write the columns into host views of >= n rows; the rows past n take the padding fill."""
        for name, _, fill, _ in COLUMNS:
            h[name][:self.n] = self.cols[name]
            h[name][self.n:] = fill

    def upload(self, offsets, dev) -> Dict[str, torch.Tensor]:
        """The n rows and their Philox ``offsets`` as ONE packed upload; returns the device views."""
        lay = PackedLayout(row_segments(self.n))
        buf = np.zeros(lay.size, np.int32)
        h = lay.views(buf)
        self.write(h)
        h["offsets"][:] = offsets
        return lay.views(_h2d(buf, torch.int32, dev))

    def sample_kwargs(self, d: dict, counts: Optional[torch.Tensor], bias: Optional[torch.Tensor]) -> dict:
        """``ops.sample`` keyword arguments from device views ``d`` and the engine's count / bias tables:
        penalty and bias operands are None unless some row uses them."""
        kw = {k: d[k] for k in ("temperature", "top_p", "top_k", "min_p", "top_a", "seeds", "offsets")}
        kw.update({k: d[k] if self.any_pen else None for k in ("freq_pen", "pres_pen", "rep_pen", "count_rows")})
        return dict(kw, counts=counts if self.any_pen else None, bias=bias if self.any_bias else None,
                    bias_rows=d["bias_rows"] if self.any_bias else None, num_logprobs=self.K, need_logprob=self.need_lp)


def output_layout(rows: int, K: int) -> PackedLayout:
    """The sampler's outputs for ``rows`` rows as one int32 buffer, tok | lp | topk ids | topk lp:
    ``tuple(layout.views(buf).values())`` over the device buffer are the sampler's four out_* operands."""
    Kb = max(K, 1)
    return PackedLayout([("tok", rows, np.int32), ("lp", rows, np.float32), ("ids", (rows, Kb), np.int32),
                         ("lps", (rows, Kb), np.float32)])


def unpack_outputs(host: np.ndarray, Bp: int, B: int, K: int):
    """The inverse on the host copy: (tok, lp, ids | None, lps | None) as lists, the first B of Bp rows."""
    tok, lp, ids, lps = output_layout(Bp, K).views(host).values()
    top = (ids[:B, :K].tolist(), lps[:B, :K].tolist()) if K else (None, None)
    return (tok[:B].tolist(), lp[:B].tolist()) + top
