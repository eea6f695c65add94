"""The engine's sampler staging (engine/staging.py) on the CPU: the column table and its padding fills, the
packed int32 layout, the agreement of the decode-style and first-token-style input paths, and the packed
output format."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from llm_weighted_consensus_amd.engine.sampling import SamplingParams
from llm_weighted_consensus_amd.engine.staging import (COLUMNS, PackedLayout, SamplerBatch, output_layout, row_segments,
                                                       unpack_outputs)


def _seq(params, seed, count_row=-1, bias_row=-1, adapter=-1, n_launched=0):
    return SimpleNamespace(params=params, seed=seed, count_row=count_row, n_launched=n_launched,
                           group=SimpleNamespace(bias_row=bias_row, adapter_id=adapter))


def _three():
    return [_seq(SamplingParams(temperature=0.0), 1),
            _seq(SamplingParams(temperature=0.7, top_k=5, presence_penalty=1.0, top_logprobs=3), 2, count_row=7),
            _seq(SamplingParams(logit_bias={3: 1.0}, logprobs=True), 3, bias_row=2, adapter=1)]


def _padded(batch, B):
    """Bucket-style staging: host views of B rows with the batch written into them, and the raw buffer."""
    lay = PackedLayout(row_segments(B))
    buf = np.zeros(lay.size, np.int32)
    h = lay.views(buf)
    batch.write(h)
    return lay, buf, h


def test_literal_columns_padded_to_four():
    batch = SamplerBatch.of(_three())
    _, _, h = _padded(batch, 4)
    want = {
        "temperature": np.array([0, 0.7, 1, 1], np.float32), "top_p": np.array([1, 1, 1, 1], np.float32),
        "top_k": np.array([0, 5, 0, 0], np.int32), "min_p": np.zeros(4, np.float32),
        "top_a": np.zeros(4, np.float32), "freq_pen": np.zeros(4, np.float32),
        "pres_pen": np.array([0, 1, 0, 0], np.float32), "rep_pen": np.array([1, 1, 1, 1], np.float32),
        "count_rows": np.array([-1, 7, -1, -1], np.int32), "bias_rows": np.array([-1, -1, 2, -1], np.int32),
        "lora_ids": np.array([-1, -1, 1, -1], np.int32), "seeds": np.array([1, 2, 3, 0], np.int64),
    }
    assert set(want) == {name for name, *_ in COLUMNS}
    for name, w in want.items():
        assert h[name].dtype == w.dtype and h[name].tolist() == w.tolist(), name
        assert batch.cols[name].tolist() == w[:3].tolist(), name
    assert (batch.n, batch.K, batch.need_lp, batch.any_pen, batch.any_bias) == (3, 3, True, True, True)


@pytest.mark.parametrize("B", [1, 3, 4])
def test_layout_segments_are_aligned_disjoint_and_alias_the_buffer(B):
    lay = PackedLayout([("block_tables", (B, 5), np.int32), ("tiles", (1, 3), np.int32)] + row_segments(B))
    spans = sorted((a, b) for a, b, _, _ in lay.segs.values())
    assert all(a % 2 == 0 for a, _ in spans)
    assert all(b0 <= a1 for (_, b0), (a1, _) in zip(spans, spans[1:])) and spans[-1][1] <= lay.size
    assert all(b - a == int(np.prod(shape)) * dt.itemsize // 4 for a, b, dt, shape in lay.segs.values())
    buf = np.zeros(lay.size, np.int32)
    h = lay.views(buf)
    assert h["block_tables"].shape == (B, 5) and h["tiles"].shape == (1, 3)
    h["temperature"][B - 1] = 0.7
    h["seeds"][0] = (5 << 32) | 9
    a = lay.segs["temperature"][0]
    assert buf[a + B - 1] == np.array([0.7], np.float32).view(np.int32)[0]
    a = lay.segs["seeds"][0]
    assert (buf[a], buf[a + 1]) == (9, 5)  # little-endian int64 over two int32 words
    t = torch.zeros(lay.size, dtype=torch.int32)
    d = lay.views(t)
    d["top_p"][0] = 0.25
    d["offsets"][B - 1] = 7
    assert t[lay.segs["top_p"][0]].item() == np.array([0.25], np.float32).view(np.int32)[0]
    assert t[lay.segs["offsets"][0] + 2 * (B - 1)].item() == 7
    assert d["seeds"].dtype == torch.int64 and d["top_k"].dtype == torch.int32 and d["rep_pen"].dtype == torch.float32


def _batches():
    plain = SamplingParams(temperature=0.5, top_p=0.9, min_p=0.05, top_a=0.1)
    pen = SamplingParams(frequency_penalty=0.5, repetition_penalty=1.2, top_k=7)
    bias = SamplingParams(logit_bias={1: -2.0}, top_logprobs=2)
    return {
        "three": _three(),
        "none": [_seq(plain, 11, n_launched=4), _seq(SamplingParams(), 12, adapter=0)],
        "pen": [_seq(plain, 21), _seq(pen, 22, count_row=3, n_launched=2), _seq(pen, 23, count_row=0)],
        "bias": [_seq(bias, 31, bias_row=5, n_launched=1), _seq(plain, 32)],
        "both": [_seq(pen, 41, count_row=1, bias_row=4), _seq(bias, 42, bias_row=4, n_launched=9), _seq(plain, 43)],
    }


@pytest.mark.parametrize("name", list(_batches()))
def test_padded_write_and_packed_upload_give_the_same_sampler_arguments(name):
    seqs = _batches()[name]
    batch = SamplerBatch.of(seqs)
    n = len(seqs)
    assert (batch.any_pen, batch.any_bias) == {"three": (True, True), "none": (False, False), "pen": (True, False),
                                               "bias": (False, True), "both": (True, True)}[name]
    offsets = [s.n_launched for s in seqs]
    lay, buf, h = _padded(batch, 4)
    h["offsets"][:n] = offsets
    counts, bias = torch.zeros(8, 16, dtype=torch.int16), torch.zeros(8, 16)
    a = batch.sample_kwargs(lay.views(torch.from_numpy(buf)), counts, bias)
    b = batch.sample_kwargs(batch.upload(offsets, "cpu"), counts, bias)
    assert list(a) == list(b)
    pen_keys = {"freq_pen", "pres_pen", "rep_pen", "counts", "count_rows"}
    for k in a:
        absent = (k in pen_keys and not batch.any_pen) or (k in ("bias", "bias_rows") and not batch.any_bias)
        assert (a[k] is None) == absent and (b[k] is None) == absent, k
        if absent:
            continue
        if k in ("counts", "bias"):
            assert a[k] is b[k] and a[k] is (counts if k == "counts" else bias)
        elif k in ("num_logprobs", "need_logprob"):
            assert a[k] == b[k] == (batch.K if k == "num_logprobs" else batch.need_lp)
        else:
            assert a[k].dtype == b[k].dtype and b[k].shape == (n,) and torch.equal(a[k][:n], b[k]), k
    assert b["offsets"].tolist() == offsets and b["seeds"].tolist() == [s.seed for s in seqs]


@pytest.mark.parametrize("Bp,B,K", [(4, 3, 0), (4, 3, 3)])
def test_output_views_round_trip_through_the_host_unpack(Bp, B, K):
    lay = output_layout(Bp, K)
    dev = torch.full((lay.size,), -7, dtype=torch.int32)
    tok, lp, ids, lps = lay.views(dev).values()
    Kb = max(K, 1)
    assert (tok.dtype, lp.dtype, ids.dtype, lps.dtype) == (torch.int32, torch.float32, torch.int32, torch.float32)
    assert tok.shape == (Bp,) and lp.shape == (Bp,) and ids.shape == (Bp, Kb) and lps.shape == (Bp, Kb)
    tok.copy_(torch.arange(100, 100 + Bp, dtype=torch.int32))
    lp.copy_(-torch.arange(Bp, dtype=torch.float32) - 0.5)
    ids.copy_(torch.arange(Bp * Kb, dtype=torch.int32).view(Bp, Kb) + 1000)
    lps.copy_(-torch.arange(Bp * Kb, dtype=torch.float32).view(Bp, Kb) - 0.25)
    got = unpack_outputs(dev.numpy(), Bp, B, K)
    assert got[0] == [100 + i for i in range(B)] and got[1] == [-i - 0.5 for i in range(B)]
    if K:
        assert got[2] == [[1000 + r * Kb + c for c in range(K)] for r in range(B)]
        assert got[3] == [[-(r * Kb + c) - 0.25 for c in range(K)] for r in range(B)]
    else:
        assert got[2] is None and got[3] is None
