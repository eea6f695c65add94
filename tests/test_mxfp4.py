"""MXFP4 weight-only decoders without a GPU: the host quantiser's properties (ops/mxfp4.py), the refused
combinations, the CPU model path and the pre-quantised checkpoint round trip."""
import copy

import pytest
import torch

from tests import torch_ref as ref

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _ops():
    from llm_weighted_consensus_amd.ops import mxfp4

    return mxfp4


def _codes(q):
    """[N, K / 2] bytes -> [N, K] codes in k order."""
    return torch.stack([q & 0xF, q >> 4], dim=-1).view(q.shape[0], -1)


def _weights(N, K, seed, spread=True):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.02
    if spread:  # block scales over 13 exponents
        n, b = torch.arange(N).view(N, 1, 1), torch.arange(K // 32).view(1, K // 32, 1)
        w = (w.view(N, K // 32, 32) * torch.exp2(((n + b) % 13 - 6).float())).view(N, K)
    return w.to(torch.bfloat16)


@pytest.mark.parametrize("K", [512, 1024, 4096])
def test_quantiser_properties(K):
    m = _ops()
    w = _weights(48, K, K)
    q, s = m.quant_mxfp4_weight(w)
    assert q.dtype == torch.uint8 and q.shape == (48, K // 2) and s.dtype == torch.uint8 and s.shape == (48, K // 32)
    assert int(s.max()) < 255
    dq = m.dequant_mxfp4(q, s)
    assert dq.dtype == torch.bfloat16 and dq.shape == w.shape
    # every value is a bf16: the fp32 value survives the bf16 round trip bit for bit
    lut = torch.tensor(GRID + [-v for v in GRID])
    f32 = (lut[_codes(q).long()].view(48, K // 32, 32) * torch.exp2(s.float() - 127).unsqueeze(-1)).view(48, K)
    assert torch.equal(f32.to(torch.bfloat16).float(), f32) and torch.equal(dq.float(), f32)
    # values are idempotent (codes need not be: 3 x 2^e re-quantises as 6 x 2^(e - 1))
    assert torch.equal(m.dequant_mxfp4(*m.quant_mxfp4_weight(dq)), dq)
    # per block: e is the smallest integer with amax / 2^e <= 6, max |w - dq| <= 2^e, no |dq| above 6 x 2^e
    e = s.float() - 127
    amax = w.float().abs().view(48, K // 32, 32).amax(-1)
    assert bool((amax <= 6 * torch.exp2(e)).all()) and bool((amax > 6 * torch.exp2(e - 1)).all())
    err = (w.float() - dq.float()).abs().view(48, K // 32, 32).amax(-1)
    assert bool((err <= torch.exp2(e)).all())
    assert bool((dq.float().abs().view(48, K // 32, 32).amax(-1) <= 6 * torch.exp2(e)).all())
    # no -0 is written
    assert not bool((_codes(q) == 8).any())


@pytest.mark.parametrize("e", [-3, 0, 5])
def test_hand_made_blocks(e):
    m = _ops()
    sc = 2.0 ** e
    # block 0: amax = 6 x 2^e exactly, every tie (to the even code), signs, values that round to zero
    b0 = [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -6.0,
          0.0, 0.125, -0.125, 0.28125, 0.71875, 1.0, 1.5, 2.0, 3.0, 4.0, -0.5, -1.0, 2.4375, 2.5625, 4.875, 5.125]
    x0 = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0, -6.0,
          0.0, 0.0, 0.0, 0.5, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, -0.5, -1.0, 2.0, 3.0, 4.0, 6.0]
    # block 1: all zero; block 2: amax a power of two (4 x 2^e: scale exponent e, 4 is on the grid);
    # block 3: amax just above 6 x 2^e moves the exponent up by one
    b2 = [4.0] + [1.0, -2.0, 0.5] * 10 + [3.0]
    b3 = [6.25] + [1.0] * 31  # bf16-exact; scale e + 1: 6.25 / 2 = 3.125 -> 3, 0.5 -> 0.5
    w = (torch.tensor([b0 + [0.0] * 32 + b2 + b3]) * sc).to(torch.bfloat16)
    assert torch.equal(w.float(), torch.tensor([b0 + [0.0] * 32 + b2 + b3]) * sc)  # the inputs are bf16-exact
    q, s = m.quant_mxfp4_weight(w)
    assert s.tolist() == [[e + 127, 0, e + 127, e + 128]]
    dq = m.dequant_mxfp4(q, s).float()
    want = torch.tensor([x0 + [0.0] * 32 + b2 + [6.0] + [1.0] * 31]) * sc
    assert torch.equal(dq, want)
    codes = _codes(q)[0]
    assert codes[32:64].eq(0).all() and not bool((codes == 8).any())
    # the tie codes themselves: 0.25 -> 0, 0.75 -> 2, 1.25 -> 2, 1.75 -> 4, 2.5 -> 4, 3.5 -> 6, 5 -> 6
    assert codes[1:8].tolist() == [0, 2, 2, 4, 4, 6, 6] and codes[8:15].tolist() == [0, 10, 10, 12, 12, 14, 14]
    # nibble order: k = 2j low, k = 2j + 1 high
    assert int(q[0, 0]) == (7 | (0 << 4)) and int(q[0, 1]) == (2 | (2 << 4))


def test_extreme_scales_do_not_saturate():
    m = _ops()
    big = torch.full((1, 32), 3.0 * 2.0 ** 100, dtype=torch.bfloat16)
    tiny = torch.full((1, 32), 2.0 ** -130, dtype=torch.bfloat16)  # a bf16 subnormal
    q, s = m.quant_mxfp4_weight(torch.cat([big, tiny], dim=1))
    assert s.tolist() == [[99 + 127, 0]]  # 3 x 2^100 = 6 x 2^99; the tiny block clamps at e = -127
    dq = m.dequant_mxfp4(q, s).float()
    assert bool((dq[0, :32] == 3.0 * 2.0 ** 100).all()) and bool((dq[0, 32:] == 0).all())  # 2^-130 / 2^-127 < 0.25
    with pytest.raises(ValueError, match="K % 32"):
        m.quant_mxfp4_weight(torch.zeros(4, 48, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="255"):
        m.dequant_mxfp4(torch.zeros(1, 16, dtype=torch.uint8), torch.full((1, 1), 255, dtype=torch.uint8))


def test_weight_class_holds_the_external_format():
    from llm_weighted_consensus_amd import ops

    w = _weights(32, 256, 1)
    mw = ops.Mxfp4Weight(w)
    q, s = ops.quant_mxfp4_weight(w)
    assert mw.shape == (32, 256) and torch.equal(mw.q, q) and torch.equal(mw.s, s)
    assert mw.nbytes == 32 * 256 // 2 + 32 * 256 // 32
    assert torch.equal(ops.Mxfp4Weight.from_packed(q, s).dequant(), ops.dequant_mxfp4(q, s))
    # the SwiGLU interleave is a row permutation: it commutes with the quantisation
    wi = ops.Mxfp4Weight(ops.swiglu_interleave(_weights(128, 256, 2)))
    w0 = ops.Mxfp4Weight(_weights(128, 256, 2))
    assert torch.equal(wi.q, ops.swiglu_interleave(w0.q)) and torch.equal(wi.s, ops.swiglu_interleave(w0.s))


# ------------------------------------------------------------------ refusals
ADS = {"a": {"weights": "random:7"}}


@pytest.mark.parametrize("extra,embedder,msg", [
    ({"fp8": True}, False, "mxfp4 weights do not combine with fp8"),
    ({"tp": 2}, False, "mxfp4 weights do not combine with tp > 1"),
    ({"adapters": ADS}, False, "mxfp4 weights do not combine with LoRA adapters"),
    ({"arch": "mixtral-tiny"}, False, "mxfp4 weights are not supported on MoE decoders"),
    ({}, True, "mxfp4 weights are served on generation models only"),
])
def test_spec_refusals(extra, embedder, msg):
    from llm_weighted_consensus_amd.models.lora import check_model_spec

    spec = dict({"arch": "llama-tiny", "weights": "random:0", "mxfp4": True}, **extra)
    with pytest.raises(ValueError, match=msg):
        check_model_spec("m", spec, embedder=embedder)
    # the factory refuses before it touches a device or a weight
    if not embedder:
        from llm_weighted_consensus_amd.engine.group import build_engine

        with pytest.raises(ValueError, match=msg):
            build_engine(spec, 0)
    else:
        from llm_weighted_consensus_amd.embeddings.service import build_embedding_service

        with pytest.raises(ValueError, match=msg):
            build_embedding_service("m", spec, "cpu")
    # without the flag nothing changes
    off = {k: v for k, v in spec.items() if k != "mxfp4"}
    if not embedder and "adapters" not in off:
        assert check_model_spec("m", off) == ()


def test_model_constructor_refusals():
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.tp import TPLlamaModel

    cfg = decoder_config("llama-tiny")
    with pytest.raises(ValueError, match="mxfp4 weights do not combine with fp8"):
        LlamaModel(cfg, device="cpu", mxfp4=True, fp8_dense=True)
    with pytest.raises(ValueError, match="mxfp4 weights do not combine with LoRA"):
        LlamaModel(cfg, device="cpu", mxfp4=True, lora=[])
    with pytest.raises(ValueError, match="mxfp4 weights do not combine with tensor parallelism"):
        TPLlamaModel(cfg, device="cpu", mxfp4=True, tp_size=2)
    with pytest.raises(ValueError, match="mxfp4 weights are not supported on MoE"):
        MixtralModel(decoder_config("mixtral-tiny"), device="cpu", mxfp4=True)
    with pytest.raises(ValueError, match="mxfp4 weights are not supported on MoE"):
        LlamaModel(decoder_config("mixtral-tiny"), device="cpu", mxfp4=True)


# ------------------------------------------------------------------ model and checkpoints
def _model(arch="llama-tiny", **kw):
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    return LlamaModel(decoder_config(arch), device="cpu", max_position=128, **kw)


def _dq(w):
    from llm_weighted_consensus_amd import ops

    return ops.dequant_mxfp4(*ops.quant_mxfp4_weight(w))


def test_cpu_model_equals_the_dequantised_twin():
    m = _model(seed=4, mxfp4=True)
    twin = _model(seed=4)
    for L, T in zip(m.layers, twin.layers):
        T.wqkv, T.wo, T.w_gate_up, T.w_down = _dq(T.wqkv), _dq(T.wo), _dq(T.w_gate_up), _dq(T.w_down)
        assert L.gu_block == T.gu_block == 0
        for a, b in ((L.wqkv, T.wqkv), (L.wo, T.wo), (L.w_gate_up, T.w_gate_up), (L.w_down, T.w_down)):
            assert a.dtype == torch.bfloat16 and torch.equal(a, b)
    assert torch.equal(m.embed, twin.embed) and torch.equal(m.lm_head, twin.lm_head)
    toks = torch.randint(0, m.cfg.vocab_size, (33,), generator=torch.Generator().manual_seed(1))
    assert torch.equal(ref.llama_forward(m, toks), ref.llama_forward(twin, toks))
    # and the quantisation is not a no-op
    plain = _model(seed=4)
    assert not torch.equal(m.layers[0].wqkv, plain.layers[0].wqkv)


def _hf_state(m):
    cfg = m.cfg
    Q, K = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    sd = {"model.embed_tokens.weight": m.embed, "model.norm.weight": m.final_norm}
    if not cfg.tie_embeddings:
        sd["lm_head.weight"] = m.lm_head
    for i, L in enumerate(m.layers):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = L.attn_norm, L.mlp_norm
        for name, lo, hi in (("q", 0, Q), ("k", Q, Q + K), ("v", Q + K, Q + 2 * K)):
            sd[p + f"self_attn.{name}_proj.weight"] = L.wqkv[lo:hi]
        sd[p + "self_attn.o_proj.weight"] = L.wo
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = L.w_gate_up.chunk(2)
        sd[p + "mlp.down_proj.weight"] = L.w_down
    return {k: v.clone().contiguous() for k, v in sd.items()}


def test_prequantised_checkpoint_round_trip(tmp_path, monkeypatch):
    import importlib.util
    from pathlib import Path

    from safetensors.torch import load_file, save_file

    from llm_weighted_consensus_amd import ops
    from llm_weighted_consensus_amd.models import llama

    spec = importlib.util.spec_from_file_location(
        "quantize_mxfp4", Path(__file__).resolve().parents[1] / "scripts" / "quantize_mxfp4.py")
    quantize_mxfp4 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(quantize_mxfp4)
    src = _model(seed=9)
    bf16 = tmp_path / "bf16.safetensors"
    save_file(_hf_state(src), str(bf16))
    out = quantize_mxfp4.quantize_checkpoint(str(bf16), str(tmp_path / "mx.safetensors"))
    sd = load_file(out)
    p = "model.layers.1.mlp.down_proj"
    assert sd[p + ".weight"].dtype == torch.uint8 and sd[p + ".weight_scale"].dtype == torch.uint8
    assert sd["model.embed_tokens.weight"].dtype == torch.bfloat16

    # what the loader hands the layer, before the device-dependent step: the packed tensors as they are
    seen = {}
    orig = llama.LlamaModel._quantise_layer

    def spy(self, L):
        seen.setdefault(id(self), []).append(copy.copy(L))
        orig(self, L)

    monkeypatch.setattr(llama.LlamaModel, "_quantise_layer", spy)
    a = _model(weights_path=out, mxfp4=True)          # pre-quantised
    b = _model(weights_path=str(bf16), mxfp4=True)    # quantised at load
    la, lb = seen[id(a)], seen[id(b)]
    assert len(la) == len(lb) == src.cfg.layers
    for A, B in zip(la, lb):
        for name in ("wqkv", "wo", "w_gate_up", "w_down"):
            pa, wb = getattr(A, name), getattr(B, name)
            assert isinstance(pa, ops.Mxfp4Weight) and isinstance(wb, torch.Tensor)
            q, s = ops.quant_mxfp4_weight(wb)
            assert torch.equal(pa.q, q) and torch.equal(pa.s, s) and pa.shape == tuple(wb.shape)
    for A, B in zip(a.layers, b.layers):
        for name in ("wqkv", "wo", "w_gate_up", "w_down"):
            assert torch.equal(getattr(A, name), getattr(B, name))
    toks = torch.arange(17)
    assert torch.equal(ref.llama_forward(a, toks), ref.llama_forward(b, toks))

    # refusals, by the tensor's name
    bad = dict(sd)
    bad[p + ".weight_scale"] = sd[p + ".weight_scale"].clone()
    bad[p + ".weight_scale"][3, 0] = 255
    save_file(bad, str(tmp_path / "nan.safetensors"))
    with pytest.raises(ValueError, match=r"model\.layers\.1\.mlp\.down_proj\.weight_scale.*255"):
        _model(weights_path=str(tmp_path / "nan.safetensors"), mxfp4=True)
    bad = dict(sd)
    k = "model.layers.0.self_attn.k_proj.weight"
    bad[k] = sd[k][:, :-1].contiguous()
    save_file(bad, str(tmp_path / "shape.safetensors"))
    with pytest.raises(ValueError, match=r"model\.layers\.0\.self_attn\.k_proj\.weight "):
        _model(weights_path=str(tmp_path / "shape.safetensors"), mxfp4=True)
    bad = dict(sd)
    del bad["model.layers.0.self_attn.o_proj.weight_scale"]
    save_file(bad, str(tmp_path / "missing.safetensors"))
    with pytest.raises(ValueError, match=r"model\.layers\.0\.self_attn\.o_proj\.weight_scale"):
        _model(weights_path=str(tmp_path / "missing.safetensors"), mxfp4=True)
    # a quantised checkpoint is not read as bf16 by a model that did not ask for it
    with pytest.raises(ValueError, match="mxfp4=True"):
        _model(weights_path=out)
