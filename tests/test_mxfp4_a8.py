"""``mxfp4_act`` (MXFP4 weights with e4m3 activations) without a GPU: the spec key's refusals through every entry
point, the unchanged spec check without it, the CPU model (the flag accepted, bf16 activations on the
dequantised weights) and the class-level default of ``act_format``."""
import pytest
import torch

from tests import torch_ref as ref

ADS = {"a": {"weights": "random:7"}}
BASE = {"arch": "llama-tiny", "weights": "random:0"}


@pytest.mark.parametrize("extra,msg", [
    # the key without the weights it describes, and values that are no format
    ({"mxfp4_act": "e4m3"}, '"mxfp4_act" needs "mxfp4": true'),
    ({"mxfp4_act": "bf16"}, '"mxfp4_act" needs "mxfp4": true'),
    ({"mxfp4": False, "mxfp4_act": "e4m3"}, '"mxfp4_act" needs "mxfp4": true'),
    ({"mxfp4": True, "mxfp4_act": "fp4"}, "mxfp4_act 'fp4': must be one of 'bf16', 'e4m3'"),
    ({"mxfp4": True, "mxfp4_act": True}, "mxfp4_act True: must be one of 'bf16', 'e4m3'"),
    ({"mxfp4": True, "mxfp4_act": ""}, "mxfp4_act '': must be one of 'bf16', 'e4m3'"),
    # everything "mxfp4" refuses, in its own words
    ({"mxfp4": True, "mxfp4_act": "e4m3", "fp8": True}, "mxfp4 weights do not combine with fp8 weights"),
    ({"mxfp4": True, "mxfp4_act": "e4m3", "tp": 2}, "mxfp4 weights do not combine with tp > 1"),
    ({"mxfp4": True, "mxfp4_act": "e4m3", "adapters": ADS}, "mxfp4 weights do not combine with LoRA adapters"),
    ({"mxfp4": True, "mxfp4_act": "e4m3", "arch": "mixtral-tiny"},
     r"mxfp4 weights are not supported on MoE decoders \(mixtral-tiny\)"),
    ({"mxfp4": True, "mxfp4_act": "nope", "fp8": True}, "mxfp4 weights do not combine with fp8 weights"),
])
def test_spec_refusals(extra, msg, monkeypatch):
    from llm_weighted_consensus_amd.engine.group import build_engine
    from llm_weighted_consensus_amd.models.lora import check_model_spec

    spec = dict(BASE, **extra)
    with pytest.raises(ValueError, match=f"^model m: {msg}$"):
        check_model_spec("m", spec)
    # the factory refuses before it touches a device or a weight
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=msg):
        build_engine(spec, 0)


def test_embedding_models_refuse_the_key():
    from llm_weighted_consensus_amd.models.lora import check_model_spec

    with pytest.raises(ValueError, match="mxfp4 weights are served on generation models only"):
        check_model_spec("m", dict(BASE, mxfp4=True, mxfp4_act="e4m3"), embedder=True)
    with pytest.raises(ValueError, match='^embedding model m: "mxfp4_act" needs "mxfp4": true$'):
        check_model_spec("m", dict(BASE, mxfp4_act="e4m3"), embedder=True)


def test_specs_that_pass():
    from llm_weighted_consensus_amd.models.lora import check_model_spec

    for act in ("e4m3", "bf16"):
        assert check_model_spec("m", dict(BASE, mxfp4=True, mxfp4_act=act)) == ()
    # without the key: what it returned before
    assert check_model_spec("m", BASE) == ()
    assert check_model_spec("m", dict(BASE, mxfp4=True)) == ()
    assert check_model_spec("m", dict(BASE, adapters=ADS)) == ("a",)
    with pytest.raises(ValueError, match="^model m: mxfp4 weights do not combine with fp8 weights$"):
        check_model_spec("m", dict(BASE, mxfp4=True, fp8=True))


def test_constructor_refusals():
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    cfg = decoder_config("llama-tiny")
    with pytest.raises(ValueError, match="^mxfp4_act needs mxfp4=True$"):
        LlamaModel(cfg, device="cpu", mxfp4_act="e4m3")
    with pytest.raises(ValueError, match="^mxfp4_act 'int8': must be one of 'bf16', 'e4m3'$"):
        LlamaModel(cfg, device="cpu", mxfp4=True, mxfp4_act="int8")
    with pytest.raises(ValueError, match="^mxfp4 weights do not combine with fp8 weights$"):
        LlamaModel(cfg, device="cpu", mxfp4=True, mxfp4_act="e4m3", fp8_dense=True)
    with pytest.raises(ValueError, match="^mxfp4 weights do not combine with LoRA adapters$"):
        LlamaModel(cfg, device="cpu", mxfp4=True, mxfp4_act="e4m3", lora=[])
    with pytest.raises(ValueError, match="mxfp4 weights are not supported on MoE"):
        LlamaModel(decoder_config("mixtral-tiny"), device="cpu", mxfp4=True, mxfp4_act="e4m3")


def test_act_format_has_a_class_level_default():
    """An object that never ran the constructor (the fact dicts of tests/test_layer_paths.py) is the bf16-activation
    model."""
    from llm_weighted_consensus_amd.models.llama import LlamaModel
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.tp import TPLlamaModel

    for cls in (LlamaModel, MixtralModel, TPLlamaModel):
        assert cls.act_format == "bf16"
        m = cls.__new__(cls)
        assert m.act_format == "bf16" and "act_format" not in vars(m)


def test_threshold_and_shape_predicate():
    from llm_weighted_consensus_amd import ops

    assert ops.MXFP4_A8_MIN_ROWS == 65
    assert ops.mxfp4_a8_ok(1, 16, 128) and ops.mxfp4_a8_ok(300, 1040, 384) and ops.mxfp4_a8_ok(1 << 20, 6144, 4096)
    assert not ops.mxfp4_a8_ok(0, 16, 128) and not ops.mxfp4_a8_ok(65, 24, 128) and not ops.mxfp4_a8_ok(65, 16, 192)
    assert not ops.mxfp4_a8_ok(65, 16, 0)
    assert ops.mxfp4_a8_ok(65, 64, 128, swiglu=True) and not ops.mxfp4_a8_ok(65, 96, 128, swiglu=True)


def test_cpu_model_with_the_flag_is_the_cpu_mxfp4_model():
    """On a CPU device the flag is accepted and changes nothing: bf16 activations on the dequantised weights."""
    from llm_weighted_consensus_amd.models.config import decoder_config
    from llm_weighted_consensus_amd.models.llama import LlamaModel

    cfg = decoder_config("llama-tiny")
    a = LlamaModel(cfg, device="cpu", max_position=128, seed=4, mxfp4=True, mxfp4_act="e4m3")
    b = LlamaModel(cfg, device="cpu", max_position=128, seed=4, mxfp4=True)
    c = LlamaModel(cfg, device="cpu", max_position=128, seed=4, mxfp4=True, mxfp4_act="bf16")
    assert a.weight_format == b.weight_format == "mxfp4" and a.mxfp4
    assert a.act_format == b.act_format == c.act_format == "bf16" and a.mx_scratch is None
    for La, Lb in zip(a.layers, b.layers):
        for n in ("wqkv", "wo", "w_gate_up", "w_down"):
            assert torch.equal(getattr(La, n), getattr(Lb, n))
    toks = torch.randint(0, cfg.vocab_size, (70,), generator=torch.Generator().manual_seed(1))  # (past 64 rows)
    want = ref.llama_forward(b, toks)
    assert torch.equal(ref.llama_forward(a, toks), want) and torch.equal(ref.llama_forward(c, toks), want)
