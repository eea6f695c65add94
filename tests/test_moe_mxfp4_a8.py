"""MXFP4 MoE experts with e4m3 activations (``"expert_act": "e4m3"``), without a GPU: the spec key, its refusals and
their precedence behind the ``expert_weights`` ones, the CPU model, and the route as a function of (rows, E, ok)."""
import pytest
import torch

from tests import qwen_moe_ref
from tests import torch_ref as ref

ADS = {"a": {"weights": "random:7"}}
NEEDS_SPEC = r'"expert_act" needs "expert_weights": "mxfp4"'
NEEDS_CTOR = r'expert_act needs expert_weights="mxfp4"'
ONE_OF = "expert_act 'x': must be one of 'bf16', 'e4m3'"


def _cfg(name):
    from llm_weighted_consensus_amd.models.config import decoder_config

    return decoder_config(name)


# ------------------------------------------------------------------ spec key and refusals
@pytest.mark.parametrize("spec,embedder,msg", [
    # the key without MXFP4 experts, whatever its value
    ({"expert_act": "e4m3"}, False, NEEDS_SPEC),
    ({"expert_act": "bf16"}, False, NEEDS_SPEC),
    ({"expert_act": "x"}, False, NEEDS_SPEC),
    ({"expert_act": "e4m3", "expert_weights": "bf16"}, False, NEEDS_SPEC),
    ({"expert_act": "e4m3", "fp8": True}, False, NEEDS_SPEC),
    ({"expert_act": "e4m3", "arch": "llama-tiny", "mxfp4": True}, False, NEEDS_SPEC),
    ({"expert_act": "e4m3"}, True, NEEDS_SPEC),
    # a value outside the two
    ({"expert_act": "x", "expert_weights": "mxfp4"}, False, ONE_OF),
    ({"expert_act": "fp8", "expert_weights": "mxfp4"}, False, "expert_act 'fp8': must be one of 'bf16', 'e4m3'"),
    # whatever expert_weights refuses is refused first, in today's words
    ({"expert_act": "e4m3", "expert_weights": "fp4"}, False, "expert_weights 'fp4': must be one of 'bf16', 'mxfp4'"),
    ({"expert_act": "e4m3", "expert_weights": "mxfp4", "arch": "llama-tiny"}, False,
     r"expert_weights applies to MoE decoders only \(llama-tiny"),
    ({"expert_act": "x", "expert_weights": "mxfp4", "fp8": True}, False,
     "mxfp4 expert weights do not combine with fp8 weights"),
    ({"expert_act": "e4m3", "expert_weights": "mxfp4", "tp": 2}, False,
     "mxfp4 expert weights do not combine with tp > 1"),
    ({"expert_act": "x", "expert_weights": "mxfp4", "adapters": ADS}, False,
     "mxfp4 expert weights do not combine with LoRA adapters"),
    ({"expert_act": "e4m3", "expert_weights": "mxfp4"}, True,
     "mxfp4 expert weights are served on generation models only"),
    # the dense flag on a MoE arch keeps its words behind an accepted pair
    ({"expert_act": "e4m3", "expert_weights": "mxfp4", "mxfp4": True}, False,
     r"mxfp4 weights are not supported on MoE decoders \(mixtral-tiny\)"),
])
def test_spec_refusals(spec, embedder, msg):
    from llm_weighted_consensus_amd.models.lora import check_model_spec

    spec = {"arch": "mixtral-tiny", "weights": "random:0", **spec}
    who = f"^{'embedding ' if embedder else ''}model m: "
    with pytest.raises(ValueError, match=who + msg):
        check_model_spec("m", spec, embedder=embedder)
    # the factories refuse before they touch a device or a weight
    if embedder:
        from llm_weighted_consensus_amd.embeddings.service import build_embedding_service

        with pytest.raises(ValueError, match=msg):
            build_embedding_service("m", spec, "cpu")
    else:
        from llm_weighted_consensus_amd.engine.group import build_engine

        with pytest.raises(ValueError, match=f"^model {spec['arch']}: " + msg):
            build_engine(spec, 0)


def test_check_variant_refusals_without_a_spec():
    """A constructor's call has no ``who``: its own words, in the same order."""
    from llm_weighted_consensus_amd.models.config import EXPERT_ACTS, check_variant

    assert EXPERT_ACTS == ("bf16", "e4m3")
    cfg = _cfg("qwen3-moe-tiny")
    for kw, msg in (({"expert_act": "e4m3"}, "^" + NEEDS_CTOR + "$"),
                    ({"expert_act": "x"}, "^" + NEEDS_CTOR + "$"),
                    ({"expert_act": "e4m3", "expert_weights": "bf16"}, "^" + NEEDS_CTOR + "$"),
                    ({"expert_act": "x", "expert_weights": "mxfp4"}, "^" + ONE_OF + "$"),
                    ({"expert_act": "e4m3", "expert_weights": "int4"}, "^expert_weights 'int4': must be one of"),
                    ({"expert_act": "x", "expert_weights": "mxfp4", "fp8": True},
                     "^mxfp4 expert weights do not combine with fp8 weights$"),
                    ({"expert_act": "x", "expert_weights": "mxfp4", "tp": True},
                     r"^mxfp4 expert weights do not combine with tensor parallelism \(tp > 1\)$"),
                    ({"expert_act": "x", "expert_weights": "mxfp4", "ep": True},
                     r"^mxfp4 expert weights do not combine with expert parallelism \(ep > 1\)$"),
                    ({"expert_act": "x", "expert_weights": "mxfp4", "adapters": True},
                     "^mxfp4 expert weights do not combine with LoRA adapters$"),
                    ({"expert_act": "e4m3", "expert_weights": "mxfp4", "embedder": True},
                     "^mxfp4 expert weights are served on generation models only$")):
        with pytest.raises(ValueError, match=msg):
            check_variant(cfg, **kw)
    with pytest.raises(ValueError, match="^model v: " + NEEDS_SPEC + "$"):
        check_variant(cfg, expert_act="e4m3", who="model v")
    with pytest.raises(ValueError, match=r"^expert_weights applies to MoE decoders only \(llama-tiny is dense\)$"):
        check_variant(_cfg("llama-tiny"), expert_act="e4m3", expert_weights="mxfp4")
    # not given, and the two values
    for act in (None, "bf16", "e4m3"):
        check_variant(cfg, expert_weights="mxfp4", expert_act=act)
    check_variant(cfg)


def test_spec_accepts_the_two_values():
    from llm_weighted_consensus_amd.models.lora import check_model_spec

    for arch in ("qwen3-moe-tiny", "mixtral-tiny", "qwen3-30b-a3b", "mixtral-8x7b"):
        for act in ("bf16", "e4m3"):
            spec = {"arch": arch, "weights": "random:0", "expert_weights": "mxfp4", "expert_act": act}
            assert check_model_spec("v", spec) == ()


def test_model_constructor_refusals():
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    for cls, arch in ((MixtralModel, "mixtral-tiny"), (Qwen3MoeModel, "qwen3-moe-tiny")):
        cfg = _cfg(arch)
        for kw, msg in (({"expert_act": "e4m3"}, "^" + NEEDS_CTOR + "$"),
                        ({"expert_act": "x"}, "^" + NEEDS_CTOR + "$"),
                        ({"expert_act": "e4m3", "fp8": True}, "^" + NEEDS_CTOR + "$"),
                        ({"expert_act": "x", "expert_weights": "mxfp4"}, "^" + ONE_OF + "$"),
                        ({"expert_act": "e4m3", "expert_weights": "int4"}, "^expert_weights 'int4': must be one of"),
                        ({"expert_act": "e4m3", "expert_weights": "mxfp4", "fp8": True},
                         "^mxfp4 expert weights do not combine with fp8"),
                        ({"expert_act": "e4m3", "expert_weights": "mxfp4", "mxfp4": True},
                         "^mxfp4 weights are not supported on MoE")):
            with pytest.raises(ValueError, match=msg):
                cls(cfg, device="cpu", **kw)
    with pytest.raises(ValueError, match="^mxfp4 expert weights do not combine with tensor par"):
        MixtralModel(_cfg("mixtral-tiny"), device="cpu", expert_weights="mxfp4", expert_act="x", tp_size=2)
    with pytest.raises(ValueError, match="^mxfp4 expert weights do not combine with expert par"):
        MixtralModel(_cfg("mixtral-tiny"), device="cpu", expert_weights="mxfp4", expert_act="e4m3", ep_size=2)


# ------------------------------------------------------------------ the CPU model
def _build(arch, **kw):
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.qwen_moe import Qwen3MoeModel

    cfg = _cfg(arch)
    return (Qwen3MoeModel if cfg.qk_norm else MixtralModel)(cfg, device="cpu", max_position=128, **kw)


@pytest.mark.parametrize("arch", ["qwen3-moe-tiny", "mixtral-tiny"])
def test_cpu_models_of_both_values_are_equal(arch):
    """On a CPU device the flag is accepted and the model computes on the dequantised bf16 experts: the tensors and
    the logits of ``"e4m3"`` are those of ``"bf16"``, and of the model built without the keyword."""
    a = _build(arch, seed=4, expert_weights="mxfp4", expert_act="e4m3")
    b = _build(arch, seed=4, expert_weights="mxfp4", expert_act="bf16")
    c = _build(arch, seed=4, expert_weights="mxfp4")
    assert (a.expert_act, b.expert_act, c.expert_act) == ("e4m3", "bf16", "bf16")
    assert a.moe_scratch is None and b.moe_scratch is None and a.graph_safe
    for L, M, N in zip(a.layers, b.layers, c.layers):
        assert L.w13.dtype == torch.bfloat16 and L.gu_block == M.gu_block == 0
        assert torch.equal(L.w13, M.w13) and torch.equal(L.w2, M.w2) and torch.equal(L.w13, N.w13)
    toks = torch.randint(0, a.cfg.vocab_size, (9,), generator=torch.Generator().manual_seed(1))
    oracle = qwen_moe_ref.qwen_moe_forward if a.cfg.qk_norm else ref.llama_forward
    want = oracle(b, toks)
    assert torch.equal(oracle(a, toks), want) and torch.equal(oracle(c, toks), want)


def test_default_is_the_model_without_the_key():
    m = _build("mixtral-tiny", seed=1)
    assert m.expert_act == "bf16" and m.expert_weights == "bf16"


# ------------------------------------------------------------------ the route
def test_route_is_a_function_of_rows_experts_and_ok():
    """Up to ``MOE_MXFP4_STREAM_AVG_ROWS`` routed rows per expert on average the weight stream, whatever ``ok`` says;
    past that the W4A8 kernel, or the dequantise path for a shape it does not take."""
    from llm_weighted_consensus_amd import ops

    lim = ops.MOE_MXFP4_STREAM_AVG_ROWS
    assert lim == 32
    for E in (1, 4, 8, 128):
        for ok in (True, False):
            for rows in (0, 1, lim * E - 1, lim * E):
                assert ops.moe_mxfp4_a8_route(rows, E, ok) == "stream"
        for rows in (lim * E + 1, 64 * E, 4096 * 8):
            assert ops.moe_mxfp4_a8_route(rows, E, True) == "a8"
            assert ops.moe_mxfp4_a8_route(rows, E, False) == "dequant"
    # the tiny archs' natural thresholds: T * k routed rows
    assert ops.moe_mxfp4_a8_route(512 * 8, 128, True) == "stream" and ops.moe_mxfp4_a8_route(513 * 8, 128, True) == "a8"
    assert ops.moe_mxfp4_a8_route(64 * 2, 4, True) == "stream" and ops.moe_mxfp4_a8_route(65 * 2, 4, True) == "a8"


def test_shape_rule_never_raises():
    from llm_weighted_consensus_amd import ops

    class W:  # (the rule reads the stack's shape alone)
        def __init__(self, *shape):
            self.shape = shape

    ok = ops.moe_mxfp4_a8_ok
    assert ok(4096, 2048, 32768, W(128, 1536, 2048), swiglu=True) and ok(32768, 768, 32768, W(128, 2048, 768))
    assert ok(8192, 4096, 16384, W(8, 28672, 4096), swiglu=True) and ok(16384, 14336, 16384, W(8, 4096, 14336))
    assert ok(1, 7, 1, W(2, 16, 128))                     # a single row's stride is arbitrary
    assert ok(0, 128, 0, W(2, 16, 128))
    assert not ok(4, 160, 4, W(2, 16, 160))               # K % 128
    assert not ok(4, 128, 4, W(2, 24, 128))               # N % 16
    assert ok(4, 128, 4, W(2, 32, 128)) and not ok(4, 128, 4, W(2, 32, 128), swiglu=True)  # SwiGLU: N % 64
    assert not ok(4, 136, 4, W(2, 16, 128))               # lda % 16
    assert not ok(4, 112, 4, W(2, 16, 128))               # lda < K
    assert not ok(4, 128, 4, W(0, 16, 128))               # E >= 1
    assert not ok(4, 128, -1, W(2, 16, 128)) and not ok(4, 128, 1 << 31, W(2, 16, 128))
    assert ok(4, 128, (1 << 31) - 1, W(2, 16, 128))       # 2^24 + 2 slots x 8
    assert not ok(4, 128, (1 << 31) - 1, W(2, 128 * 128, 128))  # x 128 n-tiles: a grid past 2^31 - 1
    assert not ok(4, 128, 4, None) and not ok("a", 128, 4, W(2, 16, 128)) and not ok(4, 128, 4, W(2, 16))
