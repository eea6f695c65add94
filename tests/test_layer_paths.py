"""The kernel sequence of LlamaModel._layers for every decoder variant, and the refusals of the variants that do
not combine, on the CPU.

The sequences: ``_layers`` runs on a two-layer fake whose ``ops`` / ``gemm_plan`` are a recorder
(tests/op_recorder.py); the exact list of (op, sorted keyword names) is compared with a list written out here.
The lists were recorded from the four-branch ``_layers`` that preceded the single layer body, and they are the
same with and without ``keep`` (the row selection launches nothing): with ``keep``, every call after the last
layer's RoPE / KV write must see the kept rows only."""
import pytest
import torch

from llm_weighted_consensus_amd.models import llama
from tests.op_recorder import Recorder

T, KEEP = 3, [1]  # rows of the step, rows kept


def facts(on_gpu: bool, weight_format: str) -> dict:
    """The stated variant of a fake model (LlamaModel.__init__ sets these on a real one)."""
    return {"on_gpu": on_gpu, "weight_format": weight_format, "moe": False, "g8_ws": object() if on_gpu else None}


def _lora(none_at: str, adapts_gate_up: bool):
    x = torch.zeros(1, 1)
    per_layer = {p: None if p == none_at else x for p in ("qkv", "o", "gate_up", "down")}
    return type("Lora", (), {"A": [per_layer] * 2, "B": [per_layer] * 2, "adapts_gate_up": adapts_gate_up})()


def trace(variant: str, keep: bool):
    """-> (calls as "op(kw,kw)", first-argument row count of every call, (name, kwargs) log)."""
    log, rows = [], []

    def ret(name, a, kw):
        rows.append(a[0].shape[0])
        return torch.zeros(a[0].shape[0], 1)

    rec = Recorder(log, ret)

    class Reduced(llama.LlamaModel):  # as the tensor-parallel decoder: both projections reduced across ranks
        single_rank_dense = False

        def _attn_out(self, attn, L):
            return rec.all_reduce(llama.LlamaModel._attn_out(self, attn, L))

        def _mlp(self, h, L):
            return rec.all_reduce(llama.LlamaModel._mlp(self, h, L))

    class RoutedMlp(llama.LlamaModel):  # as the MoE decoder: its MLP reads the bf16 rows too, from its own weights
        single_rank_dense = False
        _mlp_reads_bf16 = True

        def _mlp(self, h, L):
            return rec.experts(h)

    cls = {"tp": Reduced, "fp8-bf16-rows": RoutedMlp}.get(variant, llama.LlamaModel)
    fp8 = variant.startswith("fp8")
    w = rec.Fp8Weight() if fp8 else torch.zeros(1, 1)
    x = torch.zeros(1, 1)
    extras = {"bqkv": x if variant == "qkv-bias" else None, "q_norm": None, "k_norm": None}
    m = cls.__new__(cls)
    m.cfg = type("Cfg", (), {"heads": 1, "kv_heads": 1, "head_dim": 1, "hidden": 1, "rms_eps": 1e-5})()
    dense = {} if cls is RoutedMlp else {"w_gate_up": w, "w_down": w}  # (a MoE layer has neither)
    m.layers = [type("L", (), dict({"wqkv": w, "wo": w, "gu_block": 32, "attn_norm": x, "mlp_norm": x}, **dense,
                                   **extras))() for _ in range(2)]
    for k, v in facts(True, "fp8" if fp8 else "bf16").items():
        setattr(m, k, v)
    m.final_norm, m.cos, m.sin, m.mx_scratch = x, x, x, None
    m.lora = {"lora-gate-up": _lora("o", True), "lora-no-gate-up": _lora("gate_up", False)}.get(variant)
    ids = torch.zeros(T, dtype=torch.int32) if m.lora is not None else None
    cache = type("Cache", (), {"k": [x] * 2, "v": [x] * 2})()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(llama, "ops", rec)
        mp.setattr(llama, "gemm_plan", rec)
        h = m._layers(torch.zeros(T, 1), cache, None, None, lambda qkv, li: torch.zeros(T, 1, 1),
                      keep=torch.tensor(KEEP) if keep else None, lora_ids=ids)
    assert h.shape[0] == (len(KEEP) if keep else T)
    return [f"{name}({','.join(sorted(kw))})" for name, kw in log], rows, log


DENSE_LAYER = ["linear(ws)", "rope_kv_write(rope_q,slots)", "linear_add_(ws)", "rmsnorm()", "swiglu(ws)",
               "linear_add_(ws)", "rmsnorm()"]
SHRINK_EXPAND = ["lora_shrink()", "lora_expand_add_()"]
FP8_ATTN = ["linear_fp8()", "rope_kv_write(rope_q,slots)", "linear_fp8()", "rmsnorm_quant_fp8(keep_bf16,residual)"]
FP8_LAYER = FP8_ATTN + ["linear_fp8_swiglu()", "linear_fp8_q()"]
TP_LAYER = ["linear(ws)", "rope_kv_write(rope_q,slots)", "linear(ws)", "all_reduce()", "rmsnorm(residual)",
            "swiglu(ws)", "linear(ws)", "all_reduce()", "rmsnorm(residual)"]
EXPECTED = {
    "dense": ["rmsnorm()"] + DENSE_LAYER * 2,
    # no adapter targets o: nothing is launched for it
    "lora-gate-up": ["rmsnorm()"] + (
        ["linear(ws)"] + SHRINK_EXPAND + ["rope_kv_write(rope_q,slots)", "linear_add_(ws)", "rmsnorm()", "linear(ws)"]
        + SHRINK_EXPAND + ["silu_mul(block)", "linear_add_(ws)"] + SHRINK_EXPAND + ["rmsnorm()"]) * 2,
    "lora-no-gate-up": ["rmsnorm()"] + (
        ["linear(ws)"] + SHRINK_EXPAND + ["rope_kv_write(rope_q,slots)", "linear_add_(ws)"] + SHRINK_EXPAND
        + ["rmsnorm()", "swiglu(ws)", "linear_add_(ws)"] + SHRINK_EXPAND + ["rmsnorm()"]) * 2,
    # the last norm feeds the bf16 lm_head / pooling: the bf16 kernel
    "fp8": ["rmsnorm_quant_fp8()"] + FP8_LAYER + ["rmsnorm_quant_fp8(residual)"] + FP8_LAYER + ["rmsnorm(residual)"],
    "fp8-bf16-rows": ["rmsnorm_quant_fp8()"] + FP8_ATTN + ["experts()", "rmsnorm_quant_fp8(residual)"] + FP8_ATTN
    + ["experts()", "rmsnorm(residual)"],
    "tp": ["rmsnorm()"] + TP_LAYER * 2,
    "qkv-bias": ["rmsnorm()"] + [c if not c.startswith("rope_kv_write") else
                                 "qknorm_rope_kv_write(bias,eps,k_weight,q_weight,rope_q,slots)"
                                 for c in DENSE_LAYER] * 2,
}


@pytest.mark.parametrize("keep", [False, True], ids=["all-rows", "keep"])
@pytest.mark.parametrize("variant", list(EXPECTED))
def test_layers_launch_the_recorded_sequence(variant, keep):
    calls, rows, log = trace(variant, keep)
    assert calls == EXPECTED[variant]
    names = [name for name, _ in log]
    if keep:  # the last layer's tail runs after the row selection
        cut = max(i for i, n in enumerate(names) if n.endswith("rope_kv_write")) + 1
        assert rows == [T] * cut + [len(KEEP)] * (len(rows) - cut) and len(rows) > cut
    else:
        assert set(rows) == {T}
    if variant == "qkv-bias":
        assert "rope_kv_write" not in names and names.count("qknorm_rope_kv_write") == 2
    if variant == "tp":  # one all-reduce after o and one after down, per layer
        assert [names[i - 1] for i, n in enumerate(names) if n == "all_reduce"] == ["linear", "linear"] * 2
    if variant.startswith("fp8"):
        # every norm but the last quantises; keep_bf16 is the MLP norm's alone, true where _mlp reads bf16 rows
        norms = [(n, kw) for n, kw in log if "norm" in n and "rope" not in n]
        assert [n for n, _ in norms] == ["rmsnorm_quant_fp8"] * 4 + ["rmsnorm"]
        assert [kw.get("keep_bf16") for _, kw in norms] == [None, variant == "fp8-bf16-rows"] * 2 + [None]


def test_lora_on_an_unfused_path_is_an_error():
    m = llama.LlamaModel.__new__(llama.LlamaModel)
    for k, v in facts(False, "bf16").items():
        setattr(m, k, v)
    m.cfg = type("Cfg", (), {"heads": 1, "kv_heads": 1, "head_dim": 1})()
    m.layers, m.lora = [], _lora("o", True)
    with pytest.raises(RuntimeError, match="fused-residual"):
        m._layers(torch.zeros(T, 1), None, None, None, None, lora_ids=torch.zeros(T, dtype=torch.int32))


# ------------------------------------------------------------------ refusals: one function, five entry points
def _entry(point: str, arch: str = "llama-tiny", embedder: bool = False, **kw):
    """Call one entry point with a variant: the three constructors (CPU), lora.check_model_spec and the
    embedding service's factory (spec keys: tp / fp8 / mxfp4 / adapters)."""
    from llm_weighted_consensus_amd.models.config import decoder_config

    if point in ("spec", "service"):
        spec = dict({"arch": arch, "weights": "random:0"}, **kw)
        if point == "service":
            from llm_weighted_consensus_amd.embeddings.service import build_embedding_service

            return build_embedding_service("m", spec, "cpu")
        from llm_weighted_consensus_amd.models.lora import check_model_spec

        return check_model_spec("m", spec, embedder=embedder)
    from llm_weighted_consensus_amd.models.mixtral import MixtralModel
    from llm_weighted_consensus_amd.models.tp import TPLlamaModel

    cls = {"LlamaModel": llama.LlamaModel, "TPLlamaModel": TPLlamaModel, "MixtralModel": MixtralModel}[point]
    return cls(decoder_config(arch), device="cpu", **kw)


ADS = {"a": {"weights": "random:7"}}
MOE = "mixtral-tiny"
# (combination, entry point, its arguments, what the message names): every entry point that can state the
# combination (TPLlamaModel and MixtralModel take no adapters; LlamaModel has no tp; the service embeds only)
REFUSED = [
    ("mxfp4+fp8", "LlamaModel", dict(mxfp4=True, fp8_dense=True), "mxfp4 weights do not combine with fp8"),
    ("mxfp4+fp8", "TPLlamaModel", dict(mxfp4=True, fp8_dense=True, tp_size=2), "mxfp4 weights do not combine"),
    ("mxfp4+fp8", "MixtralModel", dict(arch=MOE, mxfp4=True, fp8=True), "mxfp4 weights do not combine with fp8"),
    ("mxfp4+fp8", "spec", dict(mxfp4=True, fp8=True), "mxfp4 weights do not combine with fp8"),
    ("mxfp4+tp", "TPLlamaModel", dict(mxfp4=True, tp_size=2), "mxfp4 weights do not combine with tensor parallelism"),
    ("mxfp4+tp", "MixtralModel", dict(arch=MOE, mxfp4=True, tp_size=2),
     "mxfp4 weights do not combine with tensor parallelism"),
    ("mxfp4+tp", "spec", dict(mxfp4=True, tp=2), "mxfp4 weights do not combine with tp > 1"),
    ("mxfp4+lora", "LlamaModel", dict(mxfp4=True, lora=[]), "mxfp4 weights do not combine with LoRA"),
    ("mxfp4+lora", "spec", dict(mxfp4=True, adapters=ADS), "mxfp4 weights do not combine with LoRA"),
    ("mxfp4+moe", "LlamaModel", dict(arch=MOE, mxfp4=True), "mxfp4 weights are not supported on MoE"),
    ("mxfp4+moe", "TPLlamaModel", dict(arch=MOE, mxfp4=True, tp_size=2), "mxfp4 weights do not combine with tensor"),
    ("mxfp4+moe", "MixtralModel", dict(arch=MOE, mxfp4=True), "mxfp4 weights are not supported on MoE"),
    ("mxfp4+moe", "spec", dict(arch=MOE, mxfp4=True), "mxfp4 weights are not supported on MoE"),
    ("mxfp4+embedder", "spec", dict(embedder=True, mxfp4=True), "mxfp4 weights are served on generation models only"),
    ("mxfp4+embedder", "service", dict(mxfp4=True), "mxfp4 weights are served on generation models only"),
    ("lora+tp", "spec", dict(adapters=ADS, tp=2), "LoRA adapters do not combine with tp > 1"),
    ("lora+fp8", "LlamaModel", dict(lora=[], fp8_dense=True), "LoRA adapters do not combine with fp8"),
    ("lora+fp8", "spec", dict(adapters=ADS, fp8=True), "LoRA adapters do not combine with fp8"),
    ("lora+moe", "LlamaModel", dict(arch=MOE, lora=[]), "LoRA adapters are not supported on MoE"),
    ("lora+moe", "spec", dict(arch=MOE, adapters=ADS), "LoRA adapters are not supported on MoE"),
    ("lora+embedder", "spec", dict(embedder=True, adapters=ADS), "LoRA adapters are served on generation models only"),
    ("lora+embedder", "service", dict(adapters=ADS), "LoRA adapters are served on generation models only"),
    ("lora+cpu", "LlamaModel", dict(lora=[]), "LoRA adapters run on the GPU kernels only"),
]


@pytest.mark.parametrize("combo,point,kw,msg", REFUSED, ids=[f"{c}-{p}" for c, p, _, _ in REFUSED])
def test_refused_combinations_raise_from_the_one_function(combo, point, kw, msg):
    with pytest.raises(ValueError, match=msg) as e:
        _entry(point, **kw)
    assert e.traceback[-1].name == "check_variant"  # raised there, whichever entry point was called
    assert str(e.value).startswith(("model m: ", "embedding model m: ")) == (point in ("spec", "service"))
