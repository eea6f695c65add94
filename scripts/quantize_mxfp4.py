#!/usr/bin/env python
"""Write an MXFP4 weight-only checkpoint from a bf16 one: ``python scripts/quantize_mxfp4.py IN OUT``.

IN is a safetensors file or a directory of them in the HF Llama / Qwen layout; OUT is one safetensors file (or a
directory, which gets ``model.safetensors``).  Every decoder projection (q / k / v / o / gate / up / down) is
stored as uint8 ``<name>.weight`` [N, K / 2] (two e2m1 codes per byte) plus uint8 ``<name>.weight_scale``
[N, K / 32] (e8m0), the format of ``llm_weighted_consensus_amd/ops/mxfp4.py``; every other tensor (embedding,
lm_head, norms, biases) is copied.  ``LlamaModel(..., weights_path=OUT, mxfp4=True)`` and a server model spec
with ``"mxfp4": true`` load it without quantising again.  This is the project's own convention.
"""
from __future__ import annotations

import os
import re
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROJ = re.compile(r"^model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")


def quantize_state(sd: dict) -> dict:
    """The checkpoint's tensors with every decoder projection in MXFP4 (already quantised ones pass through)."""
    import torch

    from llm_weighted_consensus_amd.ops.mxfp4 import quant_mxfp4_weight

    out = {}
    for name, t in sd.items():
        if PROJ.match(name) and t.dtype != torch.uint8:
            q, s = quant_mxfp4_weight(t.to(torch.bfloat16))
            out[name], out[name + "_scale"] = q, s
        else:
            out[name] = t.contiguous()
    return out


def quantize_checkpoint(src: str, dst: str) -> str:
    """Quantise the checkpoint at ``src`` into ``dst``; returns the file written."""
    from safetensors.torch import load_file, save_file

    files = sorted(Path(src).glob("*.safetensors")) if Path(src).is_dir() else [Path(src)]
    if not files:
        raise ValueError(f"{src}: no safetensors file")
    sd = {}
    for f in files:
        sd.update(load_file(str(f), device="cpu"))
    out = Path(dst)
    if out.is_dir() or not out.suffix:
        out.mkdir(parents=True, exist_ok=True)
        out = out / "model.safetensors"
    save_file(quantize_state(sd), str(out))
    return str(out)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        print(__doc__.strip().splitlines()[0], file=sys.stderr)
        return 2
    print(quantize_checkpoint(argv[0], argv[1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
