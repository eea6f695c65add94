"""MXFP4 weight-only format: OCP e2m1 elements with one e8m0 scale per 32 (torch only; runs on any device).

A block is 32 consecutive k of one output row of ``W [N, K]`` (``K % 32 == 0``).
  * element: a 4-bit code, bit 3 the sign, bits 0-2 an index into ``{0, 0.5, 1, 1.5, 2, 3, 4, 6}``;
  * ``q`` uint8 ``[N, K / 2]``: byte j of a row holds k = 2j in its low nibble and k = 2j + 1 in its high nibble;
  * ``s`` uint8 ``[N, K / 32]``: an e8m0 byte, value ``2^(s - 127)``; 255 (NaN in e8m0) is never written.

Every e2m1 x 2^e value is a bf16, so the dequantised weight is a bf16 tensor and every bf16 kernel and fp32
oracle of the project applies to it unchanged.  The device kernels are in ``csrc/kernels/mxfp4.hip``.

Every byte from 0 to 254 is in: ``dequant_mxfp4`` is the law, and the device readers follow it on all 16 x 255
(code, byte) pairs, byte 0 (2^-127, bf16-subnormal values) and the ``inf`` of bytes 253 and 254 included
(``tests/test_mxw_probes_gpu.py``, measured on an MI355X).
"""
from __future__ import annotations

from typing import Tuple

import torch

BLOCK = 32
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_ROWS = 2048  # rows quantised at a time (bounds the fp32 temporaries of a 28672 x 4096 projection)


def _block_exp(amax: torch.Tensor) -> torch.Tensor:
    """The smallest integer e with amax / 2^e <= 6, clamped to [-127, 127], from amax's fp32 bits: amax = m 2^x
    with m in [0.5, 1) and 6 x 2^e = 0.75 x 2^(e + 3), so e = x - 3 for m <= 0.75 and x - 2 above."""
    bits = amax.contiguous().view(torch.int32)
    x = ((bits >> 23) & 0xFF) - 126
    e = x - 3 + ((bits & 0x7FFFFF) > 0x400000).to(torch.int32)
    return e.clamp_(-127, 127)


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for integer e in [-127, 127] (2^-127 is the fp32 subnormal 0x00400000)."""
    e = e.to(torch.int32)
    return torch.where(e > -127, (e + 127) << 23, torch.full_like(e, 0x00400000)).view(torch.float32)


def _quant_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    N, K = w.shape
    x = w.float().view(N, K // BLOCK, BLOCK)
    e = _block_exp(x.abs().amax(-1))
    # |w| / 2^e in two exact power-of-two steps (2^-e alone is not an fp32 for e = -127)
    h = torch.div(e, 2, rounding_mode="floor")
    a = x.abs() * _pow2(-h).unsqueeze(-1) * _pow2(h - e).unsqueeze(-1)
    # nearest grid value; at a midpoint the neighbour with the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1,
    # 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4)
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8)
            + (a >= 1.75).to(torch.uint8) + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
            + (a > 5.0).to(torch.uint8))
    code = code | (((x < 0) & (code != 0)).to(torch.uint8) << 3)  # a value that rounds to zero: code 0, never -0
    code = code.view(N, K // 2, 2)
    q = code[..., 0] | (code[..., 1] << 4)
    return q.contiguous(), (e + 127).to(torch.uint8).contiguous()


def quant_mxfp4_weight(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``w [N, K]`` (bf16; computed in fp32) -> ``(q [N, K / 2] uint8, s [N, K / 32] uint8)``.  Per block the scale
    exponent is the smallest e with amax / 2^e <= 6 (nothing saturates), clamped to [-127, 127]; an all-zero
    block gets s = 0 and codes 0; elements round to the nearest grid value, ties to the even code."""
    if w.dim() != 2 or w.shape[1] % BLOCK:
        raise ValueError(f"quant_mxfp4_weight: W {tuple(w.shape)} must be [N, K] with K % {BLOCK} == 0")
    N, K = w.shape
    q = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
    s = torch.empty(N, K // BLOCK, dtype=torch.uint8, device=w.device)
    for r in range(0, N, _ROWS):
        q[r:r + _ROWS], s[r:r + _ROWS] = _quant_rows(w[r:r + _ROWS])
    return q, s


def check_mxfp4(q: torch.Tensor, s: torch.Tensor, name: str = "weight") -> None:
    """ValueError (naming the tensor) unless ``q`` / ``s`` are one weight of this format."""
    if q.dtype != torch.uint8 or s.dtype != torch.uint8:
        raise ValueError(f"{name}: MXFP4 codes and scales are uint8, got {q.dtype} / {s.dtype}")
    if q.dim() != 2 or s.dim() != 2 or s.shape[0] != q.shape[0] or q.shape[1] != 16 * s.shape[1]:
        raise ValueError(f"{name}: codes {tuple(q.shape)} / scales {tuple(s.shape)} are not [N, K / 2] / [N, K / 32]")
    if bool((s == 255).any()):
        raise ValueError(f"{name}_scale: holds the e8m0 byte 255 (NaN), which this format never writes")


def dequant_mxfp4(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """``(q, s)`` -> the bf16 weight ``[N, K]``, exact."""
    check_mxfp4(q, s)
    N = q.shape[0]
    lut = torch.tensor(GRID + tuple(-v for v in GRID), dtype=torch.float32, device=q.device)
    out = torch.empty(N, q.shape[1] * 2, dtype=torch.bfloat16, device=q.device)
    for r in range(0, N, _ROWS):
        qq = q[r:r + _ROWS]
        code = torch.stack([qq & 0xF, qq >> 4], dim=-1).view(qq.shape[0], -1, BLOCK)
        v = lut[code.long()] * _pow2(s[r:r + _ROWS].to(torch.int32) - 127).unsqueeze(-1)
        out[r:r + _ROWS] = v.view(qq.shape[0], -1).to(torch.bfloat16)
    return out


class Mxfp4Weight:
    """A dense projection weight in MXFP4 (``q``, ``s`` as above, ``shape`` = (N, K)): built once at load time from
    the bf16 weight, or around the tensors of a pre-quantised checkpoint (:meth:`from_packed`).  The kernels read
    the external format as it is: nothing is repacked."""

    __slots__ = ("q", "s", "shape")

    def __init__(self, w: torch.Tensor):
        self.q, self.s = quant_mxfp4_weight(w)
        self.shape = tuple(w.shape)

    @classmethod
    def from_packed(cls, q: torch.Tensor, s: torch.Tensor, name: str = "weight") -> "Mxfp4Weight":
        check_mxfp4(q, s, name)
        self = cls.__new__(cls)
        self.q, self.s = q.contiguous(), s.contiguous()
        self.shape = (q.shape[0], q.shape[1] * 2)
        return self

    @property
    def nbytes(self) -> int:
        return self.q.numel() + self.s.numel()

    def dequant(self) -> torch.Tensor:
        return dequant_mxfp4(self.q, self.s)


class Mxfp4Experts:
    """A stack of E expert projection weights in MXFP4 (``shape`` = (E, N, K)): ``q`` uint8 ``[E, N, K / 2]`` and
    ``s`` uint8 ``[E, N, K / 32]``, each expert in the format above, contiguous.  Built from the bf16 stack one
    expert at a time; the grouped kernel (``csrc/kernels/moe_mxfp4.hip``) reads it as stored: nothing is
    repacked."""

    __slots__ = ("q", "s", "shape")

    def __init__(self, w: torch.Tensor):
        if w.dim() != 3 or w.shape[2] % BLOCK:
            raise ValueError(f"Mxfp4Experts: W {tuple(w.shape)} must be [E, N, K] with K % {BLOCK} == 0")
        E, N, K = w.shape
        self.q = torch.empty(E, N, K // 2, dtype=torch.uint8, device=w.device)
        self.s = torch.empty(E, N, K // BLOCK, dtype=torch.uint8, device=w.device)
        for e in range(E):
            self.q[e], self.s[e] = quant_mxfp4_weight(w[e])
        self.shape = (E, N, K)

    @property
    def nbytes(self) -> int:
        return self.q.numel() + self.s.numel()

    def expert(self, e: int) -> Mxfp4Weight:
        """Expert ``e`` as a dense weight: a view, no copy."""
        w = Mxfp4Weight.__new__(Mxfp4Weight)
        w.q, w.s, w.shape = self.q[e], self.s[e], self.shape[1:]
        return w

    def dequant(self) -> torch.Tensor:
        """The bf16 stack ``[E, N, K]``, exact."""
        return torch.stack([dequant_mxfp4(self.q[e], self.s[e]) for e in range(self.shape[0])])
