"""CPU/torch reference for the MXFP4 format (numerics baseline for mxfp4.hip).

Format (OCP Microscaling v1.0, laid out for the transposed [in, out] weights
the kernels stream): E2M1 elements with one E8M0 power-of-two scale per 32
elements along `in`, per output column.

  packed u8 [in/2, out]: byte (j, o) holds column o of rows 2j (low nibble)
      and 2j+1 (high nibble). A nibble is sign (bit 3) + a 3-bit code; codes
      0..7 are the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6.
  scales u8 [in/32, out]: byte s means 2^(s-127), s in 1..254.

Blocks run along `in`, so column permutations and concatenations commute
with quantization.
"""

from __future__ import annotations

from typing import Tuple

import torch

BLOCK = 32
E2M1_LEVELS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def check_shape(in_dim: int, out_dim: int) -> None:
    if in_dim <= 0 or out_dim <= 0 or in_dim % BLOCK != 0 or out_dim % 8 != 0:
        raise ValueError(
            f"MXFP4 needs in % 32 == 0 and out % 8 == 0, got a weight of shape [{in_dim}, {out_dim}]"
        )


def _codes(q: torch.Tensor) -> torch.Tensor:
    """|v| / 2^e -> nearest E2M1 code, ties to the even code, saturating at 6."""
    return (
        (q > 0.25).to(torch.uint8)
        + (q >= 0.75).to(torch.uint8)
        + (q > 1.25).to(torch.uint8)
        + (q >= 1.75).to(torch.uint8)
        + (q > 2.5).to(torch.uint8)
        + (q >= 3.5).to(torch.uint8)
        + (q > 5.0).to(torch.uint8)
    )


def quantize(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w: [in, out] (any float dtype) -> (packed u8 [in/2, out], scales u8 [in/32, out]).

    Per column and 32-row block: e = floor(log2(amax)) - 2 clamped to
    [-126, 127], s = e + 127; an all-zero block gets s = 127. A value that
    rounds to zero is stored as code 0 without a sign."""
    assert w.dim() == 2
    in_dim, out_dim = w.shape
    check_shape(in_dim, out_dim)
    blocks = w.detach().to("cpu", torch.float64).reshape(in_dim // BLOCK, BLOCK, out_dim)
    amax = blocks.abs().amax(dim=1)  # [in/32, out]
    _, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    e = torch.where(amax > 0, ex.to(torch.int64) - 3, torch.zeros_like(ex, dtype=torch.int64))
    e = e.clamp(-126, 127)
    q = torch.ldexp(blocks.abs(), (-e).unsqueeze(1).expand_as(blocks))
    code = _codes(q)
    sign = ((blocks < 0) & (code > 0)).to(torch.uint8) << 3
    nib = (code | sign).reshape(in_dim, out_dim)
    packed = (nib[0::2] | (nib[1::2] << 4)).contiguous()
    scales = (e + 127).to(torch.uint8).contiguous()
    return packed, scales


def dequantize(packed: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """(packed u8 [in/2, out], scales u8 [in/32, out]) -> [in, out] in `dtype`.

    Every representable value is exact in bf16 except the magnitudes 2, 3, 4
    and 6 at s = 254 (>= 2^128), which overflow it; float64 holds them all."""
    half, out_dim = packed.shape
    in_dim = half * 2
    assert scales.shape == (in_dim // BLOCK, out_dim), (packed.shape, scales.shape)
    p = packed.cpu()
    nib = torch.empty(in_dim, out_dim, dtype=torch.uint8)
    nib[0::2] = p & 0xF
    nib[1::2] = p >> 4
    mag = E2M1_LEVELS[(nib & 7).long()]
    mag = torch.where((nib & 8) != 0, -mag, mag)
    e = (scales.cpu().to(torch.int64) - 127).repeat_interleave(BLOCK, dim=0)
    return torch.ldexp(mag, e).to(dtype)


def from_ocp_blocks(blocks: torch.Tensor, scales: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Import the checkpoint layout: blocks u8 [out, in/32, 16] (K-contiguous,
    low nibble = even element) and scales u8 [out, in/32] -> (packed, scales)
    in this module's layout. A lossless byte transpose."""
    assert blocks.dtype == torch.uint8 and scales.dtype == torch.uint8
    assert blocks.dim() == 3 and blocks.shape[2] == BLOCK // 2 and scales.shape == blocks.shape[:2]
    out_dim, nblk, _ = blocks.shape
    check_shape(nblk * BLOCK, out_dim)
    bad = (scales == 0) | (scales == 255)
    if bool(bad.any()):
        raise ValueError(
            f"MXFP4 import: {int(bad.sum())} scale bytes are 0 or 255 (2^-127 and NaN are not supported)"
        )
    # byte b of a block holds elements 2b, 2b+1 of one column: already rows
    # (2j, 2j+1) of packed, so only the [out, in/2] -> [in/2, out] transpose remains
    packed = blocks.reshape(out_dim, nblk * (BLOCK // 2)).t().contiguous()
    return packed, scales.t().contiguous()
