"""Reference for the opt-in FP8 KV cache: OCP E4M3 (`torch.float8_e4m3fn`).

The format is normative for the HIP kernels (attention.hip, prefill_attn.hip,
elementwise.hip) and runs on the CPU in plain torch:

* cache tensors keep their shape `[Bc, KV, Lmax, hd]`, dtype float8_e4m3fn
  (the OCP encoding gfx950 implements, never `fnuz`);
* there are no scales: a value is stored as itself;
* `quantize` clamps finite values to +-448 and rounds to nearest even. A bare
  `x.to(torch.float8_e4m3fn)` is NOT this: torch turns 500.0 into NaN. NaN
  stays NaN; values that round to zero become 0 (smallest nonzero magnitude
  2^-9, and 2^-10 ties to 0);
* `dequantize` is exact into bf16 or fp32: all 254 finite codes are
  bf16-representable, which is why the kernels' fp8 instantiations are
  bit-identical to the bf16 ones run on the dequantized cache.
"""

from __future__ import annotations

import torch

DTYPE = torch.float8_e4m3fn
E4M3_MAX = 448.0

_CACHE_DTYPES = {"bf16": torch.bfloat16, "fp8": DTYPE}


def cache_dtype(name: str) -> torch.dtype:
    """`bf16` | `fp8` (the Server / CLI spelling) -> torch dtype."""
    try:
        return _CACHE_DTYPES[name]
    except KeyError:
        raise ValueError(f"kv_cache_dtype={name!r}: expected one of {', '.join(_CACHE_DTYPES)}") from None


def cache_dtype_name(dtype: torch.dtype) -> str:
    for name, dt in _CACHE_DTYPES.items():
        if dt == dtype:
            return name
    raise ValueError(f"unsupported kv cache dtype {dtype}")


def is_fp8(t: torch.Tensor) -> bool:
    return t.dtype == DTYPE


def quantize(x: torch.Tensor) -> torch.Tensor:
    """Saturating round-to-nearest-even cast to float8_e4m3fn (NaN kept)."""
    x32 = x.to(torch.float32)
    # clamp propagates NaN; +-inf saturate like any other overflow
    return x32.clamp(-E4M3_MAX, E4M3_MAX).to(DTYPE)


def dequantize(c: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Exact for bf16 / fp32 / fp64 targets."""
    assert c.dtype == DTYPE, c.dtype
    return c.to(dtype)


def roundtrip(x: torch.Tensor) -> torch.Tensor:
    """`x` as a kernel reading the fp8 cache sees it, in x's dtype."""
    return dequantize(quantize(x), torch.float32).to(x.dtype)


def spacing(x: torch.Tensor) -> torch.Tensor:
    """Distance between neighbouring E4M3 values around |x| (float64): 2^-9 in
    the subnormal range, 2^(floor(log2|x|) - 3) above it, 32 at the top
    binade (and beyond it, where values saturate)."""
    a = x.to(torch.float64).abs().clamp(2.0**-6, E4M3_MAX)
    return torch.exp2(torch.floor(torch.log2(a)) - 3)


def index_rows(cache: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """cache[idx] along dim 0, byte-exact for fp8 (gathered through a uint8
    view: indexing kernels are not defined for float8 on every device)."""
    if is_fp8(cache):
        return cache.view(torch.uint8)[idx].view(DTYPE)
    return cache[idx]
