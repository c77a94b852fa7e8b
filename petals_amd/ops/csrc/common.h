// Shared device helpers for petals_amd CDNA4 (gfx950) kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#define WAVE 64

using short8 = __attribute__((ext_vector_type(8))) short;
using float4v = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float bf16_to_f32(unsigned short u) {
  union { float f; uint32_t i; } v;
  v.i = uint32_t(u) << 16;
  return v.f;
}

__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
  union { float f; uint32_t i; } v;
  v.f = f;
  uint32_t lsb = (v.i >> 16) & 1;            // round-to-nearest-even
  uint32_t r = (v.i + 0x7FFFu + lsb) >> 16;
  return (unsigned short)r;
}

// ---- OCP E4M3 (torch.float8_e4m3fn) KV-cache elements, no scales.
// f32 -> e4m3: finite values clamp to +-448 (v_med3_f32), then round to
// nearest even (v_cvt_pk_fp8_f32); NaN stays NaN (code 0x7F). The NaN test is
// on the bits because the extension is built with -ffast-math.
__device__ __forceinline__ float e4m3_clamp(float f) {
  return __builtin_amdgcn_fmed3f(f, -448.f, 448.f);
}

__device__ __forceinline__ unsigned char f32_to_e4m3(float f) {
  union { float f; uint32_t i; } v;
  v.f = f;
  if ((v.i & 0x7FFFFFFFu) > 0x7F800000u) return 0x7F;
  const float c = e4m3_clamp(f);
  return (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(c, c, 0, false) & 0xFF);
}

// 8 e4m3 bytes -> the same 8 values as bf16 (exact: every finite e4m3 code is
// bf16-representable), element i from byte i; v_cvt_scalef32_pk_bf16_fp8 at
// scale 1.0 converts two bytes per instruction
__device__ __forceinline__ short8 e4m3x8_to_bf16x8(uint2 w) {
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
  const u32x4 r = {
      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w.x, 1.0f, false)),
      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w.x, 1.0f, true)),
      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w.y, 1.0f, false)),
      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w.y, 1.0f, true))};
  return __builtin_bit_cast(short8, r);
}

// f32 -> KV-cache element, by the cache element type: unsigned short holds
// bf16, unsigned char holds e4m3
template <typename CT> __device__ __forceinline__ CT f32_to_kv(float f);
template <> __device__ __forceinline__ unsigned short f32_to_kv<unsigned short>(float f) { return f32_to_bf16(f); }
template <> __device__ __forceinline__ unsigned char f32_to_kv<unsigned char>(float f) { return f32_to_e4m3(f); }

// full-wave fp32 sum (64 lanes)
__device__ __forceinline__ float wave_reduce_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

__device__ __forceinline__ float wave_reduce_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, WAVE));
  return x;
}

#define HIP_CHECK_LAST()                                                     \
  do {                                                                       \
    hipError_t e = hipGetLastError();                                        \
    if (e != hipSuccess) {                                                   \
      TORCH_CHECK(false, "HIP kernel launch failed: ", hipGetErrorString(e)); \
    }                                                                        \
  } while (0)

// finite stand-ins for -inf: the extension compiles with -ffast-math, under
// which IEEE inf comparisons/arithmetic are not reliable
#define NEG_SENTINEL  (-1e30f)
#define NEG_THRESHOLD (-1e29f)
