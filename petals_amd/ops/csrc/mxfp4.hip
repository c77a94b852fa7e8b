// MXFP4 weights for CDNA4 (gfx950): quantize, dequantize and the decode GEMV.
//
// Format (OCP Microscaling v1.0 on the transposed [in, out] weight, the
// normative description is ops/mxfp4.py):
//   packed u8 [in/2, out]: byte (j, o) = column o of rows 2j (low nibble) and
//       2j+1 (high nibble); nibble = sign (bit 3) + E2M1 code (0, 0.5, 1, 1.5,
//       2, 3, 4, 6)
//   scales u8 [in/32, out]: E8M0, byte s = 2^(s-127), s in 1..254, one per
//       (32-row block, column)
// in % 32 == 0 and out % 8 == 0.
//
// The GEMV has the split-K structure of gemv.hip / int8.hip (a wave owns 512
// output columns, 8 per lane; x is a wave-uniform scalar load; gridDim.y
// splits the input dimension; gemv_reduce.h fuses the epilogue), but the
// dequant is one VALU instruction: v_cvt_scalef32_pk_f32_fp4 turns the two
// nibbles of one byte (two consecutive k of one column, which share a scale)
// into two scaled fp32 values. No LUT, no LDS, nothing on lgkmcnt but the
// scalar x loads. Scales are powers of two, so fp4 x scale is exact.

#include "common.h"
#include "gemv_reduce.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cstdlib>

#ifndef GEMV_OUT_PER_WAVE
#define GEMV_OUT_PER_WAVE 512
#endif

#define MX_BLOCK 32  // rows per scale

using f32x2_mx = __attribute__((ext_vector_type(2))) float;

// E8M0 byte -> fp32 scale: s in 1..254 is exactly the biased exponent
__device__ __forceinline__ float mx_scale_f32(unsigned int word, int byte) {
  return __uint_as_float(((word >> (8 * byte)) & 0xFFu) << 23);
}

// byte BYTE of `word` -> (low nibble, high nibble) * scale. The hardware
// returns the low nibble as element 0 (pinned by the one-hot tests).
template <int BYTE>
__device__ __forceinline__ f32x2_mx mx_cvt_pk_f32(unsigned int word, float scale) {
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, BYTE);
}

// ------------------------------------------------------------------- gemv

// UJ = packed rows (2 k each) loaded per batch of loads: 16 (a whole 32-row
// block, 128 B in flight per lane) up to batch 4, 8 for batch 5-8 where the
// 8 x BATCH accumulators leave fewer VGPRs for loads in flight. The kernel
// asks for >= 2 waves per SIMD, which caps every instantiation at 256 VGPRs.
template <int BATCH, int UJ>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2))) void gemv_mxfp4_kernel(
    const unsigned char* __restrict__ packed,  // [in/2, out]
    const unsigned char* __restrict__ scales,  // [in/32, out]
    const float* __restrict__ x,               // [BATCH, in]
    float* __restrict__ partials,              // [n_splits, BATCH, out]
    int in_dim,
    int out_dim,
    int blocks_per_split) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int out0 = blockIdx.x * GEMV_OUT_PER_WAVE + lane * 8;
  if (out0 >= out_dim) return;  // out % 8 == 0: a lane is fully live or gone
  const int split = blockIdx.y;
  const int n_blocks = in_dim / MX_BLOCK;
  const int kb0 = split * blocks_per_split;
  const int kb1 = min(kb0 + blocks_per_split, n_blocks);

  float acc[BATCH][8];
#pragma unroll
  for (int b = 0; b < BATCH; ++b)
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[b][v] = 0.f;

  const unsigned char* wp = packed + (size_t)kb0 * (MX_BLOCK / 2) * out_dim + out0;
  const unsigned char* sp = scales + (size_t)kb0 * out_dim + out0;
  for (int kb = kb0; kb < kb1; ++kb) {
    const uint2 s8 = *reinterpret_cast<const uint2*>(sp);
    float sc[8];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      sc[v] = mx_scale_f32(s8.x, v);
      sc[4 + v] = mx_scale_f32(s8.y, v);
    }
#pragma unroll
    for (int h = 0; h < (MX_BLOCK / 2) / UJ; ++h) {
      uint2 w[UJ];
#pragma unroll
      for (int u = 0; u < UJ; ++u)
        w[u] = *reinterpret_cast<const uint2*>(wp + (size_t)(h * UJ + u) * out_dim);
      const int i0 = kb * MX_BLOCK + h * UJ * 2;
#pragma unroll
      for (int u = 0; u < UJ; ++u) {
        float x0[BATCH], x1[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
          x0[b] = x[(size_t)b * in_dim + i0 + 2 * u];
          x1[b] = x[(size_t)b * in_dim + i0 + 2 * u + 1];
        }
        f32x2_mx f[8];
        f[0] = mx_cvt_pk_f32<0>(w[u].x, sc[0]);
        f[1] = mx_cvt_pk_f32<1>(w[u].x, sc[1]);
        f[2] = mx_cvt_pk_f32<2>(w[u].x, sc[2]);
        f[3] = mx_cvt_pk_f32<3>(w[u].x, sc[3]);
        f[4] = mx_cvt_pk_f32<0>(w[u].y, sc[4]);
        f[5] = mx_cvt_pk_f32<1>(w[u].y, sc[5]);
        f[6] = mx_cvt_pk_f32<2>(w[u].y, sc[6]);
        f[7] = mx_cvt_pk_f32<3>(w[u].y, sc[7]);
#pragma unroll
        for (int b = 0; b < BATCH; ++b)
#pragma unroll
          for (int v = 0; v < 8; ++v) {
            acc[b][v] = fmaf(f[v][0], x0[b], acc[b][v]);
            acc[b][v] = fmaf(f[v][1], x1[b], acc[b][v]);
          }
      }
    }
    wp += (size_t)(MX_BLOCK / 2) * out_dim;
    sp += out_dim;
  }

#pragma unroll
  for (int b = 0; b < BATCH; ++b) {
    float4v* d4 = reinterpret_cast<float4v*>(partials + ((size_t)split * BATCH + b) * out_dim + out0);
    d4[0] = float4v{acc[b][0], acc[b][1], acc[b][2], acc[b][3]};
    d4[1] = float4v{acc[b][4], acc[b][5], acc[b][6], acc[b][7]};
  }
}

// ------------------------------------------------------------------- quantize / dequantize

// one thread per (32-row block, column): 32 strided bf16 loads (coalesced
// across the wave), amax, E8M0 scale, 16 packed bytes. Plain compares; ties
// go to the even code and |q| > 5 saturates to 6, as ops/mxfp4.py.
__global__ __launch_bounds__(256) void mxfp4_quantize_kernel(
    const unsigned short* __restrict__ w,  // [in, out] bf16
    unsigned char* __restrict__ packed,    // [in/2, out]
    unsigned char* __restrict__ scales,    // [in/32, out]
    long n_cells,                          // (in/32) * out
    int out_dim) {
  const long cell = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= n_cells) return;
  const long kb = cell / out_dim;
  const int o = (int)(cell - kb * out_dim);
  const unsigned short* src = w + (size_t)kb * MX_BLOCK * out_dim + o;
  unsigned short raw[MX_BLOCK];
  unsigned int amax_bits = 0;  // |bf16| bits order like the magnitudes
#pragma unroll
  for (int r = 0; r < MX_BLOCK; ++r) {
    raw[r] = src[(size_t)r * out_dim];
    amax_bits = max(amax_bits, (unsigned int)(raw[r] & 0x7FFFu));
  }
  // floor(log2(amax)) - 2 = exponent field - 129; a subnormal amax lies below
  // the clamp either way; an all-zero block gets e = 0
  int e = (int)(amax_bits >> 7) - 129;
  e = max(e, -126);
  if (amax_bits == 0) e = 0;
  const unsigned int s = (unsigned int)(e + 127);
  // |v| * 2^-e in two exact power-of-two steps (2^126 * 2^-126 covers
  // e = -126 .. 125 without leaving the normal range of either factor)
  const float m1 = __uint_as_float((unsigned int)(127 - (e >> 1)) << 23);
  const float m2 = __uint_as_float((unsigned int)(127 - (e - (e >> 1))) << 23);
  unsigned char* dst = packed + (size_t)kb * (MX_BLOCK / 2) * out_dim + o;
#pragma unroll
  for (int j = 0; j < MX_BLOCK / 2; ++j) {
    unsigned int byte = 0;
#pragma unroll
    for (int hl = 0; hl < 2; ++hl) {
      const unsigned short bits = raw[2 * j + hl];
      float q = bf16_to_f32((unsigned short)(bits & 0x7FFFu)) * m1 * m2;
      // a subnormal input (mant * 2^-133) only reaches a nonzero code under the
      // clamped scale; take it in integers so no fp32 denormal mode matters
      if ((bits & 0x7F80u) == 0u) q = e == -126 ? (float)(bits & 0x7Fu) * 0.0078125f : 0.f;
      const unsigned int code = (unsigned int)(q > 0.25f) + (unsigned int)(q >= 0.75f) +
                                (unsigned int)(q > 1.25f) + (unsigned int)(q >= 1.75f) +
                                (unsigned int)(q > 2.5f) + (unsigned int)(q >= 3.5f) +
                                (unsigned int)(q > 5.0f);
      const unsigned int sign = (code != 0u && (bits & 0x8000u)) ? 8u : 0u;
      byte |= (code | sign) << (4 * hl);
    }
    dst[(size_t)j * out_dim] = (unsigned char)byte;
  }
  scales[cell] = (unsigned char)s;
}

// nibble + scale byte -> bf16 bits, in integers: value = 2^ue * (1 + m/2)
// with ue = -1 for code 1 (the E2M1 subnormal), so the bf16 exponent field is
// ue + s. Field 0 (code 1 at s = 1) is the bf16 subnormal 2^-127; fields past
// 254 overflow to infinity, as the fp32 product of the reference does.
__device__ __forceinline__ unsigned int mx_nibble_bf16(unsigned int nib, int s) {
  const unsigned int code = nib & 7u;
  const unsigned int sign = (nib & 8u) << 12;
  if (code == 0u) return sign;
  const int ue = code == 1u ? -1 : (int)(code >> 1) - 1;
  const unsigned int m = code >= 2u ? (code & 1u) : 0u;
  const int be = ue + s;
  if (be >= 255) return sign | 0x7F80u;
  if (be <= 0) return sign | 0x0040u;
  return sign | ((unsigned int)be << 7) | (m << 6);
}

// one thread per 4 consecutive columns of one packed row: 4-byte packed and
// scale loads, two 8-byte bf16 stores (rows 2j and 2j+1)
__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(
    const unsigned char* __restrict__ packed,  // [in/2, out]
    const unsigned char* __restrict__ scales,  // [in/32, out]
    unsigned short* __restrict__ out,          // [in, out] bf16
    long n_quads,                              // (in/2) * (out/4)
    int out_dim) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_quads) return;
  const int qpr = out_dim >> 2;
  const long j = t / qpr;
  const int o = (int)(t - j * qpr) * 4;
  const unsigned int p = *reinterpret_cast<const unsigned int*>(packed + (size_t)j * out_dim + o);
  const unsigned int s4 =
      *reinterpret_cast<const unsigned int*>(scales + (size_t)(j / (MX_BLOCK / 2)) * out_dim + o);
  unsigned int lo[4], hi[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const unsigned int byte = (p >> (8 * v)) & 0xFFu;
    const int s = (int)((s4 >> (8 * v)) & 0xFFu);
    lo[v] = mx_nibble_bf16(byte & 0xFu, s);
    hi[v] = mx_nibble_bf16(byte >> 4, s);
  }
  uint2 r0, r1;
  r0.x = lo[0] | (lo[1] << 16);
  r0.y = lo[2] | (lo[3] << 16);
  r1.x = hi[0] | (hi[1] << 16);
  r1.y = hi[2] | (hi[3] << 16);
  *reinterpret_cast<uint2*>(out + (size_t)(2 * j) * out_dim + o) = r0;
  *reinterpret_cast<uint2*>(out + (size_t)(2 * j + 1) * out_dim + o) = r1;
}

// ------------------------------------------------------------------- host

static void mx_check_weight(const torch::Tensor& packed, const torch::Tensor& scales, const char* op) {
  TORCH_CHECK(packed.is_cuda() && packed.dtype() == torch::kUInt8 && packed.dim() == 2 && packed.is_contiguous(),
              op, ": packed must be a contiguous u8 [in/2, out] GPU tensor");
  const int64_t in_dim = packed.size(0) * 2, out_dim = packed.size(1);
  TORCH_CHECK(in_dim > 0 && in_dim % MX_BLOCK == 0 && out_dim > 0 && out_dim % 8 == 0,
              op, " needs in % 32 == 0 and out % 8 == 0, got [", in_dim, ", ", out_dim, "]");
  TORCH_CHECK(scales.is_cuda() && scales.dtype() == torch::kUInt8 && scales.dim() == 2 &&
                  scales.is_contiguous() && scales.size(0) == in_dim / MX_BLOCK && scales.size(1) == out_dim,
              op, ": scales must be a contiguous u8 [in/32, out] GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(packed.data_ptr()) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(scales.data_ptr()) % 8 == 0,
              op, ": packed and scales must be 8-byte aligned");
  TORCH_CHECK(in_dim < (1LL << 31) && out_dim < (1LL << 31), op, ": weight too large");
}

std::vector<torch::Tensor> mxfp4_quantize(torch::Tensor w) {
  TORCH_CHECK(w.is_cuda() && w.dtype() == torch::kBFloat16 && w.dim() == 2,
              "mxfp4_quantize: w must be a bf16 [in, out] GPU tensor");
  const int64_t in_dim = w.size(0), out_dim = w.size(1);
  TORCH_CHECK(in_dim > 0 && in_dim % MX_BLOCK == 0 && out_dim > 0 && out_dim % 8 == 0,
              "mxfp4_quantize needs in % 32 == 0 and out % 8 == 0, got [", in_dim, ", ", out_dim, "]");
  TORCH_CHECK(out_dim < (1LL << 31), "mxfp4_quantize: weight too large");
  auto wc = w.contiguous();
  auto packed = torch::empty({in_dim / 2, out_dim}, w.options().dtype(torch::kUInt8));
  auto scales = torch::empty({in_dim / MX_BLOCK, out_dim}, w.options().dtype(torch::kUInt8));
  const long n_cells = (long)(in_dim / MX_BLOCK) * out_dim;
  auto stream = at::cuda::getCurrentCUDAStream();
  mxfp4_quantize_kernel<<<(unsigned)((n_cells + 255) / 256), 256, 0, stream>>>(
      reinterpret_cast<const unsigned short*>(wc.data_ptr()), packed.data_ptr<unsigned char>(),
      scales.data_ptr<unsigned char>(), n_cells, (int)out_dim);
  HIP_CHECK_LAST();
  return {packed, scales};
}

torch::Tensor mxfp4_dequantize(torch::Tensor packed, torch::Tensor scales) {
  mx_check_weight(packed, scales, "mxfp4_dequantize");
  const int64_t half_in = packed.size(0), out_dim = packed.size(1);
  auto out = torch::empty({half_in * 2, out_dim}, packed.options().dtype(torch::kBFloat16));
  const long n_quads = (long)half_in * (out_dim / 4);
  auto stream = at::cuda::getCurrentCUDAStream();
  mxfp4_dequant_kernel<<<(unsigned)((n_quads + 255) / 256), 256, 0, stream>>>(
      packed.data_ptr<unsigned char>(), scales.data_ptr<unsigned char>(),
      reinterpret_cast<unsigned short*>(out.data_ptr()), n_quads, (int)out_dim);
  HIP_CHECK_LAST();
  return out;
}

// workgroups over out_waves * splits. The llama-70b sweep (profiles/mxfp4.log,
// docs/KERNELS.md) wants 64 splits up to out = 10240 and 32-48 at out = 57344,
// where a target of 1024 gave 10 splits and cost 1.4-1.5x
#define MXFP4_SPLIT_TARGET 4096
#define MXFP4_DEFAULT_MAX_SPLITS 64  // the fast paths' workspace is 64 * B * max_out floats

int64_t gemv_mxfp4_splits(int64_t in_dim, int64_t out_dim, int64_t batch, int64_t splits_override) {
  (void)batch;  // the partial tile grows with batch, the split count does not
  const long out_waves = (out_dim + GEMV_OUT_PER_WAVE - 1) / GEMV_OUT_PER_WAVE;
  // PETALS_AMD_MXFP4_SPLIT_TARGET selects another target for A/B runs
  static const long target = [] {
    const char* env = std::getenv("PETALS_AMD_MXFP4_SPLIT_TARGET");
    const long t = env ? std::atol(env) : 0;
    return t > 0 ? t : (long)MXFP4_SPLIT_TARGET;
  }();
  long splits = splits_override;
  if (splits <= 0) {
    splits = (target + out_waves - 1) / out_waves;
    if (splits > MXFP4_DEFAULT_MAX_SPLITS) splits = MXFP4_DEFAULT_MAX_SPLITS;
  }
  const long n_blocks = in_dim / MX_BLOCK;
  if (splits > n_blocks) splits = n_blocks;
  if (splits < 1) splits = 1;
  // chunks are whole 32-row blocks; drop the splits that rounding left empty
  const long per = (n_blocks + splits - 1) / splits;
  return (n_blocks + per - 1) / per;
}

torch::Tensor gemv_mxfp4(
    torch::Tensor packed,    // [in/2, out] u8
    torch::Tensor scales,    // [in/32, out] u8 (E8M0)
    torch::Tensor x,         // [batch, in] f32
    torch::Tensor workspace,
    c10::optional<torch::Tensor> residual,
    int64_t epilogue,
    int64_t splits_override,
    c10::optional<torch::Tensor> bias) {
  mx_check_weight(packed, scales, "gemv_mxfp4");
  const int in_dim = (int)packed.size(0) * 2, out_dim = (int)packed.size(1);
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kFloat32 && x.dim() == 2 && x.is_contiguous(),
              "gemv_mxfp4: x must be a contiguous f32 [batch, in] GPU tensor");
  TORCH_CHECK(x.size(1) == in_dim, "x/in mismatch");
  const int batch = x.size(0);
  TORCH_CHECK(batch >= 1 && batch <= 8, "decode gemv supports batch <= 8");
  TORCH_CHECK(workspace.dtype() == torch::kFloat32, "gemv_mxfp4: workspace must be f32");

  const long out_waves = (out_dim + GEMV_OUT_PER_WAVE - 1) / GEMV_OUT_PER_WAVE;
  const long splits = gemv_mxfp4_splits(in_dim, out_dim, batch, splits_override);
  TORCH_CHECK(splits <= 65535, "gemv_mxfp4: too many splits");
  const int n_blocks = in_dim / MX_BLOCK;
  const int blocks_per_split = (n_blocks + (int)splits - 1) / (int)splits;

  torch::Tensor partials;
  auto f32opts = x.options();
  if (workspace.numel() >= (int64_t)splits * batch * out_dim) {
    TORCH_CHECK(workspace.is_cuda() && workspace.is_contiguous() &&
                    reinterpret_cast<uintptr_t>(workspace.data_ptr()) % 16 == 0,
                "gemv_mxfp4: workspace must be a contiguous 16-byte aligned GPU tensor");
    partials = workspace;
  } else {
    partials = torch::empty({(int64_t)splits, batch, out_dim}, f32opts);
  }
  dim3 grid(out_waves, splits);
  auto stream = at::cuda::getCurrentCUDAStream();

#define LAUNCH_MX(B, UJ)                                                       \
  gemv_mxfp4_kernel<B, UJ><<<grid, WAVE, 0, stream>>>(                         \
      packed.data_ptr<unsigned char>(), scales.data_ptr<unsigned char>(),      \
      x.data_ptr<float>(), partials.data_ptr<float>(), in_dim, out_dim, blocks_per_split)
  switch (batch) {
    case 1: LAUNCH_MX(1, 16); break;
    case 2: LAUNCH_MX(2, 16); break;
    case 3: LAUNCH_MX(3, 16); break;
    case 4: LAUNCH_MX(4, 16); break;
    case 5: LAUNCH_MX(5, 8); break;
    case 6: LAUNCH_MX(6, 4); break;  // UJ = 8 spills 6 VGPRs at the 256 cap
    case 7: LAUNCH_MX(7, 8); break;
    case 8: LAUNCH_MX(8, 8); break;
    default: TORCH_CHECK(false, "decode gemv supports batch <= 8");
  }
#undef LAUNCH_MX
  HIP_CHECK_LAST();

  if (epilogue < 0) {
    // RAW mode: the caller fuses its own reduce+epilogue (e.g. the qkv
    // rope+cache-write reduce); the view's shape carries the split count
    return partials.view(-1).narrow(0, 0, (int64_t)splits * batch * out_dim)
        .view({(int64_t)splits, (int64_t)batch, (int64_t)out_dim});
  }
  return launch_gemv_reduce(
      partials, residual, bias, (int)splits, batch, out_dim, (int)epilogue, f32opts,
      f32opts.dtype(torch::kBFloat16));
}
