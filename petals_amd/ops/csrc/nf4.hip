// NF4 4-bit blockwise quantization for CDNA4 (gfx950).
//
// Format (our own serving format; same 4.25 bits/param footprint as the
// reference's bitsandbytes LinearNF4 — blocksize 64, reference
// utils/convert_block.py:76-111, block_utils.py:46 — but with bf16 absmax
// instead of double-quantized int8 absmax: same size, better accuracy):
//   packed  uint8 [in, out/2]   two nibbles per byte (even elem = low nibble)
//   absmax  bf16  [in, out/64]  per-64-element scale along the OUT dim
//
// Weights stay TRANSPOSED [in, out] like the bf16 path, so the same
// x-broadcast GEMV structure applies; each lane owns 8 consecutive outputs
// (4 B packed per input row) and dequantizes in-register through an
// LDS-resident 256-entry NF4 pair LUT.

#include "common.h"
#include "gemv_reduce.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

__device__ __constant__ float NF4_LUT_C[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f,
    0.33791524171829224f, 0.4407098293304443f, 0.5626170039176941f,
    0.7229568362236023f, 1.0f};

// ------------------------------------------------------------- quantization

// one thread per 64-element block along OUT
__global__ void nf4_quantize_kernel(
    const unsigned short* __restrict__ w,  // [in, out] bf16
    unsigned char* __restrict__ packed,    // [in, out/2]
    unsigned short* __restrict__ absmax,   // [in, out/64] bf16
    long n_blocks,
    int out_dim) {
  const long blk = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (blk >= n_blocks) return;
  const long base = blk * 64;  // element offset (rows are multiples of 64 wide)
  float vals[64];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    vals[j] = bf16_to_f32(w[base + j]);
    amax = fmaxf(amax, fabsf(vals[j]));
  }
  const float amax_bf = bf16_to_f32(f32_to_bf16(amax));  // store-rounded scale
  absmax[blk] = f32_to_bf16(amax);
  const float inv = amax_bf > 0.f ? 1.0f / amax_bf : 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    unsigned char lo, hi;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const float v = vals[2 * j + half] * inv;
      // nearest NF4 level via linear scan (16 levels)
      int best = 0;
      float bd = fabsf(v - NF4_LUT_C[0]);
#pragma unroll
      for (int l = 1; l < 16; ++l) {
        const float d = fabsf(v - NF4_LUT_C[l]);
        if (d < bd) { bd = d; best = l; }
      }
      if (half == 0) lo = (unsigned char)best; else hi = (unsigned char)best;
    }
    packed[blk * 32 + j] = (unsigned char)(lo | (hi << 4));
  }
}

// --------------------------------------------------------------- dequantize

__global__ void nf4_dequant_kernel(
    const unsigned char* __restrict__ packed,
    const unsigned short* __restrict__ absmax,
    unsigned short* __restrict__ out,  // bf16
    long n_elems) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (i >= n_elems) return;
  const unsigned char byte = packed[i >> 1];
  const float scale = bf16_to_f32(absmax[i >> 6]);
  out[i] = f32_to_bf16(NF4_LUT_C[byte & 0xF] * scale);
  if (i + 1 < n_elems) out[i + 1] = f32_to_bf16(NF4_LUT_C[byte >> 4] * scale);
}

// -------------------------------------------------------------- NF4 gemv

#define NF4_OPL 8  // outputs per lane: one u32 packed word (4 B) per input row
#define NF4_OUT_PER_WAVE (WAVE * NF4_OPL)  // 64 lanes x 8 outputs

// 8 outputs per lane (rather than 16) doubles the workgroup count for the
// same split depth: the NF4 inner loop's dependent LDS gathers need more
// resident waves per SIMD to hide latency than the direct-load bf16 gemv.
template <int BATCH>
__global__ __launch_bounds__(WAVE) void gemv_nf4_kernel(
    const unsigned char* __restrict__ packed,   // [in, out/2]
    const unsigned short* __restrict__ absmax,  // [in, out/64]
    const unsigned short* __restrict__ absmax_t,  // [out/64, in] or null — the
    // transposed copy turns the per-row 2-byte strided absmax gather into ONE
    // contiguous 32 B load per 16-row unroll block (the strided stream was a
    // latency-hiding bottleneck: 16 extra scattered loads in flight per block)
    const float* __restrict__ x,                // [BATCH, in] f32
    float* __restrict__ partials,               // [n_splits, BATCH, out]
    int in_dim,
    int out_dim,
    int i_per_split) {
  // PAIR LUT: one read dequantizes a whole packed byte (two elements),
  // halving LDS traffic vs per-nibble lookups; 256 entries.
  // (the earlier 16-float bank-replicated LUT was LDS-issue bound)
  __shared__ float2 lut2[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x)
    lut2[i] = make_float2(NF4_LUT_C[i & 0xF], NF4_LUT_C[i >> 4]);
  __syncthreads();

  constexpr int OPL = NF4_OPL;
  const int lane = threadIdx.x & (WAVE - 1);
  const int out0 = blockIdx.x * (WAVE * OPL) + lane * OPL;
  if (out0 >= out_dim) return;
  const int split = blockIdx.y;
  const int i_begin = split * i_per_split;
  const int i_end = min(i_begin + i_per_split, in_dim);
  const bool full = (out0 + OPL) <= out_dim;

  float acc[BATCH][OPL];
#pragma unroll
  for (int b = 0; b < BATCH; ++b)
#pragma unroll
    for (int v = 0; v < OPL; ++v) acc[b][v] = 0.f;

  if (full) {
    // batch > 4: halve the unroll depth — xs[BATCH][UNROLL] + acc[BATCH][OPL]
    // at full depth would blow the VGPR budget below 2 waves/SIMD
    constexpr int UNROLL = (BATCH > 4) ? 8 : 16;
    const int half_out = out_dim >> 1;
    const unsigned char* pp = packed + (size_t)i_begin * half_out + (out0 >> 1);
    const unsigned short* amt = absmax_t ? absmax_t + (size_t)(out0 >> 6) * in_dim : nullptr;
    int i = i_begin;
    for (; i + UNROLL <= i_end; i += UNROLL) {
      unsigned int pk[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        pk[u] = *reinterpret_cast<const unsigned int*>(pp + (size_t)u * half_out);
      float am[UNROLL];
      if (amt) {
#pragma unroll
        for (int c8 = 0; c8 < UNROLL / 8; ++c8) {
          const short8 a8 = *reinterpret_cast<const short8*>(amt + i + c8 * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) am[c8 * 8 + e] = bf16_to_f32((unsigned short)a8[e]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          am[u] = bf16_to_f32(absmax[(size_t)(i + u) * (out_dim >> 6) + (out0 >> 6)]);
      }
      // NB: scalar (SMEM) x loads share the lgkm counter with the LDS LUT
      // gathers, limiting ds_read pipelining — but both measured alternatives
      // (volatile VMEM: cache-bypassed broadcast re-reads; buffer-load
      // intrinsics: worse scheduling) LOST to this form end to end
      // (profiles/nf4_vmem_sweep.log), so the simple loads stay.
      float xs[BATCH][UNROLL];
#pragma unroll
      for (int b = 0; b < BATCH; ++b)
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          xs[b][u] = x[(size_t)b * in_dim + i + u];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        float wf[OPL];
#pragma unroll
        for (int p2 = 0; p2 < 4; ++p2) {
          const float2 w2 = lut2[(pk[u] >> (8 * p2)) & 0xFFu];
          wf[2 * p2] = w2.x;
          wf[2 * p2 + 1] = w2.y;
        }
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
          const float xa = xs[b][u] * am[u];
#pragma unroll
          for (int v = 0; v < OPL; ++v) acc[b][v] = fmaf(wf[v], xa, acc[b][v]);
        }
      }
      pp += (size_t)UNROLL * half_out;
    }
    for (; i < i_end; ++i) {
      const float am = bf16_to_f32(absmax[(size_t)i * (out_dim >> 6) + (out0 >> 6)]);
#pragma unroll
      for (int b = 0; b < BATCH; ++b) {
        const float xa = x[(size_t)b * in_dim + i] * am;
        const unsigned int wd =
            *reinterpret_cast<const unsigned int*>(packed + (size_t)i * half_out + (out0 >> 1));
#pragma unroll
        for (int p2 = 0; p2 < 4; ++p2) {
          const float2 w2 = lut2[(wd >> (8 * p2)) & 0xFFu];
          acc[b][2 * p2] = fmaf(w2.x, xa, acc[b][2 * p2]);
          acc[b][2 * p2 + 1] = fmaf(w2.y, xa, acc[b][2 * p2 + 1]);
        }
      }
    }
  } else {
    for (int i = i_begin; i < i_end; ++i) {
      const float am = bf16_to_f32(absmax[(size_t)i * (out_dim >> 6) + (out0 >> 6)]);
#pragma unroll
      for (int b = 0; b < BATCH; ++b) {
        const float xa = x[(size_t)b * in_dim + i] * am;
        // compile-time trip count with a guard: a runtime-bounded loop here
        // makes acc[][] dynamically indexed, forcing it onto the SCRATCH
        // stack for the whole kernel (observed at BATCH>=5: ~100x slowdown)
#pragma unroll
        for (int v = 0; v < OPL; ++v) {
          if (out0 + v < out_dim) {
            const unsigned char byte = packed[(size_t)i * (out_dim >> 1) + ((out0 + v) >> 1)];
            const float2 w2 = lut2[byte];
            acc[b][v] = fmaf(((out0 + v) & 1) ? w2.y : w2.x, xa, acc[b][v]);
          }
        }
      }
    }
  }

#pragma unroll
  for (int b = 0; b < BATCH; ++b) {
    float* dst = partials + ((size_t)split * BATCH + b) * out_dim + out0;
    if (full) {
#pragma unroll
      for (int q = 0; q < OPL / 4; ++q)
        reinterpret_cast<float4v*>(dst)[q] =
            float4v{acc[b][4 * q], acc[b][4 * q + 1], acc[b][4 * q + 2], acc[b][4 * q + 3]};
    } else {
#pragma unroll
      for (int v = 0; v < OPL; ++v)
        if (out0 + v < out_dim) dst[v] = acc[b][v];
    }
  }
}

// ----------------------------------------- NF4 gemv, K split inside the workgroup

// Same inner loop, pair LUT, per-lane layout AND the same arithmetic as
// gemv_nf4_kernel followed by the reduce: for a split count S the K chunks are
// the one-wave kernel's chunks, and the result is bit for bit what that kernel
// and gemv_reduce_kernel / qkv_rope_reduce_kernel give for S splits.
//
// Both reduces sum the S partials in 16 groups, group g taking chunks g, g+16,
// g+32, ... in that order, then add the 16 group sums. Here workgroup
// blockIdx.y = g IS group g: wave w runs chunk g + 16 w, the waves park their
// accumulators in LDS, and after one barrier they are added in the order the
// reduce uses inside a group (see the combine below). The workgroup writes the group's sum
// as its one partial row, so the reduce finds min(S, 16) rows instead of S,
// one per group, and only adds the groups. Partial bytes fall by S / 16, the
// LUT is built once per WAVES chunks, and no result changes by one bit.
//
// Every thread reaches both barriers: lanes past out_dim and waves whose chunk
// index is past S run zero iterations and contribute +0. NT selects
// non-temporal loads for the packed weight words only (each is read once per
// token); absmax_t and x keep the default policy.
//
// LDS: 2 KB LUT + WAVES * BATCH * 2 KB combine buffer. WAVES 16 exists for
// BATCH <= 3 only: at 1024 threads a wave has 128 VGPRs and BATCH 4 needs 200.
// No instantiation uses scratch.
#define NF4_RED_GROUPS 16  // = GEMV_REDUCE_GROUPS = QKV_RED_GROUPS (elementwise.hip)
static_assert(NF4_RED_GROUPS == GEMV_REDUCE_GROUPS, "the wg kernel mirrors the reduce's grouping");
template <int BATCH, int WAVES, bool NT>
__global__ __launch_bounds__(WAVE * WAVES) void gemv_nf4_wg_kernel(
    const unsigned char* __restrict__ packed,     // [in, out/2]
    const unsigned short* __restrict__ absmax,    // [in, out/64]
    const unsigned short* __restrict__ absmax_t,  // [out/64, in] or null
    const float* __restrict__ x,                  // [BATCH, in] f32
    float* __restrict__ partials,                 // [n_splits, BATCH, out]
    int in_dim,
    int out_dim,
    int i_per_split,  // rows per chunk, multiple of 16 (the one-wave kernel's i_per_split)
    int n_splits) {   // S, at most NF4_RED_GROUPS * WAVES
  constexpr int OPL = NF4_OPL;
  constexpr int UNROLL = 16;
  constexpr int THREADS = WAVE * WAVES;
  __shared__ float2 lut2[256];
  __shared__ float comb[WAVES][BATCH][NF4_OUT_PER_WAVE];
  for (int i = threadIdx.x; i < 256; i += THREADS)
    lut2[i] = make_float2(NF4_LUT_C[i & 0xF], NF4_LUT_C[i >> 4]);
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  // wave-uniform by construction; readfirstlane tells the compiler so, which
  // keeps the x and absmax_t addresses scalar as in the one-wave kernel
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int out0 = blockIdx.x * (WAVE * OPL) + lane * OPL;
  const int split = blockIdx.y;  // the reduce group this workgroup stands for
  const int chunk = split + NF4_RED_GROUPS * wave;
  // a wave past the last chunk gets an empty range
  const int i_begin = chunk < n_splits ? chunk * i_per_split : in_dim;
  const int i_end = min(i_begin + i_per_split, in_dim);
  const bool live = out0 < out_dim;
  const bool full = (out0 + OPL) <= out_dim;

  float acc[BATCH][OPL];
#pragma unroll
  for (int b = 0; b < BATCH; ++b)
#pragma unroll
    for (int v = 0; v < OPL; ++v) acc[b][v] = 0.f;

  if (full) {
    const int half_out = out_dim >> 1;
    const unsigned char* pp = packed + (size_t)i_begin * half_out + (out0 >> 1);
    const unsigned short* amt = absmax_t ? absmax_t + (size_t)(out0 >> 6) * in_dim : nullptr;
    int i = i_begin;
    for (; i + UNROLL <= i_end; i += UNROLL) {
      unsigned int pk[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const unsigned int* wp = reinterpret_cast<const unsigned int*>(pp + (size_t)u * half_out);
        pk[u] = NT ? __builtin_nontemporal_load(wp) : *wp;
      }
      float am[UNROLL];
      if (amt) {
#pragma unroll
        for (int c8 = 0; c8 < UNROLL / 8; ++c8) {
          const short8 a8 = *reinterpret_cast<const short8*>(amt + i + c8 * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) am[c8 * 8 + e] = bf16_to_f32((unsigned short)a8[e]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          am[u] = bf16_to_f32(absmax[(size_t)(i + u) * (out_dim >> 6) + (out0 >> 6)]);
      }
      float xs[BATCH][UNROLL];
#pragma unroll
      for (int b = 0; b < BATCH; ++b)
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          xs[b][u] = x[(size_t)b * in_dim + i + u];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        float wf[OPL];
#pragma unroll
        for (int p2 = 0; p2 < 4; ++p2) {
          const float2 w2 = lut2[(pk[u] >> (8 * p2)) & 0xFFu];
          wf[2 * p2] = w2.x;
          wf[2 * p2 + 1] = w2.y;
        }
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
          const float xa = xs[b][u] * am[u];
#pragma unroll
          for (int v = 0; v < OPL; ++v) acc[b][v] = fmaf(wf[v], xa, acc[b][v]);
        }
      }
      pp += (size_t)UNROLL * half_out;
    }
    for (; i < i_end; ++i) {
      const float am = bf16_to_f32(absmax[(size_t)i * (out_dim >> 6) + (out0 >> 6)]);
#pragma unroll
      for (int b = 0; b < BATCH; ++b) {
        const float xa = x[(size_t)b * in_dim + i] * am;
        const unsigned int wd =
            *reinterpret_cast<const unsigned int*>(packed + (size_t)i * half_out + (out0 >> 1));
#pragma unroll
        for (int p2 = 0; p2 < 4; ++p2) {
          const float2 w2 = lut2[(wd >> (8 * p2)) & 0xFFu];
          acc[b][2 * p2] = fmaf(w2.x, xa, acc[b][2 * p2]);
          acc[b][2 * p2 + 1] = fmaf(w2.y, xa, acc[b][2 * p2 + 1]);
        }
      }
    }
  } else if (live) {
    for (int i = i_begin; i < i_end; ++i) {
      const float am = bf16_to_f32(absmax[(size_t)i * (out_dim >> 6) + (out0 >> 6)]);
#pragma unroll
      for (int b = 0; b < BATCH; ++b) {
        const float xa = x[(size_t)b * in_dim + i] * am;
        // compile-time trip count with a guard, as in gemv_nf4_kernel: a
        // runtime-bounded loop would put acc[][] on the scratch stack
#pragma unroll
        for (int v = 0; v < OPL; ++v) {
          if (out0 + v < out_dim) {
            const unsigned char byte = packed[(size_t)i * (out_dim >> 1) + ((out0 + v) >> 1)];
            const float2 w2 = lut2[byte];
            acc[b][v] = fmaf(((out0 + v) & 1) ? w2.y : w2.x, xa, acc[b][v]);
          }
        }
      }
    }
  }

  // combine: every wave parks its accumulators, then all threads sum over the
  // waves in index order and write the workgroup's one partial row
#pragma unroll
  for (int b = 0; b < BATCH; ++b)
#pragma unroll
    for (int q = 0; q < OPL / 4; ++q)
      reinterpret_cast<float4v*>(&comb[wave][b][lane * OPL])[q] =
          float4v{acc[b][4 * q], acc[b][4 * q + 1], acc[b][4 * q + 2], acc[b][4 * q + 3]};
  __syncthreads();
  const int col0 = blockIdx.x * NF4_OUT_PER_WAVE;
  // The group sum exactly as gemv_reduce_kernel and qkv_rope_reduce_kernel
  // compute it over this group's m partials. Under -ffast-math their split
  // loop `for (s = g; s < S; s += 16) a += p[s]` compiles to two interleaved
  // accumulators (even and odd members, one packed add per pair), their sum,
  // and then a scalar remainder for an odd last member; the order below is
  // that one. __fadd_rn keeps fast-math from reassociating it here.
  // tests/test_nf4_gemv_wg.py::test_bit_identical_to_one_wave_kernel holds the
  // two in step: it fails if a compiler changes either side.
  const int m = (n_splits - split + NF4_RED_GROUPS - 1) / NF4_RED_GROUPS;  // 1..WAVES
#pragma unroll
  for (int e = threadIdx.x; e < BATCH * NF4_OUT_PER_WAVE; e += THREADS) {
    const int b = e / NF4_OUT_PER_WAVE;
    const int c = e % NF4_OUT_PER_WAVE;
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int w = 0; w + 1 < WAVES; w += 2) {
      if (w + 1 < m) {
        a0 = __fadd_rn(a0, comb[w][b][c]);
        a1 = __fadd_rn(a1, comb[w + 1][b][c]);
      }
    }
    float s = __fadd_rn(a0, a1);
    if (m & 1) s = __fadd_rn(comb[m - 1][b][c], s);
    if (col0 + c < out_dim)
      partials[((size_t)split * BATCH + b) * out_dim + col0 + c] = s;
  }
}

// ------------------------------------------------------------------- host

std::vector<torch::Tensor> nf4_quantize(torch::Tensor w) {
  TORCH_CHECK(w.is_cuda() && w.dtype() == torch::kBFloat16 && w.dim() == 2);
  TORCH_CHECK(w.size(1) % 64 == 0, "out dim must be a multiple of 64");
  auto wc = w.contiguous();
  const long in_dim = wc.size(0), out_dim = wc.size(1);
  const long n_blocks = in_dim * out_dim / 64;
  auto packed = torch::empty({in_dim, out_dim / 2}, w.options().dtype(torch::kUInt8));
  auto absmax = torch::empty({in_dim, out_dim / 64}, w.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const long blocks = (n_blocks + 255) / 256;
  nf4_quantize_kernel<<<blocks, 256, 0, stream>>>(
      reinterpret_cast<const unsigned short*>(wc.data_ptr()),
      packed.data_ptr<unsigned char>(),
      reinterpret_cast<unsigned short*>(absmax.data_ptr()),
      n_blocks, (int)out_dim);
  HIP_CHECK_LAST();
  return {packed, absmax};
}

torch::Tensor nf4_dequantize(torch::Tensor packed, torch::Tensor absmax) {
  TORCH_CHECK(packed.is_cuda() && packed.dtype() == torch::kUInt8 && packed.dim() == 2);
  const long in_dim = packed.size(0), half_out = packed.size(1);
  const long n = in_dim * half_out * 2;
  auto out = torch::empty({in_dim, half_out * 2}, absmax.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const long blocks = (n / 2 + 255) / 256;
  nf4_dequant_kernel<<<blocks, 256, 0, stream>>>(
      packed.data_ptr<unsigned char>(),
      reinterpret_cast<const unsigned short*>(absmax.data_ptr()),
      reinterpret_cast<unsigned short*>(out.data_ptr()), n);
  HIP_CHECK_LAST();
  return out;
}

torch::Tensor gemv_nf4(
    torch::Tensor packed,    // [in, out/2] u8
    torch::Tensor absmax,    // [in, out/64] bf16
    torch::Tensor x,         // [batch, in] f32
    torch::Tensor workspace,
    c10::optional<torch::Tensor> residual,
    int64_t epilogue,
    int64_t splits_override,
    c10::optional<torch::Tensor> bias,        // [out] bf16, added pre-activation
    c10::optional<torch::Tensor> absmax_t,    // [out/64, in] bf16 (transposed copy)
    int64_t wg_waves,  // 0 or 1: gemv_nf4_kernel; 4, 8 or 16: gemv_nf4_wg_kernel where it fits
    bool nt) {         // non-temporal packed-weight loads (gemv_nf4_wg_kernel only)
  TORCH_CHECK(packed.is_cuda() && packed.dtype() == torch::kUInt8);
  TORCH_CHECK(x.dtype() == torch::kFloat32 && x.dim() == 2);
  const int in_dim = packed.size(0);
  const int out_dim = packed.size(1) * 2;
  const int batch = x.size(0);
  TORCH_CHECK(x.size(1) == in_dim && batch <= 8, "NF4 decode gemv supports batch <= 8");
  TORCH_CHECK(wg_waves == 0 || wg_waves == 1 || wg_waves == 4 || wg_waves == 8 || wg_waves == 16,
              "wg_waves must be 0, 1, 4, 8 or 16");
  TORCH_CHECK(!nt || wg_waves > 1, "nt selects a load policy of the wg kernel: give wg_waves 4, 8 or 16");

  const long out_waves = (out_dim + (long)NF4_OUT_PER_WAVE - 1) / NF4_OUT_PER_WAVE;
  // NF4 matrices are 4x smaller than bf16: allow chunks down to 64 input rows
  // so small projections still spread over the 256 CUs
  long splits = splits_override > 0 ? splits_override : (1536 + out_waves - 1) / out_waves;
  long max_splits = (in_dim + 31) / 32;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  // chunks must be UNROLL-aligned or the per-row fallback tail eats the
  // gain (an unaligned split count put up to a third of rows on the slow path)
  const int i_per_split = (int)(((in_dim + splits - 1) / splits + 15L) & ~15L);
  splits = (in_dim + i_per_split - 1) / i_per_split;
  // The wg kernel computes the same bits from the same chunks, one workgroup
  // per reduce group. It runs when its waves cover every chunk of a group;
  // otherwise (more chunks, batch 5..8, or 16 waves at batch 4, which has no
  // instantiation) the one-wave kernel does, with the same result.
  const int waves = (wg_waves > 1 && batch <= 4 && splits <= NF4_RED_GROUPS * wg_waves
                     && !(wg_waves == 16 && batch == 4)) ? (int)wg_waves : 1;
  const int n_chunks = (int)splits;       // K chunks
  if (waves > 1 && splits > NF4_RED_GROUPS) splits = NF4_RED_GROUPS;  // partial rows written

  torch::Tensor partials;
  auto f32opts = x.options().dtype(torch::kFloat32);
  if (workspace.numel() >= (int64_t)splits * batch * out_dim) {
    partials = workspace;
  } else {
    partials = torch::empty({(int64_t)splits, batch, out_dim}, f32opts);
  }
  dim3 grid(out_waves, splits);
  auto stream = at::cuda::getCurrentCUDAStream();

  const unsigned short* amt_p = nullptr;
  if (absmax_t.has_value() && absmax_t->defined() && absmax_t->numel() > 0) {
    TORCH_CHECK(absmax_t->is_contiguous() && absmax_t->size(0) == out_dim / 64
                && absmax_t->size(1) == in_dim);
    amt_p = reinterpret_cast<const unsigned short*>(absmax_t->data_ptr());
  }
#define LAUNCH_NF4(B)                                                         \
  case B:                                                                     \
    gemv_nf4_kernel<B><<<grid, WAVE, 0, stream>>>(                            \
        packed.data_ptr<unsigned char>(),                                     \
        reinterpret_cast<const unsigned short*>(absmax.data_ptr()), amt_p,    \
        x.data_ptr<float>(), partials.data_ptr<float>(), in_dim, out_dim, i_per_split); \
    break;
#define LAUNCH_NF4_WG(B, W, N)                                                \
  gemv_nf4_wg_kernel<B, W, N><<<grid, WAVE * W, 0, stream>>>(                 \
      packed.data_ptr<unsigned char>(),                                       \
      reinterpret_cast<const unsigned short*>(absmax.data_ptr()), amt_p,      \
      x.data_ptr<float>(), partials.data_ptr<float>(), in_dim, out_dim, i_per_split, n_chunks)
#define LAUNCH_NF4_WG_W(B, W) \
  do { if (nt) LAUNCH_NF4_WG(B, W, true); else LAUNCH_NF4_WG(B, W, false); } while (0)
#define LAUNCH_NF4_WG_B(B)                                                    \
  case B:                                                                     \
    if (waves == 4) LAUNCH_NF4_WG_W(B, 4);                                    \
    else if (waves == 8) LAUNCH_NF4_WG_W(B, 8);                               \
    else LAUNCH_NF4_WG_W(B, 16);                                              \
    break;
  if (waves > 1) {
    switch (batch) {
      LAUNCH_NF4_WG_B(1) LAUNCH_NF4_WG_B(2) LAUNCH_NF4_WG_B(3)
      case 4:
        if (waves == 4) LAUNCH_NF4_WG_W(4, 4); else LAUNCH_NF4_WG_W(4, 8);
        break;
    }
  } else {
    switch (batch) {
      LAUNCH_NF4(1) LAUNCH_NF4(2) LAUNCH_NF4(3) LAUNCH_NF4(4)
      LAUNCH_NF4(5) LAUNCH_NF4(6) LAUNCH_NF4(7) LAUNCH_NF4(8)
    }
  }
#undef LAUNCH_NF4_WG_W
#undef LAUNCH_NF4_WG_B
#undef LAUNCH_NF4_WG
#undef LAUNCH_NF4
  HIP_CHECK_LAST();

  if (epilogue < 0) {
    // RAW mode: the caller fuses its own reduce+epilogue (e.g. the qkv
    // rope+cache-write reduce); the view's shape carries the split count
    return partials.view(-1).narrow(0, 0, (int64_t)splits * batch * out_dim)
        .view({(int64_t)splits, (int64_t)batch, (int64_t)out_dim});
  }
  return launch_gemv_reduce(
      partials, residual, bias, (int)splits, batch, out_dim, (int)epilogue, f32opts,
      absmax.options());
}
