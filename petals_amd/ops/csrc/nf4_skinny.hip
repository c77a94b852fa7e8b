// NF4 skinny-M GEMM for wide decode steps (CDNA4 / gfx950):
//   partials[s, r, out] = x[r, k-chunk s] . W[k-chunk s, out],  9 <= rows <= 32
//
// The decode GEMVs (nf4.hip) keep one fp32 accumulator set per batch row in
// VGPRs and stop at 8 rows; the prefill GEMM (gemm_quant.hip) stages 128x128
// tiles through LDS and is built for hundreds of rows. This kernel streams the
// packed weight once, like a GEMV, and puts the rows on the matrix cores.
//
// Dataflow. A wave owns 256 output columns and walks k in steps of 32, one
// mfma_f32_16x16x32_bf16 depth. Lane (l15 = lane & 15, hi = lane >> 4):
//   A operand (x): row g*16 + l15 of row group g (1 or 2 groups), its 8
//     consecutive k  hi*8 .. hi*8+7: two 16-byte fp32 loads, four
//     v_cvt_pk_bf16_f32. Rows >= rows are zero fragments, never loaded.
//   B operand (W): straight from global memory, no LDS staging. For each of
//     its 8 k rows the lane loads 8 packed bytes = columns 16*l15 .. 16*l15+15
//     of the tile, so the 16 lanes of a k group read 128 contiguous bytes of a
//     weight row. Nibble v of the 8 rows is B fragment v: the 64 bytes feed 16
//     MFMAs per row group, fragment v covering tile columns {16*c + v}.
//   C: lane holds, per fragment v, rows hi*4 .. hi*4+3 of column 16*l15 + v,
//     i.e. 16 CONSECUTIVE columns of 4 rows per row group: the interleave
//     undoes itself in the store, four 16-byte stores per row.
// Dequant is gemm_quant.hip's: a 256-entry float2 pair LUT in LDS, one
// ds_read_b64 per packed byte, value = bf16(LUT[nibble] * float(absmax)) with
// v_cvt_pk_bf16_f32 packing two consecutive k of one column: bit for bit
// nf4_dequantize. One absmax covers a k row's 64 columns, so a lane needs 8 per
// step: one 16-byte load from the transposed copy [out/64, in] when the caller
// has it (AMT), 8 two-byte gathers otherwise.
//
// In flight: the loads of step i+1 (64 B packed + absmax + 32 B of x per row
// group, per lane) are issued before the dequant and MFMAs of step i, two
// register buffers, no LDS in the loop besides the LUT.
//
// Split-K twice, no atomics. grid.y slices k into S chunks of whole steps, S a
// function of (in, out, rows) alone with S * rows <= 512, so the partials
// [S, rows, out] fit the 64 * 8 * max_out floats an 8-row decode step already
// holds. Inside a workgroup the chunk is cut again over 4 waves; waves 1..3
// park their accumulators in LDS and wave 0 adds them in wave order and stores
// the workgroup's one partial row set. The partials feed the unchanged
// gemv_reduce / qkv_rope_reduce[_multi] kernels.
//
// Rounding points: W to bf16 exactly as nf4_dequantize; x to bf16 once; the
// rest fp32 (the rounding of the prefill path these shapes ran before).
// Requires in % 32 == 0 and out % 64 == 0; a lane's 16 columns are all inside
// out or all outside (16 | 64): outside lanes load nothing and store nothing.

#include "common.h"
#include "gemv_reduce.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define SK_WAVES 4
#define SK_TILE_N 256        // columns per workgroup (every wave covers all of them)
#define SK_KSTEP 32          // k per step: one MFMA depth
#define SK_MIN_ROWS 9
#define SK_MAX_ROWS 32
#define SK_PARTIAL_ROWS 512  // S * rows bound: 64 splits x 8 rows of the decode workspace
// default split policy (profiles/nf4_skinny.log, split sweep): workgroups to
// aim for with one row group (two resident workgroups per CU fit) and with two
// (one fits), and the k steps a workgroup keeps so every wave has at least two
#define SK_TARGET_WGS_G1 384
#define SK_TARGET_WGS_G2 256
#define SK_MIN_STEPS 8
#define SK_KERNEL __attribute__((target("no-packed-fp32-ops")))

using f32x2_sk = __attribute__((ext_vector_type(2))) float;
using bf16x2_sk = __attribute__((ext_vector_type(2))) __bf16;
using u32x4_sk = __attribute__((ext_vector_type(4))) unsigned int;

static __device__ __constant__ float SK_NF4_LUT[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f,
    0.33791524171829224f, 0.4407098293304443f, 0.5626170039176941f,
    0.7229568362236023f, 1.0f};

// two fp32 -> packed bf16 pair, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned int sk_pack_bf16(float lo, float hi) {
  const bf16x2_sk r = __builtin_convertvector(f32x2_sk{lo, hi}, bf16x2_sk);
  return __builtin_bit_cast(unsigned int, r);
}

// one k step's operands as they come from memory
template <int G, bool AMT>
struct SkStep {
  uint2 pk[8];                    // 8 k rows x 16 nibbles
  short8 amv;                     // AMT: the 8 absmax of the lane's k rows
  unsigned short ams[AMT ? 1 : 8];  // !AMT: the same, gathered
  float4v xa[G][2];               // 8 fp32 of one x row per row group
};

template <int G, bool AMT>
__global__ __launch_bounds__(WAVE * SK_WAVES) SK_KERNEL void nf4_skinny_kernel(
    const unsigned char* __restrict__ packed,     // [in, out/2]
    const unsigned short* __restrict__ absmax,    // [in, out/64]
    const unsigned short* __restrict__ absmax_t,  // AMT: [out/64, in]
    const float* __restrict__ x,                  // [rows, in] f32
    float* __restrict__ partials,                 // [gridDim.y, rows, out]
    int rows,
    int in_dim,
    int out_dim,
    int steps_per_split) {
  __shared__ float2 lut2[256];
  __shared__ float4v comb[SK_WAVES - 1][16][WAVE];  // one row group of waves 1..3: 48 KB
  lut2[threadIdx.x] = make_float2(SK_NF4_LUT[threadIdx.x & 0xF], SK_NF4_LUT[threadIdx.x >> 4]);
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15;
  const int hi = lane >> 4;
  const int col0 = blockIdx.x * SK_TILE_N + l15 * 16;
  const bool live = col0 < out_dim;

  // this workgroup's steps [s0, s1), this wave's share [w0, w1) of them
  const int nk = in_dim / SK_KSTEP;
  const int s0 = blockIdx.y * steps_per_split;
  const int s1 = min(nk, s0 + steps_per_split);
  const int per_wave = (steps_per_split + SK_WAVES - 1) / SK_WAVES;
  const int w0 = min(s1, s0 + wave * per_wave);
  const int w1 = min(s1, w0 + per_wave);

  const size_t half_out = (size_t)(out_dim >> 1);
  const int nblk = out_dim >> 6;
  const int blk = col0 >> 6;
  const unsigned char* wp = packed + (size_t)(hi * 8) * half_out + (col0 >> 1);
  bool xrow[G];
  const float* xp[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    xrow[g] = g * 16 + l15 < rows;
    xp[g] = x + (size_t)(xrow[g] ? g * 16 + l15 : 0) * in_dim + hi * 8;
  }

  auto load_step = [&](SkStep<G, AMT>& st, int step) __attribute__((always_inline)) {
    const int k0 = step * SK_KSTEP;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      st.pk[j] = make_uint2(0u, 0u);
      if (live) st.pk[j] = *reinterpret_cast<const uint2*>(wp + (size_t)(k0 + j) * half_out);
    }
    if constexpr (AMT) {
      st.amv = short8{0, 0, 0, 0, 0, 0, 0, 0};
      if (live) st.amv = *reinterpret_cast<const short8*>(absmax_t + (size_t)blk * in_dim + k0 + hi * 8);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        st.ams[j] = 0;
        if (live) st.ams[j] = absmax[(size_t)(k0 + hi * 8 + j) * nblk + blk];
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      st.xa[g][0] = st.xa[g][1] = float4v{0.f, 0.f, 0.f, 0.f};
      if (xrow[g]) {
        st.xa[g][0] = *reinterpret_cast<const float4v*>(xp[g] + k0);
        st.xa[g][1] = *reinterpret_cast<const float4v*>(xp[g] + k0 + 4);
      }
    }
  };

  float4v acc[G][16];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[g][v] = float4v{0.f, 0.f, 0.f, 0.f};

  auto compute_step = [&](const SkStep<G, AMT>& st) __attribute__((always_inline)) {
    short8 a[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const u32x4_sk w = {sk_pack_bf16(st.xa[g][0][0], st.xa[g][0][1]), sk_pack_bf16(st.xa[g][0][2], st.xa[g][0][3]),
                          sk_pack_bf16(st.xa[g][1][0], st.xa[g][1][1]), sk_pack_bf16(st.xa[g][1][2], st.xa[g][1][3])};
      a[g] = __builtin_bit_cast(short8, w);
    }
    float am[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (AMT) am[j] = bf16_to_f32((unsigned short)st.amv[j]);
      else am[j] = bf16_to_f32(st.ams[j]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {  // packed byte c = tile columns 2c, 2c+1 of the lane's 16
      u32x4_sk lo, hh;
#pragma unroll
      for (int t = 0; t < 4; ++t) {  // k pair (2t, 2t+1) -> one packed bf16 word per column
        const unsigned int p0 = c < 4 ? st.pk[2 * t].x : st.pk[2 * t].y;
        const unsigned int p1 = c < 4 ? st.pk[2 * t + 1].x : st.pk[2 * t + 1].y;
        const float2 e0 = lut2[(p0 >> (8 * (c & 3))) & 0xFFu];
        const float2 e1 = lut2[(p1 >> (8 * (c & 3))) & 0xFFu];
        lo[t] = sk_pack_bf16(e0.x * am[2 * t], e1.x * am[2 * t + 1]);
        hh[t] = sk_pack_bf16(e0.y * am[2 * t], e1.y * am[2 * t + 1]);
      }
      const short8 b0 = __builtin_bit_cast(short8, lo);
      const short8 b1 = __builtin_bit_cast(short8, hh);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        acc[g][2 * c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[g], b0, acc[g][2 * c], 0, 0, 0);
        acc[g][2 * c + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[g], b1, acc[g][2 * c + 1], 0, 0, 0);
      }
    }
  };

  // two register buffers: step i+1 is on its way while step i computes
  SkStep<G, AMT> buf0, buf1;
  if (w0 < w1) load_step(buf0, w0);
  for (int i = w0; i < w1; i += 2) {
    if (i + 1 < w1) load_step(buf1, i + 1);
    compute_step(buf0);
    if (i + 1 < w1) {
      if (i + 2 < w1) load_step(buf0, i + 2);
      compute_step(buf1);
    }
  }

  // in-workgroup combine, one row group at a time: waves 1..3 park, wave 0
  // adds in wave order and stores. A wave with no steps contributes +0.
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (wave > 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) comb[wave - 1][v][lane] = acc[g][v];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v)
#pragma unroll
        for (int w = 0; w < SK_WAVES - 1; ++w) acc[g][v] += comb[w][v][lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = g * 16 + hi * 4 + r;
        if (live && row < rows) {
          float* dst = partials + ((size_t)blockIdx.y * rows + row) * out_dim + col0;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            reinterpret_cast<float4v*>(dst)[q] = float4v{acc[g][4 * q][r], acc[g][4 * q + 1][r],
                                                         acc[g][4 * q + 2][r], acc[g][4 * q + 3][r]};
        }
      }
    }
    if (g + 1 < G) __syncthreads();  // comb is reused by the next row group
  }
}

// ------------------------------------------------------------------- host

// k steps per split and the split count S for a shape: S * rows <= 512, every
// split holds whole steps, no split is empty. The default aims at
// SK_TARGET_WGS_G1 / _G2 workgroups of at least SK_MIN_STEPS steps.
static int sk_policy(int64_t in_dim, int64_t out_dim, int64_t rows, int64_t splits_override, int* steps_per_split) {
  const int64_t nk = in_dim / SK_KSTEP;
  const int64_t tiles = (out_dim + SK_TILE_N - 1) / SK_TILE_N;
  int64_t want = splits_override;
  if (want <= 0) {
    const int64_t target = rows <= 16 ? SK_TARGET_WGS_G1 : SK_TARGET_WGS_G2;
    want = (target + tiles - 1) / tiles;
    want = std::min<int64_t>(want, std::max<int64_t>(1, nk / SK_MIN_STEPS));
  }
  want = std::max<int64_t>(1, std::min<int64_t>(want, std::min<int64_t>(SK_PARTIAL_ROWS / rows, nk)));
  const int64_t per = (nk + want - 1) / want;
  *steps_per_split = (int)per;
  return (int)((nk + per - 1) / per);
}

static void sk_check_shape(int64_t in_dim, int64_t out_dim, int64_t rows) {
  TORCH_CHECK(rows >= SK_MIN_ROWS && rows <= SK_MAX_ROWS, "gemm_nf4_skinny takes 9..32 rows, got ", rows,
              " (1..8 rows run gemv_nf4, more than 32 the prefill GEMM)");
  TORCH_CHECK(in_dim > 0 && in_dim % SK_KSTEP == 0, "gemm_nf4_skinny needs in % 32 == 0, got ", in_dim);
  TORCH_CHECK(out_dim > 0 && out_dim % 64 == 0, "gemm_nf4_skinny needs out % 64 == 0, got ", out_dim);
}

int64_t gemm_nf4_skinny_splits(int64_t in_dim, int64_t out_dim, int64_t rows, int64_t splits_override) {
  sk_check_shape(in_dim, out_dim, rows);
  int per;
  return sk_policy(in_dim, out_dim, rows, splits_override, &per);
}

torch::Tensor gemm_nf4_skinny(
    torch::Tensor packed,     // [in, out/2] u8
    torch::Tensor absmax,     // [in, out/64] bf16
    torch::Tensor x,          // [rows, in] f32, 9 <= rows <= 32
    torch::Tensor workspace,  // f32; holds the partials when S * rows * out floats fit
    c10::optional<torch::Tensor> residual,
    int64_t epilogue,
    int64_t splits_override,
    c10::optional<torch::Tensor> bias,        // [out] bf16, added pre-activation
    c10::optional<torch::Tensor> absmax_t) {  // [out/64, in] bf16 (transposed copy), optional
  TORCH_CHECK(packed.is_cuda() && packed.dtype() == torch::kUInt8 && packed.dim() == 2 && packed.is_contiguous(),
              "gemm_nf4_skinny: packed must be a contiguous u8 [in, out/2] GPU tensor");
  const int64_t in_dim = packed.size(0), out_dim = packed.size(1) * 2;
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kFloat32 && x.dim() == 2 && x.is_contiguous(),
              "gemm_nf4_skinny: x must be a contiguous f32 [rows, in] GPU tensor");
  TORCH_CHECK(x.size(1) == in_dim, "gemm_nf4_skinny: x has ", x.size(1), " columns, the weight has ", in_dim, " rows");
  const int64_t rows = x.size(0);
  sk_check_shape(in_dim, out_dim, rows);
  TORCH_CHECK(absmax.is_cuda() && absmax.dtype() == torch::kBFloat16 && absmax.dim() == 2 && absmax.is_contiguous() &&
                  absmax.size(0) == in_dim && absmax.size(1) * 64 == out_dim,
              "gemm_nf4_skinny: absmax must be a contiguous bf16 [in, out/64] GPU tensor");
  TORCH_CHECK(workspace.is_cuda() && workspace.dtype() == torch::kFloat32 && workspace.is_contiguous(),
              "gemm_nf4_skinny: workspace must be a contiguous f32 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(packed.data_ptr()) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "gemm_nf4_skinny: packed must be 8-byte and x 16-byte aligned");
  const unsigned short* amt_p = nullptr;
  if (absmax_t.has_value() && absmax_t->defined() && absmax_t->numel() > 0) {
    TORCH_CHECK(absmax_t->is_cuda() && absmax_t->dtype() == torch::kBFloat16 && absmax_t->is_contiguous() &&
                    absmax_t->dim() == 2 && absmax_t->size(0) == out_dim / 64 && absmax_t->size(1) == in_dim &&
                    reinterpret_cast<uintptr_t>(absmax_t->data_ptr()) % 16 == 0,
                "gemm_nf4_skinny: absmax_t must be a contiguous, 16-byte aligned bf16 [out/64, in] GPU tensor");
    amt_p = reinterpret_cast<const unsigned short*>(absmax_t->data_ptr());
  }

  int per;
  const int splits = sk_policy(in_dim, out_dim, rows, splits_override, &per);
  const int64_t need = (int64_t)splits * rows * out_dim;
  auto f32opts = x.options().dtype(torch::kFloat32);
  torch::Tensor partials = workspace.numel() >= need ? workspace : torch::empty({need}, f32opts);

  dim3 grid((unsigned)((out_dim + SK_TILE_N - 1) / SK_TILE_N), (unsigned)splits);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_SK(G, AMT)                                                              \
  nf4_skinny_kernel<G, AMT><<<grid, WAVE * SK_WAVES, 0, stream>>>(                     \
      packed.data_ptr<unsigned char>(),                                                \
      reinterpret_cast<const unsigned short*>(absmax.data_ptr()), amt_p,               \
      x.data_ptr<float>(), partials.data_ptr<float>(), (int)rows, (int)in_dim, (int)out_dim, per)
  if (rows <= 16) {
    if (amt_p) LAUNCH_SK(1, true); else LAUNCH_SK(1, false);
  } else {
    if (amt_p) LAUNCH_SK(2, true); else LAUNCH_SK(2, false);
  }
#undef LAUNCH_SK
  HIP_CHECK_LAST();

  if (epilogue < 0) {
    // RAW mode, as gemv_nf4: the caller fuses its own reduce (qkv_rope_reduce[_multi])
    return partials.view(-1).narrow(0, 0, need).view({(int64_t)splits, rows, out_dim});
  }
  return launch_gemv_reduce(partials, residual, bias, splits, (int)rows, (int)out_dim, (int)epilogue, f32opts,
                            absmax.options());
}
