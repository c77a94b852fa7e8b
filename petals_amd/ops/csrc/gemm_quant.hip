// Dense prefill GEMM with the weight dequant fused into the LDS staging
// (CDNA4 / gfx950):  C[M, out] = X[M, in] . W[in, out]  (+ bias)
//
// W stays in the packed form _FastWeight holds and is dequantized on the way
// into LDS, so its bf16 copy never exists in HBM:
//   nf4:  packed u8 [in, out/2] (even column = low nibble),
//         absmax bf16 [in, out/64] (blocks of 64 along out)
//   int8: q8 s8 [in, out], scale8 bf16 [out] (per output column)
//   mxfp4: packed u8 [in/2, out] (rows 2j / 2j+1 = low / high nibble),
//         scales u8 [in/32, out] (E8M0, blocks of 32 along in; ops/mxfp4.py)
//
// One 256-thread workgroup owns a 128x128 C tile: 4 waves as 2x2, each with
// 4x4 mfma_f32_16x16x32_bf16 accumulator blocks (64 accumulator VGPRs). The
// k loop steps 64 with two LDS buffers: the global loads of step k+1 are
// issued before the MFMAs of step k and written to the other buffer after
// them, one barrier per step. Both tiles are [row][k] images with 128-byte
// rows whose 16-byte chunks are XOR-permuted by row & 7: X rows land as
// ds_write_b128, W lands transposed as ds_write_b64 (4 k values of one
// column per write), and every MFMA fragment is one ds_read_b128. The MFMA
// runs on the transposed problem (W^T fragment as the A operand) so a lane
// ends up with 4 consecutive output columns of one row: 8-byte C stores.
//
// NF4 elements are bf16(LUT[nibble] * float(absmax)), bit for bit what
// nf4_dequantize writes, so the fused path differs from dequant + matmul only
// in summation order. int8 stages the s8 value as bf16 (exact) and applies
// the column scale to the fp32 accumulator in the epilogue. MXFP4 needs no
// LUT: a thread's two 8-byte packed loads hold its 4 k rows x 8 columns, and
// per column two v_cvt_scalef32_pk_bf16_fp4 (byte = two consecutive k, one
// shared power-of-two scale, exact) give the 4 bf16 of the ds_write_b64. The
// elements are bit for bit what mxfp4_dequantize writes.
//
// Rows >= M and columns >= out are never loaded and never stored: their
// fragments are zero-filled. Requires in % 64 == 0 and out % 64 == 0.
//
// Few-tile shapes (M <= 128 into o_proj is 64 workgroups on 256 CUs) run a
// deterministic two-phase split-K: grid.z slices of the k range write fp32
// partial tiles to a workspace, and a second kernel sums the slices in index
// order and applies scale, bias and the bf16 rounding. No atomics: the split
// count is a function of the shape alone, so two runs are bit-identical.

#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define GQ_MT 128
#define GQ_NT 128
#define GQ_KT 64
#define GQ_ROWB (GQ_KT * 2)                 // LDS row pitch in bytes (no padding)
#define GQ_TILE_B (GQ_MT * GQ_ROWB)         // one staged tile (A or B): 16384 B
#define GQ_LUT_B 2048                       // 256 x float2 pair LUT
#define GQ_LDS_B (GQ_LUT_B + 4 * GQ_TILE_B)  // LUT + 2 buffers x (A, B)

// byte offset of (row r, k byte kb) in a staged tile: the row's eight 16-byte
// chunks are permuted by r & 7, which makes the fragment reads, the A writes
// and the B writes all conflict-free (scripts/gemm_quant_lds_model.py)
#define GQ_BYTE(r, kb) \
  (((unsigned)(r)) * GQ_ROWB + (((unsigned)(kb)) ^ ((((unsigned)(r)) & 7u) << 4)))

using bf16x8_gq = __attribute__((ext_vector_type(8))) short;
using f32x4_gq = __attribute__((ext_vector_type(4))) float;
using f32x2_gq = __attribute__((ext_vector_type(2))) float;
using bf16x2_gq = __attribute__((ext_vector_type(2))) __bf16;

static __device__ __constant__ float GQ_NF4_LUT[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f,
    0.33791524171829224f, 0.4407098293304443f, 0.5626170039176941f,
    0.7229568362236023f, 1.0f};

// two fp32 -> packed bf16 pair, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned int gq_pack_bf16(float lo, float hi) {
  const bf16x2_gq r = __builtin_convertvector(f32x2_gq{lo, hi}, bf16x2_gq);
  return __builtin_bit_cast(unsigned int, r);
}

// s8 -> bf16 bits (exact: |v| <= 127 needs 7 significand bits)
__device__ __forceinline__ unsigned int gq_s8_bf16(unsigned int word, int byte) {
  const int v = (int)(word << (24 - 8 * byte)) >> 24;
  return __float_as_uint((float)v) >> 16;
}

enum GqMode : int { GQ_NF4 = 0, GQ_INT8 = 1, GQ_MXFP4 = 2 };

// byte BYTE of `word` (two consecutive-k fp4 of one column) * scale -> packed
// bf16 pair, low nibble in the low half
template <int BYTE>
__device__ __forceinline__ unsigned int gq_fp4_bf16x2(unsigned int word, float scale) {
  const bf16x2_gq r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, BYTE);
  return __builtin_bit_cast(unsigned int, r);
}

template <int BYTE>
__device__ __forceinline__ uint2 gq_fp4_quad(unsigned int w01, unsigned int w23, unsigned int s4) {
  const float sc = __uint_as_float(((s4 >> (8 * BYTE)) & 0xFFu) << 23);
  uint2 o;
  o.x = gq_fp4_bf16x2<BYTE>(w01, sc);
  o.y = gq_fp4_bf16x2<BYTE>(w23, sc);
  return o;
}

template <GqMode MODE, bool SPLIT>
__global__ __launch_bounds__(256) void gemm_quant_kernel(
    const unsigned char* __restrict__ wq,        // nf4: packed [in, out/2]; int8: q8 [in, out]; mxfp4: packed [in/2, out]
    const void* __restrict__ wscale_v,           // nf4: absmax [in, out/64]; int8: scale8 [out]; mxfp4: scales u8 [in/32, out]
    const unsigned short* __restrict__ x,        // [M, in] bf16
    const unsigned short* __restrict__ bias,     // [out] bf16 or null
    unsigned short* __restrict__ c,              // [M, out] bf16 (SPLIT: unused)
    float* __restrict__ ws,                      // SPLIT: [splits, M, out] fp32 partials
    int M,
    int in_dim,
    int out_dim,
    int ksteps_per_split) {
  constexpr bool NF4 = MODE == GQ_NF4;
  constexpr bool MX = MODE == GQ_MXFP4;
  const unsigned short* wscale = reinterpret_cast<const unsigned short*>(wscale_v);
  __shared__ __attribute__((aligned(16))) unsigned char lds[GQ_LDS_B];
  float2* lut2 = reinterpret_cast<float2*>(lds);

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int hi = lane >> 4;
  const int wr = wave >> 1;  // wave row (64 C rows)
  const int wc = wave & 1;   // wave col (64 C cols)
  const int m0 = blockIdx.x * GQ_MT;
  const int n0 = blockIdx.y * GQ_NT;

  if (NF4) {
    lut2[tid] = make_float2(GQ_NF4_LUT[tid & 0xF], GQ_NF4_LUT[tid >> 4]);
  }

  // ---- staging roles
  // A: thread moves 4 x 16 B: rows (tid>>3) + 32*i, 16-byte chunk tid&7
  const int a_chunk = tid & 7;
  const int a_row = tid >> 3;
  // B: thread owns 4 consecutive k rows (kq) x 8 consecutive columns; the 16
  // lanes one ds_write_b64 group serves hold the 16 k quads of ONE column
  const int kq = tid & 15;
  const int nloc = (tid >> 4) * 8;
  const bool b_live = n0 + nloc < out_dim;  // out % 64 == 0: all 8 columns in or out

  uint4 ra[4];
  unsigned int rb[4][2];  // nf4 uses word 0 only; mxfp4: rows [0], [1] = k pairs, [2][0..1] = scales
  float am[4];

  auto load_tiles = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + a_row + 32 * i;
      ra[i] = make_uint4(0u, 0u, 0u, 0u);
      if (m < M)
        ra[i] = *reinterpret_cast<const uint4*>(x + (size_t)m * in_dim + kt + a_chunk * 8);
    }
    if (MX) {
      // 4 k rows = packed rows k/2, k/2+1; kt and kq*4 are multiples of 4, so
      // the rows never straddle a 32-row scale block
      const size_t k = (size_t)(kt + kq * 4);
#pragma unroll
      for (int j = 0; j < 3; ++j) rb[j][0] = rb[j][1] = 0u;
      if (b_live) {
        const unsigned char* p = wq + (k >> 1) * (size_t)out_dim + n0 + nloc;
        const uint2 q0 = *reinterpret_cast<const uint2*>(p);
        const uint2 q1 = *reinterpret_cast<const uint2*>(p + out_dim);
        const uint2 s8 = *reinterpret_cast<const uint2*>(
            reinterpret_cast<const unsigned char*>(wscale_v) + (k >> 5) * (size_t)out_dim + n0 + nloc);
        rb[0][0] = q0.x; rb[0][1] = q0.y;
        rb[1][0] = q1.x; rb[1][1] = q1.y;
        rb[2][0] = s8.x; rb[2][1] = s8.y;
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t k = (size_t)(kt + kq * 4 + j);
      rb[j][0] = rb[j][1] = 0u;
      am[j] = 0.f;
      if (NF4) {
        if (b_live) {
          rb[j][0] = *reinterpret_cast<const unsigned int*>(wq + k * (size_t)(out_dim >> 1) + ((n0 + nloc) >> 1));
          am[j] = bf16_to_f32(wscale[k * (size_t)(out_dim >> 6) + ((n0 + nloc) >> 6)]);
        }
      } else {
        if (b_live) {
          const uint2 q = *reinterpret_cast<const uint2*>(wq + k * (size_t)out_dim + n0 + nloc);
          rb[j][0] = q.x;
          rb[j][1] = q.y;
        }
      }
    }
  };

  auto store_tiles = [&](int buf) {
    unsigned char* at = lds + GQ_LUT_B + buf * 2 * GQ_TILE_B;
    unsigned char* bt = at + GQ_TILE_B;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<uint4*>(&at[GQ_BYTE(a_row + 32 * i, a_chunk * 16)]) = ra[i];
    if (MX) {
      // a dead thread staged zero bytes and a zero scale byte: +0 * 2^-127
      *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 0, kq * 8)]) = gq_fp4_quad<0>(rb[0][0], rb[1][0], rb[2][0]);
      *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 1, kq * 8)]) = gq_fp4_quad<1>(rb[0][0], rb[1][0], rb[2][0]);
      *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 2, kq * 8)]) = gq_fp4_quad<2>(rb[0][0], rb[1][0], rb[2][0]);
      *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 3, kq * 8)]) = gq_fp4_quad<3>(rb[0][0], rb[1][0], rb[2][0]);
      *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 4, kq * 8)]) = gq_fp4_quad<0>(rb[0][1], rb[1][1], rb[2][1]);
      *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 5, kq * 8)]) = gq_fp4_quad<1>(rb[0][1], rb[1][1], rb[2][1]);
      *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 6, kq * 8)]) = gq_fp4_quad<2>(rb[0][1], rb[1][1], rb[2][1]);
      *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 7, kq * 8)]) = gq_fp4_quad<3>(rb[0][1], rb[1][1], rb[2][1]);
    } else if (NF4) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float2 w2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w2[j] = lut2[(rb[j][0] >> (8 * b)) & 0xFFu];
        uint2 lo, hh;
        lo.x = gq_pack_bf16(w2[0].x * am[0], w2[1].x * am[1]);
        lo.y = gq_pack_bf16(w2[2].x * am[2], w2[3].x * am[3]);
        hh.x = gq_pack_bf16(w2[0].y * am[0], w2[1].y * am[1]);
        hh.y = gq_pack_bf16(w2[2].y * am[2], w2[3].y * am[3]);
        *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 2 * b, kq * 8)]) = lo;
        *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + 2 * b + 1, kq * 8)]) = hh;
      }
    } else {
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const int w = v >> 2;
        uint2 o;
        o.x = gq_s8_bf16(rb[0][w], v & 3) | (gq_s8_bf16(rb[1][w], v & 3) << 16);
        o.y = gq_s8_bf16(rb[2][w], v & 3) | (gq_s8_bf16(rb[3][w], v & 3) << 16);
        *reinterpret_cast<uint2*>(&bt[GQ_BYTE(nloc + v, kq * 8)]) = o;
      }
    }
  };

  f32x4_gq acc[4][4];
#pragma unroll
  for (int rbk = 0; rbk < 4; ++rbk)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[rbk][nb] = f32x4_gq{0.f, 0.f, 0.f, 0.f};

  // a wave whose whole 64x64 sub-tile lies outside C still stages and syncs
  const bool wave_live = (m0 + wr * 64 < M) && (n0 + wc * 64 < out_dim);

  // this workgroup's k steps [ks0, ks1): everything, or slice blockIdx.z
  const int nk = in_dim / GQ_KT;
  const int ks0 = SPLIT ? (int)blockIdx.z * ksteps_per_split : 0;
  const int ks1 = SPLIT ? min(nk, ks0 + ksteps_per_split) : nk;
  load_tiles(ks0 * GQ_KT);
  __syncthreads();  // LUT visible
  store_tiles(0);
  __syncthreads();

  for (int ks = ks0; ks < ks1; ++ks) {
    const int cur = (ks - ks0) & 1;
    const bool more = ks + 1 < ks1;
    if (more) load_tiles((ks + 1) * GQ_KT);

    if (wave_live) {
      const unsigned char* at = lds + GQ_LUT_B + cur * 2 * GQ_TILE_B;
      const unsigned char* bt = at + GQ_TILE_B;
#pragma unroll
      for (int kc = 0; kc < GQ_KT / 32; ++kc) {
        bf16x8_gq a_frag[4], b_frag[4];
#pragma unroll
        for (int rbk = 0; rbk < 4; ++rbk)
          a_frag[rbk] = *reinterpret_cast<const bf16x8_gq*>(
              &at[GQ_BYTE(wr * 64 + rbk * 16 + col, kc * 64 + hi * 16)]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          b_frag[nb] = *reinterpret_cast<const bf16x8_gq*>(
              &bt[GQ_BYTE(wc * 64 + nb * 16 + col, kc * 64 + hi * 16)]);
        // transposed product: lane (col, hi) holds C[m = col][n = hi*4 + r]
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
          for (int rbk = 0; rbk < 4; ++rbk)
            acc[rbk][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                b_frag[nb], a_frag[rbk], acc[rbk][nb], 0, 0, 0);
      }
    }

    if (more) store_tiles(cur ^ 1);
    __syncthreads();
  }

  if (!wave_live) return;
  if (SPLIT) {
    // ---- raw fp32 partials; gemm_quant_reduce_kernel finishes them
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int n = n0 + wc * 64 + nb * 16 + hi * 4;
      if (n >= out_dim) continue;
#pragma unroll
      for (int rbk = 0; rbk < 4; ++rbk) {
        const int m = m0 + wr * 64 + rbk * 16 + col;
        if (m >= M) continue;
        *reinterpret_cast<f32x4_gq*>(ws + ((size_t)blockIdx.z * M + m) * out_dim + n) = acc[rbk][nb];
      }
    }
    return;
  }
  // ---- epilogue: (int8 column scale) + bias in fp32, one bf16 rounding
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int n = n0 + wc * 64 + nb * 16 + hi * 4;
    if (n >= out_dim) continue;  // out % 64 == 0: the 4 columns are all in or all out
    float sc[4] = {1.f, 1.f, 1.f, 1.f};
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE == GQ_INT8) {
      const uint2 s = *reinterpret_cast<const uint2*>(wscale + n);
      sc[0] = bf16_to_f32((unsigned short)(s.x & 0xFFFFu));
      sc[1] = bf16_to_f32((unsigned short)(s.x >> 16));
      sc[2] = bf16_to_f32((unsigned short)(s.y & 0xFFFFu));
      sc[3] = bf16_to_f32((unsigned short)(s.y >> 16));
    }
    if (bias != nullptr) {
      const uint2 s = *reinterpret_cast<const uint2*>(bias + n);
      bs[0] = bf16_to_f32((unsigned short)(s.x & 0xFFFFu));
      bs[1] = bf16_to_f32((unsigned short)(s.x >> 16));
      bs[2] = bf16_to_f32((unsigned short)(s.y & 0xFFFFu));
      bs[3] = bf16_to_f32((unsigned short)(s.y >> 16));
    }
#pragma unroll
    for (int rbk = 0; rbk < 4; ++rbk) {
      const int m = m0 + wr * 64 + rbk * 16 + col;
      if (m >= M) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = acc[rbk][nb][r];
        if (MODE == GQ_INT8) v[r] *= sc[r];
        if (bias != nullptr) v[r] += bs[r];
      }
      uint2 o;
      o.x = gq_pack_bf16(v[0], v[1]);
      o.y = gq_pack_bf16(v[2], v[3]);
      *reinterpret_cast<uint2*>(c + (size_t)m * out_dim + n) = o;
    }
  }
}

// split-K phase 2: one thread per 4 consecutive columns of one row sums the
// slices in index order, then the same epilogue as the direct kernel
template <GqMode MODE>
__global__ __launch_bounds__(256) void gemm_quant_reduce_kernel(
    const float* __restrict__ ws,               // [splits, M, out]
    const unsigned short* __restrict__ wscale,  // int8: scale8 [out]
    const unsigned short* __restrict__ bias,    // [out] bf16 or null
    unsigned short* __restrict__ c,             // [M, out] bf16
    long n_elems,                               // M * out
    int out_dim,
    int splits) {
  const long e = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (e >= n_elems) return;
  const int n = (int)(e % out_dim);
  f32x4_gq s = *reinterpret_cast<const f32x4_gq*>(ws + e);
  for (int z = 1; z < splits; ++z) {
    const f32x4_gq p = *reinterpret_cast<const f32x4_gq*>(ws + (size_t)z * n_elems + e);
    s += p;
  }
  float v[4] = {s[0], s[1], s[2], s[3]};
  if (MODE == GQ_INT8) {
    const uint2 q = *reinterpret_cast<const uint2*>(wscale + n);
    v[0] *= bf16_to_f32((unsigned short)(q.x & 0xFFFFu));
    v[1] *= bf16_to_f32((unsigned short)(q.x >> 16));
    v[2] *= bf16_to_f32((unsigned short)(q.y & 0xFFFFu));
    v[3] *= bf16_to_f32((unsigned short)(q.y >> 16));
  }
  if (bias != nullptr) {
    const uint2 q = *reinterpret_cast<const uint2*>(bias + n);
    v[0] += bf16_to_f32((unsigned short)(q.x & 0xFFFFu));
    v[1] += bf16_to_f32((unsigned short)(q.x >> 16));
    v[2] += bf16_to_f32((unsigned short)(q.y & 0xFFFFu));
    v[3] += bf16_to_f32((unsigned short)(q.y >> 16));
  }
  uint2 o;
  o.x = gq_pack_bf16(v[0], v[1]);
  o.y = gq_pack_bf16(v[2], v[3]);
  *reinterpret_cast<uint2*>(c + e) = o;
}

// ------------------------------------------------------------------- host

#define GQ_WG_SLOTS 512       // 256 CUs x 2 resident workgroups (LDS-bound)
#define GQ_MIN_SPLIT_STEPS 4  // k steps a slice must keep

static void gq_check_common(const torch::Tensor& x, const c10::optional<torch::Tensor>& bias,
                            int64_t in_dim, int64_t out_dim, const char* op) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.dim() == 2 && x.is_contiguous(),
              op, ": x must be a contiguous bf16 [M, in] GPU tensor");
  TORCH_CHECK(x.size(1) == in_dim, op, ": x has ", x.size(1), " columns, the weight has ", in_dim, " rows");
  TORCH_CHECK(in_dim > 0 && in_dim % GQ_KT == 0, op, " needs in % 64 == 0");
  TORCH_CHECK(out_dim > 0 && out_dim % 64 == 0, op, " needs out % 64 == 0");
  TORCH_CHECK((out_dim + GQ_NT - 1) / GQ_NT <= 65535, op, ": out too large");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, op, ": x must be 16-byte aligned");
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->dtype() == torch::kBFloat16 && bias->dim() == 1 &&
                    bias->is_contiguous() && bias->size(0) == out_dim,
                op, ": bias must be a contiguous bf16 [out] GPU tensor");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(bias->data_ptr()) % 8 == 0, op, ": bias must be 8-byte aligned");
  }
}

template <GqMode MODE>
static torch::Tensor gq_launch(const torch::Tensor& wq, const torch::Tensor& wscale, const torch::Tensor& x,
                               const c10::optional<torch::Tensor>& bias, int64_t in_dim, int64_t out_dim) {
  const int64_t M = x.size(0);
  auto c = torch::empty({M, out_dim}, x.options());
  if (M == 0) return c;
  const int64_t row_tiles = (M + GQ_MT - 1) / GQ_MT, col_tiles = (out_dim + GQ_NT - 1) / GQ_NT;
  const int nk = (int)(in_dim / GQ_KT);
  // split-K when the C tiles alone leave most of the chip idle
  int per = nk, splits = 1;
  const int64_t want = GQ_WG_SLOTS / (row_tiles * col_tiles);
  if (want >= 2 && nk >= 2 * GQ_MIN_SPLIT_STEPS) {
    per = std::max<int>(GQ_MIN_SPLIT_STEPS, (int)((nk + want - 1) / want));
    splits = (nk + per - 1) / per;
  }
  const unsigned char* wq_p = reinterpret_cast<const unsigned char*>(wq.data_ptr());
  const void* ws_p = wscale.data_ptr();
  const unsigned short* x_p = reinterpret_cast<const unsigned short*>(x.data_ptr());
  const unsigned short* b_p =
      bias.has_value() ? reinterpret_cast<const unsigned short*>(bias->data_ptr()) : nullptr;
  unsigned short* c_p = reinterpret_cast<unsigned short*>(c.data_ptr());
  auto stream = at::cuda::getCurrentCUDAStream();
  if (splits < 2) {
    dim3 grid((unsigned)row_tiles, (unsigned)col_tiles);
    gemm_quant_kernel<MODE, false><<<grid, 256, 0, stream>>>(
        wq_p, ws_p, x_p, b_p, c_p, nullptr, (int)M, (int)in_dim, (int)out_dim, nk);
    HIP_CHECK_LAST();
    return c;
  }
  // every (slice, valid row, valid column) is written by phase 1 before phase 2 reads it
  auto part = torch::empty({(int64_t)splits, M, out_dim}, x.options().dtype(torch::kFloat32));
  dim3 grid((unsigned)row_tiles, (unsigned)col_tiles, (unsigned)splits);
  gemm_quant_kernel<MODE, true><<<grid, 256, 0, stream>>>(
      wq_p, ws_p, x_p, nullptr, nullptr, part.data_ptr<float>(), (int)M, (int)in_dim, (int)out_dim, per);
  HIP_CHECK_LAST();
  const long n_elems = (long)M * out_dim;
  const long threads = n_elems / 4;
  gemm_quant_reduce_kernel<MODE><<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(
      part.data_ptr<float>(), reinterpret_cast<const unsigned short*>(ws_p), b_p, c_p, n_elems, (int)out_dim, splits);
  HIP_CHECK_LAST();
  return c;
}

torch::Tensor gemm_nf4(
    torch::Tensor packed,  // [in, out/2] u8
    torch::Tensor absmax,  // [in, out/64] bf16
    torch::Tensor x,       // [M, in] bf16
    c10::optional<torch::Tensor> bias) {
  TORCH_CHECK(packed.is_cuda() && packed.dtype() == torch::kUInt8 && packed.dim() == 2 && packed.is_contiguous(),
              "gemm_nf4: packed must be a contiguous u8 [in, out/2] GPU tensor");
  const int64_t in_dim = packed.size(0), out_dim = packed.size(1) * 2;
  TORCH_CHECK(absmax.is_cuda() && absmax.dtype() == torch::kBFloat16 && absmax.dim() == 2 &&
                  absmax.is_contiguous() && absmax.size(0) == in_dim && absmax.size(1) * 64 == out_dim,
              "gemm_nf4: absmax must be a contiguous bf16 [in, out/64] GPU tensor");
  gq_check_common(x, bias, in_dim, out_dim, "gemm_nf4");
  TORCH_CHECK(x.size(0) < (1 << 30), "gemm_nf4: too many rows");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(packed.data_ptr()) % 4 == 0, "gemm_nf4: packed must be 4-byte aligned");
  return gq_launch<GQ_NF4>(packed, absmax, x, bias, in_dim, out_dim);
}

torch::Tensor gemm_int8(
    torch::Tensor q8,      // [in, out] s8
    torch::Tensor scale8,  // [out] bf16
    torch::Tensor x,       // [M, in] bf16
    c10::optional<torch::Tensor> bias) {
  TORCH_CHECK(q8.is_cuda() && q8.dtype() == torch::kInt8 && q8.dim() == 2 && q8.is_contiguous(),
              "gemm_int8: q8 must be a contiguous s8 [in, out] GPU tensor");
  const int64_t in_dim = q8.size(0), out_dim = q8.size(1);
  TORCH_CHECK(scale8.is_cuda() && scale8.dtype() == torch::kBFloat16 && scale8.dim() == 1 &&
                  scale8.is_contiguous() && scale8.size(0) == out_dim,
              "gemm_int8: scale8 must be a contiguous bf16 [out] GPU tensor");
  gq_check_common(x, bias, in_dim, out_dim, "gemm_int8");
  TORCH_CHECK(x.size(0) < (1 << 30), "gemm_int8: too many rows");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q8.data_ptr()) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(scale8.data_ptr()) % 8 == 0,
              "gemm_int8: q8 and scale8 must be 8-byte aligned");
  return gq_launch<GQ_INT8>(q8, scale8, x, bias, in_dim, out_dim);
}

torch::Tensor gemm_mxfp4(
    torch::Tensor packed,  // [in/2, out] u8
    torch::Tensor scales,  // [in/32, out] u8 (E8M0)
    torch::Tensor x,       // [M, in] bf16
    c10::optional<torch::Tensor> bias) {
  TORCH_CHECK(packed.is_cuda() && packed.dtype() == torch::kUInt8 && packed.dim() == 2 && packed.is_contiguous(),
              "gemm_mxfp4: packed must be a contiguous u8 [in/2, out] GPU tensor");
  const int64_t in_dim = packed.size(0) * 2, out_dim = packed.size(1);
  TORCH_CHECK(scales.is_cuda() && scales.dtype() == torch::kUInt8 && scales.dim() == 2 &&
                  scales.is_contiguous() && scales.size(0) * 32 == in_dim && scales.size(1) == out_dim,
              "gemm_mxfp4: scales must be a contiguous u8 [in/32, out] GPU tensor");
  gq_check_common(x, bias, in_dim, out_dim, "gemm_mxfp4");
  TORCH_CHECK(x.size(0) < (1 << 30), "gemm_mxfp4: too many rows");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(packed.data_ptr()) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(scales.data_ptr()) % 8 == 0,
              "gemm_mxfp4: packed and scales must be 8-byte aligned");
  return gq_launch<GQ_MXFP4>(packed, scales, x, bias, in_dim, out_dim);
}
