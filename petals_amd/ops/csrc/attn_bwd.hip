// Flash-style MFMA attention backward for CDNA4 (gfx950): bf16, causal, GQA,
// head_dim 64/128, kv_len == S. The training counterpart of prefill_attn.hip
// (whose LSE form writes lse2 = m + log2(l) in the log2 domain).
//
// With p = exp2(s2 - lse2) recomputed from q~ = bf16(q*scale*log2e) and K:
//   D_i = sum_d dO_i*O_i        dP = dO V^T        dS = p o (dP - D)
//   dV = P^T dO                 dK = scale dS^T Q  dQ = scale dS K
//
// No atomics: two passes, each output element has one owner and a fixed
// summation order.
//   attn_bwd_delta_kernel  D, once, read by both passes
//   attn_bwd_dkdv_kernel   a workgroup owns 64 keys of one (batch, kv head),
//                          a wave 16 of them: K/V rows stay A-fragments, dK/dV
//                          fp32 C-layout accumulators, for the whole kernel.
//                          It loops over the kv head's q heads and over the
//                          32-row q tiles at or below the diagonal, so the GQA
//                          sum happens in registers. It forms the TRANSPOSED
//                          products S^T = K q~^T and dP^T = V dO^T directly
//                          (their B fragments are contiguous rows of the
//                          row-major staged q~ / dO), sends P^T and dS^T
//                          through a per-wave LDS scratch into A layout, and
//                          takes the B fragments of dV += P^T dO and
//                          dK += dS^T Q from transposed, swizzled images of dO
//                          and of the unscaled Q staged next to the row-major
//                          ones.
//   attn_bwd_dq_kernel     the forward's shape: 4 waves x 16 q rows of one
//                          (batch, q head), q~ and dO as A-fragments, lse2 and
//                          D in the per-lane row slots; per 64-key tile it
//                          stages K and V row-major and K transposed+swizzled,
//                          dS goes through the per-wave scratch, dQ += dS K.
//   attn_bwd_reduce_kernel only when the q heads of a kv head were split over
//                          grid.z for occupancy: sums the fp32 dK/dV slabs in
//                          slice order and rounds once.
//
// Fragment layouts (mfma_f32_16x16x32_bf16, scripts/mfma_verify.hip): A and B
// lane -> row/col = lane&15, k = (lane>>4)*8 + e; C lane -> col = lane&15,
// rows (lane>>4)*4 + r. LDS images are checked by scripts/attn_bwd_lds_model.py.
// Rounding points: q~, P and dS to bf16 before they enter an MFMA; dq, dk, dv
// to bf16 once from their fp32 sums. Everything else is fp32.

#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

#define BW_WAVES 4
#define BW_KT 64   // keys per tile, both passes
#define BW_QT 32   // q rows per staged tile of the dK/dV pass
#define BW_PAD 8   // LDS row padding (elements)
#define BW_LOG2E 1.4426950408889634f
// these kernels are compiled without packed fp32 VALU ops
#define BW_KERNEL __attribute__((target("no-packed-fp32-ops")))

// transposed image [dim][T + BW_PAD] with the forward's XOR swizzle on the
// dim group (VT_BYTE in prefill_attn.hip)
#define TR_BYTE(T, dim, row_byte) \
  ((((unsigned)(dim)) * (((T) + BW_PAD) * 2) + (unsigned)(row_byte)) ^ ((((unsigned)(dim) >> 3) & 7u) << 4))

#define BF8_ZERO (bf16x8{0, 0, 0, 0, 0, 0, 0, 0})

__device__ __forceinline__ BW_KERNEL bf16x8 bw_prescale(bf16x8 raw, float qscale) {
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    union { float f; uint32_t i; } v;
    v.i = uint32_t((unsigned short)raw[e]) << 16;
    v.f *= qscale;
    const uint32_t lsb = (v.i >> 16) & 1;  // round-to-nearest-even, as f32_to_bf16
    r[e] = (short)((v.i + 0x7FFFu + lsb) >> 16);
  }
  return r;
}

__device__ __forceinline__ BW_KERNEL unsigned short bw_bf16(float f) {
  union { float f; uint32_t i; } v;
  v.f = f;
  const uint32_t lsb = (v.i >> 16) & 1;
  return (unsigned short)((v.i + 0x7FFFu + lsb) >> 16);
}

// ---------------------------------------------------------------- D = dO . O
template <int HD>
__global__ __launch_bounds__(256) BW_KERNEL void attn_bwd_delta_kernel(
    const unsigned short* __restrict__ out,   // [rows, HD]
    const unsigned short* __restrict__ dout,  // [rows, HD]
    float* __restrict__ delta,                // [rows]
    int n_rows) {
  constexpr int LPR = HD / 8;  // lanes per row
  const int row = blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const int c8 = (threadIdx.x % LPR) * 8;
  float acc = 0.f;
  if (row < n_rows) {
    const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(out + (size_t)row * HD + c8);
    const bf16x8 d8 = *reinterpret_cast<const bf16x8*>(dout + (size_t)row * HD + c8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      union { float f; uint32_t i; } a, c;
      a.i = uint32_t((unsigned short)o8[e]) << 16;
      c.i = uint32_t((unsigned short)d8[e]) << 16;
      acc += a.f * c.f;
    }
  }
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  if (row < n_rows && c8 == 0) delta[row] = acc;
}

// -------------------------------------------------------------- dK, dV pass
template <int HD>
__global__ __launch_bounds__(BW_WAVES * 64) BW_KERNEL void attn_bwd_dkdv_kernel(
    const unsigned short* __restrict__ q,     // [B, QH, S, HD]
    const unsigned short* __restrict__ k,     // [B, KVH, S, HD]
    const unsigned short* __restrict__ v,     // [B, KVH, S, HD]
    const unsigned short* __restrict__ dout,  // [B, QH, S, HD]
    const float* __restrict__ lse,            // [B, QH, S]
    const float* __restrict__ delta,          // [B, QH, S]
    unsigned short* __restrict__ dk,          // [B, KVH, S, HD] (gridDim.z == 1)
    unsigned short* __restrict__ dv,
    float* __restrict__ part,                 // [gridDim.z][2][B, KVH, S, HD] f32 (gridDim.z > 1)
    int q_heads,
    int kv_heads,
    int s,
    float scale) {
  constexpr int KCH = HD / 32;     // 32-wide dim chunks
  constexpr int NBQ = BW_QT / 16;  // 16-row q column blocks per tile
  const int b = blockIdx.x / kv_heads;
  const int kvh = blockIdx.x - b * kv_heads;
  const int j0 = blockIdx.y * BW_KT;  // tile 0 has the most q tiles and is dispatched first
  const int gq = q_heads / kv_heads;
  const int g_per = gq / gridDim.z;
  const int g_lo = blockIdx.z * g_per;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int hi = lane >> 4;
  const int kb = j0 + wave * 16;  // this wave's first key
  const float qscale = scale * BW_LOG2E;

  __shared__ unsigned short q_lds[BW_QT][HD + BW_PAD];   // q~ row-major
  __shared__ unsigned short do_lds[BW_QT][HD + BW_PAD];  // dO row-major
  __shared__ unsigned char qt_raw[HD * (BW_QT + BW_PAD) * 2];   // Q transposed (unscaled)
  __shared__ unsigned char dot_raw[HD * (BW_QT + BW_PAD) * 2];  // dO transposed
  __shared__ unsigned short pt_lds[BW_WAVES][16][BW_QT + BW_PAD];   // P^T scratch [key][q]
  __shared__ unsigned short dst_lds[BW_WAVES][16][BW_QT + BW_PAD];  // dS^T scratch

  // ---- this wave's K and V rows as A-fragments (zero past s)
  bf16x8 kf[KCH], vf[KCH];
  const size_t kv_base = (((size_t)b * kv_heads + kvh) * s) * HD;
#pragma unroll
  for (int kc = 0; kc < KCH; ++kc) {
    kf[kc] = BF8_ZERO;
    vf[kc] = BF8_ZERO;
    if (kb + col < s) {
      kf[kc] = *reinterpret_cast<const bf16x8*>(k + kv_base + (size_t)(kb + col) * HD + kc * 32 + hi * 8);
      vf[kc] = *reinterpret_cast<const bf16x8*>(v + kv_base + (size_t)(kb + col) * HD + kc * 32 + hi * 8);
    }
  }

  f32x4 acc_dk[HD / 16], acc_dv[HD / 16];  // C layout: key = kb + hi*4 + r, dim = d*16 + col
#pragma unroll
  for (int d = 0; d < HD / 16; ++d) {
    acc_dk[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_dv[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int g = g_lo; g < g_lo + g_per; ++g) {
    const size_t row_base = ((size_t)b * q_heads + (size_t)kvh * gq + g) * s;  // in rows
    for (int i0 = j0; i0 < s; i0 += BW_QT) {
      // ---- stage the q tile: q~ and dO row-major, Q and dO transposed
      __syncthreads();
      for (int idx = tid; idx < BW_QT * (HD / 8); idx += BW_WAVES * WAVE) {
        const int row = idx / (HD / 8);
        const int c8 = (idx - row * (HD / 8)) * 8;
        bf16x8 q8 = BF8_ZERO;
        bf16x8 d8 = BF8_ZERO;
        if (i0 + row < s) {
          q8 = *reinterpret_cast<const bf16x8*>(q + (row_base + i0 + row) * HD + c8);
          d8 = *reinterpret_cast<const bf16x8*>(dout + (row_base + i0 + row) * HD + c8);
        }
        *reinterpret_cast<bf16x8*>(&q_lds[row][c8]) = bw_prescale(q8, qscale);
        *reinterpret_cast<bf16x8*>(&do_lds[row][c8]) = d8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          *reinterpret_cast<unsigned short*>(&qt_raw[TR_BYTE(BW_QT, c8 + e, row * 2)]) = (unsigned short)q8[e];
          *reinterpret_cast<unsigned short*>(&dot_raw[TR_BYTE(BW_QT, c8 + e, row * 2)]) = (unsigned short)d8[e];
        }
      }
      __syncthreads();

      // ---- lse2 and D: one value per C-layout column (q row i0 + nb*16 + col)
      float lse_c[NBQ], dl_c[NBQ];
#pragma unroll
      for (int nb = 0; nb < NBQ; ++nb) {
        const int qrow = i0 + nb * 16 + col;
        lse_c[nb] = qrow < s ? lse[row_base + qrow] : 0.f;
        dl_c[nb] = qrow < s ? delta[row_base + qrow] : 0.f;
      }

      // ---- S^T = K q~^T and dP^T = V dO^T: C[key = hi*4 + r][q = nb*16 + col]
      f32x4 st[NBQ], dpt[NBQ];
#pragma unroll
      for (int nb = 0; nb < NBQ; ++nb) {
        st[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        dpt[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) {
          // B[k = dim][n = q] = rowmajor[q = nb*16 + col][dim = kc*32 + hi*8 + e]
          const bf16x8 qb = *reinterpret_cast<const bf16x8*>(&q_lds[nb * 16 + col][kc * 32 + hi * 8]);
          const bf16x8 db = *reinterpret_cast<const bf16x8*>(&do_lds[nb * 16 + col][kc * 32 + hi * 8]);
          st[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kc], qb, st[nb], 0, 0, 0);
          dpt[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[kc], db, dpt[nb], 0, 0, 0);
        }
      }

      // ---- p = exp2(s2 - lse2), dS = p (dP - D); masked p is exactly 0.
      // Interior tiles (every key of this wave at or below every q row, no s
      // edge) skip the mask. A key >= s is above every live q row.
      const bool interior = (kb + 15 <= i0) && (i0 + BW_QT <= s);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kb + hi * 4 + r;
#pragma unroll
        for (int nb = 0; nb < NBQ; ++nb) {
          const int qrow = i0 + nb * 16 + col;
          float x = st[nb][r] - lse_c[nb];
          if (!interior && (key > qrow || qrow >= s)) x = NEG_SENTINEL;
          const float p = (x <= NEG_THRESHOLD) ? 0.f : exp2f(x);
          const float ds = p * (dpt[nb][r] - dl_c[nb]);
          pt_lds[wave][hi * 4 + r][nb * 16 + col] = bw_bf16(p);
          dst_lds[wave][hi * 4 + r][nb * 16 + col] = bw_bf16(ds);
        }
      }
      // per-wave round trip; a block barrier is the simple safe ordering
      __syncthreads();

      // ---- A[row = key][k = q = hi*8 + e]: one 32-row k-chunk per tile
      const bf16x8 pf = *reinterpret_cast<const bf16x8*>(&pt_lds[wave][col][hi * 8]);
      const bf16x8 dsf = *reinterpret_cast<const bf16x8*>(&dst_lds[wave][col][hi * 8]);
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) {
        // B[k = q][n = dim] = transposed[dim = d*16 + col][q = hi*8 + e]
        const bf16x8 dob = *reinterpret_cast<const bf16x8*>(&dot_raw[TR_BYTE(BW_QT, d * 16 + col, hi * 16)]);
        const bf16x8 qb = *reinterpret_cast<const bf16x8*>(&qt_raw[TR_BYTE(BW_QT, d * 16 + col, hi * 16)]);
        acc_dv[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, dob, acc_dv[d], 0, 0, 0);
        acc_dk[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, qb, acc_dk[d], 0, 0, 0);
      }
    }
  }

  // ---- write: C layout key = kb + hi*4 + r, dim = d*16 + col
  const size_t n_kv = (size_t)gridDim.x * s * HD;  // elements of one dk / dv tensor
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = kb + hi * 4 + r;
    if (key >= s) continue;
    const size_t off = kv_base + (size_t)key * HD;
    if (gridDim.z == 1) {
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) {
        dk[off + d * 16 + col] = bw_bf16(acc_dk[d][r] * scale);
        dv[off + d * 16 + col] = bw_bf16(acc_dv[d][r]);
      }
    } else {
      float* pk_ = part + (size_t)blockIdx.z * 2 * n_kv + off;
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) {
        pk_[d * 16 + col] = acc_dk[d][r] * scale;
        pk_[n_kv + d * 16 + col] = acc_dv[d][r];
      }
    }
  }
}

// sums the fp32 slabs of a split dK/dV pass in slice order, rounds once
__global__ __launch_bounds__(256) BW_KERNEL void attn_bwd_reduce_kernel(
    const float* __restrict__ part,  // [n_split][2][n_kv]
    unsigned short* __restrict__ dk,
    unsigned short* __restrict__ dv,
    size_t n_kv,
    int n_split) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_kv) return;
  float sk = 0.f, sv = 0.f;
  for (int z = 0; z < n_split; ++z) {
    sk += part[(size_t)z * 2 * n_kv + i];
    sv += part[(size_t)z * 2 * n_kv + n_kv + i];
  }
  dk[i] = bw_bf16(sk);
  dv[i] = bw_bf16(sv);
}

// ------------------------------------------------------------------ dQ pass
template <int HD>
__global__ __launch_bounds__(BW_WAVES * 64) BW_KERNEL void attn_bwd_dq_kernel(
    const unsigned short* __restrict__ q,     // [B, QH, S, HD]
    const unsigned short* __restrict__ k,     // [B, KVH, S, HD]
    const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ dout,  // [B, QH, S, HD]
    const float* __restrict__ lse,            // [B, QH, S]
    const float* __restrict__ delta,
    unsigned short* __restrict__ dq,          // [B, QH, S, HD]
    int q_heads,
    int kv_heads,
    int s,
    float scale) {
  constexpr int KCH = HD / 32;
  constexpr int NB = BW_KT / 16;   // 16-key column blocks per tile
  constexpr int PKC = BW_KT / 32;  // 32-key k-chunks per tile
  const int bh = blockIdx.x;  // b * q_heads + qh
  const int b = bh / q_heads;
  const int qh = bh - b * q_heads;
  const int kvh = qh / (q_heads / kv_heads);
  // the last q tile sees the most keys and is dispatched first
  const int q0_wg = (gridDim.y - 1 - blockIdx.y) * (BW_WAVES * 16);

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int hi = lane >> 4;
  const int q0 = q0_wg + wave * 16;
  const float qscale = scale * BW_LOG2E;

  __shared__ unsigned short k_lds[BW_KT][HD + BW_PAD];
  __shared__ unsigned short v_lds[BW_KT][HD + BW_PAD];
  __shared__ unsigned char kt_raw[HD * (BW_KT + BW_PAD) * 2];  // K transposed
  __shared__ unsigned short ds_lds[BW_WAVES][16][BW_KT + BW_PAD];

  // ---- q~ and dO as A-fragments (row = q0 + col, zero past s)
  bf16x8 q_frag[KCH], do_frag[KCH];
  const size_t row_base = (size_t)bh * s;  // in rows
#pragma unroll
  for (int kc = 0; kc < KCH; ++kc) {
    q_frag[kc] = BF8_ZERO;
    do_frag[kc] = BF8_ZERO;
    if (q0 + col < s) {
      const size_t o = (row_base + q0 + col) * HD + kc * 32 + hi * 8;
      q_frag[kc] = bw_prescale(*reinterpret_cast<const bf16x8*>(q + o), qscale);
      do_frag[kc] = *reinterpret_cast<const bf16x8*>(dout + o);
    }
  }
  // ---- lse2 and D in the per-lane row slots (C rows q0 + hi*4 + r)
  float lse_r[4], dl_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + hi * 4 + r;
    lse_r[r] = qrow < s ? lse[row_base + qrow] : 0.f;
    dl_r[r] = qrow < s ? delta[row_base + qrow] : 0.f;
  }

  f32x4 acc[HD / 16];
#pragma unroll
  for (int d = 0; d < HD / 16; ++d) acc[d] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kv_end = min(s, q0_wg + BW_WAVES * 16);  // the loop ends at the diagonal tile
  const size_t kv_base = (((size_t)b * kv_heads + kvh) * s) * HD;

  for (int j0 = 0; j0 < kv_end; j0 += BW_KT) {
    __syncthreads();
    for (int idx = tid; idx < BW_KT * (HD / 8); idx += BW_WAVES * WAVE) {
      const int row = idx / (HD / 8);
      const int c8 = (idx - row * (HD / 8)) * 8;
      bf16x8 k8 = BF8_ZERO;
      bf16x8 v8 = BF8_ZERO;
      if (j0 + row < kv_end) {
        k8 = *reinterpret_cast<const bf16x8*>(k + kv_base + (size_t)(j0 + row) * HD + c8);
        v8 = *reinterpret_cast<const bf16x8*>(v + kv_base + (size_t)(j0 + row) * HD + c8);
      }
      *reinterpret_cast<bf16x8*>(&k_lds[row][c8]) = k8;
      *reinterpret_cast<bf16x8*>(&v_lds[row][c8]) = v8;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        *reinterpret_cast<unsigned short*>(&kt_raw[TR_BYTE(BW_KT, c8 + e, row * 2)]) = (unsigned short)k8[e];
    }
    __syncthreads();

    // ---- S = q~ K^T and dP = dO V^T: C[q = hi*4 + r][key = nb*16 + col]
    f32x4 s_acc[NB], dp_acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      s_acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp_acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < KCH; ++kc) {
        const bf16x8 kt = *reinterpret_cast<const bf16x8*>(&k_lds[nb * 16 + col][kc * 32 + hi * 8]);
        const bf16x8 vt = *reinterpret_cast<const bf16x8*>(&v_lds[nb * 16 + col][kc * 32 + hi * 8]);
        s_acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[kc], kt, s_acc[nb], 0, 0, 0);
        dp_acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(do_frag[kc], vt, dp_acc[nb], 0, 0, 0);
      }
    }

    // ---- dS = p (dP - D) -> bf16 into the per-wave scratch [q row][key].
    // Interior: every key of the tile at or below this wave's first q row.
    const bool interior = (j0 + BW_KT <= q0 + 1) && (q0 + 16 <= s);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0 + hi * 4 + r;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int key = j0 + nb * 16 + col;
        float x = s_acc[nb][r] - lse_r[r];
        if (!interior && (key > qrow || qrow >= s)) x = NEG_SENTINEL;
        const float p = (x <= NEG_THRESHOLD) ? 0.f : exp2f(x);
        ds_lds[wave][hi * 4 + r][nb * 16 + col] = bw_bf16(p * (dp_acc[nb][r] - dl_r[r]));
      }
    }
    __syncthreads();

    // ---- dQ += dS K: A from the scratch, B[k = key][n = dim] from K transposed
    bf16x8 ds_frag[PKC];
#pragma unroll
    for (int pk = 0; pk < PKC; ++pk)
      ds_frag[pk] = *reinterpret_cast<const bf16x8*>(&ds_lds[wave][col][pk * 32 + hi * 8]);
#pragma unroll
    for (int d = 0; d < HD / 16; ++d) {
#pragma unroll
      for (int pk = 0; pk < PKC; ++pk) {
        const bf16x8 kfrag =
            *reinterpret_cast<const bf16x8*>(&kt_raw[TR_BYTE(BW_KT, d * 16 + col, pk * 64 + hi * 16)]);
        acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ds_frag[pk], kfrag, acc[d], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + hi * 4 + r;
    if (qrow >= s) continue;
    unsigned short* dst = dq + (row_base + qrow) * HD;
#pragma unroll
    for (int d = 0; d < HD / 16; ++d) dst[d * 16 + col] = bw_bf16(acc[d][r] * scale);
  }
}

// How many grid.z slices the q heads of a kv head are split into: the dK/dV
// grid has only B*KVH*ceil(S/64) workgroups and its first key tile carries the
// most work, so small grids split until there are two workgroups per CU.
static int dkdv_auto_splits(int wgs, int gq) {
  int n = 1;
  while (n < gq && wgs * n < 512 && gq % (n * 2) == 0) n *= 2;
  return n;
}

std::vector<torch::Tensor> attn_train_bwd(
    torch::Tensor q,     // [B, QH, S, HD] bf16
    torch::Tensor k,     // [B, KVH, S, HD] bf16
    torch::Tensor v,
    torch::Tensor out,   // [B, QH, S, HD] bf16, from attn_train_fwd
    torch::Tensor lse2,  // [B, QH, S] f32, from attn_train_fwd
    torch::Tensor dout,  // [B, QH, S, HD] bf16
    double scale,
    int64_t gq_splits) {  // 0: dkdv_auto_splits; else a divisor of QH/KVH
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && k.dim() == 4);
  for (const auto& t : {q, k, v, out, dout})
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous(), "bf16 contiguous CUDA tensors");
  const int B = q.size(0), QH = q.size(1), S = q.size(2), HD = q.size(3);
  const int KVH = k.size(1);
  TORCH_CHECK(HD == 128 || HD == 64, "training attention supports head_dim 64/128");
  TORCH_CHECK(KVH > 0 && QH % KVH == 0);
  TORCH_CHECK(k.size(0) == B && k.size(2) == S && k.size(3) == HD && v.sizes() == k.sizes(), "k/v must be [B, KVH, S, HD]");
  TORCH_CHECK(out.sizes() == q.sizes() && dout.sizes() == q.sizes(), "out/dout must match q");
  TORCH_CHECK(lse2.is_cuda() && lse2.scalar_type() == at::kFloat && lse2.is_contiguous() && lse2.numel() == (int64_t)B * QH * S,
              "lse2 must be [B, QH, S] f32");
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(k);
  if (q.numel() == 0) return {dq, dk, dv};
  const int gq = QH / KVH;
  const int tiles = (S + BW_KT - 1) / BW_KT;
  const int n_split = gq_splits > 0 ? (int)gq_splits : dkdv_auto_splits(B * KVH * tiles, gq);
  TORCH_CHECK(n_split >= 1 && gq % n_split == 0, "gq_splits must divide QH/KVH");
  auto delta = torch::empty({B, QH, S}, lse2.options());
  torch::Tensor part;
  if (n_split > 1) part = torch::empty({n_split, 2, (int64_t)k.numel()}, lse2.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const float sc = (float)scale;
  const int n_rows = B * QH * S;
  const size_t n_kv = (size_t)k.numel();

  const auto* qp = reinterpret_cast<const unsigned short*>(q.data_ptr());
  const auto* kp = reinterpret_cast<const unsigned short*>(k.data_ptr());
  const auto* vp = reinterpret_cast<const unsigned short*>(v.data_ptr());
  const auto* op = reinterpret_cast<const unsigned short*>(out.data_ptr());
  const auto* dop = reinterpret_cast<const unsigned short*>(dout.data_ptr());
  const float* lp = lse2.data_ptr<float>();
  float* dlp = delta.data_ptr<float>();
  float* pp = n_split > 1 ? part.data_ptr<float>() : nullptr;
  auto* dqp = reinterpret_cast<unsigned short*>(dq.data_ptr());
  auto* dkp = reinterpret_cast<unsigned short*>(dk.data_ptr());
  auto* dvp = reinterpret_cast<unsigned short*>(dv.data_ptr());

  const dim3 grid_kv(B * KVH, tiles, n_split);
  const dim3 grid_q(B * QH, (S + BW_WAVES * 16 - 1) / (BW_WAVES * 16));
#define BW_LAUNCH(HDV)                                                                           \
  do {                                                                                           \
    constexpr int RPB = 256 / (HDV / 8);                                                         \
    attn_bwd_delta_kernel<HDV><<<(n_rows + RPB - 1) / RPB, 256, 0, stream>>>(op, dop, dlp, n_rows); \
    attn_bwd_dkdv_kernel<HDV><<<grid_kv, BW_WAVES * WAVE, 0, stream>>>(                          \
        qp, kp, vp, dop, lp, dlp, dkp, dvp, pp, QH, KVH, S, sc);                                 \
    attn_bwd_dq_kernel<HDV><<<grid_q, BW_WAVES * WAVE, 0, stream>>>(                             \
        qp, kp, vp, dop, lp, dlp, dqp, QH, KVH, S, sc);                                          \
  } while (0)
  if (HD == 128) BW_LAUNCH(128); else BW_LAUNCH(64);
#undef BW_LAUNCH
  if (n_split > 1)
    attn_bwd_reduce_kernel<<<(unsigned)((n_kv + 255) / 256), 256, 0, stream>>>(pp, dkp, dvp, n_kv, n_split);
  HIP_CHECK_LAST();
  return {dq, dk, dv};
}
