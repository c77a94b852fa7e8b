// GQA decode attention for CDNA4 (gfx950), flash-decoding style.
//
// Default path (mfma_decode_kernel): the GQ query heads of one kv head form
// the rows of an mfma_f32_16x16x32_bf16 A-fragment (padded to 16), so 32
// cache keys cost 4 QK MFMAs + 8 PV MFMAs per wave instead of 32*GQ
// shuffle-reduced dot products. K is consumed directly from global as
// B-fragments (16 B/lane); V goes through the XOR-swizzled LDS transpose
// (same as the prefill kernel); 4 waves take interleaved 32-key tiles of the
// workgroup's split range and combine through LDS; attn_decode_combine merges
// splits. Measured (scripts/decode_mfma.hip, llama-2-70b shape): 1039 GB/s at
// kv=4k -> 3509 GB/s at kv=131k, 2.2-2.4x the original VALU kernel (16-lane-
// group dot products, online softmax in registers; removed, see
// docs/KERNELS.md) at every length. Those figures predate the batched loads
// ("Loads" below), which took benchmarks/benchmark_kv_fp8.py (rotating
// caches) from 577 to 751 GB/s at 4k and from 3335 to 4376 GB/s at 131k.
//
// kv_len comes from a DEVICE pointer so the whole decode step can be captured
// in a hipGraph with a moving position.
//
// Replaces the reference's torch QK^T/softmax/AV decode math
// (reference models/llama/block.py:108-127) on the MI355X fast path.

#include "attn_decode_tile.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

// Arbitrary GQ: heads are processed in ceil(GQ/16) groups of <=16 (one
// A-fragment each). The group loop sits OUTSIDE the kv loop so live registers
// stay at one group's footprint; K/V re-reads per extra group come from
// L2/HBM and are negligible for the weight-bound decode shapes that need
// GQ > 16 (falcon-7b MQA gq=71, falcon-180b gq=29 — reference
// models/falcon/block.py:100-110).
// FP8 caches and the batched tile loads (DecodeTile): attn_decode_tile.h.

// Waves per SIMD the register allocation must leave room for: LDS admits 3
// workgroups per CU at HD 128 (168 registers per lane) and the split policy
// uses them at long caches; HD 64 keeps the 4 it had. The one form that does
// not fit 168 without scratch, bf16 HD 128 with two head groups, gets 2.
constexpr int decode_waves_per_simd(int hd, int gq, bool fp8) {
  return hd == 128 ? (!fp8 && gq > 16 ? 2 : 3) : 4;
}

template <int HD, int GQ, bool FP8 = false>
__global__ __launch_bounds__(DWAVES * 64) __attribute__((amdgpu_waves_per_eu(decode_waves_per_simd(HD, GQ, FP8))))
void mfma_decode_kernel(
    const float* __restrict__ q,            // [B, KV, GQ, HD]
    const typename std::conditional<FP8, unsigned char, unsigned short>::type* __restrict__ k_cache,  // [B, KV, lmax, HD]
    const typename std::conditional<FP8, unsigned char, unsigned short>::type* __restrict__ v_cache,
    float* __restrict__ part_o,             // [B*KV, splits, GQ, HD]
    float* __restrict__ part_ml,            // [B*KV, splits, GQ, 2]
    const int* __restrict__ kv_len_ptr,
    const float* __restrict__ alibi,        // [kv_heads*GQ] slopes or null
    int kv_heads,
    int lmax,
    int n_splits,
    float scale,
    float* __restrict__ out_direct) {  // n_splits==1: normalized out [B, KV*GQ*HD]
                                       // written here; the combine kernel is skipped
  const int bkv = blockIdx.x;
  const int kvh = bkv % kv_heads;
  const int split = blockIdx.y;
  const int kv_len = *kv_len_ptr;

  const int rows_per_split = (kv_len + n_splits - 1) / n_splits;
  const int j_begin = split * rows_per_split;
  const int j_end = min(j_begin + rows_per_split, kv_len);

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);  // scalar: tile indices and loop control stay in SGPRs
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int hi = lane >> 4;

  constexpr int KCH = HD / 32;
  constexpr int GA = (GQ + 15) / 16;  // head groups of <=16

  // per-wave LDS: swizzled V^T tile + P scratch; the cross-wave combine
  // overlays the V^T storage after the main loop (one <=16-head group at a
  // time, so the overlay always fits)
  __shared__ unsigned char vt_raw[DWAVES][HD * (DKVT + DKPAD) * 2];
  __shared__ unsigned short p_lds[DWAVES][16][DKVT + DKPAD];
  __shared__ float c_ml[DWAVES][16][2];
  static_assert(16 * HD * 4 <= HD * (DKVT + DKPAD) * 2, "combine O overlay too big");

  const size_t kv_base = (size_t)bkv * lmax * HD;
  const auto* kb = k_cache + kv_base;
  const auto* vb = v_cache + kv_base;
  const size_t q_base = (size_t)bkv * GQ * HD;

  for (int a = 0; a < GA; ++a) {
    const int g0 = a * 16;  // first head of this group
    if (a > 0) __syncthreads();  // wave0's combine reads of vt_raw are done

    // ---- q tile: A-fragment rows = q heads of this group (zero-padded), pre-scaled
    // One batch: every load of the fragment (and of the slopes) is issued
    // before the first is consumed. Padding rows load a clamped head and are
    // zeroed afterwards, so no load sits behind a branch; none of the
    // addresses depends on kv_len, whose load overlaps them.
    const unsigned short q_mask = g0 + col < GQ ? 0xFFFFu : 0u;  // a mask, not a branch per element
    const float* q_src = q + q_base + (size_t)min(g0 + col, GQ - 1) * HD + hi * 8;
    f32x4 q_raw[KCH][2];
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
      q_raw[kc][0] = *reinterpret_cast<const f32x4*>(q_src + kc * 32);
      q_raw[kc][1] = *reinterpret_cast<const f32x4*>(q_src + kc * 32 + 4);
    }

    // per-lane-row ALiBi slopes (rows = heads g0 + hi*4 + r)
    float sl[4] = {0.f, 0.f, 0.f, 0.f};
    if (alibi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sl[r] = alibi[kvh * GQ + min(g0 + hi * 4 + r, GQ - 1)];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (g0 + hi * 4 + r >= GQ) sl[r] = 0.f;
    }

    bf16x8 q_frag[KCH];
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        q_frag[kc][e] = (short)(f32_to_bf16(q_raw[kc][e >> 2][e & 3] * scale) & q_mask);
    }

    f32x4 acc_o[HD / 16];
#pragma unroll
    for (int d = 0; d < HD / 16; ++d) acc_o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_row[4], l_row[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m_row[r] = NEG_SENTINEL;
      l_row[r] = 0.f;
    }

    // A tile's K B-fragments and V chunks (VN per lane) go to registers in
    // one batch of unconditional loads, K first because the QK MFMAs consume
    // it first: rows past j_end are clamped to j_end - 1 (every address stays
    // inside [j_begin, j_end)); V rows past j_end become zeros when they are
    // written to LDS. Offsets inside one (batch, head) are computed in 32
    // bits (the host checks lmax * HD), which keeps the address arithmetic
    // of the 16 loads short.
    DecodeTile<HD, FP8> tile;
    const auto load_tile = [&](int j0) {
#pragma unroll
      for (int nb = 0; nb < DKVT / 16; ++nb) {
        const auto* krow = kb + ((unsigned)min(j0 + nb * 16 + col, j_end - 1) * HD + hi * 8);
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc)
          tile.k[nb][kc] = *reinterpret_cast<const typename DecodeTile<HD, FP8>::raw_t*>(krow + kc * 32);
      }
#pragma unroll
      for (int i = 0; i < tile.VN; ++i) {
        const int idx = lane + i * WAVE;
        const int row = idx / (HD / 8);
        const int c8 = (idx - row * (HD / 8)) * 8;
        tile.v[i] = *reinterpret_cast<const typename DecodeTile<HD, FP8>::raw_t*>(
            vb + ((unsigned)min(j0 + row, j_end - 1) * HD + c8));
      }
      // nothing that waits for a load may be scheduled among the loads
      __builtin_amdgcn_sched_barrier(0);
    };

    // wave w handles tiles j_begin + (t*DWAVES + w)*DKVT
    for (int j0 = j_begin + wave * DKVT; j0 < j_end; j0 += DWAVES * DKVT) {
      const int tile_n = min(DKVT, j_end - j0);
      const bool full = tile_n == DKVT;
      load_tile(j0);

      // ---- S = Q K^T, K from the tile registers: B[k = kdim][n = key]
      f32x4 s_acc[DKVT / 16];
#pragma unroll
      for (int nb = 0; nb < DKVT / 16; ++nb) {
        s_acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc)
          s_acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[kc], tile.to_bf16(tile.k[nb][kc]), s_acc[nb], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);  // K registers are free before V is unpacked

      // ---- stage V^T (this wave only: no block barrier; a wave's LDS
      // accesses complete in order, the lgkmcnt wait orders them for the
      // compiler).
      // The 8 * VN swizzled addresses do not depend on the tile. The opaque
      // copy of the lane keeps them from being hoisted out of the tile loop
      // (64 VGPRs at HD 128), the fence from being computed all up front:
      // they are recomputed per chunk, as the rolled loop did.
      int st_lane = lane;
      asm volatile("" : "+v"(st_lane));
#pragma unroll
      for (int i = 0; i < tile.VN; ++i) {
        const int idx = st_lane + i * WAVE;
        const int row = idx / (HD / 8);
        const int c8 = (idx - row * (HD / 8)) * 8;
        bf16x8 vv8 = tile.to_bf16(tile.v[i]);
        if (j0 + row >= j_end) vv8 = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          *reinterpret_cast<unsigned short*>(&vt_raw[wave][DVT_BYTE(c8 + e, row * 2)]) = (unsigned short)vv8[e];
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);

      // ---- online softmax over this tile (rows = heads g0 + hi*4+r)
      float p[DKVT / 16][4];
      float corr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s[DKVT / 16];
#pragma unroll
        for (int nb = 0; nb < DKVT / 16; ++nb) {
          const int key = j0 + nb * 16 + col;
          s[nb] = s_acc[nb][r] + sl[r] * key;
          if (!full && key >= j_end) s[nb] = NEG_SENTINEL;
        }
        float mx = NEG_SENTINEL;
#pragma unroll
        for (int nb = 0; nb < DKVT / 16; ++nb) mx = fmaxf(mx, s[nb]);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
        const float m_new = fmaxf(m_row[r], mx);
        corr[r] = (m_row[r] <= NEG_THRESHOLD) ? 0.f : __expf(m_row[r] - m_new);
        float lsum = 0.f;
#pragma unroll
        for (int nb = 0; nb < DKVT / 16; ++nb) {
          p[nb][r] = (s[nb] <= NEG_THRESHOLD) ? 0.f : __expf(s[nb] - m_new);
          lsum += p[nb][r];
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off, WAVE);
        l_row[r] = l_row[r] * corr[r] + lsum;
        m_row[r] = m_new;
      }

#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nb = 0; nb < DKVT / 16; ++nb)
          p_lds[wave][hi * 4 + r][nb * 16 + col] = f32_to_bf16(p[nb][r]);
      __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);

      const bf16x8 p_frag = *reinterpret_cast<const bf16x8*>(&p_lds[wave][col][hi * 8]);

#pragma unroll
      for (int d = 0; d < HD / 16; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc_o[d][r] *= corr[r];
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) {
        const bf16x8 vfrag = *reinterpret_cast<const bf16x8*>(&vt_raw[wave][DVT_BYTE(d * 16 + col, hi * 16)]);
        acc_o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p_frag, vfrag, acc_o[d], 0, 0, 0);
      }
    }

    // ---- cross-wave combine for this head group (overlay V^T LDS with O rows)
    __syncthreads();
    float* c_o = reinterpret_cast<float*>(vt_raw[wave]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gl = hi * 4 + r;
      if (g0 + gl < GQ) {
#pragma unroll
        for (int d = 0; d < HD / 16; ++d) c_o[gl * HD + d * 16 + col] = acc_o[d][r];
        if (col == 0) {
          c_ml[wave][gl][0] = m_row[r];
          c_ml[wave][gl][1] = l_row[r];
        }
      }
    }
    __syncthreads();

    if (wave == 0) {
      const int gn = min(16, GQ - g0);  // heads in this group
      float* po = part_o + (((size_t)bkv * n_splits + split) * GQ + g0) * HD;
      float* pml = part_ml + (((size_t)bkv * n_splits + split) * GQ + g0) * 2;
      for (int idx = lane; idx < gn * HD; idx += WAVE) {
        const int gl = idx / HD, d = idx - gl * HD;
        float m_star = c_ml[0][gl][0];
#pragma unroll
        for (int w = 1; w < DWAVES; ++w) m_star = fmaxf(m_star, c_ml[w][gl][0]);
        float osum = 0.f, lsum = 0.f;
#pragma unroll
        for (int w = 0; w < DWAVES; ++w) {
          const float wgt = (c_ml[w][gl][0] <= NEG_THRESHOLD) ? 0.f : __expf(c_ml[w][gl][0] - m_star);
          osum += wgt * reinterpret_cast<const float*>(vt_raw[w])[gl * HD + d];
          lsum += wgt * c_ml[w][gl][1];
        }
        if (out_direct) {
          // single split: normalize here (matches the combine kernel's
          // n_splits==1 output exactly) and skip that kernel entirely —
          // at short kv both kernels are pure launch latency
          out_direct[((size_t)bkv * GQ + g0 + gl) * HD + d] = osum / fmaxf(lsum, 1e-20f);
        } else {
          po[idx] = osum;
          if (d == 0) {
            pml[gl * 2 + 0] = m_star;
            pml[gl * 2 + 1] = lsum;
          }
        }
      }
    }
  }
}

// Merges the splits of one (batch, kv head, q head). The m / l pairs and the
// O values of COMBINE_BATCH splits are loaded together and then accumulated
// one split after the other, in split order: the sums are those of a plain
// loop over the splits (reassociation is switched off for them), but a
// 64-split cache pays 8 load round trips instead of 64.
#define COMBINE_BATCH 8

__global__ void attn_decode_combine_kernel(
    const float* __restrict__ part_o,   // [B*KV, splits, GQ, HD]
    const float* __restrict__ part_ml,  // [B*KV, splits, GQ, 2]
    float* __restrict__ out,            // [B, KV*GQ*HD]
    int n_splits, int gq, int hd) {
#pragma clang fp reassociate(off)
  const int bkv = blockIdx.x;
  const int g = blockIdx.y;
  // row of split s in both workspaces; loads past the last split repeat it
  const auto row = [&](int s) { return ((size_t)bkv * n_splits + min(s, n_splits - 1)) * gq + g; };
  float m_star = NEG_SENTINEL;
  for (int s0 = 0; s0 < n_splits; s0 += COMBINE_BATCH) {
    float ms[COMBINE_BATCH];
#pragma unroll
    for (int i = 0; i < COMBINE_BATCH; ++i) ms[i] = part_ml[row(s0 + i) * 2];
#pragma unroll
    for (int i = 0; i < COMBINE_BATCH; ++i) m_star = fmaxf(m_star, ms[i]);
  }
  for (int d = threadIdx.x; d < hd; d += blockDim.x) {
    float osum = 0.f, lsum = 0.f;
    for (int s0 = 0; s0 < n_splits; s0 += COMBINE_BATCH) {
      float ms[COMBINE_BATCH], ls[COMBINE_BATCH], po[COMBINE_BATCH];
#pragma unroll
      for (int i = 0; i < COMBINE_BATCH; ++i) {
        ms[i] = part_ml[row(s0 + i) * 2];
        ls[i] = part_ml[row(s0 + i) * 2 + 1];
        po[i] = part_o[row(s0 + i) * hd + d];
      }
#pragma unroll
      for (int i = 0; i < COMBINE_BATCH; ++i) {
        if (s0 + i >= n_splits || ms[i] <= NEG_THRESHOLD) continue;
        const float w = __expf(ms[i] - m_star);
        osum += w * po[i];
        lsum += w * ls[i];
      }
    }
    out[(size_t)bkv * gq * hd + (size_t)g * hd + d] = osum / fmaxf(lsum, 1e-20f);
  }
}

// ---------------------------------------------------------------- host API

// q: [B, KV*GQ*HD] f32 (token per row); caches [Bc, KV, Lmax, HD] bf16 or
// float8_e4m3fn (both alike);
// kv_len: device int32 scalar tensor. Returns [B, KV*GQ*HD] f32.
torch::Tensor attn_decode_fused(
    torch::Tensor q,
    torch::Tensor k_cache,
    torch::Tensor v_cache,
    torch::Tensor kv_len,  // device int32 [1]
    int64_t gq,
    int64_t n_splits_i,
    torch::Tensor part_o,   // workspace [B*KV, splits, GQ, HD] f32 (or empty)
    torch::Tensor part_ml,  // workspace [B*KV, splits, GQ, 2] f32 (or empty)
    double scale,
    c10::optional<torch::Tensor> alibi_slopes) {  // [kv_heads*GQ] f32
  TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kFloat32);
  const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK((fp8 || k_cache.scalar_type() == at::kBFloat16) && k_cache.dim() == 4,
              "kv cache must be bf16 or float8_e4m3fn");
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type(), "k and v caches must share a dtype");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes() && k_cache.is_contiguous() && v_cache.is_contiguous());
  const int b = q.size(0);
  TORCH_CHECK(b <= k_cache.size(0), "more q rows than cache rows");
  const int kv_heads = k_cache.size(1), lmax = k_cache.size(2), hd = k_cache.size(3);
  TORCH_CHECK((int64_t)lmax * hd < (int64_t(1) << 32), "one (batch, head) of the cache must stay below 2^32 elements");
  const int GQi = (int)gq;
  int n_splits = (int)n_splits_i;
  if (n_splits <= 0) {
    // 4-wave workgroups; fill ~256 CUs (chunks >= 128 rows) and go up to
    // 3 wgs/CU only when chunks stay >= 512 rows (measured knees,
    // profiles/decode_longctx_sweep.log + scripts/decode_mfma.hip).
    // Forcing one split at short caches to skip the combine kernel LOST
    // 1.4 tok/s end to end (profiles/attn_direct_ab.log): halving the split
    // occupancy costs more than the removed launch.
    const int bkv = std::max(1, b * kv_heads);
    const int by_occ = std::min(768 / bkv, lmax / 512);
    const int by_min = std::min(256 / bkv, (lmax + 127) / 128);
    n_splits = std::max(1, std::max(by_occ, by_min));
  }
  auto opts = q.options();
  const bool direct = n_splits == 1;  // parts go unused
  if (!direct && part_o.numel() < (int64_t)b * kv_heads * n_splits * GQi * hd)
    part_o = torch::empty({(int64_t)b * kv_heads, n_splits, GQi, hd}, opts);
  if (!direct && part_ml.numel() < (int64_t)b * kv_heads * n_splits * GQi * 2)
    part_ml = torch::empty({(int64_t)b * kv_heads, n_splits, GQi, 2}, opts);
  auto out = torch::empty({(int64_t)b, (int64_t)kv_heads * GQi * hd}, opts);

  dim3 grid(b * kv_heads, n_splits);
  auto stream = at::cuda::getCurrentCUDAStream();
  const float* qp = q.data_ptr<float>();
  const unsigned short* kp = reinterpret_cast<const unsigned short*>(k_cache.data_ptr());
  const unsigned short* vp = reinterpret_cast<const unsigned short*>(v_cache.data_ptr());
  float* pop = part_o.data_ptr<float>();
  float* pmlp = part_ml.data_ptr<float>();
  const int* lenp = kv_len.data_ptr<int>();
  const float sc = (float)scale;
  const float* alibi_p = nullptr;
  if (alibi_slopes.has_value() && alibi_slopes->defined() && alibi_slopes->numel() > 0) {
    TORCH_CHECK(alibi_slopes->is_contiguous() && alibi_slopes->dtype() == torch::kFloat32);
    TORCH_CHECK(alibi_slopes->numel() == (int64_t)kv_heads * GQi, "alibi slopes must be [q_heads]");
    alibi_p = alibi_slopes->data_ptr<float>();
  }

  // single split: the decode kernel normalizes and writes the output itself —
  // the combine kernel (pure launch latency at short kv) is skipped entirely
  float* direct_p = direct ? out.data_ptr<float>() : nullptr;
  bool launched = false;
#define ATTN_CASE(HDV, GQV)                                                   \
  if (hd == HDV && GQi == GQV) {                                              \
    if (fp8)                                                                  \
      mfma_decode_kernel<HDV, GQV, true><<<grid, DWAVES * WAVE, 0, stream>>>( \
          qp, reinterpret_cast<const unsigned char*>(kp),                     \
          reinterpret_cast<const unsigned char*>(vp), pop, pmlp, lenp,        \
          alibi_p, kv_heads, lmax, n_splits, sc, direct_p);                   \
    else                                                                      \
      mfma_decode_kernel<HDV, GQV><<<grid, DWAVES * WAVE, 0, stream>>>(       \
          qp, kp, vp, pop, pmlp, lenp, alibi_p, kv_heads, lmax, n_splits, sc, \
          direct_p);                                                          \
    launched = true;                                                          \
  }
  ATTN_CASE(128, 1) ATTN_CASE(128, 2) ATTN_CASE(128, 4) ATTN_CASE(128, 6)
  ATTN_CASE(128, 8) ATTN_CASE(128, 16)
  ATTN_CASE(64, 1) ATTN_CASE(64, 2) ATTN_CASE(64, 4) ATTN_CASE(64, 8) ATTN_CASE(64, 16)
  // GQ > 16 (multi-group): falcon-7b MQA (gq=71), falcon-180b (gq=29)
  ATTN_CASE(64, 29) ATTN_CASE(64, 71) ATTN_CASE(64, 32)
  ATTN_CASE(128, 32)
#undef ATTN_CASE
  TORCH_CHECK(launched, "unsupported (head_dim, gqa) = (", hd, ", ", GQi, ")");
  HIP_CHECK_LAST();

  if (direct_p == nullptr) {
    dim3 cgrid(b * kv_heads, GQi);
    attn_decode_combine_kernel<<<cgrid, std::min(hd, 256), 0, stream>>>(
        pop, pmlp, out.data_ptr<float>(), n_splits, GQi, hd);
    HIP_CHECK_LAST();
  }
  return out;
}
