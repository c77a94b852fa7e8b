// Multi-token decode attention for CDNA4 (gfx950): T = 2..8 new tokens per
// sequence (a speculative-decoding verify step) against the KV cache, causal
// among the new tokens, flash-decoding split over the cache.
//
// The rows of the mfma_f32_16x16x32_bf16 A-fragments of one kv head are the
// (token, q head) pairs r = t * GQ + g, R = T * GQ <= 128 of them, in groups
// of 16 (the last one zero-padded through a mask). The decode kernel
// (attention.hip) pads its GQ heads to 16 rows and puts its head-group loop
// outside the kv loop, re-reading K/V per group; here ONE pass over a tile's
// K/V serves RG row groups: the tile's K B-fragments are loaded once and feed
// RG QK MFMA sets, its V^T LDS image is staged once and feeds RG x HD/16 PV
// MFMAs. ceil(R / (16 * RG)) passes cover all rows, so llama-70b (GQ 8) reads
// the cache once for up to 4 tokens and twice for 8.
//
// Shared with the decode kernel (attn_decode_tile.h and the same code shape):
// DecodeTile and its one-batch loads clamped to the split's rows, V zero-fill
// past j_end, the XOR-swizzled V^T image, 4 waves on interleaved 32-key tiles,
// lgkmcnt-only ordering inside a wave, and the rounding points (q*scale ->
// bf16, P -> bf16 before PV, fp32 normaliser of the unrounded P).
//
// Causality: token t sees keys j <= *pos + t, where *pos (device memory, so
// the step stays graph-capturable) is the prefix length before the step and
// the new tokens' K/V rows are already in the cache at pos .. pos+T-1. Tiles
// that end at or below *pos are visible to every row and take the mask-free
// path; only the last tiles pay the per-row compare. A row with no visible key
// in a split (the last split may begin past pos + t) keeps m = NEG_SENTINEL
// and l = 0, which the combine skips.

#include "attn_decode_tile.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

// Row groups per pass: the largest count that leaves no scratch at the waves
// per SIMD the kernel is built for. Two groups hold 2 x (16 q + 32 acc + 8 m/l)
// registers at HD 128 next to the 64 of a bf16 DecodeTile: that spills at 3
// waves per SIMD (168 registers) and fits at 2 (243 used); three groups spill
// there too. HD 64 fits two groups at 3 waves per SIMD (163), spills at 4, and
// three groups spill at 3. Resource table: docs/KERNELS.md, "Multi-token
// decode".
constexpr int multi_row_groups(int hd, bool fp8) { return 2; }
constexpr int multi_waves_per_simd(int hd, bool fp8) { return hd == 128 ? 2 : 3; }

template <int HD, int GQ, bool FP8, int RG>
__global__ __launch_bounds__(DWAVES * 64) __attribute__((amdgpu_waves_per_eu(multi_waves_per_simd(HD, FP8))))
void mfma_decode_multi_kernel(
    const float* __restrict__ q,            // [B*T, KV*GQ*HD], row b*T + t
    const typename std::conditional<FP8, unsigned char, unsigned short>::type* __restrict__ k_cache,  // [Bc, KV, lmax, HD]
    const typename std::conditional<FP8, unsigned char, unsigned short>::type* __restrict__ v_cache,
    float* __restrict__ part_o,             // [B*KV, splits, R, HD]
    float* __restrict__ part_ml,            // [B*KV, splits, R, 2]
    const int* __restrict__ pos_ptr,        // prefix length before the step
    int kv_heads,
    int lmax,
    int tokens,
    int n_splits,
    float scale,
    float* __restrict__ out_direct) {  // n_splits==1: normalized out [B*T, KV*GQ*HD]
  const int bkv = blockIdx.x;
  const int bi = bkv / kv_heads;
  const int kvh = bkv - bi * kv_heads;
  const int split = blockIdx.y;
  const int pos = *pos_ptr;
  const int kv_len = pos + tokens;
  const int R = tokens * GQ;

  const int rows_per_split = (kv_len + n_splits - 1) / n_splits;
  const int j_begin = split * rows_per_split;
  const int j_end = min(j_begin + rows_per_split, kv_len);

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int hi = lane >> 4;

  constexpr int KCH = HD / 32;

  // per-wave LDS: swizzled V^T tile + P scratch for RG row groups; the
  // cross-wave combine overlays the V^T storage one 16-row group at a time
  __shared__ unsigned char vt_raw[DWAVES][HD * (DKVT + DKPAD) * 2];
  __shared__ unsigned short p_lds[DWAVES][RG * 16][DKVT + DKPAD];
  __shared__ float c_ml[DWAVES][RG * 16][2];
  static_assert(16 * HD * 4 <= HD * (DKVT + DKPAD) * 2, "combine O overlay too big");

  const size_t kv_base = (size_t)bkv * lmax * HD;
  const auto* kb = k_cache + kv_base;
  const auto* vb = v_cache + kv_base;
  const size_t q_stride = (size_t)kv_heads * GQ * HD;  // one token row of q / out
  const size_t tok_base = ((size_t)bi * tokens) * q_stride + (size_t)kvh * GQ * HD;

  const int n_groups = (R + 15) / 16;
  for (int g0 = 0; g0 < n_groups; g0 += RG) {
    const int ng = min(RG, n_groups - g0);  // live row groups of this pass (uniform)
    if (g0 > 0) __syncthreads();            // wave0's combine reads of vt_raw are done

    // ---- q tiles: A-fragment row = (token, head) pair (g0 + rg) * 16 + col,
    // pre-scaled; all loads of all groups in one batch, padding rows load a
    // clamped row and are zeroed by the mask
    f32x4 q_raw[RG][KCH][2];
    unsigned short q_mask[RG];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
      const int ra = (g0 + rg) * 16 + col;
      q_mask[rg] = ra < R ? 0xFFFFu : 0u;
      const int rc = min(ra, R - 1);
      const int t = rc / GQ, g = rc - t * GQ;
      const float* q_src = q + tok_base + (size_t)t * q_stride + g * HD + hi * 8;
#pragma unroll
      for (int kc = 0; kc < KCH; ++kc) {
        q_raw[rg][kc][0] = *reinterpret_cast<const f32x4*>(q_src + kc * 32);
        q_raw[rg][kc][1] = *reinterpret_cast<const f32x4*>(q_src + kc * 32 + 4);
      }
    }
    bf16x8 q_frag[RG][KCH];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg)
#pragma unroll
      for (int kc = 0; kc < KCH; ++kc)
#pragma unroll
        for (int e = 0; e < 8; ++e)
          q_frag[rg][kc][e] = (short)(f32_to_bf16(q_raw[rg][kc][e >> 2][e & 3] * scale) & q_mask[rg]);

    f32x4 acc_o[RG][HD / 16];
    float m_row[RG][4], l_row[RG][4];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) acc_o[rg][d] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        m_row[rg][r] = NEG_SENTINEL;
        l_row[rg][r] = 0.f;
      }
    }

    // One batch of unconditional loads per tile, K first: rows past j_end are
    // clamped to j_end - 1 (every address stays inside [j_begin, j_end), and
    // j_end <= *pos + T <= lmax); offsets inside one (batch, head) are 32-bit
    // (the host checks lmax * HD).
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
      __builtin_amdgcn_sched_barrier(0);
    };

    // wave w handles tiles j_begin + (i*DWAVES + w)*DKVT
    for (int j0 = j_begin + wave * DKVT; j0 < j_end; j0 += DWAVES * DKVT) {
      // full and interior: 32 live keys, all at or below *pos, so every row
      // of every token sees all of them
      const bool interior = j0 + DKVT <= min(j_end, pos + 1);
      load_tile(j0);

      // ---- S = Q K^T for every live row group from the one K image
      f32x4 s_acc[RG][DKVT / 16];
#pragma unroll
      for (int nb = 0; nb < DKVT / 16; ++nb) {
        bf16x8 kf[KCH];
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) kf[kc] = tile.to_bf16(tile.k[nb][kc]);
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) {
          s_acc[rg][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (rg < ng) {
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc)
              s_acc[rg][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[rg][kc], kf[kc], s_acc[rg][nb], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // K registers are free before V is unpacked

      // ---- stage V^T once (this wave only; see attention.hip for the
      // opaque lane copy and the per-chunk fences)
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

      // ---- online softmax per row group (C rows (g0 + rg) * 16 + hi*4 + r)
      float corr[RG][4];
#pragma unroll
      for (int rg = 0; rg < RG; ++rg) {
#pragma unroll
        for (int r = 0; r < 4; ++r) corr[rg][r] = 0.f;
        if (rg >= ng) continue;
        float p[DKVT / 16][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // last key this row may see inside the tile's split: its token's
          // causal limit *pos + t, and the split's end
          const int rr = min((g0 + rg) * 16 + hi * 4 + r, R - 1);
          const int last = min(pos + rr / GQ, j_end - 1);
          float s[DKVT / 16];
#pragma unroll
          for (int nb = 0; nb < DKVT / 16; ++nb) {
            const int key = j0 + nb * 16 + col;
            s[nb] = s_acc[rg][nb][r];
            if (!interior && key > last) s[nb] = NEG_SENTINEL;
          }
          float mx = NEG_SENTINEL;
#pragma unroll
          for (int nb = 0; nb < DKVT / 16; ++nb) mx = fmaxf(mx, s[nb]);
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
          const float m_new = fmaxf(m_row[rg][r], mx);
          corr[rg][r] = (m_row[rg][r] <= NEG_THRESHOLD) ? 0.f : __expf(m_row[rg][r] - m_new);
          float lsum = 0.f;
#pragma unroll
          for (int nb = 0; nb < DKVT / 16; ++nb) {
            p[nb][r] = (s[nb] <= NEG_THRESHOLD) ? 0.f : __expf(s[nb] - m_new);
            lsum += p[nb][r];
          }
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off, WAVE);
          l_row[rg][r] = l_row[rg][r] * corr[rg][r] + lsum;
          m_row[rg][r] = m_new;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int nb = 0; nb < DKVT / 16; ++nb)
            p_lds[wave][rg * 16 + hi * 4 + r][nb * 16 + col] = f32_to_bf16(p[nb][r]);
      }
      __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);

      // ---- O += P V: each V^T fragment is read once and feeds every group
      bf16x8 p_frag[RG];
#pragma unroll
      for (int rg = 0; rg < RG; ++rg) {
        p_frag[rg] = *reinterpret_cast<const bf16x8*>(&p_lds[wave][rg * 16 + col][hi * 8]);
#pragma unroll
        for (int d = 0; d < HD / 16; ++d)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc_o[rg][d][r] *= corr[rg][r];
      }
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) {
        const bf16x8 vfrag = *reinterpret_cast<const bf16x8*>(&vt_raw[wave][DVT_BYTE(d * 16 + col, hi * 16)]);
#pragma unroll
        for (int rg = 0; rg < RG; ++rg)
          if (rg < ng) acc_o[rg][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p_frag[rg], vfrag, acc_o[rg][d], 0, 0, 0);
      }
    }

    // ---- cross-wave combine, one 16-row group at a time (overlay V^T LDS)
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
      if (rg >= ng) break;
      const int gbase = (g0 + rg) * 16;
      __syncthreads();  // main loop / the previous group's wave0 reads are done
      float* c_o = reinterpret_cast<float*>(vt_raw[wave]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gl = hi * 4 + r;
        if (gbase + gl < R) {
#pragma unroll
          for (int d = 0; d < HD / 16; ++d) c_o[gl * HD + d * 16 + col] = acc_o[rg][d][r];
          if (col == 0) {
            c_ml[wave][rg * 16 + gl][0] = m_row[rg][r];
            c_ml[wave][rg * 16 + gl][1] = l_row[rg][r];
          }
        }
      }
      __syncthreads();

      if (wave == 0) {
        const int gn = min(16, R - gbase);  // live rows of this group
        const size_t prow = ((size_t)bkv * n_splits + split) * R + gbase;
        for (int idx = lane; idx < gn * HD; idx += WAVE) {
          const int gl = idx / HD, d = idx - gl * HD;
          float m_star = c_ml[0][rg * 16 + gl][0];
#pragma unroll
          for (int w = 1; w < DWAVES; ++w) m_star = fmaxf(m_star, c_ml[w][rg * 16 + gl][0]);
          float osum = 0.f, lsum = 0.f;
#pragma unroll
          for (int w = 0; w < DWAVES; ++w) {
            const float mw = c_ml[w][rg * 16 + gl][0];
            const float wgt = (mw <= NEG_THRESHOLD) ? 0.f : __expf(mw - m_star);
            osum += wgt * reinterpret_cast<const float*>(vt_raw[w])[gl * HD + d];
            lsum += wgt * c_ml[w][rg * 16 + gl][1];
          }
          if (out_direct) {
            // single split: every row sees at least keys 0 .. *pos, lsum > 0
            const int t = (gbase + gl) / GQ, g = (gbase + gl) - t * GQ;
            out_direct[tok_base + (size_t)t * q_stride + g * HD + d] = osum / fmaxf(lsum, 1e-20f);
          } else {
            part_o[(prow + gl) * HD + d] = osum;
            if (d == 0) {
              part_ml[(prow + gl) * 2 + 0] = m_star;
              part_ml[(prow + gl) * 2 + 1] = lsum;
            }
          }
        }
      }
    }
  }
}

// attn_decode_combine_kernel (attention.hip) for the [B*KV, splits, R, HD]
// partials of the multi-token kernel: the same batched loads (8 splits per
// round trip) and the same accumulation in split order with reassociation
// off; row r = t * GQ + g goes to out[b*T + t, (kvh*GQ + g)*HD + d]. A row
// whose split saw no key carries m = NEG_SENTINEL and is skipped.
#define MULTI_COMBINE_BATCH 8

__global__ void attn_decode_multi_combine_kernel(
    const float* __restrict__ part_o,   // [B*KV, splits, R, HD]
    const float* __restrict__ part_ml,  // [B*KV, splits, R, 2]
    float* __restrict__ out,            // [B*T, KV*GQ*HD]
    int n_splits, int rows, int gq, int hd, int kv_heads, int tokens) {
#pragma clang fp reassociate(off)
  const int bkv = blockIdx.x;
  const int r = blockIdx.y;
  const auto row = [&](int s) { return ((size_t)bkv * n_splits + min(s, n_splits - 1)) * rows + r; };
  float m_star = NEG_SENTINEL;
  for (int s0 = 0; s0 < n_splits; s0 += MULTI_COMBINE_BATCH) {
    float ms[MULTI_COMBINE_BATCH];
#pragma unroll
    for (int i = 0; i < MULTI_COMBINE_BATCH; ++i) ms[i] = part_ml[row(s0 + i) * 2];
#pragma unroll
    for (int i = 0; i < MULTI_COMBINE_BATCH; ++i) m_star = fmaxf(m_star, ms[i]);
  }
  const int bi = bkv / kv_heads, kvh = bkv - bi * kv_heads;
  const int t = r / gq, g = r - t * gq;
  float* orow = out + ((size_t)(bi * tokens + t) * kv_heads + kvh) * gq * hd + (size_t)g * hd;
  for (int d = threadIdx.x; d < hd; d += blockDim.x) {
    float osum = 0.f, lsum = 0.f;
    for (int s0 = 0; s0 < n_splits; s0 += MULTI_COMBINE_BATCH) {
      float ms[MULTI_COMBINE_BATCH], ls[MULTI_COMBINE_BATCH], po[MULTI_COMBINE_BATCH];
#pragma unroll
      for (int i = 0; i < MULTI_COMBINE_BATCH; ++i) {
        ms[i] = part_ml[row(s0 + i) * 2];
        ls[i] = part_ml[row(s0 + i) * 2 + 1];
        po[i] = part_o[row(s0 + i) * hd + d];
      }
#pragma unroll
      for (int i = 0; i < MULTI_COMBINE_BATCH; ++i) {
        if (s0 + i >= n_splits || ms[i] <= NEG_THRESHOLD) continue;
        const float w = __expf(ms[i] - m_star);
        osum += w * po[i];
        lsum += w * ls[i];
      }
    }
    orow[d] = osum / fmaxf(lsum, 1e-20f);
  }
}

// ---------------------------------------------------------------- host API

// q: [B*T, KV*GQ*HD] f32, row b*T + t (what qkv_rope_reduce_multi writes and
// the o-projection GEMV reads); caches [Bc, KV, lmax, HD] bf16 or
// float8_e4m3fn holding the new tokens' rows at pos .. pos+T-1 already;
// pos: device int32 prefix length before the step. Returns [B*T, KV*GQ*HD] f32.
torch::Tensor attn_decode_multi(
    torch::Tensor q,
    torch::Tensor k_cache,
    torch::Tensor v_cache,
    torch::Tensor pos,  // device int32 [1]
    int64_t tokens,
    int64_t gq,
    int64_t n_splits_i,
    torch::Tensor part_o,   // workspace [B*KV, splits, T*GQ, HD] f32 (or empty)
    torch::Tensor part_ml,  // workspace [B*KV, splits, T*GQ, 2] f32 (or empty)
    double scale) {
  TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kFloat32 && q.dim() == 2 && q.is_contiguous());
  const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK((fp8 || k_cache.scalar_type() == at::kBFloat16) && k_cache.dim() == 4,
              "kv cache must be bf16 or float8_e4m3fn");
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type(), "k and v caches must share a dtype");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes() && k_cache.is_contiguous() && v_cache.is_contiguous());
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt && pos.numel() == 1, "pos must be a device int32 scalar");
  TORCH_CHECK(1 <= tokens && tokens <= 8, "attn_decode_multi takes 1..8 tokens per sequence, got ", tokens);
  TORCH_CHECK(q.size(0) % tokens == 0, "q rows must be B * tokens");
  const int T = (int)tokens;
  const int b = q.size(0) / T;
  TORCH_CHECK(b >= 1 && b <= k_cache.size(0), "more sequences than cache rows");
  const int kv_heads = k_cache.size(1), lmax = k_cache.size(2), hd = k_cache.size(3);
  TORCH_CHECK((int64_t)lmax * hd < (int64_t(1) << 32), "one (batch, head) of the cache must stay below 2^32 elements");
  TORCH_CHECK(T <= lmax, "the cache is shorter than the step");
  const int GQi = (int)gq;
  TORCH_CHECK(GQi >= 1 && GQi <= 16,
              "attn_decode_multi: gq = ", GQi, " is not built (one row group holds <= 16 heads; gq > 16 "
              "and ALiBi families take the single-token decode kernel)");
  TORCH_CHECK(q.size(1) == (int64_t)kv_heads * GQi * hd, "q width must be KV*GQ*HD");
  const int R = T * GQi;
  int n_splits = (int)n_splits_i;
  if (n_splits <= 0) {
    // attn_decode_fused's policy with bkv = B*KV: the T tokens of a sequence
    // share its workgroups. A starting point, not a knee measured for T > 1.
    const int bkv = std::max(1, b * kv_heads);
    const int by_occ = std::min(768 / bkv, lmax / 512);
    const int by_min = std::min(256 / bkv, (lmax + 127) / 128);
    n_splits = std::max(1, std::max(by_occ, by_min));
  }
  auto opts = q.options();
  const bool direct = n_splits == 1;  // parts go unused
  if (!direct && part_o.numel() < (int64_t)b * kv_heads * n_splits * R * hd)
    part_o = torch::empty({(int64_t)b * kv_heads, n_splits, R, hd}, opts);
  if (!direct && part_ml.numel() < (int64_t)b * kv_heads * n_splits * R * 2)
    part_ml = torch::empty({(int64_t)b * kv_heads, n_splits, R, 2}, opts);
  auto out = torch::empty({(int64_t)b * T, (int64_t)kv_heads * GQi * hd}, opts);

  dim3 grid(b * kv_heads, n_splits);
  auto stream = at::cuda::getCurrentCUDAStream();
  const float* qp = q.data_ptr<float>();
  const void* kp = k_cache.data_ptr();
  const void* vp = v_cache.data_ptr();
  float* pop = part_o.data_ptr<float>();
  float* pmlp = part_ml.data_ptr<float>();
  const int* posp = pos.data_ptr<int>();
  const float sc = (float)scale;
  float* direct_p = direct ? out.data_ptr<float>() : nullptr;
  bool launched = false;
#define MULTI_CASE(HDV, GQV)                                                                  \
  if (hd == HDV && GQi == GQV) {                                                              \
    if (fp8)                                                                                  \
      mfma_decode_multi_kernel<HDV, GQV, true, multi_row_groups(HDV, true)>                   \
          <<<grid, DWAVES * WAVE, 0, stream>>>(                                               \
              qp, static_cast<const unsigned char*>(kp), static_cast<const unsigned char*>(vp), \
              pop, pmlp, posp, kv_heads, lmax, T, n_splits, sc, direct_p);                    \
    else                                                                                      \
      mfma_decode_multi_kernel<HDV, GQV, false, multi_row_groups(HDV, false)>                 \
          <<<grid, DWAVES * WAVE, 0, stream>>>(                                               \
              qp, static_cast<const unsigned short*>(kp), static_cast<const unsigned short*>(vp), \
              pop, pmlp, posp, kv_heads, lmax, T, n_splits, sc, direct_p);                    \
    launched = true;                                                                          \
  }
  MULTI_CASE(128, 1) MULTI_CASE(128, 2) MULTI_CASE(128, 4) MULTI_CASE(128, 6)
  MULTI_CASE(128, 8) MULTI_CASE(128, 16)
  MULTI_CASE(64, 1) MULTI_CASE(64, 2) MULTI_CASE(64, 4) MULTI_CASE(64, 6)
  MULTI_CASE(64, 8) MULTI_CASE(64, 16)
#undef MULTI_CASE
  TORCH_CHECK(launched, "attn_decode_multi: unsupported (head_dim, gqa) = (", hd, ", ", GQi, ")");
  HIP_CHECK_LAST();

  if (direct_p == nullptr) {
    dim3 cgrid(b * kv_heads, R);
    attn_decode_multi_combine_kernel<<<cgrid, std::min(hd, 256), 0, stream>>>(
        pop, pmlp, out.data_ptr<float>(), n_splits, R, GQi, hd, kv_heads, T);
    HIP_CHECK_LAST();
  }
  return out;
}
