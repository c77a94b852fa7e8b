// Expert-grouped NF4 skinny-M GEMM for wide Mixtral decode steps (CDNA4 / gfx950):
//   partials[s, r, out] = x[r / k_per_tok, k-chunk s] . W[sel[r]][k-chunk s, out],  1 <= R <= 64
//
// The routed decode GEMVs (moe.hip gemv_*_moe) run one workgroup column per
// virtual row and stream that row's whole expert: past 16 rows every expert
// would be read once per row. The grouped prefill GEMM (moe.hip moe_gemm) wants
// a host-side sort, pads every expert to 32-row tiles and has no split-K. This
// kernel is the routed counterpart of nf4_skinny.hip: each ACTIVE expert's
// packed weight is streamed once per step and its rows sit on the matrix cores.
//
// Grid (ceil(out/256), S, E), 4 waves: a workgroup is one 256-column tile, one
// k chunk of whole 32-k steps and one expert e = blockIdx.z.
//
// Grouping, on the device. Every wave loads sel[lane] (lane < R) and ballots
// sel == e. The 64-bit mask is the same in all four waves, so the row count
// n_e = popcount(mask) is workgroup-uniform: with n_e == 0 the whole workgroup
// leaves before the LUT build and before any barrier (an idle expert costs one
// load and an exit). Otherwise lanes with a set bit write
// rowlist[popcount(mask below lane)] = lane to LDS, ascending, and one barrier
// covers the list and the LUT.
//
// The expert's rows run 16 at a time, ceil(n_e / 16) passes (a uniform trip
// count; a router with distinct top-k experts over 8 experts gives one pass,
// more passes re-stream the chunk). A pass is nf4_skinny_kernel<1, AMT>'s
// loop on packed_all + e * in * out/2: per 32-k step a lane loads 8 x 8 packed
// bytes = its 16 columns of 8 k rows, the 8 absmax (one 16-byte load from the
// transposed copy [E, out/64, in] when given, 8 two-byte gathers otherwise) and
// 8 fp32 of its x row; dequant through the 256-entry float2 pair LUT in LDS as
// bf16(LUT[nibble] * float(absmax)), one rounding, bit for bit nf4_dequantize;
// 16 mfma_f32_16x16x32_bf16; two register buffers, so step i+1 loads under
// step i. The A operand of pass p, lane (l15, hi), is slot p*16 + l15: 8 fp32
// of x[rowlist[slot] / k_per_tok] at k0 + hi*8, or a zero fragment, never
// loaded, for slots >= n_e.
//
// Combine and store: waves 1..3 park their accumulators in LDS (48 KB), wave 0
// adds them in wave order and stores rows hi*4 .. hi*4+3 of the pass to
// partials[(s * R + rowlist[slot]) * out + col0 ..], four 16-byte stores per
// row. Every virtual row belongs to exactly one expert, so each (s, r) row of
// [S, R, out] is written exactly once, and gemv_reduce runs unchanged.
//
// A sel value outside [0, E) matches no workgroup: that row's partials stay
// unwritten and nothing is read or written out of bounds. Lanes whose 16
// columns lie past out load and store nothing (16 | 64 | out).
//
// Rounding points: W to bf16 exactly as nf4_dequantize; x to bf16 once; the
// rest fp32 (the rounding of the prefill path these shapes ran before).

#include "common.h"
#include "gemv_reduce.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define MSK_WAVES 4
#define MSK_TILE_N 256        // columns per workgroup (every wave covers all of them)
#define MSK_KSTEP 32          // k per step: one MFMA depth
#define MSK_GROUP 16          // rows per pass: one MFMA row group
#define MSK_MAX_ROWS 64       // virtual rows: one ballot
#define MSK_PARTIAL_ROWS 512  // S * R bound: 64 splits x 8 rows of the decode workspace
// default split policy (profiles/moe_skinny.log, split sweep): the most
// workgroups tiles * min(E, R) * S may reach, two resident per CU on 256 CUs (the
// sweep steps with every multiple of 512 and loses just past one), and the k
// steps a workgroup keeps so every wave has at least two
#define MSK_TARGET_WGS 512
#define MSK_MIN_STEPS 8
#define MSK_KERNEL __attribute__((target("no-packed-fp32-ops"), amdgpu_waves_per_eu(2)))

using f32x2_msk = __attribute__((ext_vector_type(2))) float;
using bf16x2_msk = __attribute__((ext_vector_type(2))) __bf16;
using u32x4_msk = __attribute__((ext_vector_type(4))) unsigned int;

static __device__ __constant__ float MSK_NF4_LUT[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f,
    0.33791524171829224f, 0.4407098293304443f, 0.5626170039176941f,
    0.7229568362236023f, 1.0f};

// two fp32 -> packed bf16 pair, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned int msk_pack_bf16(float lo, float hi) {
  const bf16x2_msk r = __builtin_convertvector(f32x2_msk{lo, hi}, bf16x2_msk);
  return __builtin_bit_cast(unsigned int, r);
}

// one k step's operands as they come from memory
template <bool AMT>
struct MskStep {
  uint2 pk[8];                      // 8 k rows x 16 nibbles
  short8 amv;                       // AMT: the 8 absmax of the lane's k rows
  unsigned short ams[AMT ? 1 : 8];  // !AMT: the same, gathered
  float4v xa[2];                    // 8 fp32 of the lane's x row
};

template <bool AMT>
__global__ __launch_bounds__(WAVE * MSK_WAVES) MSK_KERNEL void nf4_moe_skinny_kernel(
    const unsigned char* __restrict__ packed_all,     // [E, in, out/2]
    const unsigned short* __restrict__ absmax_all,    // [E, in, out/64]
    const unsigned short* __restrict__ absmax_t_all,  // AMT: [E, out/64, in]
    const float* __restrict__ x,                      // [R / k_per_tok, in] f32
    const int* __restrict__ sel,                      // [R] expert of each virtual row
    float* __restrict__ partials,                     // [gridDim.y, R, out]
    int n_rows,
    int k_per_tok,
    int in_dim,
    int out_dim,
    int steps_per_split) {
  __shared__ float2 lut2[256];
  __shared__ float4v comb[MSK_WAVES - 1][16][WAVE];  // one row group of waves 1..3: 48 KB
  __shared__ int rowlist[MSK_MAX_ROWS];

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int e = blockIdx.z;

  // this expert's rows: the same mask in every wave, so n_e is workgroup-uniform
  const int my_sel = lane < n_rows ? sel[lane] : -1;
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(my_sel == e);
  if (mask == 0ull) return;  // idle expert: before the LUT build, before any barrier
  const int n_e = __builtin_popcountll(mask);
  if (wave == 0 && ((mask >> lane) & 1ull)) rowlist[__builtin_popcountll(mask & ((1ull << lane) - 1ull))] = lane;
  lut2[threadIdx.x] = make_float2(MSK_NF4_LUT[threadIdx.x & 0xF], MSK_NF4_LUT[threadIdx.x >> 4]);
  __syncthreads();

  const int l15 = lane & 15;
  const int hi = lane >> 4;
  const int col0 = blockIdx.x * MSK_TILE_N + l15 * 16;
  const bool live = col0 < out_dim;

  // this workgroup's steps [s0, s1), this wave's share [w0, w1) of them
  const int nk = in_dim / MSK_KSTEP;
  const int s0 = blockIdx.y * steps_per_split;
  const int s1 = min(nk, s0 + steps_per_split);
  const int per_wave = (steps_per_split + MSK_WAVES - 1) / MSK_WAVES;
  const int w0 = min(s1, s0 + wave * per_wave);
  const int w1 = min(s1, w0 + per_wave);

  const size_t half_out = (size_t)(out_dim >> 1);
  const int nblk = out_dim >> 6;
  const int blk = col0 >> 6;
  const unsigned char* wp = packed_all + (size_t)e * in_dim * half_out + (size_t)(hi * 8) * half_out + (col0 >> 1);
  const unsigned short* amp = absmax_all + (size_t)e * in_dim * nblk + blk;
  const unsigned short* amtp = AMT ? absmax_t_all + ((size_t)e * nblk + blk) * in_dim + hi * 8 : nullptr;

  const int passes = (n_e + MSK_GROUP - 1) / MSK_GROUP;
#pragma clang loop unroll(disable)
  for (int p = 0; p < passes; ++p) {
    const int slot = p * MSK_GROUP + l15;
    const bool xrow = slot < n_e;
    const float* xp = x + (size_t)(xrow ? rowlist[slot] / k_per_tok : 0) * in_dim + hi * 8;

    auto load_step = [&](MskStep<AMT>& st, int step) __attribute__((always_inline)) {
      const int k0 = step * MSK_KSTEP;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        st.pk[j] = make_uint2(0u, 0u);
        if (live) st.pk[j] = *reinterpret_cast<const uint2*>(wp + (size_t)(k0 + j) * half_out);
      }
      if constexpr (AMT) {
        st.amv = short8{0, 0, 0, 0, 0, 0, 0, 0};
        if (live) st.amv = *reinterpret_cast<const short8*>(amtp + k0);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          st.ams[j] = 0;
          if (live) st.ams[j] = amp[(size_t)(k0 + hi * 8 + j) * nblk];
        }
      }
      st.xa[0] = st.xa[1] = float4v{0.f, 0.f, 0.f, 0.f};
      if (xrow) {
        st.xa[0] = *reinterpret_cast<const float4v*>(xp + k0);
        st.xa[1] = *reinterpret_cast<const float4v*>(xp + k0 + 4);
      }
    };

    float4v acc[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = float4v{0.f, 0.f, 0.f, 0.f};

    auto compute_step = [&](const MskStep<AMT>& st) __attribute__((always_inline)) {
      const u32x4_msk w = {msk_pack_bf16(st.xa[0][0], st.xa[0][1]), msk_pack_bf16(st.xa[0][2], st.xa[0][3]),
                           msk_pack_bf16(st.xa[1][0], st.xa[1][1]), msk_pack_bf16(st.xa[1][2], st.xa[1][3])};
      const short8 a = __builtin_bit_cast(short8, w);
      float am[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if constexpr (AMT) am[j] = bf16_to_f32((unsigned short)st.amv[j]);
        else am[j] = bf16_to_f32(st.ams[j]);
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {  // packed byte c = tile columns 2c, 2c+1 of the lane's 16
        u32x4_msk lo, hh;
#pragma unroll
        for (int t = 0; t < 4; ++t) {  // k pair (2t, 2t+1) -> one packed bf16 word per column
          const unsigned int p0 = c < 4 ? st.pk[2 * t].x : st.pk[2 * t].y;
          const unsigned int p1 = c < 4 ? st.pk[2 * t + 1].x : st.pk[2 * t + 1].y;
          const float2 e0 = lut2[(p0 >> (8 * (c & 3))) & 0xFFu];
          const float2 e1 = lut2[(p1 >> (8 * (c & 3))) & 0xFFu];
          lo[t] = msk_pack_bf16(e0.x * am[2 * t], e1.x * am[2 * t + 1]);
          hh[t] = msk_pack_bf16(e0.y * am[2 * t], e1.y * am[2 * t + 1]);
        }
        acc[2 * c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(short8, lo), acc[2 * c], 0, 0, 0);
        acc[2 * c + 1] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(short8, hh), acc[2 * c + 1], 0, 0, 0);
      }
    };

    // two register buffers: step i+1 is on its way while step i computes
    MskStep<AMT> buf0, buf1;
    if (w0 < w1) load_step(buf0, w0);
    for (int i = w0; i < w1; i += 2) {
      if (i + 1 < w1) load_step(buf1, i + 1);
      compute_step(buf0);
      if (i + 1 < w1) {
        if (i + 2 < w1) load_step(buf0, i + 2);
        compute_step(buf1);
      }
    }

    // in-workgroup combine: waves 1..3 park, wave 0 adds in wave order and
    // stores the pass's rows where the reduce expects them. A wave with no
    // steps contributes +0.
    if (wave > 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) comb[wave - 1][v][lane] = acc[v];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v)
#pragma unroll
        for (int w = 0; w < MSK_WAVES - 1; ++w) acc[v] += comb[w][v][lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oslot = p * MSK_GROUP + hi * 4 + r;
        if (live && oslot < n_e) {
          float* dst = partials + ((size_t)blockIdx.y * n_rows + rowlist[oslot]) * out_dim + col0;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            reinterpret_cast<float4v*>(dst)[q] =
                float4v{acc[4 * q][r], acc[4 * q + 1][r], acc[4 * q + 2][r], acc[4 * q + 3][r]};
        }
      }
    }
    if (p + 1 < passes) __syncthreads();  // comb is reused by the next pass
  }
}

// ------------------------------------------------------------------- host

// k steps per split and the split count S for a shape: a function of
// (in, out, R, E) alone, S * R <= 512, every split holds whole steps, no split
// is empty. The default is the largest S that keeps the tiles * min(E, R) * S
// workgroups a step is expected to run within MSK_TARGET_WGS, each with at
// least MSK_MIN_STEPS steps.
static int msk_policy(int64_t in_dim, int64_t out_dim, int64_t rows, int64_t experts, int64_t splits_override,
                      int* steps_per_split) {
  const int64_t nk = in_dim / MSK_KSTEP;
  const int64_t tiles = (out_dim + MSK_TILE_N - 1) / MSK_TILE_N;
  int64_t want = splits_override;
  if (want <= 0) {
    const int64_t wgs = tiles * std::min<int64_t>(experts, rows);
    want = std::min<int64_t>(MSK_TARGET_WGS / wgs, nk / MSK_MIN_STEPS);
  }
  want = std::max<int64_t>(1, std::min<int64_t>(want, std::min<int64_t>(MSK_PARTIAL_ROWS / rows, nk)));
  const int64_t per = (nk + want - 1) / want;
  *steps_per_split = (int)per;
  return (int)((nk + per - 1) / per);
}

static void msk_check_shape(int64_t in_dim, int64_t out_dim, int64_t rows, int64_t experts) {
  TORCH_CHECK(rows >= 1 && rows <= MSK_MAX_ROWS, "gemm_nf4_moe_skinny takes 1..64 virtual rows, got ", rows);
  TORCH_CHECK(experts >= 1 && experts <= 65535, "gemm_nf4_moe_skinny takes 1..65535 experts, got ", experts);
  TORCH_CHECK(in_dim > 0 && in_dim % MSK_KSTEP == 0, "gemm_nf4_moe_skinny needs in % 32 == 0, got ", in_dim);
  TORCH_CHECK(out_dim > 0 && out_dim % 64 == 0, "gemm_nf4_moe_skinny needs out % 64 == 0, got ", out_dim);
}

int64_t gemm_nf4_moe_skinny_splits(int64_t in_dim, int64_t out_dim, int64_t rows, int64_t experts,
                                   int64_t splits_override) {
  msk_check_shape(in_dim, out_dim, rows, experts);
  int per;
  return msk_policy(in_dim, out_dim, rows, experts, splits_override, &per);
}

torch::Tensor gemm_nf4_moe_skinny(
    torch::Tensor packed_all,  // [E, in, out/2] u8
    torch::Tensor absmax_all,  // [E, in, out/64] bf16
    torch::Tensor x,           // [tokens, in] f32
    torch::Tensor sel,         // [R] int32, R = tokens * k_per_tok
    int64_t k_per_tok,
    torch::Tensor workspace,   // f32; holds the partials when S * R * out floats fit
    int64_t epilogue,
    int64_t splits_override,
    c10::optional<torch::Tensor> absmax_t_all) {  // [E, out/64, in] bf16 (transposed copy), optional
  TORCH_CHECK(packed_all.is_cuda() && packed_all.dtype() == torch::kUInt8 && packed_all.dim() == 3 &&
                  packed_all.is_contiguous(),
              "gemm_nf4_moe_skinny: packed_all must be a contiguous u8 [E, in, out/2] GPU tensor");
  const int64_t experts = packed_all.size(0), in_dim = packed_all.size(1), out_dim = packed_all.size(2) * 2;
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kFloat32 && x.dim() == 2 && x.is_contiguous(),
              "gemm_nf4_moe_skinny: x must be a contiguous f32 [tokens, in] GPU tensor");
  TORCH_CHECK(x.size(1) == in_dim, "gemm_nf4_moe_skinny: x has ", x.size(1), " columns, the weights have ", in_dim,
              " rows");
  TORCH_CHECK(sel.is_cuda() && sel.dtype() == torch::kInt32 && sel.dim() == 1 && sel.is_contiguous(),
              "gemm_nf4_moe_skinny: sel must be a contiguous i32 [R] GPU tensor");
  const int64_t rows = sel.size(0);
  msk_check_shape(in_dim, out_dim, rows, experts);
  TORCH_CHECK(k_per_tok >= 1 && x.size(0) * k_per_tok == rows, "gemm_nf4_moe_skinny: sel has ", rows,
              " virtual rows, x has ", x.size(0), " tokens of ", k_per_tok);
  TORCH_CHECK(epilogue == EPI_PLAIN_F32 || epilogue == EPI_SWIGLU_F32,
              "gemm_nf4_moe_skinny has the plain-f32 and swiglu-f32 epilogues only (no raw-partials mode), got ",
              epilogue);
  TORCH_CHECK(absmax_all.is_cuda() && absmax_all.dtype() == torch::kBFloat16 && absmax_all.dim() == 3 &&
                  absmax_all.is_contiguous() && absmax_all.size(0) == experts && absmax_all.size(1) == in_dim &&
                  absmax_all.size(2) * 64 == out_dim,
              "gemm_nf4_moe_skinny: absmax_all must be a contiguous bf16 [E, in, out/64] GPU tensor");
  TORCH_CHECK(workspace.is_cuda() && workspace.dtype() == torch::kFloat32 && workspace.is_contiguous(),
              "gemm_nf4_moe_skinny: workspace must be a contiguous f32 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(packed_all.data_ptr()) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(workspace.data_ptr()) % 16 == 0,
              "gemm_nf4_moe_skinny: packed_all must be 8-byte, x and workspace 16-byte aligned");
  const unsigned short* amt_p = nullptr;
  if (absmax_t_all.has_value() && absmax_t_all->defined() && absmax_t_all->numel() > 0) {
    TORCH_CHECK(absmax_t_all->is_cuda() && absmax_t_all->dtype() == torch::kBFloat16 &&
                    absmax_t_all->is_contiguous() && absmax_t_all->dim() == 3 && absmax_t_all->size(0) == experts &&
                    absmax_t_all->size(1) == out_dim / 64 && absmax_t_all->size(2) == in_dim &&
                    reinterpret_cast<uintptr_t>(absmax_t_all->data_ptr()) % 16 == 0,
                "gemm_nf4_moe_skinny: absmax_t_all must be a contiguous, 16-byte aligned bf16 [E, out/64, in] "
                "GPU tensor");
    amt_p = reinterpret_cast<const unsigned short*>(absmax_t_all->data_ptr());
  }

  int per;
  const int splits = msk_policy(in_dim, out_dim, rows, experts, splits_override, &per);
  const int64_t need = (int64_t)splits * rows * out_dim;
  auto f32opts = x.options().dtype(torch::kFloat32);
  torch::Tensor partials = workspace.numel() >= need ? workspace : torch::empty({need}, f32opts);

  dim3 grid((unsigned)((out_dim + MSK_TILE_N - 1) / MSK_TILE_N), (unsigned)splits, (unsigned)experts);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_MSK(AMT)                                                                 \
  nf4_moe_skinny_kernel<AMT><<<grid, WAVE * MSK_WAVES, 0, stream>>>(                    \
      packed_all.data_ptr<unsigned char>(),                                             \
      reinterpret_cast<const unsigned short*>(absmax_all.data_ptr()), amt_p,            \
      x.data_ptr<float>(), sel.data_ptr<int>(), partials.data_ptr<float>(), (int)rows,  \
      (int)k_per_tok, (int)in_dim, (int)out_dim, per)
  if (amt_p) LAUNCH_MSK(true); else LAUNCH_MSK(false);
#undef LAUNCH_MSK
  HIP_CHECK_LAST();
  return launch_gemv_reduce(partials, c10::nullopt, c10::nullopt, splits, (int)rows, (int)out_dim, (int)epilogue,
                            f32opts, absmax_all.options());
}
