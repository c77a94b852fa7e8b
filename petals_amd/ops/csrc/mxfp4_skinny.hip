// MXFP4 skinny-M GEMM for wide decode steps (CDNA4 / gfx950):
//   partials[s, r, out] = x[r, k-chunk s] . W[k-chunk s, out],  9 <= rows <= 32
//
// The MXFP4 sibling of nf4_skinny.hip: same work split, same partial layout,
// same reduce kernels behind it, another dequant. gemv_mxfp4 (mxfp4.hip) keeps
// one fp32 accumulator set per batch row and stops at 8 rows; gemm_mxfp4
// (gemm_quant.hip) stages 128x128 tiles through LDS. This kernel streams the
// packed weight once and puts the rows on the matrix cores.
//
// Dataflow. A workgroup is 4 waves over one 256-column tile and one K chunk;
// every wave covers all 256 columns and a quarter of the chunk's steps. A step
// is 32 k: one mfma_f32_16x16x32_bf16 depth and exactly one MX scale block.
// Lane (l15 = lane & 15, hi = lane >> 4):
//   A operand (x): row g*16 + l15 of row group g (1 or 2 groups), k
//     hi*8 .. hi*8+7: two 16-byte fp32 loads, four v_cvt_pk_bf16_f32. Rows
//     >= rows are zero fragments, never loaded.
//   B operand (W): straight from global memory, no LDS. The lane's 8 k are 4
//     packed rows (k0 + hi*8)/2 + 0..3; from each it loads 16 bytes = tile
//     columns 16*l15 .. 16*l15+15, so the 16 lanes of a k group read 256
//     contiguous bytes of a packed row. Byte v of load t holds k 2t (low
//     nibble) and 2t+1 of column 16*l15 + v: one v_cvt_scalef32_pk_bf16_fp4
//     makes it word t of B fragment v. No LUT, no multiply, no rounding.
//   Scales: one 16-byte load of scales[k0/32, 16*l15 .. +15] per step; byte v
//     << 23 is the fp32 scale operand of fragment v's four conversions.
//   C: lane holds, per fragment v, rows hi*4 .. hi*4+3 of column 16*l15 + v:
//     16 consecutive columns, four 16-byte stores per row.
//
// In flight: the loads of step i+1 (64 B packed + 16 B scales + 32 B of x per
// row group, per lane) are issued before the conversions and MFMAs of step i,
// two register buffers.
//
// Split-K twice, no atomics, as nf4_skinny.hip: grid.y slices k into S chunks
// of whole steps, S a function of (in, out, rows) alone with S * rows <= 512,
// so the partials [S, rows, out] fit the 64 * 8 * max_out floats an 8-row
// decode step already holds. Waves 1..3 park their accumulators in LDS and
// wave 0 adds them in wave order and stores the workgroup's one partial row
// set. (The combine and the S bounds are a copy of nf4_skinny.hip's, which
// stays byte for byte what it was; the default S has its own target.)
//
// Rounding points: W is exact (E2M1 times a power of two is a bf16 value); x
// to bf16 once; the rest fp32. Requires in % 32 == 0 and out % 16 == 0: a
// lane's 16 columns are all inside out or all outside, and outside lanes load
// nothing and store nothing.

#include "common.h"
#include "gemv_reduce.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define MS_WAVES 4
#define MS_TILE_N 256        // columns per workgroup (every wave covers all of them)
#define MS_KSTEP 32          // k per step: one MFMA depth, one MX scale block
#define MS_MIN_ROWS 9
#define MS_MAX_ROWS 32
#define MS_PARTIAL_ROWS 512  // S * rows bound: 64 splits x 8 rows of the decode workspace
// default split policy (profiles/mxfp4_skinny.log, split sweep): the most
// workgroups that still run in one round of one per CU (the sweep's optima sit
// at tiles * S = 240..256 or twice that; 384, the NF4 kernel's target, falls
// between the rounds and cost up to 15 %), and the k steps a workgroup keeps so
// every wave has at least two
#define MS_TARGET_WGS 256
#define MS_MIN_STEPS 8

using f32x2_ms = __attribute__((ext_vector_type(2))) float;
using bf16x2_ms = __attribute__((ext_vector_type(2))) __bf16;
using u32x4_ms = __attribute__((ext_vector_type(4))) unsigned int;

// two fp32 -> packed bf16 pair, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned int ms_pack_bf16(float lo, float hi) {
  const bf16x2_ms r = __builtin_convertvector(f32x2_ms{lo, hi}, bf16x2_ms);
  return __builtin_bit_cast(unsigned int, r);
}

// byte BYTE of `word` (two consecutive-k fp4 of one column) * scale -> packed
// bf16 pair, low nibble (the even k) in the low half
template <int BYTE>
__device__ __forceinline__ unsigned int ms_fp4_bf16x2(unsigned int word, float scale) {
  const bf16x2_ms r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, BYTE);
  return __builtin_bit_cast(unsigned int, r);
}

// B fragment of the column in byte BYTE of the four packed rows' words, under
// the E8M0 scale in byte BYTE of `sc` (byte s in 1..254 is the fp32 exponent)
template <int BYTE>
__device__ __forceinline__ short8 ms_bfrag(unsigned int p0, unsigned int p1, unsigned int p2, unsigned int p3,
                                           unsigned int sc) {
  const float scale = __uint_as_float(((sc >> (8 * BYTE)) & 0xFFu) << 23);
  const u32x4_ms w = {ms_fp4_bf16x2<BYTE>(p0, scale), ms_fp4_bf16x2<BYTE>(p1, scale),
                      ms_fp4_bf16x2<BYTE>(p2, scale), ms_fp4_bf16x2<BYTE>(p3, scale)};
  return __builtin_bit_cast(short8, w);
}

// one k step's operands as they come from memory
template <int G>
struct MsStep {
  u32x4_ms pk[4];    // 4 packed rows (8 k) x 16 columns
  u32x4_ms sc;       // the 16 columns' scale bytes
  float4v xa[G][2];  // 8 fp32 of one x row per row group
};

template <int G>
__global__ __launch_bounds__(WAVE * MS_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void mxfp4_skinny_kernel(
    const unsigned char* __restrict__ packed,  // [in/2, out]
    const unsigned char* __restrict__ scales,  // [in/32, out]
    const float* __restrict__ x,               // [rows, in] f32
    float* __restrict__ partials,              // [gridDim.y, rows, out]
    int rows,
    int in_dim,
    int out_dim,
    int steps_per_split) {
  __shared__ float4v comb[MS_WAVES - 1][16][WAVE];  // one row group of waves 1..3: 48 KB

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15;
  const int hi = lane >> 4;
  const int col0 = blockIdx.x * MS_TILE_N + l15 * 16;
  const bool live = col0 < out_dim;

  // this workgroup's steps [s0, s1), this wave's share [w0, w1) of them
  const int nk = in_dim / MS_KSTEP;
  const int s0 = blockIdx.y * steps_per_split;
  const int s1 = min(nk, s0 + steps_per_split);
  const int per_wave = (steps_per_split + MS_WAVES - 1) / MS_WAVES;
  const int w0 = min(s1, s0 + wave * per_wave);
  const int w1 = min(s1, w0 + per_wave);

  const unsigned char* wp = packed + (size_t)(hi * 4) * out_dim + col0;
  const unsigned char* sp = scales + col0;
  bool xrow[G];
  const float* xp[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    xrow[g] = g * 16 + l15 < rows;
    xp[g] = x + (size_t)(xrow[g] ? g * 16 + l15 : 0) * in_dim + hi * 8;
  }

  auto load_step = [&](MsStep<G>& st, int step) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st.pk[t] = u32x4_ms{0u, 0u, 0u, 0u};
      if (live) st.pk[t] = *reinterpret_cast<const u32x4_ms*>(wp + (size_t)(step * (MS_KSTEP / 2) + t) * out_dim);
    }
    st.sc = u32x4_ms{0u, 0u, 0u, 0u};
    if (live) st.sc = *reinterpret_cast<const u32x4_ms*>(sp + (size_t)step * out_dim);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      st.xa[g][0] = st.xa[g][1] = float4v{0.f, 0.f, 0.f, 0.f};
      if (xrow[g]) {
        st.xa[g][0] = *reinterpret_cast<const float4v*>(xp[g] + step * MS_KSTEP);
        st.xa[g][1] = *reinterpret_cast<const float4v*>(xp[g] + step * MS_KSTEP + 4);
      }
    }
  };

  float4v acc[G][16];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[g][v] = float4v{0.f, 0.f, 0.f, 0.f};

  auto compute_step = [&](const MsStep<G>& st) __attribute__((always_inline)) {
    short8 a[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const u32x4_ms w = {ms_pack_bf16(st.xa[g][0][0], st.xa[g][0][1]), ms_pack_bf16(st.xa[g][0][2], st.xa[g][0][3]),
                          ms_pack_bf16(st.xa[g][1][0], st.xa[g][1][1]), ms_pack_bf16(st.xa[g][1][2], st.xa[g][1][3])};
      a[g] = __builtin_bit_cast(short8, w);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // word q of the loads = columns 4q .. 4q+3 of the lane's 16
      const unsigned int p0 = st.pk[0][q], p1 = st.pk[1][q], p2 = st.pk[2][q], p3 = st.pk[3][q], sc = st.sc[q];
      const short8 b[4] = {ms_bfrag<0>(p0, p1, p2, p3, sc), ms_bfrag<1>(p0, p1, p2, p3, sc),
                           ms_bfrag<2>(p0, p1, p2, p3, sc), ms_bfrag<3>(p0, p1, p2, p3, sc)};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int g = 0; g < G; ++g)
          acc[g][4 * q + c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[g], b[c], acc[g][4 * q + c], 0, 0, 0);
    }
  };

  // two register buffers: step i+1 is on its way while step i computes
  MsStep<G> buf0, buf1;
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
        for (int w = 0; w < MS_WAVES - 1; ++w) acc[g][v] += comb[w][v][lane];
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
// split holds whole steps, no split is empty. The default is the largest S
// with tiles * S <= MS_TARGET_WGS and at least MS_MIN_STEPS steps per workgroup.
static int ms_policy(int64_t in_dim, int64_t out_dim, int64_t rows, int64_t splits_override, int* steps_per_split) {
  const int64_t nk = in_dim / MS_KSTEP;
  const int64_t tiles = (out_dim + MS_TILE_N - 1) / MS_TILE_N;
  int64_t want = splits_override;
  if (want <= 0) {
    want = std::min<int64_t>(MS_TARGET_WGS / tiles, nk / MS_MIN_STEPS);
  }
  want = std::max<int64_t>(1, std::min<int64_t>(want, std::min<int64_t>(MS_PARTIAL_ROWS / rows, nk)));
  const int64_t per = (nk + want - 1) / want;
  *steps_per_split = (int)per;
  return (int)((nk + per - 1) / per);
}

static void ms_check_shape(int64_t in_dim, int64_t out_dim, int64_t rows) {
  TORCH_CHECK(rows >= MS_MIN_ROWS && rows <= MS_MAX_ROWS, "gemm_mxfp4_skinny takes 9..32 rows, got ", rows,
              " (1..8 rows run gemv_mxfp4, more than 32 the prefill GEMM)");
  TORCH_CHECK(in_dim > 0 && in_dim % MS_KSTEP == 0, "gemm_mxfp4_skinny needs in % 32 == 0, got ", in_dim);
  TORCH_CHECK(out_dim > 0 && out_dim % 16 == 0, "gemm_mxfp4_skinny needs out % 16 == 0, got ", out_dim);
  TORCH_CHECK(in_dim < (1LL << 31) && out_dim < (1LL << 31), "gemm_mxfp4_skinny: weight too large");
}

int64_t gemm_mxfp4_skinny_splits(int64_t in_dim, int64_t out_dim, int64_t rows, int64_t splits_override) {
  ms_check_shape(in_dim, out_dim, rows);
  int per;
  return ms_policy(in_dim, out_dim, rows, splits_override, &per);
}

torch::Tensor gemm_mxfp4_skinny(
    torch::Tensor packed,     // [in/2, out] u8
    torch::Tensor scales,     // [in/32, out] u8 (E8M0)
    torch::Tensor x,          // [rows, in] f32, 9 <= rows <= 32
    torch::Tensor workspace,  // f32; holds the partials when S * rows * out floats fit
    c10::optional<torch::Tensor> residual,
    int64_t epilogue,
    int64_t splits_override,
    c10::optional<torch::Tensor> bias) {  // [out] bf16, added pre-activation
  TORCH_CHECK(packed.is_cuda() && packed.dtype() == torch::kUInt8 && packed.dim() == 2 && packed.is_contiguous(),
              "gemm_mxfp4_skinny: packed must be a contiguous u8 [in/2, out] GPU tensor");
  const int64_t in_dim = packed.size(0) * 2, out_dim = packed.size(1);
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kFloat32 && x.dim() == 2 && x.is_contiguous(),
              "gemm_mxfp4_skinny: x must be a contiguous f32 [rows, in] GPU tensor");
  TORCH_CHECK(x.size(1) == in_dim, "gemm_mxfp4_skinny: x has ", x.size(1), " columns, the weight has ", in_dim,
              " rows");
  const int64_t rows = x.size(0);
  ms_check_shape(in_dim, out_dim, rows);
  TORCH_CHECK(scales.is_cuda() && scales.dtype() == torch::kUInt8 && scales.dim() == 2 && scales.is_contiguous() &&
                  scales.size(0) == in_dim / MS_KSTEP && scales.size(1) == out_dim,
              "gemm_mxfp4_skinny: scales must be a contiguous u8 [in/32, out] GPU tensor");
  TORCH_CHECK(workspace.is_cuda() && workspace.dtype() == torch::kFloat32 && workspace.is_contiguous(),
              "gemm_mxfp4_skinny: workspace must be a contiguous f32 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(packed.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(scales.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "gemm_mxfp4_skinny: packed, scales and x must be 16-byte aligned");

  int per;
  const int splits = ms_policy(in_dim, out_dim, rows, splits_override, &per);
  const int64_t need = (int64_t)splits * rows * out_dim;
  auto f32opts = x.options().dtype(torch::kFloat32);
  const bool fits = workspace.numel() >= need && reinterpret_cast<uintptr_t>(workspace.data_ptr()) % 16 == 0;
  torch::Tensor partials = fits ? workspace : torch::empty({need}, f32opts);

  dim3 grid((unsigned)((out_dim + MS_TILE_N - 1) / MS_TILE_N), (unsigned)splits);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_MS(G)                                                                \
  mxfp4_skinny_kernel<G><<<grid, WAVE * MS_WAVES, 0, stream>>>(                     \
      packed.data_ptr<unsigned char>(), scales.data_ptr<unsigned char>(),           \
      x.data_ptr<float>(), partials.data_ptr<float>(), (int)rows, (int)in_dim, (int)out_dim, per)
  if (rows <= 16) LAUNCH_MS(1); else LAUNCH_MS(2);
#undef LAUNCH_MS
  HIP_CHECK_LAST();

  if (epilogue < 0) {
    // RAW mode, as gemv_mxfp4: the caller fuses its own reduce (qkv_rope_reduce[_multi])
    return partials.view(-1).narrow(0, 0, need).view({(int64_t)splits, rows, out_dim});
  }
  return launch_gemv_reduce(partials, residual, bias, splits, (int)rows, (int)out_dim, (int)epilogue, f32opts,
                            f32opts.dtype(torch::kBFloat16));
}
