// LoRA inside the decode kernel chain (gfx950): a projection group under an
// adapter runs  base GEMV (RAW partials) -> lora_shrink -> lora_reduce.
//
// A group is the projections that share an input (q|k|v, o, gate|up, down).
// Its present members' A matrices are stacked into a_cat [R, in] (PEFT's
// K-contiguous rows, bf16), its B matrices are stored transposed one after the
// other in bt (member p: [r_p, out_p] row-major, bf16).
//
//   lora_shrink_kernel  t_part[s, b, j] = x[b, chunk s] . a_cat[j, chunk s]
//       A workgroup of 4 waves owns LS_TILE = 8 rows of a_cat (2 per wave) and
//       one K chunk. Per 512-k step every lane issues its rows' 16-byte loads
//       (8 k of a row), then the workgroup stages x[rows][512] fp32 in LDS,
//       split into two float4 planes so that a lane's two reads per batch row
//       are conflict-free, and every wave reads it from there. At the end of
//       the chunk each (row, b) accumulator goes through a fixed xor butterfly
//       and lane 0 writes it. No atomics; S and the tile depend on (R, in)
//       only, so two runs give the same bits.
//
//   lora_reduce_kernel  gemv_reduce_kernel with the expand folded in, before
//       the epilogue. The workgroup first sums t_part over S in index order
//       into LDS (only the batch rows its 64 outputs touch). Then thread
//       (output o, group g) sums the base partial rows g, g+16, ... exactly as
//       gemv_reduce_kernel does, and next to them rank rows g, g+16, ... of
//       B^T[j][o] * t[b][j] for the member that owns column o: the 64 output
//       lanes read 128 contiguous bytes of bt per rank row. Base groups and
//       delta groups are added in index order, apart from each other;
//       sum = base + scale_p * delta in fp32; then the unchanged epilogue, so
//       o and down round to bf16 once. A column with no member never touches
//       its sum. The member table travels by value: nothing to sync, the op
//       is hipGraph-capturable.
//
// Rounding points: none before the epilogue. x stays fp32, A and B are bf16
// read as themselves, every product and sum is fp32.

#include "common.h"
#include "gemv_reduce.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

// compiled without packed fp32 VALU ops
#define LORA_KERNEL __attribute__((target("no-packed-fp32-ops")))

#define LS_WAVES 4
#define LS_ROWS_PER_WAVE 2
#define LS_TILE (LS_WAVES * LS_ROWS_PER_WAVE)
#define LS_STEP 512       // k per wave step: 64 lanes x 8 bf16
#define LS_MAX_SPLITS 32
#define LORA_MAX_R 256
#define LORA_MAX_ROWS 8
#define LORA_MAX_SEGS 4

// K chunk (a multiple of LS_STEP) and split count, from in_dim alone
static inline void lora_shrink_policy(int in_dim, int* chunk, int* splits) {
  const int steps = (in_dim + LS_STEP - 1) / LS_STEP;
  const int steps_per_chunk = (steps + LS_MAX_SPLITS - 1) / LS_MAX_SPLITS;
  *chunk = steps_per_chunk * LS_STEP;
  *splits = (steps + steps_per_chunk - 1) / steps_per_chunk;
}

template <int ROWS>
__global__ __launch_bounds__(64 * LS_WAVES) LORA_KERNEL void lora_shrink_kernel(
    const float* __restrict__ x,           // [ROWS, in_dim]
    const unsigned short* __restrict__ a,  // [R, in_dim] bf16
    float* __restrict__ t_part,            // [S, ROWS, R]
    int in_dim, int R, int chunk) {
  // plane p of batch row b holds the float4s 2*lane + p of the step
  __shared__ float4 xs[ROWS][2][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * LS_TILE + wave * LS_ROWS_PER_WAVE;
  const int k_begin = blockIdx.y * chunk;
  const int k_end = min(k_begin + chunk, in_dim);

  float acc[LS_ROWS_PER_WAVE][ROWS];
#pragma unroll
  for (int r = 0; r < LS_ROWS_PER_WAVE; ++r)
#pragma unroll
    for (int b = 0; b < ROWS; ++b) acc[r][b] = 0.f;

  // uniform trip count: every thread reaches every barrier
  for (int k0 = k_begin; k0 < k_end; k0 += LS_STEP) {
    const int k = k0 + lane * 8;
    uint4 av[LS_ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < LS_ROWS_PER_WAVE; ++r) {
      av[r] = make_uint4(0u, 0u, 0u, 0u);
      if (row0 + r < R && k < in_dim)  // in_dim % 8 == 0: the 8 k are all in or all out
        av[r] = *reinterpret_cast<const uint4*>(a + (size_t)(row0 + r) * in_dim + k);
    }
    if (k0 != k_begin) __syncthreads();  // the previous step's reads are done
    for (int i = threadIdx.x; i < ROWS * 128; i += 64 * LS_WAVES) {
      const int b = i >> 7, f = i & 127;
      const int kx = k0 + f * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kx < in_dim) v = *reinterpret_cast<const float4*>(x + (size_t)b * in_dim + kx);
      xs[b][f & 1][f >> 1] = v;
    }
    __syncthreads();
    float af[LS_ROWS_PER_WAVE][8];
#pragma unroll
    for (int r = 0; r < LS_ROWS_PER_WAVE; ++r) {
      const unsigned w[4] = {av[r].x, av[r].y, av[r].z, av[r].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        af[r][2 * e] = __uint_as_float(w[e] << 16);
        af[r][2 * e + 1] = __uint_as_float(w[e] & 0xFFFF0000u);
      }
    }
#pragma unroll
    for (int b = 0; b < ROWS; ++b) {
      const float4 lo = xs[b][0][lane], hi = xs[b][1][lane];
      const float xv[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int r = 0; r < LS_ROWS_PER_WAVE; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r][b] += af[r][e] * xv[e];
    }
  }

#pragma unroll
  for (int r = 0; r < LS_ROWS_PER_WAVE; ++r)
#pragma unroll
    for (int b = 0; b < ROWS; ++b) {
      const float s = wave_reduce_sum(acc[r][b]);
      if (lane == 0 && row0 + r < R)
        t_part[((size_t)blockIdx.y * ROWS + b) * R + row0 + r] = s;
    }
}

torch::Tensor lora_shrink(torch::Tensor x, torch::Tensor a_cat) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kFloat32 && x.dim() == 2 && x.is_contiguous(),
              "lora_shrink: x must be a contiguous f32 [rows, in] device tensor");
  TORCH_CHECK(a_cat.is_cuda() && a_cat.dtype() == torch::kBFloat16 && a_cat.dim() == 2 && a_cat.is_contiguous(),
              "lora_shrink: a_cat must be a contiguous bf16 [R, in] device tensor");
  TORCH_CHECK(x.device() == a_cat.device(), "lora_shrink: x and a_cat on different devices");
  const int rows = x.size(0), in_dim = x.size(1), R = a_cat.size(0);
  TORCH_CHECK(a_cat.size(1) == in_dim, "lora_shrink: x/in mismatch");
  TORCH_CHECK(in_dim > 0 && in_dim % 8 == 0, "lora_shrink: in must be a positive multiple of 8");
  TORCH_CHECK(R >= 1 && R <= LORA_MAX_R, "lora_shrink: R must be in 1..256");
  TORCH_CHECK(rows >= 1 && rows <= LORA_MAX_ROWS, "lora_shrink: rows must be in 1..8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0
              && reinterpret_cast<uintptr_t>(a_cat.data_ptr()) % 16 == 0,
              "lora_shrink: x and a_cat must be 16-byte aligned");
  int chunk, splits;
  lora_shrink_policy(in_dim, &chunk, &splits);
  auto t_part = torch::empty({(int64_t)splits, (int64_t)rows, (int64_t)R}, x.options());
  dim3 grid((R + LS_TILE - 1) / LS_TILE, splits);
  auto stream = at::cuda::getCurrentCUDAStream();
  const unsigned short* a_p = reinterpret_cast<const unsigned short*>(a_cat.data_ptr());
#define LAUNCH_SHRINK(B)                                                          \
  case B:                                                                         \
    lora_shrink_kernel<B><<<grid, 64 * LS_WAVES, 0, stream>>>(                    \
        x.data_ptr<float>(), a_p, t_part.data_ptr<float>(), in_dim, R, chunk);    \
    break;
  switch (rows) {
    LAUNCH_SHRINK(1) LAUNCH_SHRINK(2) LAUNCH_SHRINK(3) LAUNCH_SHRINK(4)
    LAUNCH_SHRINK(5) LAUNCH_SHRINK(6) LAUNCH_SHRINK(7) LAUNCH_SHRINK(8)
  }
#undef LAUNCH_SHRINK
  HIP_CHECK_LAST();
  return t_part;
}

// one present member of a group: columns [c0, c1) of the fused output, ranks
// [t_off, t_off + rank) of t, B^T at bt + bt_off as [rank, c1 - c0]
struct LoraSeg {
  int c0, c1, t_off, rank, bt_off;
  float scale;
};
struct LoraSegs {
  int n;
  LoraSeg s[LORA_MAX_SEGS];
};

// group g's share of column o's delta: rank rows g, g+16, ... of its member;
// *scale is the member's scale, 0 members leave both untouched
static __device__ __forceinline__ LORA_KERNEL float lora_delta_group(
    const LoraSegs& segs, const unsigned short* __restrict__ bt, const float* t_row,
    int o, int sg, float* scale, bool* owned) {
  float d = 0.f;
  for (int p = 0; p < segs.n; ++p) {
    const LoraSeg m = segs.s[p];
    if (o >= m.c0 && o < m.c1) {
      const int width = m.c1 - m.c0;
      const unsigned short* col = bt + (size_t)m.bt_off + (o - m.c0);
      for (int j = sg; j < m.rank; j += GEMV_REDUCE_GROUPS)
        d += bf16_to_f32(col[(size_t)j * width]) * t_row[m.t_off + j];
      *scale = m.scale;
      *owned = true;
    }
  }
  return d;
}

static __global__ __launch_bounds__(64 * GEMV_REDUCE_GROUPS) LORA_KERNEL void lora_reduce_kernel(
    const float* __restrict__ partials,  // [n_splits, batch, out]
    const float* __restrict__ t_part,    // [t_splits, batch, R]
    const unsigned short* __restrict__ bt,
    const LoraSegs segs,
    const unsigned short* __restrict__ residual,  // [batch, out] or null
    const unsigned short* __restrict__ bias,      // [out] bf16 or null
    void* __restrict__ y,
    int n_splits,
    int t_splits,
    int R,
    int batch,
    int out_dim,
    int epilogue) {
  constexpr int G = GEMV_REDUCE_GROUPS;
  __shared__ float acc_g[G][64];
  __shared__ float acc_u[G][64];
  __shared__ float dl_g[G][64];
  __shared__ float dl_u[G][64];
  __shared__ float t_s[LORA_MAX_ROWS * LORA_MAX_R];
  const int half = out_dim >> 1;
  const int n_out = (epilogue == EPI_SWIGLU_F32) ? half : out_dim;
  const int total = batch * n_out;
  const int ol = threadIdx.x & 63;
  const int sg = threadIdx.x >> 6;
  const int idx = blockIdx.x * 64 + ol;
  const bool live = idx < total;
  const int b = live ? idx / n_out : 0;
  const int o = live ? idx - b * n_out : 0;
  const size_t stride = (size_t)batch * out_dim;
  const size_t row = (size_t)b * out_dim;

  // t = sum over S of t_part, index order, for the batch rows of this block
  const int b_lo = (blockIdx.x * 64) / n_out;
  const int b_hi = min(blockIdx.x * 64 + 63, total - 1) / n_out;
  const int t_elems = (b_hi - b_lo + 1) * R;
  for (int i = threadIdx.x; i < t_elems; i += 64 * G) {
    const float* src = t_part + (size_t)b_lo * R + i;
    float s = 0.f;
    for (int k = 0; k < t_splits; ++k) s += src[(size_t)k * batch * R];
    t_s[i] = s;
  }
  __syncthreads();

  float g = 0.f, u = 0.f, dg = 0.f, du = 0.f;
  float scale_g = 0.f, scale_u = 0.f;
  bool own_g = false, own_u = false;
  if (live) {
    for (int s = sg; s < n_splits; s += G) g += partials[(size_t)s * stride + row + o];
    if (epilogue == EPI_SWIGLU_F32)
      for (int s = sg; s < n_splits; s += G) u += partials[(size_t)s * stride + row + o + half];
    const float* t_row = t_s + (b - b_lo) * R;
    dg = lora_delta_group(segs, bt, t_row, o, sg, &scale_g, &own_g);
    if (epilogue == EPI_SWIGLU_F32)
      du = lora_delta_group(segs, bt, t_row, o + half, sg, &scale_u, &own_u);
  }
  acc_g[sg][ol] = g;
  acc_u[sg][ol] = u;
  dl_g[sg][ol] = dg;
  dl_u[sg][ol] = du;
  __syncthreads();
  if (sg != 0 || !live) return;
  float sum = 0.f, usum = 0.f;
#pragma unroll
  for (int k = 0; k < G; ++k) {
    sum += acc_g[k][ol];
    usum += acc_u[k][ol];
  }
  float dsum = 0.f, dusum = 0.f;
#pragma unroll
  for (int k = 0; k < G; ++k) {
    dsum += dl_g[k][ol];
    dusum += dl_u[k][ol];
  }
  if (own_g) sum = sum + scale_g * dsum;
  if (own_u) usum = usum + scale_u * dusum;
  if (epilogue == EPI_SWIGLU_F32) {
    if (bias) {
      sum += bf16_to_f32(bias[o]);
      usum += bf16_to_f32(bias[o + half]);
    }
    const float act = sum / (1.f + __expf(-sum)) * usum;
    reinterpret_cast<float*>(y)[(size_t)b * half + o] = act;
  } else {
    if (bias) sum += bf16_to_f32(bias[o]);
    if (epilogue == EPI_PLAIN_F32) {
      reinterpret_cast<float*>(y)[row + o] = sum;
    } else {  // EPI_RESIDUAL_BF16
      const float r = bf16_to_f32(residual[row + o]);
      reinterpret_cast<unsigned short*>(y)[row + o] = f32_to_bf16(r + sum);
    }
  }
}

torch::Tensor lora_reduce(
    torch::Tensor partials,   // [n, rows, out] f32: a gemv's RAW partials
    torch::Tensor t_part,     // [S, rows, R] f32: lora_shrink's output
    torch::Tensor bt,         // bf16, the members' B^T one after the other
    std::vector<int64_t> segments,  // per member: c0, c1, t_off, rank, bt_off
    std::vector<double> scales,     // per member
    c10::optional<torch::Tensor> residual,
    c10::optional<torch::Tensor> bias,
    int64_t epilogue) {
  TORCH_CHECK(partials.is_cuda() && partials.dtype() == torch::kFloat32 && partials.dim() == 3
              && partials.is_contiguous(), "lora_reduce: partials must be contiguous f32 [n, rows, out]");
  TORCH_CHECK(t_part.is_cuda() && t_part.dtype() == torch::kFloat32 && t_part.dim() == 3
              && t_part.is_contiguous(), "lora_reduce: t_part must be contiguous f32 [S, rows, R]");
  TORCH_CHECK(bt.is_cuda() && bt.dtype() == torch::kBFloat16 && bt.is_contiguous(),
              "lora_reduce: bt must be a contiguous bf16 device tensor");
  TORCH_CHECK(partials.device() == t_part.device() && partials.device() == bt.device(),
              "lora_reduce: tensors on different devices");
  TORCH_CHECK(epilogue == EPI_PLAIN_F32 || epilogue == EPI_RESIDUAL_BF16 || epilogue == EPI_SWIGLU_F32,
              "lora_reduce: epilogue must be plain f32, residual bf16 or swiglu f32");
  const int n_splits = partials.size(0), batch = partials.size(1), out_dim = partials.size(2);
  const int t_splits = t_part.size(0), R = t_part.size(2);
  TORCH_CHECK(n_splits >= 1 && t_splits >= 1 && out_dim >= 1);
  TORCH_CHECK(batch >= 1 && batch <= LORA_MAX_ROWS, "lora_reduce: rows must be in 1..8");
  TORCH_CHECK(t_part.size(1) == batch, "lora_reduce: partials/t_part rows mismatch");
  TORCH_CHECK(R >= 1 && R <= LORA_MAX_R, "lora_reduce: R must be in 1..256");
  TORCH_CHECK(epilogue != EPI_SWIGLU_F32 || out_dim % 2 == 0, "lora_reduce: swiglu needs an even out");
  const int n_seg = (int)scales.size();
  TORCH_CHECK(n_seg >= 1 && n_seg <= LORA_MAX_SEGS && segments.size() == (size_t)n_seg * 5,
              "lora_reduce: 1..4 members of (c0, c1, t_off, rank, bt_off)");
  LoraSegs segs;
  segs.n = n_seg;
  int64_t prev_c1 = 0;
  for (int p = 0; p < n_seg; ++p) {
    const int64_t c0 = segments[5 * p], c1 = segments[5 * p + 1], t_off = segments[5 * p + 2];
    const int64_t rank = segments[5 * p + 3], bt_off = segments[5 * p + 4];
    TORCH_CHECK(prev_c1 <= c0 && c0 < c1 && c1 <= out_dim, "lora_reduce: member columns out of order or range");
    TORCH_CHECK(rank >= 1 && t_off >= 0 && t_off + rank <= R, "lora_reduce: member ranks outside t");
    TORCH_CHECK(bt_off >= 0 && bt_off + rank * (c1 - c0) <= bt.numel(), "lora_reduce: member B^T outside bt");
    segs.s[p] = LoraSeg{(int)c0, (int)c1, (int)t_off, (int)rank, (int)bt_off, (float)scales[p]};
    prev_c1 = c1;
  }
  for (int p = n_seg; p < LORA_MAX_SEGS; ++p) segs.s[p] = LoraSeg{0, 0, 0, 0, 0, 0.f};

  const int half = out_dim / 2;
  const int n_out = (epilogue == EPI_SWIGLU_F32) ? half : out_dim;
  auto f32_opts = partials.options();
  torch::Tensor y;
  const unsigned short* res_p = nullptr;
  if (epilogue == EPI_RESIDUAL_BF16) {
    TORCH_CHECK(residual.has_value(), "residual required for EPI_RESIDUAL_BF16");
    TORCH_CHECK(residual->is_cuda() && residual->is_contiguous() && residual->dtype() == torch::kBFloat16
                && residual->numel() == (int64_t)batch * out_dim, "lora_reduce: residual must be bf16 [rows, out]");
    res_p = reinterpret_cast<const unsigned short*>(residual->data_ptr());
    y = torch::empty({batch, out_dim}, residual->options());
  } else {
    y = torch::empty({batch, n_out}, f32_opts);
  }
  const unsigned short* bias_p = nullptr;
  if (bias.has_value() && bias->defined() && bias->numel() > 0) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() && bias->dtype() == torch::kBFloat16);
    TORCH_CHECK(bias->numel() == out_dim, "bias must be [out_dim] (pre-activation)");
    bias_p = reinterpret_cast<const unsigned short*>(bias->data_ptr());
  }
  const int total = batch * n_out;
  const int rblocks = (total + 63) / 64;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  lora_reduce_kernel<<<rblocks, 64 * GEMV_REDUCE_GROUPS, 0, stream>>>(
      partials.data_ptr<float>(), t_part.data_ptr<float>(),
      reinterpret_cast<const unsigned short*>(bt.data_ptr()), segs, res_p, bias_p, y.data_ptr(),
      n_splits, t_splits, R, batch, out_dim, (int)epilogue);
  HIP_CHECK_LAST();
  return y;
}
