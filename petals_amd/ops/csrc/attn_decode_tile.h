// Pieces shared by the decode attention kernels (attention.hip: one token per
// sequence; attn_multi.hip: a few tokens per sequence): the 32-key wave tile,
// its register image and the swizzled V^T LDS layout.
#pragma once

#include "common.h"
#include <type_traits>

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

#define DKVT 32    // keys per wave-tile (MFMA path)
#define DWAVES 4   // waves per workgroup (MFMA path)
#define DKPAD 8

#define DVT_BYTE(dim, key_byte) \
  ((((unsigned)(dim)) * ((DKVT + DKPAD) * 2) + (unsigned)(key_byte)) ^ ((((unsigned)(dim) >> 3) & 7u) << 4))

// FP8: the caches hold OCP E4M3 bytes (torch.float8_e4m3fn, no scales)
// instead of bf16. Only the two global reads differ: the K B-fragment is 8
// bytes per lane and V rows arrive as 8-byte chunks, both converted (exactly)
// to the bf16x8 the bf16 instantiation loads. Everything downstream is shared.
//
// Loads: q (and the ALiBi slopes) arrive in one batch in the prologue, and a
// tile's V chunks and K fragments are loaded into registers in one batch
// before anything consumes them (DecodeTile), so a tile costs one memory
// round trip instead of one per load group. (Issuing the wave's next tile
// under the softmax and PV of the current one was measured and did not win,
// see docs/KERNELS.md.)
template <int HD, bool FP8>
struct DecodeTile {
  static constexpr int VN = DKVT * (HD / 8) / WAVE;  // V chunks of 8 elements per lane
  using raw_t = typename std::conditional<FP8, uint2, bf16x8>::type;
  raw_t v[VN];
  raw_t k[DKVT / 16][HD / 32];
  static __device__ __forceinline__ bf16x8 to_bf16(raw_t w) {
    if constexpr (FP8)
      return e4m3x8_to_bf16x8(w);
    else
      return w;
  }
};

// s_waitcnt lgkmcnt(0) alone (gfx9 encoding: vmcnt and expcnt at their
// maxima), so global loads in flight are not waited for
#define WAIT_LGKM0 0xC07F
