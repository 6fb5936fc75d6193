// The epilogue that the forward convolutions with 64-channel tiles share
// (conv3x3_kernels.hip, conv_stem_kernels.hip): rounding an accumulator tile to
// bf16 and storing it as whole 128-byte pixel rows.  Device code: only .hip
// files include this.
#pragma once

#include <hip/hip_runtime.h>

#include "wrw_image.h"

namespace cgx {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// as pack_bf16 of conv1x1_kernels.hip: what bf16_bits gives, a in the low half
__device__ inline unsigned fwd_pack_bf16(float a, float b) {
  const f32x2 f = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}

// A wave's 32 x 64 sub-tile, pk[j][e] the packed rows acc_row(2e, h) and
// acc_row(2e+1, h) of channel 32j + c, through the wave's `stage` to rows
// r0 .. r0+live-1 (live may be <= 0), channels n0 .. n0+63 of out[., 8*nvec],
// as 16-byte row vectors.
__device__ __forceinline__ void fwd_store_subtile(
    const unsigned (&pk)[2][8], uint4* stage, uint4* __restrict__ out, int r0,
    int live, int nvec, int n0, int lane) {
  unsigned* stage32 = reinterpret_cast<unsigned*>(stage);
  const int c = lane & 31, h = lane >> 5;
  // Lanes c and c^1 trade words so that the even lane writes channels
  // (c, c+1) of row 2e and the odd one channels (c-1, c) of row 2e+1;
  // odd rows swap their 64-byte halves.
  const int odd = c & 1;
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const unsigned own = pk[j][e];
      // quad_perm [1, 0, 3, 2]
      const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(
          0, (int)own, 0xB1, 0xf, 0xf, false);
      const unsigned word = odd ? (other >> 16) | (own & 0xffff0000u)
                                : (own & 0xffffu) | (other << 16);
      const int row = acc_row(2 * e, h) + odd;
      stage32[row * 32 + ((j * 16 + (c >> 1)) ^ ((row & 1) << 4))] = word;
    }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int idx = u * 64 + lane, row = idx >> 3, q = idx & 7;
    const uint4 v = stage[row * 8 + (q ^ ((row & 1) << 2))];
    if (row < live) out[(int64_t)(r0 + row) * nvec + n0 / 8 + q] = v;
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace cgx
