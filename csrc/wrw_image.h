// The LDS image and the transposed operand read that the weight-gradient
// kernels share (conv1x1_kernels.hip, conv3x3_kernels.hip,
// conv_stem_kernels.hip).  Device code: only
// .hip files include this.  The layout is argued at conv1x1_wrw.
#pragma once

#include <hip/hip_runtime.h>

namespace cgx {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Row of a 32x32 accumulator tile that register i of lane half h holds.
__device__ inline int acc_row(int i, int h) {
  return (i & 3) + 8 * (i >> 2) + 4 * h;
}

// Byte of cell u (32 channels, 64 bytes) of row r of a [rows][C channels]
// image.
template <int C>
__device__ inline int wrw_cell(int r, int u) {
  const int lin = r * (C / 32) + u;
  const int swz = C == 64 ? (r >> 1) & 1 : r & 3;
  return 256 * (lin >> 2) + 64 * ((lin & 3) ^ swz);
}

// The operand of one 16-row step from a lane's base address: rows +0 .. +3 in
// elements 0 .. 3, rows +4 .. +7 in elements 4 .. 7.
template <int C>
__device__ inline bf16x8 wrw_operand(char* img, int base, int s) {
  char* a = img + base + s * 16 * 2 * C;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4*)a);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4*)(a + 4 * 2 * C));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

}  // namespace cgx
