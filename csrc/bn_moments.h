// Device helpers shared by the BatchNorm sweeps (bn_kernels.hip) and the 1x1
// convolution that produces BatchNorm partials (conv1x1_kernels.hip): the
// bf16 rounding every kernel applies and the running moments every statistics
// pass keeps.
#pragma once

#include <hip/hip_runtime.h>

namespace cgx {

// fp32 -> bf16 bits, round to nearest even; NaN stays a (quiet) NaN
__device__ inline unsigned bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// ---- running (count, mean, M2) over K channels that share one count --------

template <int K>
struct Moments {
  float n = 0.f;
  float mean[K] = {};
  float m2[K] = {};

  // Welford step; the count, hence 1/n, is shared by the K channels
  __device__ void push(const float (&x)[K]) {
    n += 1.f;
    const float inv = __builtin_amdgcn_rcpf(n);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const float d = x[j] - mean[j];
      mean[j] = fmaf(d, inv, mean[j]);
      m2[j] = fmaf(d, x[j] - mean[j], m2[j]);
    }
  }

  // Chan et al. merge of another run; either side may be empty
  __device__ void merge(float nb, const float (&mb)[K], const float (&m2b)[K]) {
    const float nt = n + nb;
    const float fb = nt > 0.f ? nb / nt : 0.f;
    const float w = n * fb;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const float d = mb[j] - mean[j];
      mean[j] = fmaf(d, fb, mean[j]);
      m2[j] = (m2[j] + m2b[j]) + (d * d) * w;
    }
    n = nt;
  }
};

}  // namespace cgx
