// Training-mode BatchNorm2d on a channels_last bf16 activation, fused with the
// ReLU and the residual add that follow it in a ResNet bottleneck.
//
// The activation is a dense [R, C] matrix (R = N*H*W); parameters and
// statistics are fp32.  Every thread handles one 16-byte vector (8 channels of
// one row) per iteration and keeps its channel group for the whole sweep
// (geometry: bn_plan.h), so per-channel values live in registers.
//
//   forward   bn_stats          per-thread Welford over its rows, Chan merge
//                               across the workgroup through LDS, one
//                               (mean, M2) partial per (split, channel)
//             bn_stats_finalize fixed-order Chan merge of the partials ->
//                               mean, invstd, running statistics
//             bn_apply          y = ((x-mean)*invstd)*gamma + beta -> bf16,
//                               [+ identity -> bf16], [ReLU + 1 mask bit]
//   backward  bn_bwd_reduce     per-channel sum(g), sum(g*xhat), g = dy under
//                               the mask
//             bn_bwd_finalize   fixed-order sum of the partials -> dbeta,
//                               dgamma
//             bn_bwd_dx         dx = gamma*invstd*(g - sum(g)/R
//                                                    - xhat*sum(g*xhat)/R),
//                               [masked dy for the identity branch]
//
// Two fusions run on the same sweeps.  The *_join kernels take a second
// BatchNorm (a bottleneck's downsample branch) as the identity operand:
// relu(bn3(x3) + bn_d(xd)) without writing bn_d's output or its gradient.
// The *_pool kernels fold the stem's 3x3/2/1 max-pool in: the forward writes
// the pooled tensor and one argmax byte per pooled element, the backward
// sweeps build g from those.
//
// No atomics anywhere: every reduction has a fixed order, so results are
// bitwise reproducible.  Compiled with -ffp-contract=off; the fused
// multiply-adds below are explicit.
#include <hip/hip_runtime.h>

#include "bn_moments.h"
#include "bn_plan.h"
#include "check.h"

namespace cgx {
namespace {

constexpr int kT = kBnThreads;

__device__ inline void unpack8(const uint4& v, float (&f)[8]) {
  f[0] = __uint_as_float(v.x << 16);
  f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16);
  f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16);
  f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16);
  f[7] = __uint_as_float(v.w & 0xffff0000u);
}

__device__ inline uint4 pack8(const unsigned (&b)[8]) {
  return make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16),
                    b[4] | (b[5] << 16), b[6] | (b[7] << 16));
}

__device__ inline unsigned half_of(const uint4& v, int j) {
  const unsigned w = j < 2 ? v.x : j < 4 ? v.y : j < 6 ? v.z : v.w;
  return (j & 1) ? w >> 16 : w & 0xffffu;
}

template <int K>
__device__ inline void load_k(float (&dst)[K], const float* src) {
#pragma unroll
  for (int j = 0; j < K; j++) dst[j] = src[j];
}

// Tree merge across the threads tid, tid+lo, tid+2*lo, ... of a workgroup (lo
// a power of two); threads below `lo` end up with the result.
template <int K>
__device__ inline void wg_merge(Moments<K>& m, float (*sh)[kT], int tid,
                                int lo) {
#pragma unroll
  for (int j = 0; j < K; j++) {
    sh[j][tid] = m.mean[j];
    sh[K + j][tid] = m.m2[j];
  }
  sh[2 * K][tid] = m.n;
  __syncthreads();
  for (int h = kT / 2; h >= lo; h >>= 1) {
    if (tid < h) {
      float mb[K], m2b[K];
#pragma unroll
      for (int j = 0; j < K; j++) {
        mb[j] = sh[j][tid + h];
        m2b[j] = sh[K + j][tid + h];
      }
      m.merge(sh[2 * K][tid + h], mb, m2b);
#pragma unroll
      for (int j = 0; j < K; j++) {
        sh[j][tid] = m.mean[j];
        sh[K + j][tid] = m.m2[j];
      }
      sh[2 * K][tid] = m.n;
    }
    __syncthreads();
  }
}

// Same for K plain sums.
template <int K>
__device__ inline void wg_sum(float (&s)[K], float (*sh)[kT], int tid, int lo) {
#pragma unroll
  for (int j = 0; j < K; j++) sh[j][tid] = s[j];
  __syncthreads();
  for (int h = kT / 2; h >= lo; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int j = 0; j < K; j++) {
        s[j] += sh[j][tid + h];
        sh[j][tid] = s[j];
      }
    }
    __syncthreads();
  }
}

// ---- forward ---------------------------------------------------------------

__global__ __launch_bounds__(kT) void bn_stats(const uint4* __restrict__ x,
                                               float* __restrict__ pmean,
                                               float* __restrict__ pm2,
                                               float* __restrict__ pcnt,
                                               BnPlan p) {
  __shared__ float sh[17][kT];
  const int tid = threadIdx.x;
  const BnSweep sw = bn_sweep(p, blockIdx.x, tid);
  Moments<8> m;
  float f[8];
  int64_t r = sw.row;
  // four independent loads in flight per thread
  for (; r + 3 * sw.stride < p.rows; r += 4 * sw.stride) {
    const uint4 v0 = x[bn_vec(p, r, sw.cg)];
    const uint4 v1 = x[bn_vec(p, r + sw.stride, sw.cg)];
    const uint4 v2 = x[bn_vec(p, r + 2 * sw.stride, sw.cg)];
    const uint4 v3 = x[bn_vec(p, r + 3 * sw.stride, sw.cg)];
    unpack8(v0, f);
    m.push(f);
    unpack8(v1, f);
    m.push(f);
    unpack8(v2, f);
    m.push(f);
    unpack8(v3, f);
    m.push(f);
  }
  for (; r < p.rows; r += sw.stride) {
    unpack8(x[bn_vec(p, r, sw.cg)], f);
    m.push(f);
  }
  wg_merge<8>(m, sh, tid, p.tc);
  if (tid < p.tc) {
    const int64_t o = bn_partial_offset(p, blockIdx.x, sw.cg);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      pmean[o + j] = m.mean[j];
      pm2[o + j] = m.m2[j];
    }
    if (tid == 0) pcnt[blockIdx.x] = m.n;
  }
}

// kBnFinChannels channels per workgroup, kFinLanes lanes per channel: lane l
// merges splits l, l+kFinLanes, ... in order (four loads in flight), then the
// lanes merge as a tree.
constexpr int kFinLanes = kT / kBnFinChannels;

__global__ __launch_bounds__(kT) void bn_stats_finalize(
    BnPartials q, float* __restrict__ mean, float* __restrict__ invstd,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    float momentum, float eps) {
  __shared__ float sh[3][kT];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * kBnFinChannels + tid % kBnFinChannels;
  const int lane = tid / kBnFinChannels;
  Moments<1> m;
  if (c < q.channels) {
    const int ct = (c / 8) / q.tc;
    for (int s0 = lane; s0 < q.splits; s0 += 4 * kFinLanes) {
      float nb[4], mb[4][1], m2b[4][1];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int s = s0 + u * kFinLanes;
        const bool live = s < q.splits;
        const int64_t o = (int64_t)s * q.pstride + c;
        nb[u] = live ? q.cnt[(int64_t)s * q.cstride + ct] : 0.f;
        mb[u][0] = live ? q.mean[o] : 0.f;
        m2b[u][0] = live ? q.m2[o] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) m.merge(nb[u], mb[u], m2b[u]);
    }
  }
  wg_merge<1>(m, sh, tid, kBnFinChannels);
  if (tid < kBnFinChannels && c < q.channels) {
    const float var = m.m2[0] / m.n;
    mean[c] = m.mean[0];
    invstd[c] = 1.f / sqrtf(var + eps);
    running_mean[c] =
        (1.f - momentum) * running_mean[c] + momentum * m.mean[0];
    running_var[c] =
        (1.f - momentum) * running_var[c] + momentum * (m.m2[0] / (m.n - 1.f));
  }
}

template <bool RELU, bool ADD>
__device__ inline void apply_one(const uint4& xv, const uint4& iv,
                                 const float (&mean)[8],
                                 const float (&invstd)[8],
                                 const float (&gamma)[8],
                                 const float (&beta)[8], uint4* out,
                                 uint8_t* mask, int64_t i) {
  float x[8], idn[8];
  unpack8(xv, x);
  if (ADD) unpack8(iv, idn);
  unsigned o[8], mbits = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float y = ((x[j] - mean[j]) * invstd[j]) * gamma[j] + beta[j];
    unsigned b = bf16_bits(y);
    if (ADD) {
      // the unfused graph rounds the BN output to bf16 before the add
      y = __uint_as_float(b << 16) + idn[j];
      b = bf16_bits(y);
    }
    if (RELU) {
      // like clamp_min: a NaN stays; like threshold_backward: its gradient
      // passes (the bit is clear only where the output is <= 0)
      const float z = __uint_as_float(b << 16);
      if (z <= 0.f) b = 0;
      else mbits |= 1u << j;
    }
    o[j] = b;
  }
  out[i] = pack8(o);
  if (RELU) mask[i] = (uint8_t)mbits;
}

template <bool RELU, bool ADD>
__global__ __launch_bounds__(kT) void bn_apply(
    const uint4* __restrict__ x, const uint4* __restrict__ identity,
    const float* __restrict__ mean_, const float* __restrict__ invstd_,
    const float* __restrict__ weight, const float* __restrict__ bias,
    uint4* __restrict__ out, uint8_t* __restrict__ mask, BnPlan p) {
  const BnSweep sw = bn_sweep(p, blockIdx.x, threadIdx.x);
  float mean[8], invstd[8], gamma[8], beta[8];
  load_k(mean, mean_ + sw.cg * 8);
  load_k(invstd, invstd_ + sw.cg * 8);
  load_k(gamma, weight + sw.cg * 8);
  load_k(beta, bias + sw.cg * 8);
  const uint4 none = make_uint4(0, 0, 0, 0);
  int64_t r = sw.row;
  for (; r + sw.stride < p.rows; r += 2 * sw.stride) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    const int64_t i1 = bn_vec(p, r + sw.stride, sw.cg);
    const uint4 x0 = x[i0], x1 = x[i1];
    const uint4 d0 = ADD ? identity[i0] : none, d1 = ADD ? identity[i1] : none;
    apply_one<RELU, ADD>(x0, d0, mean, invstd, gamma, beta, out, mask, i0);
    apply_one<RELU, ADD>(x1, d1, mean, invstd, gamma, beta, out, mask, i1);
  }
  if (r < p.rows) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    apply_one<RELU, ADD>(x[i0], ADD ? identity[i0] : none, mean, invstd, gamma,
                         beta, out, mask, i0);
  }
}

// ---- backward --------------------------------------------------------------

// g = dy where the mask bit is set, +0 elsewhere; returned as bf16 bits too.
template <bool RELU>
__device__ inline void masked_dy(const uint4& dyv, unsigned mbits,
                                 float (&g)[8], unsigned (&gb)[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    gb[j] = half_of(dyv, j);
    if (RELU && !((mbits >> j) & 1u)) gb[j] = 0;
    g[j] = __uint_as_float(gb[j] << 16);
  }
}

template <bool RELU>
__global__ __launch_bounds__(kT) void bn_bwd_reduce(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    const uint8_t* __restrict__ mask, const float* __restrict__ mean_,
    const float* __restrict__ invstd_, float* __restrict__ psg,
    float* __restrict__ psgx, BnPlan p) {
  __shared__ float sh[16][kT];
  const int tid = threadIdx.x;
  const BnSweep sw = bn_sweep(p, blockIdx.x, tid);
  float mean[8], invstd[8];
  load_k(mean, mean_ + sw.cg * 8);
  load_k(invstd, invstd_ + sw.cg * 8);
  float s[16] = {};  // sum(g) in 0..7, sum(g*xhat) in 8..15
  auto accumulate = [&](const uint4& dyv, const uint4& xv, unsigned mbits) {
    float g[8], xf[8];
    unsigned gb[8];
    masked_dy<RELU>(dyv, mbits, g, gb);
    unpack8(xv, xf);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xhat = (xf[j] - mean[j]) * invstd[j];
      s[j] += g[j];
      s[8 + j] = fmaf(g[j], xhat, s[8 + j]);
    }
  };
  int64_t r = sw.row;
  for (; r + sw.stride < p.rows; r += 2 * sw.stride) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    const int64_t i1 = bn_vec(p, r + sw.stride, sw.cg);
    const uint4 a0 = dy[i0], a1 = dy[i1];
    const uint4 b0 = x[i0], b1 = x[i1];
    const unsigned m0 = RELU ? mask[i0] : 0xffu, m1 = RELU ? mask[i1] : 0xffu;
    accumulate(a0, b0, m0);
    accumulate(a1, b1, m1);
  }
  if (r < p.rows) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    accumulate(dy[i0], x[i0], RELU ? mask[i0] : 0xffu);
  }
  wg_sum<16>(s, sh, tid, p.tc);
  if (tid < p.tc) {
    const int64_t o = bn_partial_offset(p, blockIdx.x, sw.cg);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      psg[o + j] = s[j];
      psgx[o + j] = s[8 + j];
    }
  }
}

__global__ __launch_bounds__(kT) void bn_bwd_finalize(
    const float* __restrict__ psg, const float* __restrict__ psgx,
    float* __restrict__ dbeta, float* __restrict__ dgamma, BnPlan p) {
  __shared__ float sh[2][kT];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * kBnFinChannels + tid % kBnFinChannels;
  const int lane = tid / kBnFinChannels;
  float s[2] = {0.f, 0.f};
  if (c < p.channels) {
    for (int s0 = lane; s0 < p.splits; s0 += 4 * kFinLanes) {
      float a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int sp = s0 + u * kFinLanes;
        const bool live = sp < p.splits;
        const int64_t o = (int64_t)sp * p.channels + c;
        a[u] = live ? psg[o] : 0.f;
        b[u] = live ? psgx[o] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        s[0] += a[u];
        s[1] += b[u];
      }
    }
  }
  wg_sum<2>(s, sh, tid, kBnFinChannels);
  if (tid < kBnFinChannels && c < p.channels) {
    dbeta[c] = s[0];
    dgamma[c] = s[1];
  }
}

template <bool RELU, bool ADD>
__global__ __launch_bounds__(kT) void bn_bwd_dx(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    const uint8_t* __restrict__ mask, const float* __restrict__ mean_,
    const float* __restrict__ invstd_, const float* __restrict__ weight,
    const float* __restrict__ dbeta, const float* __restrict__ dgamma,
    uint4* __restrict__ dx, uint4* __restrict__ didentity, BnPlan p) {
  const BnSweep sw = bn_sweep(p, blockIdx.x, threadIdx.x);
  float mean[8], invstd[8], scale[8], mg[8], mgx[8];
  load_k(mean, mean_ + sw.cg * 8);
  load_k(invstd, invstd_ + sw.cg * 8);
  load_k(scale, weight + sw.cg * 8);
  load_k(mg, dbeta + sw.cg * 8);
  load_k(mgx, dgamma + sw.cg * 8);
  const float inv_r = 1.f / (float)p.rows;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    scale[j] *= invstd[j];
    mg[j] *= inv_r;
    mgx[j] *= inv_r;
  }
  auto one = [&](const uint4& dyv, const uint4& xv, unsigned mbits, int64_t i) {
    float g[8], xf[8];
    unsigned gb[8], o[8];
    masked_dy<RELU>(dyv, mbits, g, gb);
    unpack8(xv, xf);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xhat = (xf[j] - mean[j]) * invstd[j];
      o[j] = bf16_bits(scale[j] * ((g[j] - mg[j]) - xhat * mgx[j]));
    }
    dx[i] = pack8(o);
    if (ADD) didentity[i] = pack8(gb);
  };
  int64_t r = sw.row;
  for (; r + sw.stride < p.rows; r += 2 * sw.stride) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    const int64_t i1 = bn_vec(p, r + sw.stride, sw.cg);
    const uint4 a0 = dy[i0], a1 = dy[i1];
    const uint4 b0 = x[i0], b1 = x[i1];
    const unsigned m0 = RELU ? mask[i0] : 0xffu, m1 = RELU ? mask[i1] : 0xffu;
    one(a0, b0, m0, i0);
    one(a1, b1, m1, i1);
  }
  if (r < p.rows) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    one(dy[i0], x[i0], RELU ? mask[i0] : 0xffu, i0);
  }
}

// ---- residual join: relu(bf16(bn3(x3)) + bf16(bn_d(xd))) -------------------
//
// The roundings and the order of every sum are those of bn_apply<false,false>
// on xd followed by bn_apply<relu,add>, and of bn_bwd_*<relu,add> followed by
// bn_bwd_*<false,false> on the masked dy: the results are the same bits, and
// neither the identity nor its gradient goes through memory.

struct Affine {
  float mean[8], invstd[8], gamma[8], beta[8];
  __device__ void load(const float* mean_, const float* invstd_,
                       const float* weight, const float* bias, int cg) {
    load_k(mean, mean_ + cg * 8);
    load_k(invstd, invstd_ + cg * 8);
    load_k(gamma, weight + cg * 8);
    load_k(beta, bias + cg * 8);
  }
};

template <bool RELU>
__global__ __launch_bounds__(kT) void bn_apply_join(
    const uint4* __restrict__ x3, const uint4* __restrict__ xd,
    const float* __restrict__ mean3, const float* __restrict__ invstd3,
    const float* __restrict__ weight3, const float* __restrict__ bias3,
    const float* __restrict__ meand, const float* __restrict__ invstdd,
    const float* __restrict__ weightd, const float* __restrict__ biasd,
    uint4* __restrict__ out, uint8_t* __restrict__ mask, BnPlan p) {
  const BnSweep sw = bn_sweep(p, blockIdx.x, threadIdx.x);
  Affine a, b;
  a.load(mean3, invstd3, weight3, bias3, sw.cg);
  b.load(meand, invstdd, weightd, biasd, sw.cg);
  auto one = [&](const uint4& xv, const uint4& dv, int64_t i) {
    float d[8];
    unsigned idb[8];
    unpack8(dv, d);
#pragma unroll
    for (int j = 0; j < 8; j++)
      idb[j] = bf16_bits(((d[j] - b.mean[j]) * b.invstd[j]) * b.gamma[j] +
                         b.beta[j]);
    apply_one<RELU, true>(xv, pack8(idb), a.mean, a.invstd, a.gamma, a.beta,
                          out, mask, i);
  };
  int64_t r = sw.row;
  for (; r + sw.stride < p.rows; r += 2 * sw.stride) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    const int64_t i1 = bn_vec(p, r + sw.stride, sw.cg);
    const uint4 a0 = x3[i0], a1 = x3[i1];
    const uint4 d0 = xd[i0], d1 = xd[i1];
    one(a0, d0, i0);
    one(a1, d1, i1);
  }
  if (r < p.rows) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    one(x3[i0], xd[i0], i0);
  }
}

template <bool RELU>
__global__ __launch_bounds__(kT) void bn_bwd_reduce_join(
    const uint4* __restrict__ dy, const uint4* __restrict__ x3,
    const uint4* __restrict__ xd, const uint8_t* __restrict__ mask,
    const float* __restrict__ mean3_, const float* __restrict__ invstd3_,
    const float* __restrict__ meand_, const float* __restrict__ invstdd_,
    float* __restrict__ psg, float* __restrict__ psgx3,
    float* __restrict__ psgxd, BnPlan p) {
  __shared__ float sh[24][kT];
  const int tid = threadIdx.x;
  const BnSweep sw = bn_sweep(p, blockIdx.x, tid);
  float mean3[8], invstd3[8], meand[8], invstdd[8];
  load_k(mean3, mean3_ + sw.cg * 8);
  load_k(invstd3, invstd3_ + sw.cg * 8);
  load_k(meand, meand_ + sw.cg * 8);
  load_k(invstdd, invstdd_ + sw.cg * 8);
  // sum(g) in 0..7, sum(g*xhat3) in 8..15, sum(g*xhatd) in 16..23
  float s[24] = {};
  auto accumulate = [&](const uint4& dyv, const uint4& av, const uint4& bv,
                        unsigned mbits) {
    float g[8], af[8], bf[8];
    unsigned gb[8];
    masked_dy<RELU>(dyv, mbits, g, gb);
    unpack8(av, af);
    unpack8(bv, bf);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xhat3 = (af[j] - mean3[j]) * invstd3[j];
      const float xhatd = (bf[j] - meand[j]) * invstdd[j];
      s[j] += g[j];
      s[8 + j] = fmaf(g[j], xhat3, s[8 + j]);
      s[16 + j] = fmaf(g[j], xhatd, s[16 + j]);
    }
  };
  int64_t r = sw.row;
  for (; r + sw.stride < p.rows; r += 2 * sw.stride) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    const int64_t i1 = bn_vec(p, r + sw.stride, sw.cg);
    const uint4 a0 = dy[i0], a1 = dy[i1];
    const uint4 b0 = x3[i0], b1 = x3[i1];
    const uint4 c0 = xd[i0], c1 = xd[i1];
    const unsigned m0 = RELU ? mask[i0] : 0xffu, m1 = RELU ? mask[i1] : 0xffu;
    accumulate(a0, b0, c0, m0);
    accumulate(a1, b1, c1, m1);
  }
  if (r < p.rows) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    accumulate(dy[i0], x3[i0], xd[i0], RELU ? mask[i0] : 0xffu);
  }
  wg_sum<24>(s, sh, tid, p.tc);
  if (tid < p.tc) {
    const int64_t o = bn_partial_offset(p, blockIdx.x, sw.cg);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      psg[o + j] = s[j];
      psgx3[o + j] = s[8 + j];
      psgxd[o + j] = s[16 + j];
    }
  }
}

// dbeta3 and dbetad are the same sum(g); the kernel reads dbeta3.
template <bool RELU>
__global__ __launch_bounds__(kT) void bn_bwd_dx_join(
    const uint4* __restrict__ dy, const uint4* __restrict__ x3,
    const uint4* __restrict__ xd, const uint8_t* __restrict__ mask,
    const float* __restrict__ mean3_, const float* __restrict__ invstd3_,
    const float* __restrict__ weight3, const float* __restrict__ dgamma3,
    const float* __restrict__ meand_, const float* __restrict__ invstdd_,
    const float* __restrict__ weightd, const float* __restrict__ dgammad,
    const float* __restrict__ dbeta, uint4* __restrict__ dx3,
    uint4* __restrict__ dxd, BnPlan p) {
  const BnSweep sw = bn_sweep(p, blockIdx.x, threadIdx.x);
  float mean3[8], invstd3[8], scale3[8], mgx3[8];
  float meand[8], invstdd[8], scaled[8], mgxd[8], mg[8];
  load_k(mean3, mean3_ + sw.cg * 8);
  load_k(invstd3, invstd3_ + sw.cg * 8);
  load_k(scale3, weight3 + sw.cg * 8);
  load_k(mgx3, dgamma3 + sw.cg * 8);
  load_k(meand, meand_ + sw.cg * 8);
  load_k(invstdd, invstdd_ + sw.cg * 8);
  load_k(scaled, weightd + sw.cg * 8);
  load_k(mgxd, dgammad + sw.cg * 8);
  load_k(mg, dbeta + sw.cg * 8);
  const float inv_r = 1.f / (float)p.rows;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    scale3[j] *= invstd3[j];
    scaled[j] *= invstdd[j];
    mg[j] *= inv_r;
    mgx3[j] *= inv_r;
    mgxd[j] *= inv_r;
  }
  auto one = [&](const uint4& dyv, const uint4& av, const uint4& bv,
                 unsigned mbits, int64_t i) {
    float g[8], af[8], bf[8];
    unsigned gb[8], o3[8], od[8];
    masked_dy<RELU>(dyv, mbits, g, gb);
    unpack8(av, af);
    unpack8(bv, bf);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xhat3 = (af[j] - mean3[j]) * invstd3[j];
      const float xhatd = (bf[j] - meand[j]) * invstdd[j];
      o3[j] = bf16_bits(scale3[j] * ((g[j] - mg[j]) - xhat3 * mgx3[j]));
      od[j] = bf16_bits(scaled[j] * ((g[j] - mg[j]) - xhatd * mgxd[j]));
    }
    dx3[i] = pack8(o3);
    dxd[i] = pack8(od);
  };
  int64_t r = sw.row;
  for (; r + sw.stride < p.rows; r += 2 * sw.stride) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    const int64_t i1 = bn_vec(p, r + sw.stride, sw.cg);
    const uint4 a0 = dy[i0], a1 = dy[i1];
    const uint4 b0 = x3[i0], b1 = x3[i1];
    const uint4 c0 = xd[i0], c1 = xd[i1];
    const unsigned m0 = RELU ? mask[i0] : 0xffu, m1 = RELU ? mask[i1] : 0xffu;
    one(a0, b0, c0, m0, i0);
    one(a1, b1, c1, m1, i1);
  }
  if (r < p.rows) {
    const int64_t i0 = bn_vec(p, r, sw.cg);
    one(dy[i0], x3[i0], xd[i0], RELU ? mask[i0] : 0xffu, i0);
  }
}

// ---- stem: BatchNorm + ReLU + 3x3/2/1 max-pool (geometry: bn_plan.h) -------

// One thread per (pooled pixel, channel group): relu(bf16(bn(x))) of the up to
// nine pixels of the window, as bn_apply<relu> computes it, and their maximum
// with max_pool2d's rule (the first of equal values in (row, column) order
// wins, a NaN always does).  arg holds the winning window position, kPoolNone
// where the maximum is <= 0: the ReLU passes no gradient there.
__global__ __launch_bounds__(kT) void bn_apply_pool(
    const uint4* __restrict__ x, const float* __restrict__ mean_,
    const float* __restrict__ invstd_, const float* __restrict__ weight,
    const float* __restrict__ bias, uint4* __restrict__ out,
    uint2* __restrict__ arg, BnPoolPlan g) {
  const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (t >= g.threads) return;
  const int cg = (int)(t % g.cgs);
  int pix = (int)(t / g.cgs);
  const int ow = pix % g.ow;
  pix /= g.ow;
  const int oh = pix % g.oh, n = pix / g.oh;
  float mean[8], invstd[8], gamma[8], beta[8];
  load_k(mean, mean_ + cg * 8);
  load_k(invstd, invstd_ + cg * 8);
  load_k(gamma, weight + cg * 8);
  load_k(beta, bias + cg * 8);
  uint4 v[9];
  bool live[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int ih = pool_in(oh, k / 3), iw = pool_in(ow, k % 3);
    live[k] = ih >= 0 && ih < g.h && iw >= 0 && iw < g.w;
    v[k] = live[k] ? x[(((int64_t)n * g.h + ih) * g.w + iw) * g.cgs + cg]
                   : make_uint4(0, 0, 0, 0);
  }
  float best[8];
  unsigned bits[8], pos[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    best[j] = -INFINITY;
    bits[j] = 0;
    pos[j] = kPoolNone;
  }
#pragma unroll
  for (int k = 0; k < 9; k++) {
    if (!live[k]) continue;
    float f[8];
    unpack8(v[k], f);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float y = ((f[j] - mean[j]) * invstd[j]) * gamma[j] + beta[j];
      unsigned b = bf16_bits(y);
      float z = __uint_as_float(b << 16);
      if (z <= 0.f) {
        b = 0;
        z = 0.f;
      }
      if (z > best[j] || z != z) {
        best[j] = z;
        bits[j] = b;
        pos[j] = k;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; j++)
    if (best[j] <= 0.f) pos[j] = kPoolNone;
  out[t] = pack8(bits);
  arg[t] = make_uint2(pos[0] | (pos[1] << 8) | (pos[2] << 16) | (pos[3] << 24),
                      pos[4] | (pos[5] << 8) | (pos[6] << 16) | (pos[7] << 24));
}

// g of input row r: the pooled dy of the windows that cover the pixel and name
// it as their maximum, added in fp32 in ascending (oh, ow) order and rounded
// to bf16, which is what max_pool2d's backward followed by the ReLU mask gives.
__device__ inline void pooled_g(const uint4* __restrict__ dy,
                                const uint2* __restrict__ arg,
                                const BnPoolPlan& pl, int64_t row, int cg,
                                float (&g)[8]) {
  int pix = (int)row;
  const int iw = pix % pl.w;
  pix /= pl.w;
  const int ih = pix % pl.h, n = pix / pl.h;
  const int oh0 = pool_cover_lo(ih), oh1 = pool_cover_hi(ih, pl.oh);
  const int ow0 = pool_cover_lo(iw), ow1 = pool_cover_hi(iw, pl.ow);
  float acc[8] = {};
  for (int oh = oh0; oh <= oh1; oh++)
    for (int ow = ow0; ow <= ow1; ow++) {
      const int64_t i = (((int64_t)n * pl.oh + oh) * pl.ow + ow) * pl.cgs + cg;
      const unsigned k = pool_k(ih, oh) * 3 + pool_k(iw, ow);
      const uint4 dv = dy[i];
      const uint2 av = arg[i];
      float d[8];
      unpack8(dv, d);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const unsigned a = ((j < 4 ? av.x : av.y) >> (8 * (j & 3))) & 0xffu;
        if (a == k) acc[j] += d[j];
      }
    }
#pragma unroll
  for (int j = 0; j < 8; j++) g[j] = __uint_as_float(bf16_bits(acc[j]) << 16);
}

__global__ __launch_bounds__(kT) void bn_pool_bwd_reduce(
    const uint4* __restrict__ dy, const uint2* __restrict__ arg,
    const uint4* __restrict__ x, const float* __restrict__ mean_,
    const float* __restrict__ invstd_, float* __restrict__ psg,
    float* __restrict__ psgx, BnPlan p, BnPoolPlan pl) {
  __shared__ float sh[16][kT];
  const int tid = threadIdx.x;
  const BnSweep sw = bn_sweep(p, blockIdx.x, tid);
  float mean[8], invstd[8];
  load_k(mean, mean_ + sw.cg * 8);
  load_k(invstd, invstd_ + sw.cg * 8);
  float s[16] = {};  // sum(g) in 0..7, sum(g*xhat) in 8..15
#pragma unroll 2
  for (int64_t r = sw.row; r < p.rows; r += sw.stride) {
    const uint4 xv = x[bn_vec(p, r, sw.cg)];
    float g[8], xf[8];
    pooled_g(dy, arg, pl, r, sw.cg, g);
    unpack8(xv, xf);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xhat = (xf[j] - mean[j]) * invstd[j];
      s[j] += g[j];
      s[8 + j] = fmaf(g[j], xhat, s[8 + j]);
    }
  }
  wg_sum<16>(s, sh, tid, p.tc);
  if (tid < p.tc) {
    const int64_t o = bn_partial_offset(p, blockIdx.x, sw.cg);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      psg[o + j] = s[j];
      psgx[o + j] = s[8 + j];
    }
  }
}

__global__ __launch_bounds__(kT) void bn_pool_bwd_dx(
    const uint4* __restrict__ dy, const uint2* __restrict__ arg,
    const uint4* __restrict__ x, const float* __restrict__ mean_,
    const float* __restrict__ invstd_, const float* __restrict__ weight,
    const float* __restrict__ dbeta, const float* __restrict__ dgamma,
    uint4* __restrict__ dx, BnPlan p, BnPoolPlan pl) {
  const BnSweep sw = bn_sweep(p, blockIdx.x, threadIdx.x);
  float mean[8], invstd[8], scale[8], mg[8], mgx[8];
  load_k(mean, mean_ + sw.cg * 8);
  load_k(invstd, invstd_ + sw.cg * 8);
  load_k(scale, weight + sw.cg * 8);
  load_k(mg, dbeta + sw.cg * 8);
  load_k(mgx, dgamma + sw.cg * 8);
  const float inv_r = 1.f / (float)p.rows;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    scale[j] *= invstd[j];
    mg[j] *= inv_r;
    mgx[j] *= inv_r;
  }
#pragma unroll 2
  for (int64_t r = sw.row; r < p.rows; r += sw.stride) {
    const int64_t i = bn_vec(p, r, sw.cg);
    const uint4 xv = x[i];
    float g[8], xf[8];
    unsigned o[8];
    pooled_g(dy, arg, pl, r, sw.cg, g);
    unpack8(xv, xf);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xhat = (xf[j] - mean[j]) * invstd[j];
      o[j] = bf16_bits(scale[j] * ((g[j] - mg[j]) - xhat * mgx[j]));
    }
    dx[i] = pack8(o);
  }
}

int fin_grid(const BnPlan& p) {
  return (p.channels + kBnFinChannels - 1) / kBnFinChannels;
}

// bn_stats + bn_stats_finalize of one activation; `part` as in BnForwardArgs.
// With `stats` the partials are someone else's and only the finalize runs.
void launch_bn_stats(const BnPlan& p, const void* x_, float* part,
                     const BnPartials* stats, float* mean, float* invstd,
                     float* running_mean, float* running_var, float momentum,
                     float eps, hipStream_t stream) {
  BnPartials q;
  if (stats) {
    q = *stats;
  } else {
    float* pmean = part;
    float* pm2 = part + p.partial_floats;
    float* pcnt = part + 2 * p.partial_floats;
    hipLaunchKernelGGL(bn_stats, dim3(p.grid), dim3(kT), 0, stream,
                       static_cast<const uint4*>(x_), pmean, pm2, pcnt, p);
    q.mean = pmean;
    q.m2 = pm2;
    q.cnt = pcnt;
    q.channels = p.channels;
    q.splits = p.splits;
    q.tc = p.tc;
    q.pstride = p.channels;
    q.cstride = p.ctiles;
  }
  hipLaunchKernelGGL(bn_stats_finalize, dim3(fin_grid(p)), dim3(kT), 0, stream,
                     q, mean, invstd, running_mean, running_var, momentum, eps);
}

}  // namespace

void launch_bn_forward(const BnPlan& p, const BnForwardArgs& a,
                       hipStream_t stream) {
  const uint4* x = static_cast<const uint4*>(a.x);
  const uint4* idn = static_cast<const uint4*>(a.identity);
  uint4* out = static_cast<uint4*>(a.out);
  const dim3 grid(p.grid), block(kT);
  launch_bn_stats(p, a.x, a.part, a.stats, a.mean, a.invstd, a.running_mean,
                  a.running_var, a.momentum, a.eps, stream);
#define CGX_BN_APPLY(RELU, ADD)                                              \
  hipLaunchKernelGGL((bn_apply<RELU, ADD>), grid, block, 0, stream, x, idn,  \
                     a.mean, a.invstd, a.weight, a.bias, out, a.mask, p)
  if (a.relu && idn) CGX_BN_APPLY(true, true);
  else if (a.relu) CGX_BN_APPLY(true, false);
  else if (idn) CGX_BN_APPLY(false, true);
  else CGX_BN_APPLY(false, false);
#undef CGX_BN_APPLY
  CGX_HIP_CHECK(hipGetLastError());
}

void launch_bn_backward(const BnPlan& p, const BnBackwardArgs& a,
                        hipStream_t stream) {
  float* psg = a.part;
  float* psgx = a.part + p.partial_floats;
  const uint4* dy = static_cast<const uint4*>(a.dy);
  const uint4* x = static_cast<const uint4*>(a.x);
  uint4* dx = static_cast<uint4*>(a.dx);
  uint4* did = static_cast<uint4*>(a.didentity);
  const dim3 grid(p.grid), block(kT);
  if (a.mask)
    hipLaunchKernelGGL(bn_bwd_reduce<true>, grid, block, 0, stream, dy, x,
                       a.mask, a.mean, a.invstd, psg, psgx, p);
  else
    hipLaunchKernelGGL(bn_bwd_reduce<false>, grid, block, 0, stream, dy, x,
                       a.mask, a.mean, a.invstd, psg, psgx, p);
  hipLaunchKernelGGL(bn_bwd_finalize, dim3(fin_grid(p)), block, 0, stream, psg,
                     psgx, a.dbeta, a.dgamma, p);
#define CGX_BN_DX(RELU, ADD)                                                 \
  hipLaunchKernelGGL((bn_bwd_dx<RELU, ADD>), grid, block, 0, stream, dy, x,  \
                     a.mask, a.mean, a.invstd, a.weight, a.dbeta, a.dgamma,  \
                     dx, did, p)
  if (a.mask && did) CGX_BN_DX(true, true);
  else if (a.mask) CGX_BN_DX(true, false);
  else CGX_BN_DX(false, false);
#undef CGX_BN_DX
  CGX_HIP_CHECK(hipGetLastError());
}

void launch_bn_join_forward(const BnPlan& p, const BnJoinArgs& j,
                            hipStream_t stream) {
  const BnOperand &a = j.a, &b = j.b;
  float* part_b = j.part + 2 * p.partial_floats + p.grid;
  launch_bn_stats(p, a.x, j.part, a.stats, a.mean, a.invstd, a.running_mean,
                  a.running_var, a.momentum, a.eps, stream);
  launch_bn_stats(p, b.x, part_b, b.stats, b.mean, b.invstd, b.running_mean,
                  b.running_var, b.momentum, b.eps, stream);
  const uint4* x3 = static_cast<const uint4*>(a.x);
  const uint4* xd = static_cast<const uint4*>(b.x);
  uint4* out = static_cast<uint4*>(j.out);
  const dim3 grid(p.grid), block(kT);
  if (j.relu)
    hipLaunchKernelGGL(bn_apply_join<true>, grid, block, 0, stream, x3, xd,
                       a.mean, a.invstd, a.weight, a.bias, b.mean, b.invstd,
                       b.weight, b.bias, out, j.mask, p);
  else
    hipLaunchKernelGGL(bn_apply_join<false>, grid, block, 0, stream, x3, xd,
                       a.mean, a.invstd, a.weight, a.bias, b.mean, b.invstd,
                       b.weight, b.bias, out, j.mask, p);
  CGX_HIP_CHECK(hipGetLastError());
}

void launch_bn_join_backward(const BnPlan& p, const BnJoinArgs& j,
                             hipStream_t stream) {
  const BnOperand &a = j.a, &b = j.b;
  float* psg = j.part;
  float* psgx3 = j.part + p.partial_floats;
  float* psgxd = j.part + 2 * p.partial_floats;
  const uint4* dy = static_cast<const uint4*>(j.dy);
  const uint4* x3 = static_cast<const uint4*>(a.x);
  const uint4* xd = static_cast<const uint4*>(b.x);
  uint4* dx3 = static_cast<uint4*>(a.dx);
  uint4* dxd = static_cast<uint4*>(b.dx);
  const dim3 grid(p.grid), block(kT), fin(fin_grid(p));
  if (j.mask)
    hipLaunchKernelGGL(bn_bwd_reduce_join<true>, grid, block, 0, stream, dy, x3,
                       xd, j.mask, a.mean, a.invstd, b.mean, b.invstd, psg,
                       psgx3, psgxd, p);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_join<false>, grid, block, 0, stream, dy,
                       x3, xd, j.mask, a.mean, a.invstd, b.mean, b.invstd, psg,
                       psgx3, psgxd, p);
  hipLaunchKernelGGL(bn_bwd_finalize, fin, block, 0, stream, psg, psgx3,
                     a.dbeta, a.dgamma, p);
  hipLaunchKernelGGL(bn_bwd_finalize, fin, block, 0, stream, psg, psgxd,
                     b.dbeta, b.dgamma, p);
  if (j.mask)
    hipLaunchKernelGGL(bn_bwd_dx_join<true>, grid, block, 0, stream, dy, x3, xd,
                       j.mask, a.mean, a.invstd, a.weight, a.dgamma, b.mean,
                       b.invstd, b.weight, b.dgamma, a.dbeta, dx3, dxd, p);
  else
    hipLaunchKernelGGL(bn_bwd_dx_join<false>, grid, block, 0, stream, dy, x3,
                       xd, j.mask, a.mean, a.invstd, a.weight, a.dgamma, b.mean,
                       b.invstd, b.weight, b.dgamma, a.dbeta, dx3, dxd, p);
  CGX_HIP_CHECK(hipGetLastError());
}

void launch_bn_pool_forward(const BnPlan& p, const BnPoolPlan& g,
                            const BnPoolArgs& a, hipStream_t stream) {
  launch_bn_stats(p, a.x, a.part, nullptr, a.mean, a.invstd, a.running_mean,
                  a.running_var, a.momentum, a.eps, stream);
  hipLaunchKernelGGL(bn_apply_pool, dim3(g.grid), dim3(kT), 0, stream,
                     static_cast<const uint4*>(a.x), a.mean, a.invstd, a.weight,
                     a.bias, static_cast<uint4*>(a.out),
                     reinterpret_cast<uint2*>(a.arg), g);
  CGX_HIP_CHECK(hipGetLastError());
}

void launch_bn_pool_backward(const BnPlan& p, const BnPoolPlan& g,
                             const BnPoolArgs& a, hipStream_t stream) {
  float* psg = a.part;
  float* psgx = a.part + p.partial_floats;
  const uint4* dy = static_cast<const uint4*>(a.dy);
  const uint2* arg = reinterpret_cast<const uint2*>(a.arg);
  const uint4* x = static_cast<const uint4*>(a.x);
  const dim3 grid(p.grid), block(kT);
  hipLaunchKernelGGL(bn_pool_bwd_reduce, grid, block, 0, stream, dy, arg, x,
                     a.mean, a.invstd, psg, psgx, p, g);
  hipLaunchKernelGGL(bn_bwd_finalize, dim3(fin_grid(p)), block, 0, stream, psg,
                     psgx, a.dbeta, a.dgamma, p);
  hipLaunchKernelGGL(bn_pool_bwd_dx, grid, block, 0, stream, dy, arg, x, a.mean,
                     a.invstd, a.weight, a.dbeta, a.dgamma,
                     static_cast<uint4*>(a.dx), p, g);
  CGX_HIP_CHECK(hipGetLastError());
}

}  // namespace cgx
