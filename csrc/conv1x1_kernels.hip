// Forward of a 1x1 / stride 1 convolution on a channels_last bf16 activation,
// Y[R, N] = X[R, K] * W[N, K]^T, that also leaves the per-channel
// (count, mean, M2) partials of Y for the BatchNorm that follows: the output is
// written once and never read back for its statistics.  Geometry:
// conv1x1_plan.h.
//
//   W   the workgroup's [bn, K] tile is copied to LDS once (or one [bn, kc]
//       chunk per step where it does not fit), rows XOR-swizzled so that the
//       ds_read_b128 of a B operand is conflict-free
//   X   each lane loads the 16 bytes of its A operand (row lane&31, k
//       8*(lane>>5) .. +7 of a 16-deep step) straight from global memory, one K
//       chunk ahead of the MFMAs that use it
//   Y   v_mfma_f32_32x32x16_bf16 leaves channel lane&31 of 16 rows in a lane.
//       The accumulators are rounded to bf16 (as bf16_bits does), the rounded
//       values go into the lane's running moments, and the tile is turned
//       into 16-byte row vectors through a per-wave LDS strip of
//       [32 rows][64 channels] and stored.
//
// A lane keeps its moments across all tiles of its workgroup; at the end the
// eight runs of a channel (4 waves x 2 lane halves) merge as a tree in a fixed
// order.  No atomics: two runs give the same bits.
//
// The backward-data GEMM of the same convolution, which can add a second
// tensor in its epilogue, follows the forward below.
#include <hip/hip_runtime.h>

#include "bn_moments.h"
#include "check.h"
#include "conv1x1_plan.h"

namespace cgx {
namespace {

constexpr int kT = kConvThreads;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Where 16-byte chunk q of row n of a [rows][KC] bf16 image sits in LDS.  A
// B-operand read takes the same q of 16 rows that differ in n & 15; the XOR
// puts them on the 16 different slots of a 256-byte bank row.
template <int KC>
__device__ inline int w_slot(int n, int q) {
  return n * (KC / 8) + (q ^ (KC == 64 ? (n >> 1) & 7 : n & 15));
}

// Row of a 32x32 accumulator tile that register i of lane half h holds.
__device__ inline int acc_row(int i, int h) {
  return (i & 3) + 8 * (i >> 2) + 4 * h;
}

// Two accumulators -> two bf16 (round to nearest even, quiet NaN), a in the
// low half.
__device__ inline unsigned pack_bf16(float a, float b) {
  const f32x2 f = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}

template <int NT, int KC>
__device__ inline void stage_w(uint4* dst, const uint4* __restrict__ w, int n0,
                               int k, int chunk, int tid) {
  constexpr int cpr = KC / 8;
  for (int idx = tid; idx < 32 * NT * cpr; idx += kT) {
    const int n = idx / cpr, q = idx % cpr;
    dst[w_slot<KC>(n, q)] = w[((int64_t)(n0 + n) * k + chunk * KC) / 8 + q];
  }
}

template <int NT, int KC, bool RES>
__global__ __launch_bounds__(kT) void conv1x1_stats(
    const uint4* __restrict__ x, const uint4* __restrict__ w,
    uint4* __restrict__ y, float* __restrict__ part, Conv1x1Plan p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = 32 * NT, cpr = KC / 8, steps = KC / 16;
  constexpr int wchunks = BN * cpr;  // 16-byte chunks of one K chunk of W
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int ntile = conv1x1_ntile(p, blockIdx.x);
  const int split = conv1x1_split(p, blockIdx.x);
  const int n0 = ntile * BN;
  const int kvec = p.k / 8, nvec = p.n / 8;
  uint4* stage = lds + (RES ? p.nchunks : 1) * wchunks + wave * 256;
  unsigned* stage32 = reinterpret_cast<unsigned*>(stage);

  if (RES) {
    for (int kc = 0; kc < p.nchunks; kc++)
      stage_w<NT, KC>(lds + kc * wchunks, w, n0, p.k, kc, tid);
    __syncthreads();
  }

  // the lane's A row of row tile t; rows past R read row R-1 and are dropped
  auto a_row = [&](int t) {
    int64_t r = (int64_t)t * kConvTileRows + wave * 32 + c;
    r = r < p.rows ? r : p.rows - 1;
    return x + r * kvec;
  };

  Moments<NT> st;
  uint4 a[steps], an[steps];
  const uint4* xr = a_row(split);
#pragma unroll
  for (int s = 0; s < steps; s++) a[s] = xr[2 * s + h];

  for (int i = 0; i < p.tiles_per_split; i++) {
    const int t = conv1x1_tile(p, split, i);
    if (t >= p.row_tiles) break;
    const int tn = conv1x1_tile(p, split, i + 1);
    const uint4* xn = a_row(tn < p.row_tiles ? tn : t);

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[j][e] = 0.f;

    for (int kc = 0; kc < p.nchunks; kc++) {
      // the next chunk's A operands: of this tile, or the first of the next
      const uint4* src = kc + 1 < p.nchunks ? xr + (kc + 1) * cpr : xn;
#pragma unroll
      for (int s = 0; s < steps; s++) an[s] = src[2 * s + h];
      if (!RES) {
        __syncthreads();
        stage_w<NT, KC>(lds, w, n0, p.k, kc, tid);
        __syncthreads();
      }
      const uint4* wl = lds + (RES ? kc * wchunks : 0);
#pragma unroll
      for (int s = 0; s < steps; s++) {
        const bf16x8 av = __builtin_bit_cast(bf16x8, a[s]);
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const uint4 b = wl[w_slot<KC>(j * 32 + c, 2 * s + h)];
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              av, __builtin_bit_cast(bf16x8, b), acc[j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int s = 0; s < steps; s++) a[s] = an[s];
    }
    xr = xn;

    // rows of this wave's strip that exist
    const int64_t r0 = (int64_t)t * kConvTileRows + wave * 32;
    const int live = (int)(p.rows - r0 < 32 ? p.rows - r0 : 32);

    // registers 2e, 2e+1 (two consecutive rows) rounded into one word
    unsigned pk[NT][8];
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int e = 0; e < 8; e++)
        pk[j][e] = pack_bf16(acc[j][2 * e], acc[j][2 * e + 1]);

    // the moments of the rounded values: what bn_apply will normalise
#pragma unroll
    for (int e = 0; e < 8; e++) {
      float lo[NT], hi[NT];
#pragma unroll
      for (int j = 0; j < NT; j++) {
        lo[j] = __uint_as_float(pk[j][e] << 16);
        hi[j] = __uint_as_float(pk[j][e] & 0xffff0000u);
      }
      if (acc_row(2 * e, h) < live) st.push(lo);
      if (acc_row(2 * e + 1, h) < live) st.push(hi);
    }

    // Two MFMA tiles (64 channels) at a time through the wave's strip: lanes
    // c and c^1 trade words so that the even lane writes channels (c, c+1) of
    // row 2e and the odd one channels (c-1, c) of row 2e+1.  Odd rows swap
    // their 64-byte halves, which keeps both the 4-byte writes and the
    // 16-byte reads conflict-free.
    const int odd = c & 1;
#pragma unroll
    for (int jp = 0; jp < NT / 2; jp++) {
#pragma unroll
      for (int jj = 0; jj < 2; jj++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const unsigned own = pk[2 * jp + jj][e];
          // quad_perm [1, 0, 3, 2]
          const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(
              0, (int)own, 0xB1, 0xf, 0xf, false);
          const unsigned word = odd ? (other >> 16) | (own & 0xffff0000u)
                                    : (own & 0xffffu) | (other << 16);
          const int row = acc_row(2 * e, h) + odd;
          stage32[row * 32 + ((jj * 16 + (c >> 1)) ^ ((row & 1) << 4))] = word;
        }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int idx = u * 64 + lane, row = idx >> 3, q = idx & 7;
        const uint4 v = stage[row * 8 + (q ^ ((row & 1) << 2))];
        if (row < live) y[(r0 + row) * nvec + (n0 + jp * 64) / 8 + q] = v;
      }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
  }

  // the eight runs of every channel -> one partial, as a tree
  __syncthreads();
  float* sc = reinterpret_cast<float*>(lds);
  const int run = wave * 2 + h;
#pragma unroll
  for (int j = 0; j < NT; j++) {
    sc[run * BN + j * 32 + c] = st.mean[j];
    sc[(8 + run) * BN + j * 32 + c] = st.m2[j];
  }
  if (c == 0) sc[16 * BN + run] = st.n;
  __syncthreads();
  if (tid < BN) {
    Moments<1> m[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
      m[r].n = sc[16 * BN + r];
      m[r].mean[0] = sc[r * BN + tid];
      m[r].m2[0] = sc[(8 + r) * BN + tid];
    }
#pragma unroll
    for (int step = 1; step < 8; step *= 2)
#pragma unroll
      for (int r = 0; r < 8; r += 2 * step)
        m[r].merge(m[r + step].n, m[r + step].mean, m[r + step].m2);
    float* row = part + (int64_t)split * p.pstride;
    row[n0 + tid] = m[0].mean[0];
    row[p.n + n0 + tid] = m[0].m2[0];
    if (tid == 0) row[2 * p.n + ntile] = m[0].n;
  }
}

template <int NT, int KC, bool RES>
void launch(const Conv1x1Plan& p, const void* x, const void* w, void* y,
            float* part, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv1x1_stats<NT, KC, RES>),
      hipFuncAttributeMaxDynamicSharedMemorySize,
      kConvWLdsBytes + kConvStageBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL((conv1x1_stats<NT, KC, RES>), dim3(p.grid), dim3(kT),
                     p.lds_bytes, stream, static_cast<const uint4*>(x),
                     static_cast<const uint4*>(w), static_cast<uint4*>(y), part,
                     p);
}

template <int NT>
void launch_nt(const Conv1x1Plan& p, const void* x, const void* w, void* y,
               float* part, hipStream_t stream) {
  if (p.kc == 64) launch<NT, 64, true>(p, x, w, y, part, stream);
  else if (p.resident) launch<NT, 128, true>(p, x, w, y, part, stream);
  else launch<NT, 128, false>(p, x, w, y, part, stream);
}

// ---- backward-data ----------------------------------------------------------
//
// dX[R, K] = dY[R, N] * W[N, K] is the GEMM above with dY as the A operand and
// W^T as B (plan: conv1x1_bwd_plan, whose `k` is N and whose `n` is K).  The
// weight stays the convolution's [N, K]: the staging loop transposes it on the
// way into the same swizzled [bn][KC] image.  The epilogue differs: the
// accumulators go through the wave's strip as fp32, and the lane that reads a
// 16-byte row vector back adds the skip gradient's vector of the same place
// before the one rounding to bf16.

// The chunk `chunk` of W^T for output channels k0 .. k0 + 32*NT: a thread takes
// an 8x8 block, eight 16-byte loads along K of eight consecutive rows n, and
// writes it as eight 16-byte vectors along n.  Eight consecutive lanes take
// eight different n-blocks of the same channels, so their writes fall on the
// eight 16-byte slots of a 128-byte bank row.
template <int NT, int KC>
__device__ inline void stage_wt(uint4* dst, const uint4* __restrict__ w, int k0,
                                int kw, int chunk, int tid) {
  constexpr int kblocks = 4 * NT;  // 8-channel blocks of the tile
  for (int idx = tid; idx < kblocks * (KC / 8); idx += kT) {
    const int n8 = (idx & 7) + 8 * (idx / (8 * kblocks));
    const int k8 = (idx >> 3) % kblocks;
    unsigned r[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint4 v =
          w[((int64_t)(chunk * KC + n8 * 8 + i) * kw + k0) / 8 + k8];
      r[i][0] = v.x, r[i][1] = v.y, r[i][2] = v.z, r[i][3] = v.w;
    }
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
      unsigned o[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const unsigned a = r[2 * m][kk >> 1], b = r[2 * m + 1][kk >> 1];
        o[m] = kk & 1 ? (a >> 16) | (b & 0xffff0000u)
                      : (a & 0xffffu) | (b << 16);
      }
      dst[w_slot<KC>(k8 * 8 + kk, n8)] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int NT, int KC, bool RES, bool ADD>
__global__ __launch_bounds__(kT) void conv1x1_bwd_data(
    const uint4* __restrict__ dy, const uint4* __restrict__ w,
    const uint4* __restrict__ skip, uint4* __restrict__ dx, Conv1x1Plan p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = 32 * NT, cpr = KC / 8, steps = KC / 16;
  constexpr int wchunks = BN * cpr;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int split = conv1x1_split(p, blockIdx.x);
  const int n0 = conv1x1_ntile(p, blockIdx.x) * BN;
  const int kvec = p.k / 8, nvec = p.n / 8;
  // the wave's strip: [32 rows][64 channels] of fp32
  uint4* stage = lds + (RES ? p.nchunks : 1) * wchunks + wave * 512;
  float* stagef = reinterpret_cast<float*>(stage);

  if (RES) {
    for (int kc = 0; kc < p.nchunks; kc++)
      stage_wt<NT, KC>(lds + kc * wchunks, w, n0, p.n, kc, tid);
    __syncthreads();
  }

  auto a_row = [&](int t) {
    int64_t r = (int64_t)t * kConvTileRows + wave * 32 + c;
    r = r < p.rows ? r : p.rows - 1;
    return dy + r * kvec;
  };

  uint4 a[steps], an[steps];
  const uint4* xr = a_row(split);
#pragma unroll
  for (int s = 0; s < steps; s++) a[s] = xr[2 * s + h];

  for (int i = 0; i < p.tiles_per_split; i++) {
    const int t = conv1x1_tile(p, split, i);
    if (t >= p.row_tiles) break;
    const int tn = conv1x1_tile(p, split, i + 1);
    const uint4* xn = a_row(tn < p.row_tiles ? tn : t);

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[j][e] = 0.f;

    for (int kc = 0; kc < p.nchunks; kc++) {
      const uint4* src = kc + 1 < p.nchunks ? xr + (kc + 1) * cpr : xn;
#pragma unroll
      for (int s = 0; s < steps; s++) an[s] = src[2 * s + h];
      if (!RES) {
        __syncthreads();
        stage_wt<NT, KC>(lds, w, n0, p.n, kc, tid);
        __syncthreads();
      }
      const uint4* wl = lds + (RES ? kc * wchunks : 0);
#pragma unroll
      for (int s = 0; s < steps; s++) {
        const bf16x8 av = __builtin_bit_cast(bf16x8, a[s]);
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const uint4 b = wl[w_slot<KC>(j * 32 + c, 2 * s + h)];
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              av, __builtin_bit_cast(bf16x8, b), acc[j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int s = 0; s < steps; s++) a[s] = an[s];
    }
    xr = xn;

    const int64_t r0 = (int64_t)t * kConvTileRows + wave * 32;
    const int live = (int)(p.rows - r0 < 32 ? p.rows - r0 : 32);

    // Two MFMA tiles (64 channels) at a time through the strip.  A 4-byte
    // write goes to bank (row's 64 + channel) % 32 from 32 lanes of one row:
    // no conflict.  Odd rows swap the 16-byte halves of every 32 bytes, which
    // spreads the 16-byte reads of a lane group (rows r .. r+3, half a row
    // each) over all 64 banks.
#pragma unroll
    for (int jp = 0; jp < NT / 2; jp++) {
      uint4 sk[4];
      if (ADD) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int idx = u * 64 + lane, row = idx >> 3, q = idx & 7;
          sk[u] = make_uint4(0, 0, 0, 0);
          if (row < live)
            sk[u] = skip[(r0 + row) * nvec + (n0 + jp * 64) / 8 + q];
        }
      }
#pragma unroll
      for (int jj = 0; jj < 2; jj++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int row = acc_row(e, h);
          stagef[row * 64 + ((jj * 32 + c) ^ ((row & 1) << 2))] =
              acc[2 * jp + jj][e];
        }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int idx = u * 64 + lane, row = idx >> 3, q = idx & 7;
        const uint4 lo = stage[row * 16 + 2 * q + (row & 1)];
        const uint4 hi = stage[row * 16 + 2 * q + ((row & 1) ^ 1)];
        float f[8] = {__uint_as_float(lo.x), __uint_as_float(lo.y),
                      __uint_as_float(lo.z), __uint_as_float(lo.w),
                      __uint_as_float(hi.x), __uint_as_float(hi.y),
                      __uint_as_float(hi.z), __uint_as_float(hi.w)};
        if (ADD) {
          const unsigned s4[4] = {sk[u].x, sk[u].y, sk[u].z, sk[u].w};
#pragma unroll
          for (int m = 0; m < 4; m++) {
            f[2 * m] += __uint_as_float(s4[m] << 16);
            f[2 * m + 1] += __uint_as_float(s4[m] & 0xffff0000u);
          }
        }
        const uint4 v = make_uint4(pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]),
                                   pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7]));
        if (row < live) dx[(r0 + row) * nvec + (n0 + jp * 64) / 8 + q] = v;
      }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <int NT, int KC, bool RES, bool ADD>
void launch_bwd(const Conv1x1Plan& p, const void* dy, const void* w,
                const void* skip, void* dx, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv1x1_bwd_data<NT, KC, RES, ADD>),
      hipFuncAttributeMaxDynamicSharedMemorySize,
      kConvWLdsBytes + kConvBwdStageBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL((conv1x1_bwd_data<NT, KC, RES, ADD>), dim3(p.grid),
                     dim3(kT), p.lds_bytes, stream,
                     static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(w),
                     static_cast<const uint4*>(skip), static_cast<uint4*>(dx),
                     p);
}

template <int NT, bool ADD>
void launch_bwd_nt(const Conv1x1Plan& p, const void* dy, const void* w,
                   const void* skip, void* dx, hipStream_t stream) {
  if (p.kc == 64) launch_bwd<NT, 64, true, ADD>(p, dy, w, skip, dx, stream);
  else if (p.resident)
    launch_bwd<NT, 128, true, ADD>(p, dy, w, skip, dx, stream);
  else launch_bwd<NT, 128, false, ADD>(p, dy, w, skip, dx, stream);
}

template <bool ADD>
void launch_bwd_add(const Conv1x1Plan& p, const void* dy, const void* w,
                    const void* skip, void* dx, hipStream_t stream) {
  if (p.nt == 2) launch_bwd_nt<2, ADD>(p, dy, w, skip, dx, stream);
  else if (p.nt == 4) launch_bwd_nt<4, ADD>(p, dy, w, skip, dx, stream);
  else launch_bwd_nt<8, ADD>(p, dy, w, skip, dx, stream);
}

}  // namespace

void launch_conv1x1_bwd_data(const Conv1x1Plan& p, const void* dy,
                             const void* w, const void* skip, void* dx,
                             hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1_bwd_data: shape is not eligible");
  if (skip) launch_bwd_add<true>(p, dy, w, skip, dx, stream);
  else launch_bwd_add<false>(p, dy, w, skip, dx, stream);
  CGX_HIP_CHECK(hipGetLastError());
}

void launch_conv1x1_stats(const Conv1x1Plan& p, const void* x, const void* w,
                          void* y, float* part, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1_stats: shape is not eligible");
  if (p.nt == 2) launch_nt<2>(p, x, w, y, part, stream);
  else if (p.nt == 4) launch_nt<4>(p, x, w, y, part, stream);
  else launch_nt<8>(p, x, w, y, part, stream);
  CGX_HIP_CHECK(hipGetLastError());
}

}  // namespace cgx
