// Weight gradient of a 3x3 / stride 1 / padding 1 convolution on
// channels_last bf16 tensors as an implicit GEMM.  Geometry: conv3x3_plan.h.
//
// dW[n][(3r+s)*C + c] = sum over pixels of dY[b, h, w, n] * X[b, h+r-1, w+s-1, c].
// Both operands have the contracted index slow, so both MFMA operands are
// read transposed from LDS images as in conv1x1_wrw (wrw_image.h): dY^T is
// the A operand and X the B operand of v_mfma_f32_32x32x16_bf16.  What is new
// is that the nine taps share one staged copy of both:
//
//   dY strip  position j = row*P + w of the chunk's rows, P = W+1; the pad
//             w = W, the rows past the chunk and the positions up to the
//             next multiple of 16 are zeros
//   X strip   rows -1 .. hr of the chunk at index i = (row+1)*P + wx + 1;
//             column 0 is zero and serves as column W of the row before;
//             rows that are no image row (conv3x3_wrw_row) are zeros
//
// Tap (r, s) then pairs position j with index j + r*P + s: at w = 0, s = 0
// and at w = W-1, s = 2 that is a zero column of X, above the first and
// below the last row of an image a zero row, and at a pad of dY the dY factor
// is zero.  Every index that a position below strip_dy reaches, up to
// strip_dy + 2P + 1, is written on every chunk, so no product has a stale
// factor (0 * NaN is not 0).  The inner loop has no masks and no loads per
// tap: one A operand and nine B operands, at nine LDS offsets, feed nine MFMAs
// per 32x32 tile and 16-position step.
//
// Bank conflicts.  A transposed read takes, per 32-lane half, one 64-byte cell
// of four consecutive positions (conv1x1_wrw argues why these must sit in the
// four different 64-byte columns of a 256-byte line).  With the taps the four
// positions start anywhere, not at a multiple of four.  The swizzle still
// separates them.  The one instantiation is the 64 x 64 tile, so both images
// are wrw_cell<64>: the column is 2*(r & 1) + (u ^ ((r >> 1) & 1)) and the
// pair (r & 1, (r >> 1) & 1) takes all four values on four consecutive
// positions.  (A 128-wide image, which no instantiation has yet, would have
// column (u ^ r) & 3, and r & 3 takes four values likewise.)  A step moves
// every address by 16 positions and the second read of an operand by 4, which
// changes neither r & 3 nor the pair: a lane keeps one base address per tap
// and 32-channel tile, and the loop adds a multiple of the position stride.  Every address is a multiple of 8 and
// inside the image, and no divergent branch encloses the reads: EXEC is all
// ones.
//
// The global loads of the next chunk are issued before the MFMAs of the
// current one and wait in registers.  A load that is to give zeros is
// pointed at the first pixel and replaced, so nothing outside the two
// tensors is read.  Each workgroup stores its fp32 tile to its split's plane
// of `part`; conv1x1_wrw_finalize sums the planes in a fixed order and rounds
// once: no atomics, the same bits every run.
#include <hip/hip_runtime.h>

#include "check.h"
#include "conv3x3_plan.h"
#include "wrw_image.h"

namespace cgx {
namespace {

constexpr int kT = kConvThreads;

// Thread tid's vectors of one strip of `chunk`: C channels from c0 of
// src[pixels, width].  IS_X: the strip starts a row and a column early.
template <int C, int NV, bool IS_X>
__device__ inline void conv3x3_load(uint4 (&v)[NV],
                                    const uint4* __restrict__ src,
                                    const Conv3x3WrwPlan& p, int chunk, int c0,
                                    int tid) {
  const int group = chunk / p.chunks_per_image;
  const int t0 = (chunk % p.chunks_per_image) * p.hr - (IS_X ? 1 : 0);
  const int strip = IS_X ? p.strip_x : p.strip_dy;
  const int width = IS_X ? p.c : p.n;
  const int rows = p.hr + (IS_X ? 2 : 0);
  const int nv = (strip * (C / 8) + kT - 1) / kT;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    if (i < nv) {  // uniform
      const int idx = tid + i * kT, j = idx / (C / 8), q = idx % (C / 8);
      const int rr = (int)(((unsigned)j * p.magic_pitch) >> kConv3x3MagicShift);
      const int col = j - rr * p.pitch - (IS_X ? 1 : 0);
      const int row = conv3x3_wrw_row(p, group, t0 + rr);
      const bool live = row >= 0 && rr < rows && col >= 0 && col < p.w;
      const int64_t pixel = live ? (int64_t)row * p.w + col : 0;
      const uint4 t = src[(pixel * width + c0) / 8 + q];
      v[i] = live ? t : make_uint4(0, 0, 0, 0);
    }
  }
}

// ... into the image: position j's 16-byte vector q, as wrw_store.
template <int C, int NV>
__device__ inline void conv3x3_store(char* img, const uint4 (&v)[NV], int strip,
                                     int tid) {
#pragma unroll
  for (int i = 0; i < NV; i++) {
    const int idx = tid + i * kT, j = idx / (C / 8), q = idx % (C / 8);
    if (j < strip)
      *reinterpret_cast<uint4*>(img + wrw_cell<C>(j, q >> 2) + 16 * (q & 3)) =
          v[i];
  }
}

template <int BN, int BK>
__global__ __launch_bounds__(kT) void conv3x3_wrw(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    float* __restrict__ part, Conv3x3WrwPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int MT = BN / 64, KT = BK / 64;  // 32x32 tiles of a wave, per tap
  // the registers a thread stages with hold the same bytes at every tile
  constexpr int DV = kConv3x3DyVecs, XV = kConv3x3XVecs;
  char* img_n = reinterpret_cast<char*>(lds);
  char* img_k = img_n + p.strip_dy * BN * 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int wn = wave >> 1, wk = wave & 1;
  const int tile = conv3x3_wrw_tile(p, blockIdx.x);
  const int split = conv3x3_wrw_split(p, blockIdx.x);
  const int n0 = (tile / p.ntiles_k) * BN, k0 = (tile % p.ntiles_k) * BK;

  // as conv1x1_wrw: lane 4q+pp of a 16-lane group supplies position 8h+q of
  // the step's first read; tap (r, s) shifts X by r*P + s positions
  const int q = (lane >> 2) & 3;
  const int in_cell = 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  int an[MT], ak[9][KT];
#pragma unroll
  for (int j = 0; j < MT; j++)
    an[j] = wrw_cell<BN>(8 * h + q, wn * MT + j) + in_cell;
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int j = 0; j < KT; j++)
      ak[tap][j] = wrw_cell<BK>(8 * h + q + (tap / 3) * p.pitch + tap % 3,
                                wk * KT + j) +
                   in_cell;

  f32x16 acc[9][MT][KT];
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int jm = 0; jm < MT; jm++)
#pragma unroll
      for (int jk = 0; jk < KT; jk++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[tap][jm][jk][e] = 0.f;

  uint4 vn[DV], vk[XV];
  int chunk = split;  // < p.chunks: no more splits than chunks
  conv3x3_load<BN, DV, false>(vn, dy, p, chunk, n0, tid);
  conv3x3_load<BK, XV, true>(vk, x, p, chunk, k0, tid);
  const int steps = p.strip_dy / 16;

  while (chunk < p.chunks) {
    __syncthreads();  // the previous chunk has been read
    conv3x3_store<BN, DV>(img_n, vn, p.strip_dy, tid);
    conv3x3_store<BK, XV>(img_k, vk, p.strip_x, tid);
    __syncthreads();
    chunk += p.splits;
    if (chunk < p.chunks) {
      conv3x3_load<BN, DV, false>(vn, dy, p, chunk, n0, tid);
      conv3x3_load<BK, XV, true>(vk, x, p, chunk, k0, tid);
    }
    // Two sets of operand registers: the reads of a step are issued before
    // the MFMAs of the step before it, so that no MFMA waits for LDS.
    bf16x8 a0[MT], b0[9][KT], a1[MT], b1[9][KT];
    auto read = [&](bf16x8 (&a)[MT], bf16x8 (&b)[9][KT], int s) {
#pragma unroll
      for (int j = 0; j < MT; j++) a[j] = wrw_operand<BN>(img_n, an[j], s);
#pragma unroll
      for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int j = 0; j < KT; j++)
          b[tap][j] = wrw_operand<BK>(img_k, ak[tap][j], s);
    };
    auto mma = [&](const bf16x8 (&a)[MT], const bf16x8 (&b)[9][KT]) {
#pragma unroll
      for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int jm = 0; jm < MT; jm++)
#pragma unroll
          for (int jk = 0; jk < KT; jk++)
            acc[tap][jm][jk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a[jm], b[tap][jk], acc[tap][jm][jk], 0, 0, 0);
    };
    read(a0, b0, 0);
    int s = 0;
    for (; s + 2 <= steps; s += 2) {
      read(a1, b1, s + 1);
      mma(a0, b0);
      if (s + 2 < steps) read(a0, b0, s + 2);
      mma(a1, b1);
    }
    if (s < steps) mma(a0, b0);  // an odd count's last step
  }

  // lane (c, h) holds dW[n][tap][k] for k = its column c and 16 rows n
  const int64_t ld = 9 * (int64_t)p.c;
  float* out = part + (int64_t)split * p.n * ld;
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int jm = 0; jm < MT; jm++)
#pragma unroll
      for (int jk = 0; jk < KT; jk++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int n = n0 + (wn * MT + jm) * 32 + acc_row(e, h);
          const int k = k0 + (wk * KT + jk) * 32 + c;
          out[n * ld + tap * p.c + k] = acc[tap][jm][jk][e];
        }
}

template <int BN, int BK>
void launch_wrw3x3(const Conv3x3WrwPlan& p, const void* dy, const void* x,
                   float* part, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv3x3_wrw<BN, BK>),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL((conv3x3_wrw<BN, BK>), dim3(p.grid), dim3(kT),
                     p.lds_bytes, stream, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x), part, p);
  CGX_HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_conv3x3_wrw(const Conv3x3WrwPlan& p, const void* dy, const void* x,
                        float* part, void* dw, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv3x3_wrw: shape is not eligible");
  TORCH_CHECK(p.bn == 64 && p.bk == 64 && p.lds_bytes <= kConvLdsBytes &&
                  p.splits <= p.chunks,
              "conv3x3_wrw: plan and kernel disagree");
  launch_wrw3x3<64, 64>(p, dy, x, part, stream);
  launch_wrw_finalize(part, dw, p.splits, (int64_t)p.n * 9 * p.c, stream);
}

}  // namespace cgx
