// The forward of the 1x1 / stride 2 / padding 0 convolution on channels_last
// bf16 activations, with the BatchNorm partials of its output: the three
// downsample convolutions of ResNet-50.  Geometry: Conv1x1S2Plan in
// conv1x1_plan.h.
//
// Y[R, N] = gather(X)[R, K] * W[N, K]^T, where row (b, oh, ow) of the gathered
// matrix is the K contiguous channels of input pixel (b, 2*oh, 2*ow).  Both
// operands go through a ring of two LDS stages that global_load_lds_dwordx4
// fills, so neither passes through registers on its way in:
//
//   A   [256 rows][64 channels] of one K chunk.  An instruction of a wave
//       writes 1 KiB of LDS contiguously, lane l at 16 * l, so both the
//       swizzle of the image and the stride-2 gather sit in the address the
//       lane loads from: the lane that fills slot p reads vector `vec` of the
//       input pixel of the row conv1x1s2_stage_slot(p) names.  A lane fills
//       the same eight rows of every chunk of a tile; their pixel offsets are
//       worked out once a tile, with two divisions (conv1x1s2_lane_pixels)
//   B   [256 channels][64] of the same chunk of W, behind A in the stage, in
//       the same layout
//   C   the four waves sit 2 x 2 on the 256 x 256 tile, each 128 x 128:
//       sixteen 32x32 accumulators.  A 16-deep step is four ds_read_b128 of A,
//       four of B and sixteen v_mfma_f32_32x32x16_bf16; both reads are the
//       conflict-free ones of the stride-1 kernels (w_slot<64>)
//
// Per stage, as in conv1x1_wrw_ring:
//
//   s_waitcnt vmcnt(16)   this wave's loads of the stage have landed; the 16
//                         of the younger stage stay in flight.  Stores of an
//                         epilogue in between only raise the count, and loads
//                         return in order among themselves, so the wait can
//                         be early but not late
//   s_barrier             ... and those of every wave
//   4 steps of reads and MFMAs
//   s_waitcnt lgkmcnt(0), s_barrier   every wave has read the stage
//   global_load_lds       stage g + 2 into the buffer just freed
//
// The stages of a workgroup are numbered through all its tiles, so the ring
// never drains at a tile's end: the first chunks of the next tile load behind
// the last MFMAs and the epilogue of this one.  The operand reads are
// instructions of the kernel's own (lds_read_b128), because the compiler puts
// s_waitcnt vmcnt(0) before any LDS read it knows of while a load to LDS is
// pending; the kernel waits for them by count itself.
//
// The epilogue is the stride-1 forward's: one rounding to bf16, the rounded
// values into the lane's running moments (of v - pivot, as in conv3x3_stats),
// 32 x 64 sub-tiles through the wave's strip to 16-byte row vectors.  A
// channel has four runs in a workgroup (two waves x two lane halves), which
// merge as a tree in a fixed order.  No atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "bn_moments.h"
#include "check.h"
#include "conv1x1_plan.h"
#include "conv_epilogue.h"

namespace cgx {
namespace {

constexpr int kT = kConvThreads;
constexpr int kRows = kS2TileRows, kBn = kS2TileChannels;
static_assert(kRows == 256 && kBn == 256 && kS2Kc == 64 && kS2Stages == 2 &&
              kS2Glds == 8);

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(1))) const void global_cvoid;

template <int N>
__device__ inline void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ inline void wait_lgkmcnt() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// 16 bytes at LDS address `addr` + OFF.  The compiler does not see an LDS
// read here, so nothing waits for it but the kernel's own s_waitcnt lgkmcnt;
// source order and the sched_barrier(0) after each wait keep the MFMAs that
// take the result behind that wait.  After a change of toolchain read the .s
// again: the result registers must be the MFMAs' own operands, with no copy
// between the read and the wait.
template <int OFF>
__device__ inline u32x4 lds_read_b128(unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536);
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}

// the four operands 32 rows (4 KiB of a [.][64] image) apart
__device__ inline void read4(u32x4 (&v)[4], unsigned addr) {
  v[0] = lds_read_b128<0>(addr);
  v[1] = lds_read_b128<4096>(addr);
  v[2] = lds_read_b128<8192>(addr);
  v[3] = lds_read_b128<12288>(addr);
}

__global__ __launch_bounds__(kT) void conv1x1s2_stats(
    const uint4* __restrict__ x, const uint4* __restrict__ w,
    uint4* __restrict__ y, float* __restrict__ part, Conv1x1S2Plan p) {
  extern __shared__ uint4 lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;  // the wave's 128 x 128 of the tile
  const int ntile = conv1x1_tiled_ntile(p, blockIdx.x);
  const int split = conv1x1_tiled_split(p, blockIdx.x);
  const int n0 = ntile * kBn, nvec = p.n / 8, kvec = p.k / 8;
  lds_char* ring = (lds_char*)lds;
  uint4* strip = lds + kS2Stages * kS2StageBytes / 16 + wave * 256;

  // What the lane loads: vector `vec` of the rows (of B: channels) 32 apart
  // from the first, which is the same for A and B, as is the swizzle.
  const Conv1x1S2Slot first =
      conv1x1s2_stage_slot(conv1x1s2_piece(wave, 0) / 16 + lane);
  int asrc[kS2Glds], bsrc[kS2Glds];  // in vectors, at chunk 0
#pragma unroll
  for (int j = 0; j < kS2Glds; j++)
    bsrc[j] = (n0 + first.row + 32 * j) * kvec + first.vec;
  auto aim = [&](int tile) {
    conv1x1s2_lane_pixels(p, tile, wave, lane, asrc);
#pragma unroll
    for (int j = 0; j < kS2Glds; j++) asrc[j] = asrc[j] * kvec + first.vec;
  };
  auto issue = [&](int kc, int slot) {
    lds_char* dst = ring + slot * kS2StageBytes;
#pragma unroll
    for (int j = 0; j < kS2Glds; j++)
      __builtin_amdgcn_global_load_lds(
          (global_cvoid*)(x + asrc[j] + kc * (kS2Kc / 8)),
          dst + conv1x1s2_piece(wave, j), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < kS2Glds; j++)
      __builtin_amdgcn_global_load_lds(
          (global_cvoid*)(w + bsrc[j] + kc * (kS2Kc / 8)),
          dst + kS2ImageBytes + conv1x1s2_piece(wave, j), 16, 0, 0);
  };

  // What the lane multiplies: of step q, vector 2q + h of row (channel) c of
  // each of its four 32-row (32-channel) blocks: w_slot<64>, whose XOR is
  // that of c for every block.
  const unsigned ring_addr = (unsigned)(unsigned long)ring;
  unsigned pa[4], pb[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const unsigned in_block = 128 * c + 16 * ((2 * q + h) ^ ((c >> 1) & 7));
    pa[q] = ring_addr + wm * (kS2ImageBytes / 2) + in_block;
    pb[q] = ring_addr + kS2ImageBytes + wn * (kS2ImageBytes / 2) + in_block;
  }

  // the lane's moments of v - pivot, pivot the first value it pushes
  Moments<4> mo;
  float pivot[4] = {0.f, 0.f, 0.f, 0.f};
  auto push = [&](const float (&v)[4]) __attribute__((always_inline)) {
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      pivot[j] = mo.n == 0.f ? v[j] : pivot[j];
      d[j] = v[j] - pivot[j];
    }
    mo.push(d);
  };

  // The stages 0 .. S-1 of this workgroup: chunk g % nchunks of its tile
  // g / nchunks.  (tile_i, kc) is the stage being multiplied, (load_i,
  // load_kc) the next one to load.
  const int tiles = (p.row_tiles - split + p.splits - 1) / p.splits;
  const int S = tiles * p.nchunks;
  int load_i = 0, load_kc = 0;
  auto issue_next = [&](int slot) {
    if (load_kc == 0) aim(conv1x1_tile(p, split, load_i));
    issue(load_kc, slot);
    if (++load_kc == p.nchunks) load_kc = 0, load_i++;
  };
  issue_next(0);
  if (S > 1) issue_next(1);

  int g = 0;
  for (int tile_i = 0; tile_i < tiles; tile_i++) {
    f32x16 acc[4][4];  // [row block s][channel block j]
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[s][j][e] = 0.f;

    for (int kc = 0; kc < p.nchunks; kc++, g++) {
      const unsigned sb = (g & 1) * kS2StageBytes;
      if (g + 1 < S) wait_vmcnt<2 * kS2Glds>();
      else wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();

      // The reads of step q + 1 are issued before the MFMAs of step q and
      // waited for by count: see lds_read_b128.
      u32x4 a[2][4], b[2][4];
      read4(a[0], pa[0] + sb);
      read4(b[0], pb[0] + sb);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (q + 1 < 4) {
          read4(a[(q + 1) & 1], pa[q + 1] + sb);
          read4(b[(q + 1) & 1], pb[q + 1] + sb);
          wait_lgkmcnt<8>();
        } else {
          wait_lgkmcnt<0>();
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
          for (int j = 0; j < 4; j++)
            acc[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                __builtin_bit_cast(bf16x8, a[q & 1][s]),
                __builtin_bit_cast(bf16x8, b[q & 1][j]), acc[s][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // every read has been waited for; every wave has read the stage
      __builtin_amdgcn_s_barrier();
      if (g + 2 < S) issue_next(g & 1);
    }

    // The tile is complete: round, push, store (stats_body in
    // conv1x1_kernels.hip), one 32-row block at a time.
    const int tile = conv1x1_tile(p, split, tile_i);
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int r0 = tile * kRows + wm * 128 + s * 32;
      const int live = p.rows - r0 < 32 ? (int)(p.rows - r0) : 32;  // or <= 0
      unsigned pk[4][8];
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int e = 0; e < 8; e++)
          pk[j][e] = fwd_pack_bf16(acc[s][j][2 * e], acc[s][j][2 * e + 1]);
      // the moments of the rounded values: what bn_apply will normalise
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float lo[4], hi[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          lo[j] = __uint_as_float(pk[j][e] << 16);
          hi[j] = __uint_as_float(pk[j][e] & 0xffff0000u);
        }
        if (acc_row(2 * e, h) < live) push(lo);
        if (acc_row(2 * e + 1, h) < live) push(hi);
      }
#pragma unroll
      for (int jp = 0; jp < 2; jp++) {
        unsigned half[2][8];
#pragma unroll
        for (int jj = 0; jj < 2; jj++)
#pragma unroll
          for (int e = 0; e < 8; e++) half[jj][e] = pk[2 * jp + jj][e];
        fwd_store_subtile(half, strip, y, r0, live, nvec,
                          n0 + wn * 128 + jp * 64, lane);
      }
    }
  }

  // The four runs of every channel (wm, h) -> one partial, as a tree.  A
  // merge keeps the pivot of its first run (of the second where the first is
  // empty) and moves the other mean there, as in conv3x3_stats.  Nothing is
  // in flight and the ring is free: the last wait was vmcnt(0).
  __syncthreads();
  float* sc = reinterpret_cast<float*>(lds);
  const int run = wm * 2 + h;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int ch = wn * 128 + j * 32 + c;
    sc[run * kBn + ch] = mo.mean[j];
    sc[(4 + run) * kBn + ch] = mo.m2[j];
    sc[(8 + run) * kBn + ch] = pivot[j];
  }
  if (c == 0 && wn == 0) sc[12 * kBn + run] = mo.n;
  __syncthreads();
  Moments<1> m[4];
  float pv[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    m[r].n = sc[12 * kBn + r];
    m[r].mean[0] = sc[r * kBn + tid];
    m[r].m2[0] = sc[(4 + r) * kBn + tid];
    pv[r] = sc[(8 + r) * kBn + tid];
  }
#pragma unroll
  for (int step = 1; step < 4; step *= 2)
#pragma unroll
    for (int r = 0; r < 4; r += 2 * step) {
      pv[r] = m[r].n > 0.f ? pv[r] : pv[r + step];
      const float mb[1] = {m[r + step].n > 0.f
                               ? (pv[r + step] - pv[r]) + m[r + step].mean[0]
                               : 0.f};
      m[r].merge(m[r + step].n, mb, m[r + step].m2);
    }
  float* row = part + (int64_t)split * p.pstride;
  row[n0 + tid] = pv[0] + m[0].mean[0];
  row[p.n + n0 + tid] = m[0].m2[0];
  if (tid == 0) row[2 * p.n + ntile] = m[0].n;
}

}  // namespace

void launch_conv1x1s2_stats(const Conv1x1S2Plan& p, const void* x,
                            const void* w, void* y, float* part,
                            hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1s2_stats: shape is not eligible");
  TORCH_CHECK(p.bn == kBn && p.tile_rows == kRows && p.kc == kS2Kc &&
                  p.stages == kS2Stages &&
                  p.lds_bytes == kS2Stages * kS2StageBytes + kConvStageBytes &&
                  p.lds_bytes <= kConvLdsBytes && p.splits <= p.row_tiles,
              "conv1x1s2_stats: plan and kernel disagree");
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv1x1s2_stats),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL(conv1x1s2_stats, dim3(p.grid), dim3(kT), p.lds_bytes,
                     stream, static_cast<const uint4*>(x),
                     static_cast<const uint4*>(w), static_cast<uint4*>(y),
                     part, p);
  CGX_HIP_CHECK(hipGetLastError());
}

}  // namespace cgx
