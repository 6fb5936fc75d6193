// The stem of a ResNet, Conv2d(3, 64, 7, stride 2, padding 3) on channels_last
// bf16 tensors, as an implicit GEMM built for three input channels, which also
// produces the BatchNorm partials of its output as conv3x3_stats does
// (conv_stem_stats).  Its weight gradient (conv_stem_wrw) follows, with its
// own description.  Geometry: conv_stem_plan.h.
//
//   B   the whole weight, padded from [64][7][21] to [64][7][24] + 8, stays in
//       registers for the workgroup's whole walk: lane (c, h) holds for the
//       two 32-channel tiles j and the eleven 16-deep steps u the elements
//       8h .. 8h+7 of step u of channel 32j + c, group G = 2u + h: 88
//       registers.  The raw [64][147] weight goes through LDS once, where the
//       strips will be, and every lane picks its elements, zeros in the pads
//   A   read straight out of the strip, the raw input rows of the band: lane
//       (c, h) reads for step u the 16 bytes of group 2u + h of the tile's
//       pixel c (conv_stem_operand + conv_stem_group_offset) and clears what
//       lies beyond the filter row's 21 elements (conv_stem_keep), so that a
//       non-finite value of the next pixel never meets a zero weight.  The
//       main loop reads nothing else from LDS: 11 reads feed 22 MFMAs per
//       tile of 32 pixels
//   C   two accumulator tiles per 32-pixel tile; the four waves take the
//       tiles of a band in turn.  A tile is 32 consecutive pixels of the band
//       in memory order and may cross output rows; the last one may be short
//
// The strip's rows are shifted by one element against the input's 16-byte
// vectors (row element 0 sits at byte 18), so that the operands are 4-byte
// aligned.  The shift happens in registers on the way in: a thread loads an
// input vector and the one element before it and writes them as one aligned
// 16-byte vector of the strip.  Consecutive pixels are 12 bytes apart, three
// banks, and 3 is invertible modulo 64: the 32 lanes of a half wave read
// without bank conflicts wherever a tile stays in one output row.
//
// A thread loads its share of the next band's strip into registers before the
// MFMAs of this band and writes it to the other buffer after them, so one
// barrier a band orders both.  A load that is to give zeros is pointed at the
// tensor's first element and replaced: nothing outside x is read.  Every
// accumulator is one chain over the steps in ascending order and the moments
// merge in a fixed tree: the same bits every run.
#include <hip/hip_runtime.h>

#include "bn_moments.h"
#include "check.h"
#include "conv_epilogue.h"
#include "conv_stem_plan.h"

namespace cgx {
namespace {

constexpr int kT = kConvThreads;
constexpr int kStemSteps = kConvStemGroups / 2;
constexpr int kStemRowElems = kConvStemTaps * kConvStemC;           // 21
constexpr int kStemFilter = kConvStemTaps * kStemRowElems;          // 147
constexpr int kStemWVecs = kConvStemN * kStemFilter * 2 / 16;       // 1176
static_assert(kConvStemN * kStemFilter * 2 % 16 == 0 && kConvStemN == 64 &&
              kConvStemTile == 32 && kConvStemRowK == 24);

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// an operand of the strip: 16 bytes at a 4-byte aligned address
typedef u32x4 __attribute__((aligned(4))) u32x4_a4;

// A thread's share of one strip in registers: input vectors and the element
// before each.
struct StemStage {
  u32x4 v[kConvStemXVecs];
  unsigned short e[kConvStemXVecs];
  __device__ __forceinline__ void load(const uint4* __restrict__ x,
                                       const ConvStemPlan& p, int band,
                                       int tid) {
    const unsigned short* xs = reinterpret_cast<const unsigned short*>(x);
    const ConvStemBand b = conv_stem_band(p, band);
    const int row_vecs = 3 * p.w / 8;
#pragma unroll
    for (int i = 0; i < kConvStemXVecs; i++)
      if (i < p.xvecs) {  // uniform
        // The source of a vector is the same for every band but for its
        // image and row.  Opaque, so that it is worked out again per band
        // and not kept in sixteen registers across the MFMAs: without this
        // the kernel spills to scratch (32 bytes a lane with ROCm 7.2's clang;
        // check -Rpass-analysis=kernel-resource-usage after a compiler
        // change, benchmarks/RESULTS.md).
        int idx = tid + i * kT;
        asm volatile("" : "+v"(idx));
        const ConvStemSrc s = conv_stem_src(p, b, idx);
        const u32x4 t = *reinterpret_cast<const u32x4*>(
            x + (s.vec >= 0 ? (int64_t)s.row * row_vecs + s.vec : 0));
        const unsigned short a =
            xs[s.elem >= 0 ? (int64_t)s.row * 3 * p.w + s.elem : 0];
        v[i] = s.vec >= 0 ? t : u32x4{0, 0, 0, 0};
        e[i] = s.elem >= 0 ? a : (unsigned short)0;
      }
  }
  // the element, then the vector's first seven: byte 16*idx of the strip
  __device__ __forceinline__ void store(char* strip, const ConvStemPlan& p,
                                        int tid) const {
#pragma unroll
    for (int i = 0; i < kConvStemXVecs; i++) {
      const int idx = tid + i * kT;
      if (i < p.xvecs && idx < p.in_rows * p.nvec) {
        const u32x4 t = v[i];
        *reinterpret_cast<u32x4*>(strip + 16 * idx) =
            u32x4{(unsigned)e[i] | t.x << 16, t.x >> 16 | t.y << 16,
                  t.y >> 16 | t.z << 16, t.z >> 16 | t.w << 16};
      }
    }
  }
};

__global__ __launch_bounds__(kT, 2) void conv_stem_stats(
    const uint4* __restrict__ x, const uint4* __restrict__ w,
    uint4* __restrict__ y, float* __restrict__ part, ConvStemPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = kConvStemN;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;
  const int strip_bytes = p.in_rows * p.pitch;
  char* strips = reinterpret_cast<char*>(lds);
  const int strips_end = 2 * strip_bytes > kStemWVecs * 16 ? 2 * strip_bytes
                                                           : kStemWVecs * 16;
  uint4* stage = reinterpret_cast<uint4*>(strips + strips_end) + wave * 256;

  StemStage st;
  int band = split, buf = 0;  // split < bands
  st.load(x, p, band, tid);

  // The weight, once: raw into LDS, then every lane's 22 operands.
  for (int idx = tid; idx < kStemWVecs; idx += kT) lds[idx] = w[idx];
  __syncthreads();
  bf16x8 bw[2][kStemSteps];
  {
    const unsigned short* wl = reinterpret_cast<const unsigned short*>(lds);
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int u = 0; u < kStemSteps; u++) {
        const int group = 2 * u + h, r = group / 3, g = group - 3 * r;
        const unsigned short* src =
            wl + (32 * j + c) * kStemFilter + r * kStemRowElems + 8 * g;
        unsigned short el[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const bool real = r < kConvStemTaps && 8 * g + i < kStemRowElems;
          el[i] = real ? src[i] : (unsigned short)0;
        }
        const u32x4 t = {el[0] | (unsigned)el[1] << 16,
                         el[2] | (unsigned)el[3] << 16,
                         el[4] | (unsigned)el[5] << 16,
                         el[6] | (unsigned)el[7] << 16};
        bw[j][u] = __builtin_bit_cast(bf16x8, t);
      }
  }
  __syncthreads();  // the weight has been read: the strips may be written
  st.store(strips, p, tid);

  // The lane's moments are those of v - pivot, pivot the first value the lane
  // pushes, as in conv3x3_stats.
  Moments<2> mo;
  float pivot[2] = {0.f, 0.f};
  auto push = [&](const float (&v)[2]) __attribute__((always_inline)) {
    float d[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      pivot[j] = mo.n == 0.f ? v[j] : pivot[j];
      d[j] = v[j] - pivot[j];
    }
    mo.push(d);
  };

  while (band < p.bands) {
    const int nband = band + p.splits;
    const bool more = nband < p.bands;
    if (more) st.load(x, p, nband, tid);
    // buffer `buf` is written, and the other one, read a band ago, is free
    __syncthreads();
    const char* strip = strips + buf * strip_bytes;
    const ConvStemBand b = conv_stem_band(p, band);
    const int pixels = b.live * p.ow;
    const int row0 = (b.image * p.oh + b.oh0) * p.ow;  // the band's first pixel
    const int tiles = (pixels + kConvStemTile - 1) / kConvStemTile;
    for (int t = wave; t < tiles; t += 4) {
      // a lane past the band's last pixel computes that pixel once more
      const int pl = t * kConvStemTile + c;
      const char* a0 =
          strip + conv_stem_operand(p, pl < pixels ? pl : pixels - 1);
      f32x16 acc[2];
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.f;
      // the reads run three steps ahead of the MFMAs
      constexpr int kAhead = 3;
      u32x4 av[kAhead + 1];
      auto read = [&](int u) {
        // group 2u + h (the pad group 21 reads group 20 and is cleared): a
        // choice between two scalars, which costs no register for the walk
        const int last = kConvStemGroups - 2;
        const int off =
            h ? conv_stem_group_offset(p, 2 * u + 1 < last ? 2 * u + 1 : last)
              : conv_stem_group_offset(p, 2 * u);
        av[u & kAhead] = *reinterpret_cast<const u32x4_a4*>(a0 + off);
      };
#pragma unroll
      for (int u = 0; u < kAhead; u++) read(u);
#pragma unroll
      for (int u = 0; u < kStemSteps; u++) {
        if (u + kAhead < kStemSteps) read(u + kAhead);
        const u32x4 in = av[u & kAhead];
        // after unrolling each mask is a choice between two constants
        auto keep = [&](int dword) {
          return h ? conv_stem_keep(2 * u + 1, dword)
                   : conv_stem_keep(2 * u, dword);
        };
        const u32x4 a = {in.x & keep(0), in.y & keep(1), in.z & keep(2),
                         in.w & keep(3)};
#pragma unroll
        for (int j = 0; j < 2; j++)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(bf16x8, a), bw[j][u], acc[j], 0, 0, 0);
      }
      // round, push, store: as conv3x3_stats
      const int live = pixels - t * kConvStemTile < kConvStemTile
                           ? pixels - t * kConvStemTile
                           : kConvStemTile;
      unsigned pk[2][8];
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int e = 0; e < 8; e++)
          pk[j][e] = fwd_pack_bf16(acc[j][2 * e], acc[j][2 * e + 1]);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float lo[2], hi[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          lo[j] = __uint_as_float(pk[j][e] << 16);
          hi[j] = __uint_as_float(pk[j][e] & 0xffff0000u);
        }
        if (acc_row(2 * e, h) < live) push(lo);
        if (acc_row(2 * e + 1, h) < live) push(hi);
      }
      fwd_store_subtile(pk, stage, y, row0 + t * kConvStemTile, live, BN / 8,
                        0, lane);
    }
    // nothing that waits for the loads above may move up among the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    buf ^= 1;
    if (more) st.store(strips + buf * strip_bytes, p, tid);
    band = nband;
  }

  // The eight runs of every channel -> one partial, the tree of conv3x3_stats:
  // a merge keeps the pivot of its first run (of the second where the first
  // is empty) and moves the other mean there; the pivot is added at the end.
  __syncthreads();
  float* sc = reinterpret_cast<float*>(lds);
  const int run = wave * 2 + h;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    sc[run * BN + j * 32 + c] = mo.mean[j];
    sc[(8 + run) * BN + j * 32 + c] = mo.m2[j];
    sc[(16 + run) * BN + j * 32 + c] = pivot[j];
  }
  if (c == 0) sc[24 * BN + run] = mo.n;
  __syncthreads();
  if (tid < BN) {
    Moments<1> m[8];
    float pv[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
      m[r].n = sc[24 * BN + r];
      m[r].mean[0] = sc[r * BN + tid];
      m[r].m2[0] = sc[(8 + r) * BN + tid];
      pv[r] = sc[(16 + r) * BN + tid];
    }
#pragma unroll
    for (int step = 1; step < 8; step *= 2)
#pragma unroll
      for (int r = 0; r < 8; r += 2 * step) {
        pv[r] = m[r].n > 0.f ? pv[r] : pv[r + step];
        const float mb[1] = {m[r + step].n > 0.f
                                 ? (pv[r + step] - pv[r]) + m[r + step].mean[0]
                                 : 0.f};
        m[r].merge(m[r + step].n, mb, m[r + step].m2);
      }
    float* row = part + (int64_t)split * p.pstride;
    row[tid] = pv[0] + m[0].mean[0];
    row[BN + tid] = m[0].m2[0];
    if (tid == 0) row[2 * BN] = m[0].n;
  }
}

// ---- weight gradient ----------------------------------------------------------
//
// dW[64][147] = dY^T[64][R] * Xcol[R][147], contracted over the R output pixels
// (plan and layout of the planes: conv_stem_plan.h).
//
//   A   dY^T.  The band's pixels, contiguous in memory, are copied into a
//       wrw_cell<64> image and read transposed by wrw_operand<64>, as in
//       conv1x1_wrw and conv3x3_wrw.  A 16-deep step is 16 consecutive
//       pixels: group 2s in lane half 0, group 2s + 1 in half 1
//   B   lane (c, h) of column tile jk is column 32jk + c = 21r + 6a + q, and
//       its eight K values are eight consecutive bf16 of plane q, from element
//       ow0 + a + off(q) of strip row 2*ohl + r.  That run is only 2-byte
//       aligned where a + off(q) is odd, so the lane reads the five aligned
//       dwords around it and funnel-shifts them (four v_alignbit, by 0 or 16).
//       Per lane and tile the address is a constant plus the group's
//       2*ohl*row_bytes + 2*ow0: nothing but the group is worked out per step
//   C   every wave holds all ten 32 x 32 tiles, 160 registers, and the four
//       waves take the band's steps in turn: 2 A and 5 B operands feed ten
//       MFMAs.  At the end of the walk waves 1 .. 3 hand their tiles to wave
//       0 through LDS, which adds them in that order and stores the partial
//
// Staging.  A thread's unit of x is three 16-byte vectors, 24 elements, which
// are exactly four elements of each of the six planes: six 8-byte LDS writes.
// The first and last unit of every plane, and every unit of a strip row above
// or below the image, are written as zeros on every band; a read reaches at
// most element OW + 7 of a plane, the last of the last unit.  The next band
// waits in registers during the MFMAs of this one and goes to the other
// buffer after them: one barrier a band.
//
// Zeros.  The 13 pad columns and the half step past a band's last group are
// cleared by a select, the half step on both operands; what the cleared lanes
// read (the last real column's operand, the last group's, and for A whatever
// follows the pixels in the buffer) lies inside the buffer.  No data is ever
// multiplied by a zero that is not itself part of the convolution's padding.
//
// Every accumulator is one chain over the wave's steps in ascending order,
// the waves and the splits are added in a fixed order: the same bits each run.

struct StemWrwStage {
  u32x4 dyv[kConvStemWrwDyVecs];
  u32x4 xv[kConvStemWrwXUnits][3];

  __device__ __forceinline__ void load(const uint4* __restrict__ dy,
                                       const uint4* __restrict__ x,
                                       const ConvStemWrwPlan& p, int band,
                                       int tid) {
    const ConvStemBand b = conv_stem_wrw_band(p, band);
    const int vecs = b.live * p.ow * (kConvStemN / 8);
    const uint4* src = dy + (int64_t)(b.image * p.oh + b.oh0) * p.ow *
                                (kConvStemN / 8);
#pragma unroll
    for (int i = 0; i < kConvStemWrwDyVecs; i++)
      if (i < p.dyvecs) {  // uniform
        const int idx = tid + i * kT;
        const u32x4 t =
            *reinterpret_cast<const u32x4*>(src + (idx < vecs ? idx : 0));
        dyv[i] = idx < vecs ? t : u32x4{0, 0, 0, 0};
      }
    const int row_vecs = 3 * p.w / 8;
#pragma unroll
    for (int i = 0; i < kConvStemWrwXUnits; i++)
      if (i < p.xunits) {  // uniform
        // opaque, so that the source is worked out per band and not kept in
        // registers across the MFMAs (as StemStage::load)
        int idx = tid + i * kT;
        asm volatile("" : "+v"(idx));
        const int rr = conv_stem_div((unsigned)idx, p.magic_units);
        const int uu = idx - rr * p.units;
        const int ih = 2 * b.oh0 - 3 + rr;
        const bool live = rr < p.in_rows && ih >= 0 && ih < p.h && uu >= 1 &&
                          uu <= p.units - 2;
        const uint4* s =
            x + (live ? (int64_t)(b.image * p.h + ih) * row_vecs + 3 * (uu - 1)
                      : 0);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const u32x4 t = *reinterpret_cast<const u32x4*>(s + k);
          xv[i][k] = live ? t : u32x4{0, 0, 0, 0};
        }
      }
  }

  __device__ __forceinline__ void store(char* buf, const ConvStemWrwPlan& p,
                                        int tid) const {
#pragma unroll
    for (int i = 0; i < kConvStemWrwDyVecs; i++) {
      const int idx = tid + i * kT;
      if (i < p.dyvecs && idx < p.groups * 64)
        *reinterpret_cast<u32x4*>(buf + wrw_cell<64>(idx >> 3, (idx >> 2) & 1) +
                                  16 * (idx & 3)) = dyv[i];
    }
    char* planes = buf + p.dy_bytes;
#pragma unroll
    for (int i = 0; i < kConvStemWrwXUnits; i++) {
      const int idx = tid + i * kT;
      if (i < p.xunits && idx < p.in_rows * p.units) {
        const int rr = conv_stem_div((unsigned)idx, p.magic_units);
        const int uu = idx - rr * p.units;
        char* at = planes + rr * p.row_bytes + 8 * uu;
        // element k of the unit is strip position 24(uu-1) + 9 + k: plane
        // (k + 3) % 6, so plane q takes the elements (q + 3) % 6 + 6j
        auto el = [&](int k) {
          const unsigned d = xv[i][k >> 3][(k >> 1) & 3];
          return k & 1 ? d >> 16 : d & 0xffffu;
        };
#pragma unroll
        for (int q = 0; q < 6; q++) {
          const int k = (q + 3) % 6;
          typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
          *reinterpret_cast<u32x2*>(at + q * p.plane) =
              u32x2{el(k) | el(k + 6) << 16, el(k + 12) | el(k + 18) << 16};
        }
      }
    }
  }
};

__device__ __forceinline__ u32x4 stem_wrw_keep(bool keep, u32x4 v) {
  return keep ? v : u32x4{0, 0, 0, 0};
}

__global__ __launch_bounds__(kT) void conv_stem_wrw(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    float* __restrict__ part, ConvStemWrwPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int NT = kConvStemWrwCols / 32;  // column tiles
  char* bufs = reinterpret_cast<char*>(lds);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;

  // A: as conv1x1_wrw, lane 4q+pp of a 16-lane group supplies pixel 8h+q
  const int in_cell = 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  int an[2];
#pragma unroll
  for (int j = 0; j < 2; j++)
    an[j] = wrw_cell<64>(8 * h + ((lane >> 2) & 3), j) + in_cell;
  // B: the lane's column of each tile; a pad column reads the last real one
  int cb[NT], sh[NT];
#pragma unroll
  for (int jk = 0; jk < NT; jk++) {
    const int col = 32 * jk + c;
    const ConvStemWrwCol cc = conv_stem_wrw_col(
        p, col < kConvStemWrwReal ? col : kConvStemWrwReal - 1);
    cb[jk] = cc.byte, sh[jk] = cc.shift;
  }
  const bool real_last = 32 * (NT - 1) + c < kConvStemWrwReal;

  f32x16 acc[2][NT];
#pragma unroll
  for (int jm = 0; jm < 2; jm++)
#pragma unroll
    for (int jk = 0; jk < NT; jk++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[jm][jk][e] = 0.f;

  int band = conv_stem_wrw_first(p, split);  // < end: no split is empty
  const int end = conv_stem_wrw_end(p, split);
  int buf = 0;
  StemWrwStage st;
  st.load(dy, x, p, band, tid);
  st.store(bufs, p, tid);

  struct Ops {
    u32x4 a[2], b[NT];
  };
  while (band < end) {
    const bool more = band + 1 < end;
    if (more) st.load(dy, x, p, band + 1, tid);
    // buffer `buf` is written, and the other one, read a band ago, is free
    __syncthreads();
    char* img = bufs + buf * p.buf_bytes;
    const char* planes = img + p.dy_bytes;
    const int groups = conv_stem_wrw_band(p, band).live * p.gpr;
    const int steps = (groups + 1) / 2;

    auto read = [&](Ops& o, int s) __attribute__((always_inline)) {
      const int g = 2 * s + h;
      const bool live = g < groups;
      const int gc = live ? g : groups - 1;
      const int ohl = p.gpr > 1 ? conv_stem_div((unsigned)gc, p.magic_gpr) : gc;
      const char* xb =
          planes + 2 * ohl * p.row_bytes + 16 * (gc - ohl * p.gpr);
#pragma unroll
      for (int j = 0; j < 2; j++)
        o.a[j] = stem_wrw_keep(
            live, __builtin_bit_cast(u32x4, wrw_operand<64>(img, an[j], s)));
#pragma unroll
      for (int jk = 0; jk < NT; jk++) {
        const unsigned* d = reinterpret_cast<const unsigned*>(xb + cb[jk]);
        const unsigned d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
        const u32x4 t = {__builtin_amdgcn_alignbit(d1, d0, sh[jk]),
                         __builtin_amdgcn_alignbit(d2, d1, sh[jk]),
                         __builtin_amdgcn_alignbit(d3, d2, sh[jk]),
                         __builtin_amdgcn_alignbit(d4, d3, sh[jk])};
        o.b[jk] = stem_wrw_keep(live && (jk < NT - 1 || real_last), t);
      }
    };
    auto mma = [&](const Ops& o) __attribute__((always_inline)) {
#pragma unroll
      for (int jk = 0; jk < NT; jk++)
#pragma unroll
        for (int jm = 0; jm < 2; jm++)
          acc[jm][jk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(bf16x8, o.a[jm]),
              __builtin_bit_cast(bf16x8, o.b[jk]), acc[jm][jk], 0, 0, 0);
    };
    // two sets of operands: a step's reads are issued before the MFMAs of
    // the wave's step before it
    Ops o0, o1;
    int s = wave;
    if (s < steps) read(o0, s);
    for (; s + 4 < steps; s += 8) {
      read(o1, s + 4);
      mma(o0);
      if (s + 8 < steps) read(o0, s + 8);
      mma(o1);
    }
    if (s < steps) mma(o0);
    // nothing that waits for the loads above may move up among the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    buf ^= 1;
    if (more) st.store(bufs + buf * p.buf_bytes, p, tid);
    band++;
  }

  // waves 1 .. 3 -> wave 0, register i of lane l at [wave-1][i][l]
  __syncthreads();
  float* sum = reinterpret_cast<float*>(lds);
  constexpr int kRegs = 2 * NT * 16;
  if (wave > 0) {
#pragma unroll
    for (int jm = 0; jm < 2; jm++)
#pragma unroll
      for (int jk = 0; jk < NT; jk++)
#pragma unroll
        for (int e = 0; e < 16; e++)
          sum[((wave - 1) * kRegs + (jm * NT + jk) * 16 + e) * 64 + lane] =
              acc[jm][jk][e];
  }
  __syncthreads();
  if (wave == 0) {
    float* out = part + (int64_t)split * kConvStemN * kConvStemWrwCols;
#pragma unroll
    for (int jm = 0; jm < 2; jm++)
#pragma unroll
      for (int jk = 0; jk < NT; jk++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
          float v = acc[jm][jk][e];
#pragma unroll
          for (int w = 0; w < 3; w++)
            v += sum[(w * kRegs + (jm * NT + jk) * 16 + e) * 64 + lane];
          out[(32 * jm + acc_row(e, h)) * kConvStemWrwCols + 32 * jk + c] = v;
        }
  }
}

// dw[64][147] = bf16(part[0] + part[1] + ...) without the pad columns, by the
// lane groups of conv1x1_wrw_finalize: a vector of eight outputs is summed by
// 16 lanes, lane j of them adding the splits j*per .. (j+1)*per - 1 in index
// order, then the 16 sums as a tree over the lanes.  A wave takes four
// vectors; the waves past the last vector repeat it and store nothing.
__global__ __launch_bounds__(kT) void conv_stem_wrw_finalize(
    const float* __restrict__ part, uint4* __restrict__ dw, int splits) {
  constexpr int G = 16, VW = 64 / G;
  constexpr int kVecs = kConvStemN * kConvStemWrwReal / 8;
  static_assert(kConvStemN * kConvStemWrwReal % 8 == 0);
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * kT + threadIdx.x) >> 6;
  const int v = wave * VW + lane % VW;
  const int vc = v < kVecs ? v : kVecs - 1;
  const int j = lane / VW, per = (splits + G - 1) / G;
  const int s1 = (j + 1) * per < splits ? (j + 1) * per : splits;
  int at[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int o = 8 * vc + e, n = o / kConvStemWrwReal;
    at[e] = n * kConvStemWrwCols + o - n * kConvStemWrwReal;
  }
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = j * per; s < s1; s++) {
    const float* src = part + (int64_t)s * kConvStemN * kConvStemWrwCols;
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] += src[at[e]];
  }
  for (int off = 32; off >= VW; off >>= 1)
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] += __shfl_down(f[e], off);
  if (j == 0 && v < kVecs)
    dw[v] = make_uint4(fwd_pack_bf16(f[0], f[1]), fwd_pack_bf16(f[2], f[3]),
                       fwd_pack_bf16(f[4], f[5]), fwd_pack_bf16(f[6], f[7]));
}

}  // namespace

void launch_conv_stem_wrw(const ConvStemWrwPlan& p, const void* dy,
                          const void* x, float* part, void* dw,
                          hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv_stem_wrw: shape is not eligible");
  TORCH_CHECK(
      p.dyvecs <= kConvStemWrwDyVecs && p.xunits <= kConvStemWrwXUnits &&
          p.units == p.ow / 4 + 2 && p.plane == 8 * p.units &&
          p.row_bytes == 6 * p.plane && p.in_rows == 2 * p.band_rows + 5 &&
          p.gpr * 8 == p.ow && p.groups == p.band_rows * p.gpr &&
          p.dy_bytes == (p.groups + 1) / 2 * 16 * kConvStemN * 2 &&
          p.buf_bytes == p.dy_bytes + p.in_rows * p.row_bytes &&
          p.grid == p.splits &&
          (int64_t)(p.splits - 1) * p.bands_per_split < p.bands &&
          (int64_t)p.splits * p.bands_per_split >= p.bands &&
          p.lds_bytes >= 2 * p.buf_bytes &&
          p.lds_bytes >= kConvStemWrwSumBytes && p.lds_bytes <= kConvLdsBytes,
      "conv_stem_wrw: plan and kernel disagree");
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv_stem_wrw),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL(conv_stem_wrw, dim3(p.grid), dim3(kT), p.lds_bytes, stream,
                     static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x), part, p);
  CGX_HIP_CHECK(hipGetLastError());
  constexpr int kWaves = (kConvStemN * kConvStemWrwReal / 8 + 3) / 4;
  hipLaunchKernelGGL(conv_stem_wrw_finalize, dim3((kWaves + 3) / 4), dim3(kT),
                     0, stream, part, static_cast<uint4*>(dw), p.splits);
  CGX_HIP_CHECK(hipGetLastError());
}

void launch_conv_stem_stats(const ConvStemPlan& p, const void* x, const void* w,
                            void* y, float* part, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv_stem_stats: shape is not eligible");
  TORCH_CHECK(p.xvecs <= kConvStemXVecs && p.pitch == 16 * p.nvec &&
                  p.nvec == 3 * p.w / 8 + 3 && p.in_rows == 2 * p.band_rows + 5 &&
                  p.splits <= p.bands && p.grid == p.splits &&
                  p.pstride == 2 * kConvStemN + 1 &&
                  p.lds_bytes >= 2 * p.in_rows * p.pitch + kConvStageBytes &&
                  p.lds_bytes >= kStemWVecs * 16 + kConvStageBytes &&
                  p.lds_bytes <= kConvLdsBytes,
              "conv_stem_stats: plan and kernel disagree");
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv_stem_stats),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL(conv_stem_stats, dim3(p.grid), dim3(kT), p.lds_bytes,
                     stream, static_cast<const uint4*>(x),
                     static_cast<const uint4*>(w), static_cast<uint4*>(y), part,
                     p);
  CGX_HIP_CHECK(hipGetLastError());
}

}  // namespace cgx
