// The three GEMMs of a 1x1 / stride 1 convolution on channels_last bf16
// activations.  Geometry: conv1x1_plan.h.
//
// Forward and backward-data are one persistent walk, gemm_walk, of
// C[R, n] = A[R, k] * B[n, k]^T with two epilogues:
//
//   B   the workgroup's [bn, k] tile is copied to LDS once (or one [bn, kc]
//       chunk per step where it does not fit), rows XOR-swizzled so that the
//       ds_read_b128 of a B operand is conflict-free
//   A   each lane loads the 16 bytes of its A operand (row lane&31, k
//       8*(lane>>5) .. +7 of a 16-deep step) straight from global memory, one
//       chunk ahead of the MFMAs that use it
//   C   v_mfma_f32_32x32x16_bf16 leaves channel lane&31 of 16 rows in a lane;
//       the epilogue turns the tile into 16-byte row vectors through a
//       per-wave LDS strip of [32 rows][64 channels] and stores them
//
// Where B does not stay in LDS a second walk, gemm_walk_tiled, takes over
// (conv1x1_tiled_stats, conv1x1_tiled_bwd_data): taller tiles and B in two
// LDS buffers, the same epilogues and the same bits.
//
// conv1x1_stats is Y = X * W^T: its epilogue rounds the accumulators to bf16
// (as bf16_bits does) and the rounded values go into the lane's running
// moments, so that the output is never read back for the statistics of the
// BatchNorm that follows.  A lane keeps its moments across all tiles of its
// workgroup; at the end the eight runs of a channel (4 waves x 2 lane halves)
// merge as a tree in a fixed order.  conv1x1_bwd_data is dX = dY * W with W^T
// as B, transposed on the way into LDS; its epilogue can add a second tensor
// before the one rounding.  conv1x1_wrw, the weight gradient, contracts the
// rows and is an algorithm of its own.  No atomics anywhere: two runs give the
// same bits.
#include <hip/hip_runtime.h>

#include <type_traits>

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
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

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

// Vector u of the four that `lane` takes of the 256 16-byte vectors of a
// wave's [32 rows][64 channels] bf16 strip: vector q of the strip's `row`,
// which is vector g of a [R][8*nvec] tensor whose row r0 is the strip's first
// and whose vector cv its leftmost.
struct StripVec {
  int row, q;
  int64_t g;
};
__device__ inline StripVec strip_vec(int u, int lane, int64_t r0, int nvec,
                                     int cv) {
  const int idx = u * 64 + lane, row = idx >> 3, q = idx & 7;
  return {row, q, (r0 + row) * nvec + cv + q};
}

// The walk of a workgroup over the row tiles of its split, for the channels
// n0 .. n0 + 32*NT of C.  kStageB(dst, w, n0, width, kc, tid), stage_w or
// stage_wt, copies chunk kc of the workgroup's B tile from the weight `w`,
// `width` elements a row, to LDS at dst.  tile_done(t, r0, live, acc) takes
// the accumulators of row tile t: of the wave's 32 rows from r0 on, the first
// `live` exist.  tid and the wave, column c = lane & 31 and half h = lane >> 5
// it gives are the kernel's own values: defined once, they compile as if the
// walk were written out in the kernel.
template <int NT, int KC, bool RES, auto kStageB, typename TileDone>
__device__ __forceinline__ void gemm_walk(const uint4* am, const uint4* w,
                                          int width, int n0, uint4* lds,
                                          const Conv1x1Plan& p, int split,
                                          int tid, int wave, int c, int h,
                                          TileDone tile_done) {
  constexpr int cpr = KC / 8, steps = KC / 16;
  constexpr int wchunks = 32 * NT * cpr;  // 16-byte chunks of one chunk of B
  const int kvec = p.k / 8;

  if (RES) {
    for (int kc = 0; kc < p.nchunks; kc++)
      kStageB(lds + kc * wchunks, w, n0, width, kc, tid);
    __syncthreads();
  }

  // the lane's A row of row tile t; rows past R read row R-1 and are dropped
  auto a_row = [&](int t) {
    int64_t r = (int64_t)t * kConvTileRows + wave * 32 + c;
    r = r < p.rows ? r : p.rows - 1;
    return am + r * kvec;
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
      // the next chunk's A operands: of this tile, or the first of the next
      const uint4* src = kc + 1 < p.nchunks ? xr + (kc + 1) * cpr : xn;
#pragma unroll
      for (int s = 0; s < steps; s++) an[s] = src[2 * s + h];
      if (!RES) {
        __syncthreads();
        kStageB(lds, w, n0, width, kc, tid);
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
    tile_done(t, r0, (int)(p.rows - r0 < 32 ? p.rows - r0 : 32), acc);
  }
}

// ---- the tiled walk ---------------------------------------------------------
//
// The same GEMM for shapes whose B tile does not stay in LDS (plan:
// conv1x1_tiled_plan).  B goes to LDS one [bn, 64] chunk at a time into two
// buffers: a thread loads its share of chunk g+1 into registers before the
// MFMAs of chunk g and writes it to the other buffer after them, so the loads
// are in flight behind the MFMAs and one barrier per chunk orders both
// buffers.  The tile is 256 rows: a wave owns two 32-row sub-tiles, so every
// ds_read_b128 of B feeds two MFMAs and every A register NT of them, and the
// B bytes staged per tile are at most half the A bytes streamed.  Every
// accumulator is one chain over k in ascending order, as in gemm_walk: the
// same bits.
//
// A Stage is the share of a thread in one chunk of B held in registers:
// load() reads it from the weight, store() writes it to the swizzled image.
// StageW / StageWt move exactly what stage_w / stage_wt<NT, 64> move; those
// two cannot be used here because they wait for their loads before they
// return.
template <int NT>
struct StageW {
  unsigned v[NT][4];
  __device__ __forceinline__ void load(const uint4* __restrict__ w, int n0,
                                       int k, int chunk, int tid) {
#pragma unroll
    for (int i = 0; i < NT; i++) {
      const int idx = tid + i * kT, n = idx / 8, q = idx % 8;
      const uint4 t = w[((int64_t)(n0 + n) * k + chunk * kTiledKc) / 8 + q];
      v[i][0] = t.x, v[i][1] = t.y, v[i][2] = t.z, v[i][3] = t.w;
    }
  }
  __device__ __forceinline__ void store(uint4* dst, int tid) const {
#pragma unroll
    for (int i = 0; i < NT; i++) {
      const int idx = tid + i * kT;
      dst[w_slot<kTiledKc>(idx / 8, idx % 8)] =
          make_uint4(v[i][0], v[i][1], v[i][2], v[i][3]);
    }
  }
};

constexpr int kTiledSub = kTiledTileRows / kConvTileRows;  // sub-tiles a wave

// tile_done(t, r0, live, acc) is called once per 32-row sub-tile.  All waves
// of a workgroup run the same tiles and chunks, so each reaches every barrier.
template <int NT, typename Stage, typename TileDone>
__device__ __forceinline__ void gemm_walk_tiled(const uint4* am, const uint4* w,
                                                int width, int n0, uint4* lds,
                                                const Conv1x1Plan& p, int split,
                                                int tid, int wave, int c, int h,
                                                TileDone tile_done) {
  constexpr int cpr = kTiledKc / 8, steps = kTiledKc / 16;
  constexpr int wchunks = 32 * NT * cpr;  // 16-byte chunks of one chunk of B
  const int kvec = p.k / 8;

  // the lane's A row of sub-tile s of row tile t; rows past R read row R-1
  auto a_row = [&](int t, int s) {
    int64_t r = (int64_t)t * kTiledTileRows + (wave * kTiledSub + s) * 32 + c;
    r = r < p.rows ? r : p.rows - 1;
    return am + r * kvec;
  };

  Stage b;
  b.load(w, n0, width, 0, tid);
  // the A operands of two consecutive chunks: one multiplied, one in flight
  uint4 a[kTiledSub][steps], an[kTiledSub][steps];
  const uint4 *xr[kTiledSub], *xn[kTiledSub];
#pragma unroll
  for (int s = 0; s < kTiledSub; s++) {
    xr[s] = a_row(split, s);
#pragma unroll
    for (int q = 0; q < steps; q++) a[s][q] = xr[s][2 * q + h];
  }
  b.store(lds, tid);
  // An empty statement that uses the first A operands, so that the wait for
  // their loads stands here.  Without it every turn of the chunk loop below
  // waits for its own loads as if they were these.
#pragma unroll
  for (int s = 0; s < kTiledSub; s++)
#pragma unroll
    for (int q = 0; q < steps; q++) {
      u32x4 v = {a[s][q].x, a[s][q].y, a[s][q].z, a[s][q].w};
      asm volatile("" : "+v"(v));
      a[s][q] = make_uint4(v.x, v.y, v.z, v.w);
    }
  int buf = 0;  // the buffer that holds the chunk about to be multiplied

  for (int i = 0; i < p.tiles_per_split; i++) {
    const int t = conv1x1_tile(p, split, i);
    if (t >= p.row_tiles) break;
    const int tn = conv1x1_tile(p, split, i + 1);
    const bool has_next = tn < p.row_tiles;
#pragma unroll
    for (int s = 0; s < kTiledSub; s++) xn[s] = a_row(has_next ? tn : t, s);

    f32x16 acc[kTiledSub][NT];
#pragma unroll
    for (int s = 0; s < kTiledSub; s++)
#pragma unroll
      for (int j = 0; j < NT; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[s][j][e] = 0.f;

    for (int kc = 0; kc < p.nchunks; kc++) {
      // The next chunk of both operands (of this tile, or the first of the
      // next tile; the last chunk of the last tile has none) is loaded before
      // the MFMAs of this one: A into `an`, B into the Stage.
      const bool last = kc + 1 == p.nchunks;
      const bool more = !last || has_next;
#pragma unroll
      for (int s = 0; s < kTiledSub; s++) {
        const uint4* src = last ? xn[s] : xr[s] + (kc + 1) * cpr;
#pragma unroll
        for (int q = 0; q < steps; q++) an[s][q] = src[2 * q + h];
      }
      if (more) b.load(w, n0, width, last ? 0 : kc + 1, tid);
      // buffer `buf` is written, and the other one, read a chunk ago, is free
      __syncthreads();
      const uint4* wl = lds + buf * wchunks;
      uint4 bv[2][NT];  // the B operands of this 16-deep step and the next
#pragma unroll
      for (int j = 0; j < NT; j++)
        bv[0][j] = wl[w_slot<kTiledKc>(j * 32 + c, h)];
#pragma unroll
      for (int q = 0; q < steps; q++) {
        if (q + 1 < steps)
#pragma unroll
          for (int j = 0; j < NT; j++)
            bv[(q + 1) & 1][j] =
                wl[w_slot<kTiledKc>(j * 32 + c, 2 * (q + 1) + h)];
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
          for (int s = 0; s < kTiledSub; s++)
            acc[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                __builtin_bit_cast(bf16x8, a[s][q]),
                __builtin_bit_cast(bf16x8, bv[q & 1][j]), acc[s][j], 0, 0, 0);
      }
      // nothing that waits for the loads above may move up among the MFMAs
      __builtin_amdgcn_sched_barrier(0);
      buf ^= 1;
      if (more) b.store(lds + buf * wchunks, tid);
#pragma unroll
      for (int s = 0; s < kTiledSub; s++)
#pragma unroll
        for (int q = 0; q < steps; q++) a[s][q] = an[s][q];
    }
#pragma unroll
    for (int s = 0; s < kTiledSub; s++) {
      xr[s] = xn[s];
      const int64_t r0 =
          (int64_t)t * kTiledTileRows + (wave * kTiledSub + s) * 32;
      const int64_t left = p.rows - r0;
      tile_done(t, r0, (int)(left < 32 ? left : 32), acc[s]);
    }
  }
}

// gemm_walk, or gemm_walk_tiled with `Stage` in place of kStageB.
template <int NT, int KC, bool RES, bool TILED, auto kStageB, typename Stage,
          typename TileDone>
__device__ __forceinline__ void walk(const uint4* am, const uint4* w, int width,
                                     int n0, uint4* lds, const Conv1x1Plan& p,
                                     int split, int tid, int wave, int c, int h,
                                     TileDone tile_done) {
  if constexpr (TILED)
    gemm_walk_tiled<NT, Stage>(am, w, width, n0, lds, p, split, tid, wave, c,
                               h, tile_done);
  else
    gemm_walk<NT, KC, RES, kStageB>(am, w, width, n0, lds, p, split, tid, wave,
                                    c, h, tile_done);
}

// The forward with either walk: TILED is gemm_walk_tiled, and then KC is
// kTiledKc and RES false.
template <int NT, int KC, bool RES, bool TILED>
__device__ __forceinline__ void stats_body(const uint4* __restrict__ x,
                                           const uint4* __restrict__ w,
                                           uint4* __restrict__ y,
                                           float* __restrict__ part,
                                           const Conv1x1Plan& p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = 32 * NT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int ntile = TILED ? conv1x1_tiled_ntile(p, blockIdx.x)
                          : conv1x1_ntile(p, blockIdx.x);
  const int split = TILED ? conv1x1_tiled_split(p, blockIdx.x)
                          : conv1x1_split(p, blockIdx.x);
  const int n0 = ntile * BN;
  const int nvec = p.n / 8;
  uint4* stage =
      lds + (TILED ? 2 : RES ? p.nchunks : 1) * BN * (KC / 8) + wave * 256;
  unsigned* stage32 = reinterpret_cast<unsigned*>(stage);

  Moments<NT> st;
  walk<NT, KC, RES, TILED, &stage_w<NT, KC>, StageW<NT>>(
      x, w, p.k, n0, lds, p, split, tid, wave, c, h,
      [&](int, int64_t r0, int live, const f32x16(&acc)[NT])
          __attribute__((always_inline)) {
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

        // Two MFMA tiles (64 channels) at a time through the wave's strip:
        // lanes c and c^1 trade words so that the even lane writes channels
        // (c, c+1) of row 2e and the odd one channels (c-1, c) of row 2e+1.
        // Odd rows swap their 64-byte halves, which keeps both the 4-byte
        // writes and the 16-byte reads conflict-free.
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
              stage32[row * 32 + ((jj * 16 + (c >> 1)) ^ ((row & 1) << 4))] =
                  word;
            }
          asm volatile("" ::: "memory");
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const StripVec s = strip_vec(u, lane, r0, nvec, (n0 + jp * 64) / 8);
            const uint4 v = stage[s.row * 8 + (s.q ^ ((s.row & 1) << 2))];
            if (s.row < live) y[s.g] = v;
          }
          asm volatile("" ::: "memory");
          __builtin_amdgcn_wave_barrier();
        }
      });

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
__global__ __launch_bounds__(kT) void conv1x1_stats(
    const uint4* __restrict__ x, const uint4* __restrict__ w,
    uint4* __restrict__ y, float* __restrict__ part, Conv1x1Plan p) {
  stats_body<NT, KC, RES, false>(x, w, y, part, p);
}

template <int NT>
__global__ __launch_bounds__(kT) void conv1x1_tiled_stats(
    const uint4* __restrict__ x, const uint4* __restrict__ w,
    uint4* __restrict__ y, float* __restrict__ part, Conv1x1Plan p) {
  stats_body<NT, kTiledKc, false, true>(x, w, y, part, p);
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

// stage_wt<NT, 64> in two halves (see StageW): 32*NT threads take a block each.
template <int NT>
struct StageWt {
  unsigned r[8][4];
  __device__ __forceinline__ void load(const uint4* __restrict__ w, int k0,
                                       int kw, int chunk, int tid) {
    if (tid >= 32 * NT) return;
    const int n8 = tid & 7, k8 = tid >> 3;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint4 v =
          w[((int64_t)(chunk * kTiledKc + n8 * 8 + i) * kw + k0) / 8 + k8];
      r[i][0] = v.x, r[i][1] = v.y, r[i][2] = v.z, r[i][3] = v.w;
    }
  }
  __device__ __forceinline__ void store(uint4* dst, int tid) const {
    if (tid >= 32 * NT) return;
    const int n8 = tid & 7, k8 = tid >> 3;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
      unsigned o[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const unsigned a = r[2 * m][kk >> 1], b = r[2 * m + 1][kk >> 1];
        o[m] = kk & 1 ? (a >> 16) | (b & 0xffff0000u)
                      : (a & 0xffffu) | (b << 16);
      }
      dst[w_slot<kTiledKc>(k8 * 8 + kk, n8)] =
          make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
};

template <int NT, int KC, bool RES, bool ADD, bool TILED>
__device__ __forceinline__ void bwd_data_body(const uint4* __restrict__ dy,
                                              const uint4* __restrict__ w,
                                              const uint4* __restrict__ skip,
                                              uint4* __restrict__ dx,
                                              const Conv1x1Plan& p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = 32 * NT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int split = TILED ? conv1x1_tiled_split(p, blockIdx.x)
                          : conv1x1_split(p, blockIdx.x);
  const int n0 = (TILED ? conv1x1_tiled_ntile(p, blockIdx.x)
                        : conv1x1_ntile(p, blockIdx.x)) * BN;
  const int nvec = p.n / 8;
  // the wave's strip: [32 rows][64 channels] of fp32
  uint4* stage =
      lds + (TILED ? 2 : RES ? p.nchunks : 1) * BN * (KC / 8) + wave * 512;
  float* stagef = reinterpret_cast<float*>(stage);

  walk<NT, KC, RES, TILED, &stage_wt<NT, KC>, StageWt<NT>>(
      dy, w, p.n, n0, lds, p, split, tid, wave, c, h,
      [&](int, int64_t r0, int live, const f32x16(&acc)[NT])
          __attribute__((always_inline)) {
        // Two MFMA tiles (64 channels) at a time through the strip.  A 4-byte
        // write goes to bank (row's 64 + channel) % 32 from 32 lanes of one
        // row: no conflict.  Odd rows swap the 16-byte halves of every 32
        // bytes, which spreads the 16-byte reads of a lane group (rows r ..
        // r+3, half a row each) over all 64 banks.
#pragma unroll
        for (int jp = 0; jp < NT / 2; jp++) {
          const int cv = (n0 + jp * 64) / 8;
          uint4 sk[4];
          if (ADD) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const StripVec s = strip_vec(u, lane, r0, nvec, cv);
              sk[u] = make_uint4(0, 0, 0, 0);
              if (s.row < live) sk[u] = skip[s.g];
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
            const StripVec s = strip_vec(u, lane, r0, nvec, cv);
            const uint4 lo = stage[s.row * 16 + 2 * s.q + (s.row & 1)];
            const uint4 hi = stage[s.row * 16 + 2 * s.q + ((s.row & 1) ^ 1)];
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
            const uint4 v =
                make_uint4(pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]),
                           pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7]));
            if (s.row < live) dx[s.g] = v;
          }
          asm volatile("" ::: "memory");
          __builtin_amdgcn_wave_barrier();
        }
      });
}

template <int NT, int KC, bool RES, bool ADD>
__global__ __launch_bounds__(kT) void conv1x1_bwd_data(
    const uint4* __restrict__ dy, const uint4* __restrict__ w,
    const uint4* __restrict__ skip, uint4* __restrict__ dx, Conv1x1Plan p) {
  bwd_data_body<NT, KC, RES, ADD, false>(dy, w, skip, dx, p);
}

template <int NT, bool ADD>
__global__ __launch_bounds__(kT) void conv1x1_tiled_bwd_data(
    const uint4* __restrict__ dy, const uint4* __restrict__ w,
    const uint4* __restrict__ skip, uint4* __restrict__ dx, Conv1x1Plan p) {
  bwd_data_body<NT, kTiledKc, false, ADD, true>(dy, w, skip, dx, p);
}

// f(nt, kc, resident) with the plan's three as integral constants.
template <typename F>
void with_tile_constants(const Conv1x1Plan& p, F f) {
  auto with_nt = [&](auto nt) {
    using I64 = std::integral_constant<int, 64>;
    using I128 = std::integral_constant<int, 128>;
    if (p.kc == 64) f(nt, I64{}, std::true_type{});
    else if (p.resident) f(nt, I128{}, std::true_type{});
    else f(nt, I128{}, std::false_type{});
  };
  if (p.nt == 2) with_nt(std::integral_constant<int, 2>{});
  else if (p.nt == 4) with_nt(std::integral_constant<int, 4>{});
  else with_nt(std::integral_constant<int, 8>{});
}

// Launches an instantiation of one of the two kernels above, whose waves'
// strips take kStage bytes; the first launch of each raises its LDS limit.
template <auto kKernel, int kStage, typename... Args>
void launch_gemm(const Conv1x1Plan& p, hipStream_t stream, Args... args) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(kKernel),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvWLdsBytes + kStage);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL(kKernel, dim3(p.grid), dim3(kT), p.lds_bytes, stream,
                     args..., p);
  CGX_HIP_CHECK(hipGetLastError());
}

// ---- backward-weights -------------------------------------------------------
//
// dW[N, K] = sum_r dY[r, n] * X[r, k] (plan: conv1x1_wrw_plan).  The contracted
// index r is the slow one of both operands, so both MFMA operands are read
// transposed.  A 64-row chunk of the tile's BN channels of dY and BK channels
// of X is copied row by row into two LDS images; dY^T is the A operand and X
// the B operand of v_mfma_f32_32x32x16_bf16, whose lane l wants channel l & 31
// at the eight rows 8*(l >> 5) .. +7 of a 16-row step: two ds_read_b64_tr_b16,
// each taking per 16-lane group a block of 4 rows x 16 channels.
//
// Image of a [64 rows][C channels] chunk: 64-byte cells (32 channels) in
// 256-byte lines, cell u of row r at wrw_cell(r, u).  A transposed read of a
// 32-lane half takes one cell (its two groups the cell's two 32-byte halves)
// of the four rows 4m .. 4m+3, 8 bytes per lane: 256 bytes that must fall on
// the 64 banks once.  Bank = (byte / 4) % 64, so the four cells must sit in
// the four different 64-byte columns of a line:
//   C >= 128  a row is C/128 whole lines, its cell u in column u & 3; the XOR
//             with r & 3 moves the four rows to four different columns
//   C == 64   a line holds rows 2v, 2v+1, cell u of row r in column
//             2*(r & 1) + u; rows 4m, 4m+1 take columns {u, u+2} of their
//             line, and the XOR with (r >> 1) & 1 moves rows 4m+2, 4m+3 to
//             the other two
// The 16-byte writes of the copy fill whole lines from consecutive lanes and
// are conflict-free under any permutation of a line's cells.  Every address
// is a multiple of 8 and inside the image, and no branch that diverges within
// a wave encloses the reads: EXEC is all ones.
//
// The global loads of the next chunk are issued before the MFMAs of the
// current one and wait in registers; rows past R are loaded from row R-1 and
// replaced by zeros.  Each workgroup stores its fp32 tile to its split's
// plane of `part`; conv1x1_wrw_finalize sums the planes in a fixed order.

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

template <int C>
__device__ inline int wrw_cell(int r, int u) {
  const int lin = r * (C / 32) + u;
  const int swz = C == 64 ? (r >> 1) & 1 : r & 3;
  return 256 * (lin >> 2) + 64 * ((lin & 3) ^ swz);
}

// The chunk's rows r0 .. r0+63 of channels c0 .. c0+C of src[R, width]: thread
// tid's C/32 vectors.
template <int C>
__device__ inline void wrw_load(uint4 (&v)[C / 32], const uint4* __restrict__ src,
                                int width, int c0, int64_t r0, int64_t rows,
                                int tid) {
#pragma unroll
  for (int i = 0; i < C / 32; i++) {
    const int idx = tid + i * kT, row = idx / (C / 8), q = idx % (C / 8);
    const bool live = r0 + row < rows;
    const int64_t r = live ? r0 + row : rows - 1;
    const uint4 t = src[(r * width + c0) / 8 + q];
    v[i] = live ? t : make_uint4(0, 0, 0, 0);
  }
}

template <int C>
__device__ inline void wrw_store(char* img, const uint4 (&v)[C / 32], int tid) {
#pragma unroll
  for (int i = 0; i < C / 32; i++) {
    const int idx = tid + i * kT, row = idx / (C / 8), q = idx % (C / 8);
    *reinterpret_cast<uint4*>(img + wrw_cell<C>(row, q >> 2) + 16 * (q & 3)) =
        v[i];
  }
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

template <int BN, int BK>
__global__ __launch_bounds__(kT) void conv1x1_wrw(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    float* __restrict__ part, Conv1x1WrwPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int MT = BN / 64, KT = BK / 64;  // 32x32 tiles of a wave
  char* img_n = reinterpret_cast<char*>(lds);
  char* img_k = img_n + kWrwChunkRows * BN * 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int wn = wave >> 1, wk = wave & 1;
  const int tile = conv1x1_wrw_tile(p, blockIdx.x);
  const int split = conv1x1_wrw_split(p, blockIdx.x);
  const int n0 = (tile / p.ntiles_k) * BN, k0 = (tile % p.ntiles_k) * BK;

  // Lane 4q+pp of 16-lane group g supplies row q, channels 4pp .. 4pp+3 of the
  // group's block: rows 8h+q of the step's first read, channels 16*(g & 1) ..
  // of the cell.
  const int q = (lane >> 2) & 3;
  const int in_cell = 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  int an[MT], ak[KT];
#pragma unroll
  for (int j = 0; j < MT; j++)
    an[j] = wrw_cell<BN>(8 * h + q, wn * MT + j) + in_cell;
#pragma unroll
  for (int j = 0; j < KT; j++)
    ak[j] = wrw_cell<BK>(8 * h + q, wk * KT + j) + in_cell;

  f32x16 acc[MT][KT];
#pragma unroll
  for (int jm = 0; jm < MT; jm++)
#pragma unroll
    for (int jk = 0; jk < KT; jk++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[jm][jk][e] = 0.f;

  uint4 vn[BN / 32], vk[BK / 32];
  wrw_load<BN>(vn, dy, p.n, n0, (int64_t)split * kWrwChunkRows, p.rows, tid);
  wrw_load<BK>(vk, x, p.k, k0, (int64_t)split * kWrwChunkRows, p.rows, tid);

  for (int i = 0; i < p.chunks_per_split; i++) {
    if (conv1x1_wrw_chunk(p, split, i) >= p.row_chunks) break;
    __syncthreads();  // the previous chunk has been read
    wrw_store<BN>(img_n, vn, tid);
    wrw_store<BK>(img_k, vk, tid);
    __syncthreads();
    const int next = conv1x1_wrw_chunk(p, split, i + 1);
    if (next < p.row_chunks) {
      wrw_load<BN>(vn, dy, p.n, n0, (int64_t)next * kWrwChunkRows, p.rows, tid);
      wrw_load<BK>(vk, x, p.k, k0, (int64_t)next * kWrwChunkRows, p.rows, tid);
    }
#pragma unroll
    for (int s = 0; s < kWrwChunkRows / 16; s++) {
      bf16x8 a[MT], b[KT];
#pragma unroll
      for (int j = 0; j < MT; j++) a[j] = wrw_operand<BN>(img_n, an[j], s);
#pragma unroll
      for (int j = 0; j < KT; j++) b[j] = wrw_operand<BK>(img_k, ak[j], s);
#pragma unroll
      for (int jm = 0; jm < MT; jm++)
#pragma unroll
        for (int jk = 0; jk < KT; jk++)
          acc[jm][jk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              a[jm], b[jk], acc[jm][jk], 0, 0, 0);
    }
  }

  // lane (c, h) holds dW[n][k] for k = its column c and 16 rows n
  float* out = part + (int64_t)split * p.n * p.k;
#pragma unroll
  for (int jm = 0; jm < MT; jm++)
#pragma unroll
    for (int jk = 0; jk < KT; jk++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int n = n0 + (wn * MT + jm) * 32 + acc_row(e, h);
        const int k = k0 + (wk * KT + jk) * 32 + c;
        out[(int64_t)n * p.k + k] = acc[jm][jk][e];
      }
}

// dw[v] = bf16(part[0][v] + part[1][v] + ...) for the vectors v of eight
// elements, each summed by a group of g lanes (a power of two up to 16): lane
// j of the group adds the splits j*per .. (j+1)*per - 1 in index order, then
// the g sums are added as a tree over the lanes.  The order is fixed: two
// runs give the same bits.  A wave takes 64/g consecutive vectors and its
// lane l the vector l % (64/g) of them as j = l / (64/g), so that the lanes
// of one j read consecutive memory.  vecs * g is a multiple of the workgroup.
__global__ __launch_bounds__(kT) void conv1x1_wrw_finalize(
    const float4* __restrict__ part, uint4* __restrict__ dw, int splits,
    int64_t vecs, int g) {
  const int lane = threadIdx.x & 63, vw = 64 / g;
  const int64_t wave = ((int64_t)blockIdx.x * kT + threadIdx.x) >> 6;
  const int64_t v = wave * vw + lane % vw;
  const int j = lane / vw, per = (splits + g - 1) / g;
  const int s1 = (j + 1) * per < splits ? (j + 1) * per : splits;
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = j * per; s < s1; s++) {
    const float4 lo = part[(s * vecs + v) * 2];
    const float4 hi = part[(s * vecs + v) * 2 + 1];
    f[0] += lo.x, f[1] += lo.y, f[2] += lo.z, f[3] += lo.w;
    f[4] += hi.x, f[5] += hi.y, f[6] += hi.z, f[7] += hi.w;
  }
  for (int off = 32; off >= vw; off >>= 1)
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] += __shfl_down(f[e], off);
  if (j == 0)
    dw[v] = make_uint4(pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]),
                       pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7]));
}

// ---- backward-weights through a ring of LDS stages ---------------------------
//
// conv1x1_wrw with the chunks loaded straight into LDS (plan:
// conv1x1_wrw_ring_plan): the same images, transposed reads and MFMA order,
// so the same bits at the same tile and splits.  A stage of the ring is the
// two images of one chunk, filled by global_load_lds_dwordx4: no registers,
// and kStages stages stay in flight across the barriers.  Per stage:
//
//   s_waitcnt vmcnt(N)   the oldest stage of this wave has landed; N counts
//                        the instructions of the younger ones, kGlds each
//   s_barrier            ... and that of every wave
//   ds_read_b64_tr_b16, MFMAs
//   s_waitcnt lgkmcnt(0), s_barrier   every wave has read the stage
//   global_load_lds      stage t + kStages into the buffer just freed
//
// The loop is unrolled by kStages, so that every LDS address is a constant
// offset; there is no __syncthreads() and no load into registers while a
// stage is in flight, and the transposed reads are instructions of the
// kernel's own (wrw_read_tr), so that the compiler places no vmcnt(0) of its
// own anywhere in the loop.  A load cannot put zeros in place of rows past R:
// the chunk with those rows, the last of the workgroup that owns it, is
// staged through registers as in conv1x1_wrw, once the ring has drained.

typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(1))) const void global_cvoid;

template <int BN, int BK>
struct WrwRing {
  static constexpr int kStageBytes = kWrwChunkRows * (BN + BK) * 2;
  static constexpr int kStages =
      kConvLdsBytes / kStageBytes < kWrwRingMaxStages
          ? kConvLdsBytes / kStageBytes
          : kWrwRingMaxStages;
  static constexpr int kGlds = kStageBytes / 4096;  // of a wave, per stage
  static_assert(kStages >= 2 && (kStages - 1) * kGlds < 64);
};

template <int N>
__device__ inline void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int N>
__device__ inline void wait_lgkmcnt() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// wrw_operand's read at LDS address `addr` + OFF, as an instruction of the
// kernel's own.  The compiler orders a ds_read it knows of behind every
// pending global_load_lds with s_waitcnt vmcnt(0), which would drain the
// ring at each stage; this one it does not see, so the kernel waits for
// it itself (lgkmcnt, at most 15) before the MFMAs that take its result.
// Nothing but source order and the sched_barrier(0) after each wait keeps
// the MFMAs, and any copy of the result registers, behind that wait: after a
// change of toolchain read the .s again (the reads must land in the MFMAs'
// own operand registers, the MFMAs must follow the waits).
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
template <int OFF>
__device__ inline u32x2 wrw_read_tr(unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536);
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(v)
               : "v"(addr), "n"(OFF));
  return v;
}
// rows +0 .. +3 in elements 0 .. 3, rows +4 .. +7 in elements 4 .. 7
__device__ inline bf16x8 wrw_pair(const u32x2 (&v)[2]) {
  const u32x4 w = {v[0][0], v[0][1], v[1][0], v[1][1]};
  return __builtin_bit_cast(bf16x8, w);
}

// the wait before stage t of T: min(T - 1 - t, ST - 1) younger stages stay
template <int G, int ST>
__device__ inline void wrw_ring_wait(int left) {
  if (left >= ST - 1) wait_vmcnt<(ST - 1) * G>();
  else if (ST > 3 && left == 2) wait_vmcnt<2 * G>();
  else if (left == 1) wait_vmcnt<G>();
  else wait_vmcnt<0>();
}

// The chunk's rows r0 .. r0+63 of channels c0 .. c0+C of src[R, width] into
// the image at dst, which the wave shares.
template <int C>
__device__ inline void wrw_ring_issue(lds_char* dst, const uint4* __restrict__ src,
                                      int width, int c0, int64_t r0, int wave,
                                      int lane) {
  const uint4* base = src + (r0 * width + c0) / 8;
#pragma unroll
  for (int j = 0; j < kWrwChunkRows * C / 2048; j++) {
    const int piece = conv1x1_wrw_ring_piece(wave, j);
    const WrwImageSlot s = conv1x1_wrw_image_slot(C, piece + 16 * lane);
    __builtin_amdgcn_global_load_lds(
        (global_cvoid*)(base + (s.row * width + s.channel) / 8), dst + piece,
        16, 0, 0);
  }
}

template <int BN, int BK>
__global__ __launch_bounds__(kT) void conv1x1_wrw_ring(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    float* __restrict__ part, Conv1x1WrwRingPlan p) {
  extern __shared__ uint4 lds[];
  using G = WrwRing<BN, BK>;
  constexpr int MT = BN / 64, KT = BK / 64;  // 32x32 tiles of a wave
  constexpr int ST = G::kStages, SB = G::kStageBytes;
  char* ring = reinterpret_cast<char*>(lds);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  const int wn = wave >> 1, wk = wave & 1;
  const int tile = conv1x1_wrw_tile(p, blockIdx.x);
  const int split = conv1x1_wrw_split(p, blockIdx.x);
  const int n0 = (tile / p.ntiles_k) * BN, k0 = (tile % p.ntiles_k) * BK;

  // as conv1x1_wrw
  const int q = (lane >> 2) & 3;
  const int in_cell = 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  int an[MT], ak[KT];
#pragma unroll
  for (int j = 0; j < MT; j++)
    an[j] = wrw_cell<BN>(8 * h + q, wn * MT + j) + in_cell;
#pragma unroll
  for (int j = 0; j < KT; j++)
    ak[j] = wrw_cell<BK>(8 * h + q, wk * KT + j) + in_cell;

  f32x16 acc[MT][KT];
#pragma unroll
  for (int jm = 0; jm < MT; jm++)
#pragma unroll
    for (int jk = 0; jk < KT; jk++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[jm][jk][e] = 0.f;

  // the chunks split, split + splits, ... below row_chunks; the last one is
  // left to the end where it has rows past R
  const int mine = (p.row_chunks - split + p.splits - 1) / p.splits;
  const bool tail = p.rows % kWrwChunkRows != 0 &&
                    conv1x1_wrw_chunk(p, split, mine - 1) == p.row_chunks - 1;
  const int T = mine - (tail ? 1 : 0);

  auto issue = [&](int t, int slot) {
    const int64_t r0 =
        (int64_t)conv1x1_wrw_chunk(p, split, t) * kWrwChunkRows;
    lds_char* dst = (lds_char*)ring + slot * SB;
    wrw_ring_issue<BN>(dst, dy, p.n, n0, r0, wave, lane);
    wrw_ring_issue<BK>(dst + kWrwChunkRows * BN * 2, x, p.k, k0, r0, wave,
                       lane);
  };
  // The 16-row steps of the images at LDS addresses img_n and img_k.  The
  // reads of step s+1 are issued before the MFMAs of step s and waited for
  // by count, by hand: see wrw_read_tr.
  const unsigned ring_addr = (unsigned)(unsigned long)(lds_char*)ring;
  auto steps = [&](unsigned img_n, unsigned img_k) {
    constexpr int NS = kWrwChunkRows / 16;
    u32x2 a[2][MT][2], b[2][KT][2];
    unsigned pn[MT], pk[KT];
#pragma unroll
    for (int j = 0; j < MT; j++) pn[j] = img_n + an[j];
#pragma unroll
    for (int j = 0; j < KT; j++) pk[j] = img_k + ak[j];
    auto read = [&](auto step) {
      constexpr int s = decltype(step)::value;
#pragma unroll
      for (int j = 0; j < MT; j++) {
        a[s & 1][j][0] = wrw_read_tr<s * 32 * BN>(pn[j]);
        a[s & 1][j][1] = wrw_read_tr<s * 32 * BN + 8 * BN>(pn[j]);
      }
#pragma unroll
      for (int j = 0; j < KT; j++) {
        b[s & 1][j][0] = wrw_read_tr<s * 32 * BK>(pk[j]);
        b[s & 1][j][1] = wrw_read_tr<s * 32 * BK + 8 * BK>(pk[j]);
      }
    };
    auto step_at = [&](auto self, auto step) {
      constexpr int s = decltype(step)::value;
      if constexpr (s < NS) {
        if constexpr (s + 1 < NS) {
          read(std::integral_constant<int, s + 1>{});
          wait_lgkmcnt<2 * (MT + KT)>();
        } else {
          wait_lgkmcnt<0>();
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int jm = 0; jm < MT; jm++)
#pragma unroll
          for (int jk = 0; jk < KT; jk++)
            acc[jm][jk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                wrw_pair(a[s & 1][jm]), wrw_pair(b[s & 1][jk]), acc[jm][jk], 0,
                0, 0);
        __builtin_amdgcn_sched_barrier(0);
        self(self, std::integral_constant<int, s + 1>{});
      }
    };
    read(std::integral_constant<int, 0>{});
    step_at(step_at, std::integral_constant<int, 0>{});
  };

#pragma unroll
  for (int s = 0; s < ST; s++)
    if (s < T) issue(s, s);
  for (int t0 = 0; t0 < T; t0 += ST) {
#pragma unroll
    for (int s = 0; s < ST; s++) {
      const int t = t0 + s;
      if (t >= T) break;
      wrw_ring_wait<G::kGlds, ST>(T - 1 - t);
      __builtin_amdgcn_s_barrier();
      steps(ring_addr + s * SB, ring_addr + s * SB + kWrwChunkRows * BN * 2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (t + ST < T) issue(t + ST, s);
    }
  }
  if (tail) {
    // nothing is in flight and every wave is past its last read
    uint4 vn[BN / 32], vk[BK / 32];
    const int64_t r0 = (int64_t)(p.row_chunks - 1) * kWrwChunkRows;
    wrw_load<BN>(vn, dy, p.n, n0, r0, p.rows, tid);
    wrw_load<BK>(vk, x, p.k, k0, r0, p.rows, tid);
    wrw_store<BN>(ring, vn, tid);
    wrw_store<BK>(ring + kWrwChunkRows * BN * 2, vk, tid);
    __syncthreads();
    steps(ring_addr, ring_addr + kWrwChunkRows * BN * 2);
  }

  float* out = part + (int64_t)split * p.n * p.k;
#pragma unroll
  for (int jm = 0; jm < MT; jm++)
#pragma unroll
    for (int jk = 0; jk < KT; jk++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int n = n0 + (wn * MT + jm) * 32 + acc_row(e, h);
        const int k = k0 + (wk * KT + jk) * 32 + c;
        out[(int64_t)n * p.k + k] = acc[jm][jk][e];
      }
}

template <int BN, int BK>
void launch_wrw(const Conv1x1WrwPlan& p, const void* dy, const void* x,
                float* part, hipStream_t stream) {
  hipLaunchKernelGGL((conv1x1_wrw<BN, BK>), dim3(p.grid), dim3(kT),
                     p.lds_bytes, stream, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x), part, p);
}

template <int BN>
void launch_wrw_bn(const Conv1x1WrwPlan& p, const void* dy, const void* x,
                   float* part, hipStream_t stream) {
  if (p.bk == 64) launch_wrw<BN, 64>(p, dy, x, part, stream);
  else if (p.bk == 128) launch_wrw<BN, 128>(p, dy, x, part, stream);
  else if constexpr (BN < 256) launch_wrw<BN, 256>(p, dy, x, part, stream);
  else TORCH_CHECK(false, "conv1x1_wrw: no 256 x 256 tile");
}

template <int BN, int BK>
void launch_wrw_ring(const Conv1x1WrwRingPlan& p, const void* dy,
                     const void* x, float* part, hipStream_t stream) {
  using G = WrwRing<BN, BK>;
  TORCH_CHECK(p.bn == BN && p.bk == BK && p.stages == G::kStages &&
                  p.lds_bytes == G::kStages * G::kStageBytes,
              "conv1x1_wrw_ring: plan and kernel disagree on the ring");
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv1x1_wrw_ring<BN, BK>),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL((conv1x1_wrw_ring<BN, BK>), dim3(p.grid), dim3(kT),
                     p.lds_bytes, stream, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x), part, p);
  CGX_HIP_CHECK(hipGetLastError());
}

// the sum of the planes that either kernel wrote
void launch_wrw_finalize(const Conv1x1WrwPlan& p, const float* part, void* dw,
                         hipStream_t stream) {
  // lanes per vector: as many as the splits give work to, until the grid
  // has four waves for every SIMD
  const int64_t vecs = (int64_t)p.n * p.k / 8;
  int g = 1;
  while (g < 16 && 2 * g <= p.splits && vecs * g < 4 * kConvCus * kT) g *= 2;
  hipLaunchKernelGGL(conv1x1_wrw_finalize, dim3((unsigned)(vecs * g / kT)),
                     dim3(kT), 0, stream,
                     reinterpret_cast<const float4*>(part),
                     static_cast<uint4*>(dw), p.splits, vecs, g);
  CGX_HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_conv1x1_wrw(const Conv1x1WrwPlan& p, const void* dy, const void* x,
                        float* part, void* dw, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1_wrw: shape is not eligible");
  if (p.bn == 64) launch_wrw_bn<64>(p, dy, x, part, stream);
  else if (p.bn == 128) launch_wrw_bn<128>(p, dy, x, part, stream);
  else launch_wrw_bn<256>(p, dy, x, part, stream);
  CGX_HIP_CHECK(hipGetLastError());
  launch_wrw_finalize(p, part, dw, stream);
}

void launch_conv1x1_wrw_ring(const Conv1x1WrwRingPlan& p, const void* dy,
                             const void* x, float* part, void* dw,
                             hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1_wrw_ring: shape is not eligible");
  launch_wrw_ring<kWrwRingTile, kWrwRingTile>(p, dy, x, part, stream);
  launch_wrw_finalize(p, part, dw, stream);
}

void launch_conv1x1_bwd_data(const Conv1x1Plan& p, const void* dy,
                             const void* w, const void* skip, void* dx,
                             hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1_bwd_data: shape is not eligible");
  with_tile_constants(p, [&](auto nt, auto kc, auto res) {
    auto launch = [&](auto add) {
      launch_gemm<&conv1x1_bwd_data<decltype(nt)::value, decltype(kc)::value,
                                    decltype(res)::value,
                                    decltype(add)::value>,
                  kConvBwdStageBytes>(
          p, stream, static_cast<const uint4*>(dy),
          static_cast<const uint4*>(w), static_cast<const uint4*>(skip),
          static_cast<uint4*>(dx));
    };
    if (skip) launch(std::true_type{});
    else launch(std::false_type{});
  });
}

void launch_conv1x1_stats(const Conv1x1Plan& p, const void* x, const void* w,
                          void* y, float* part, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1_stats: shape is not eligible");
  with_tile_constants(p, [&](auto nt, auto kc, auto res) {
    launch_gemm<&conv1x1_stats<decltype(nt)::value, decltype(kc)::value,
                               decltype(res)::value>,
                kConvStageBytes>(p, stream, static_cast<const uint4*>(x),
                                 static_cast<const uint4*>(w),
                                 static_cast<uint4*>(y), part);
  });
}

void launch_conv1x1_tiled_stats(const Conv1x1Plan& p, const void* x,
                                const void* w, void* y, float* part,
                                hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1_tiled_stats: shape is not eligible");
  auto launch = [&](auto nt) {
    launch_gemm<&conv1x1_tiled_stats<decltype(nt)::value>, kConvStageBytes>(
        p, stream, static_cast<const uint4*>(x), static_cast<const uint4*>(w),
        static_cast<uint4*>(y), part);
  };
  if (p.nt == 2) launch(std::integral_constant<int, 2>{});
  else launch(std::integral_constant<int, 4>{});
}

void launch_conv1x1_tiled_bwd_data(const Conv1x1Plan& p, const void* dy,
                                   const void* w, const void* skip, void* dx,
                                   hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv1x1_tiled_bwd_data: shape is not eligible");
  auto launch = [&](auto nt, auto add) {
    launch_gemm<&conv1x1_tiled_bwd_data<decltype(nt)::value,
                                        decltype(add)::value>,
                kConvBwdStageBytes>(
        p, stream, static_cast<const uint4*>(dy), static_cast<const uint4*>(w),
        static_cast<const uint4*>(skip), static_cast<uint4*>(dx));
  };
  auto with_nt = [&](auto nt) {
    if (skip) launch(nt, std::true_type{});
    else launch(nt, std::false_type{});
  };
  if (p.nt == 2) with_nt(std::integral_constant<int, 2>{});
  else with_nt(std::integral_constant<int, 4>{});
}

}  // namespace cgx
