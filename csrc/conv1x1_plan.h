// Launch geometry of the 1x1-convolution forward that also produces the
// BatchNorm partials of its output (conv1x1_kernels.hip).
//
// Pure host arithmetic, like bn_plan.h.  The convolution is the GEMM
// Y[R, N] = X[R, K] * W[N, K]^T on a channels_last bf16 activation (R = N*H*W
// rows) and the convolution's weight, both with K contiguous.
//
// A 256-thread workgroup owns `bn` = 32*nt output channels (nt tiles of the
// 32x32x16 MFMA per wave) and walks 128-row tiles: wave w takes rows
// 32*w .. 32*w+31 of the tile.  K is cut into chunks of `kc`; the W tile of the
// workgroup ([bn, K], or one [bn, kc] chunk at a time where that does not fit)
// sits in LDS, X goes from global memory straight into the MFMA operand
// registers.  The grid is persistent: `splits` workgroups share one channel
// tile, workgroup `split` walks row tiles split, split+splits, ... and keeps
// each lane's running moments in registers across them, so a lane's run is
// 16 rows per tile it visits.  Each workgroup writes one partial row
// [mean(N) | M2(N) | count(ntiles)] of floats, which bn_stats_finalize merges
// (BnPartials in bn_plan.h).
#pragma once

#include <cstdint>

#include "bn_plan.h"

namespace cgx {

constexpr int kConvThreads = 256;
constexpr int kConvTileRows = 128;        // 4 waves x 32 rows
constexpr int kConvMaxNt = 8;             // 32-channel MFMA tiles per wave
constexpr int kConvCus = 256;
constexpr int kConvLdsBytes = 160 * 1024;
constexpr int kConvWLdsBytes = 128 * 1024;  // most of it for a resident W tile
constexpr int kConvStageBytes = 16 * 1024;  // 4 waves x [32 rows][64 channels]
// backward-data: the strips hold fp32, so that the skip gradient is added
// before the one rounding
constexpr int kConvBwdStageBytes = 32 * 1024;

struct Conv1x1Plan {
  int64_t rows = 0;  // R
  int k = 0, n = 0;
  bool eligible = false;
  bool native = false;  // measured faster than MIOpen + bn_stats at this shape
  int nt = 0;           // MFMA tiles across the workgroup's channels
  int bn = 0;           // channels per workgroup, 32*nt
  int ntiles = 0;       // workgroups across N
  int kc = 0;           // K chunk: 64 if K == 64, else 128
  int nchunks = 0;      // K / kc
  bool resident = false;  // the whole [bn, K] W tile stays in LDS
  int row_tiles = 0;      // ceil(R / 128)
  int splits = 0;         // persistent workgroups per channel tile
  int grid = 0;           // ntiles * splits
  int tiles_per_split = 0;  // longest walk
  int run = 0;              // per-lane run length: 16 * tiles_per_split
  int lds_bytes = 0;
  int pstride = 0;             // floats per partial row: 2*N + ntiles
  int64_t partial_floats = 0;  // splits * pstride
};

// K and N powers of two in [64, 2048], 2 <= R <= 2^24 (as bn_plan).
// `max_workgroups` > 0 caps the grid; here and below, values above 2^20 count
// as 2^20.
Conv1x1Plan conv1x1_plan(int64_t rows, int64_t k, int64_t n,
                         int64_t max_workgroups = 0);

// Backward-data of the same convolution, dX[R, K] = dY[R, N] * W[N, K], with
// the skip gradient of a residual fork optionally added in the epilogue
// (conv1x1_bwd_data in conv1x1_kernels.hip).  It is the forward GEMM with the
// roles of k and n exchanged: in the returned plan `k` is the contracted
// width (the convolution's N, the channels of dY) and `n` the produced one
// (the convolution's K, the channels of dX); `bn`, `ntiles` and the walk are
// over dX's channels.  There are no partials: run, pstride and partial_floats
// stay 0.  `native` comes from this problem's own measurement and depends on
// `with_add`.
Conv1x1Plan conv1x1_bwd_plan(int64_t rows, int64_t k, int64_t n, bool with_add,
                             int64_t max_workgroups = 0);

// Workgroup `wg` owns channels [n0, n0 + bn) and, as its i-th tile, the rows
// [row0, row1): the walk of the kernel and of the CPU replay.
__host__ __device__ inline int conv1x1_ntile(const Conv1x1Plan& p, int wg) {
  return wg % p.ntiles;
}
__host__ __device__ inline int conv1x1_split(const Conv1x1Plan& p, int wg) {
  return wg / p.ntiles;
}
// the i-th row tile of a split
__host__ __device__ inline int conv1x1_tile(const Conv1x1Plan& p, int split,
                                            int i) {
  return split + i * p.splits;
}

// The same two GEMMs for shapes whose B tile does not stay in LDS
// (gemm_walk_tiled in conv1x1_kernels.hip).  The workgroup's tile is 256 rows
// x `bn` = min(N, 128) channels: wave w takes rows 64*w .. 64*w+63 as two
// 32-row sub-tiles, so bn / tile rows <= 1/2.  B is staged one [bn, 64] chunk
// at a time into two LDS buffers, never resident: `kc` is 64, `resident`
// false, `lds_bytes` two chunks and the strips.  `run`, the per-lane run of
// the forward's moments, is 32 rows per tile visited.  The partials have the
// layout of conv1x1_plan.  `native` is this walk's own measurement against
// the path the shape takes without it.
constexpr int kTiledTileRows = 256;
constexpr int kTiledKc = 64;
constexpr int kTiledMaxNt = 4;

Conv1x1Plan conv1x1_tiled_plan(int64_t rows, int64_t k, int64_t n,
                               int64_t max_workgroups = 0);
Conv1x1Plan conv1x1_tiled_bwd_plan(int64_t rows, int64_t k, int64_t n,
                                   bool with_add, int64_t max_workgroups = 0);

// Workgroup `wg` of a tiled plan.  The workgroups of one split read the same
// rows of A once per channel tile, so they are given block indices 8 apart,
// which land on one XCD and share its L2, wherever the splits divide by 8
// (as conv1x1_wrw_tile); this is for speed only.  Its i-th row tile is
// conv1x1_tile, of kTiledTileRows rows.
__host__ __device__ inline int conv1x1_tiled_ntile(const Conv1x1Plan& p,
                                                   int wg) {
  return p.splits % 8 == 0 ? (wg / 8) % p.ntiles : wg % p.ntiles;
}
__host__ __device__ inline int conv1x1_tiled_split(const Conv1x1Plan& p,
                                                   int wg) {
  return p.splits % 8 == 0 ? (wg / 8 / p.ntiles) * 8 + wg % 8 : wg / p.ntiles;
}

// The partials of a [splits, 2N + ntiles] buffer as the finalize reads them.
inline BnPartials conv1x1_partials(const float* part, int n, int splits,
                                   int ntiles) {
  BnPartials q;
  q.mean = part;
  q.m2 = part + n;
  q.cnt = part + 2 * n;
  q.channels = n;
  q.splits = splits;
  q.tc = n / ntiles / 8;
  q.pstride = q.cstride = 2 * n + ntiles;
  return q;
}

// Backward-weights of the same convolution, dW[N, K] = dY[R, N]^T * X[R, K]
// (conv1x1_wrw in conv1x1_kernels.hip).  The contracted index R is the slow
// one of both operands.  A workgroup owns a bn x bk tile of dW (its four waves
// 2 x 2, each bn/2 x bk/2) and one of `splits` slices of the rows: it walks
// 64-row chunks split, split + splits, ... of dY's and X's channels of the
// tile, and writes its fp32 tile to part[split][N][K].  conv1x1_wrw_finalize
// sums the splits of an element in a fixed order and rounds once to bf16: no
// atomics, the same bits every run.
constexpr int kWrwChunkRows = 64;

struct Conv1x1WrwPlan {
  int64_t rows = 0;  // R
  int k = 0, n = 0;
  bool eligible = false;
  bool native = false;  // measured faster than MIOpen's fill + igemm + cast
  int bn = 0, bk = 0;   // the workgroup's tile of dW
  int ntiles_n = 0, ntiles_k = 0;
  int chunk_rows = 0;
  int row_chunks = 0;  // ceil(R / chunk_rows)
  int splits = 0;      // workgroups per channel tile
  int grid = 0;        // ntiles_n * ntiles_k * splits
  int chunks_per_split = 0;  // longest walk
  int lds_bytes = 0;
  int64_t partial_floats = 0;  // splits * N * K
};

// K and N powers of two in [64, 2048], 2 <= R <= kBnMaxRows, as the other two.
// `max_workgroups` > 0 caps the grid.
Conv1x1WrwPlan conv1x1_wrw_plan(int64_t rows, int64_t k, int64_t n,
                                int64_t max_workgroups = 0);

// Workgroup `wg` owns channel tile conv1x1_wrw_tile (tile t covers rows
// (t / ntiles_k) * bn of dW and columns (t % ntiles_k) * bk) and row slice
// conv1x1_wrw_split.  The workgroups of one slice read the same rows, so they
// are given block indices 8 apart, which land on one XCD and share its L2,
// wherever the splits divide by 8; this is for speed only.
__host__ __device__ inline int conv1x1_wrw_tiles(const Conv1x1WrwPlan& p) {
  return p.ntiles_n * p.ntiles_k;
}
__host__ __device__ inline int conv1x1_wrw_tile(const Conv1x1WrwPlan& p,
                                                int wg) {
  const int tiles = conv1x1_wrw_tiles(p);
  return p.splits % 8 == 0 ? (wg / 8) % tiles : wg % tiles;
}
__host__ __device__ inline int conv1x1_wrw_split(const Conv1x1WrwPlan& p,
                                                 int wg) {
  const int tiles = conv1x1_wrw_tiles(p);
  return p.splits % 8 == 0 ? (wg / 8 / tiles) * 8 + wg % 8 : wg / tiles;
}
// the i-th row chunk of a split; the walk ends at the first one >= row_chunks
__host__ __device__ inline int conv1x1_wrw_chunk(const Conv1x1WrwPlan& p,
                                                 int split, int i) {
  return split + i * p.splits;
}

// The same GEMM with the chunks loaded straight into a ring of LDS buffers
// (conv1x1_wrw_ring in conv1x1_kernels.hip), for the problems whose walk of
// few, large chunks leaves conv1x1_wrw waiting for memory once per chunk.
// Chunks, the walk (conv1x1_wrw_tile / _split / _chunk) and the partials are
// those above, so equal (bn, bk, splits) give equal bits.  The tile is always
// 128 x 128, so K and N are at least 128: the wider tiles measured no faster
// (benchmarks/RESULTS.md).  A stage of the ring holds one chunk of both
// operands, the n image first; `stages` of them are in flight, 128 KiB for
// one workgroup per CU, and the splits fill the CUs once.  `native` is the
// ring's own measurement against the path the problem takes without it.
constexpr int kWrwRingTile = 128;
constexpr int kWrwRingMaxStages = 4;

struct Conv1x1WrwRingPlan : Conv1x1WrwPlan {
  int stages = 0;
  int stage_bytes = 0;  // chunk_rows * (bn + bk) * 2; lds_bytes = stages * it
};

Conv1x1WrwRingPlan conv1x1_wrw_ring_plan(int64_t rows, int64_t k, int64_t n,
                                         int64_t max_workgroups = 0);

// A stage is filled by global_load_lds_dwordx4: one instruction of a wave
// writes 1 KiB of LDS, lane l the 16 bytes at 16*l from a base the wave
// shares.  So the permutation of the image's cells (wrw_cell in the kernel)
// goes onto the address each lane loads from: conv1x1_wrw_image_slot is the
// row of the chunk and the first of the eight channels that the image of a
// [64 rows][c channels] chunk holds at byte p, a multiple of 16.
struct WrwImageSlot {
  int row, channel;
};
__host__ __device__ inline WrwImageSlot conv1x1_wrw_image_slot(int c, int p) {
  const int line = p >> 8, col = (p >> 6) & 3, cells = c / 32;
  // the row of the line's first cell decides the XOR of the whole line
  const int swz = c == 64 ? line & 1 : (4 * line / cells) & 3;
  const int lin = 4 * line + (col ^ swz);
  return {lin / cells, 32 * (lin % cells) + 8 * ((p >> 4) & 3)};
}
// Where the j-th instruction of `wave` for one operand lands, in bytes from
// the start of that operand's image in the stage: the four waves take
// consecutive KiB.  An operand of c channels takes 64 * c / 2048 instructions
// of each wave.
__host__ __device__ inline int conv1x1_wrw_ring_piece(int wave, int j) {
  return (4 * j + wave) * 1024;
}
// ... and in bytes from the start of LDS, in stage `slot` of the ring;
// `operand` 0 is dY (bn channels), 1 is X (bk channels).
__host__ __device__ inline int conv1x1_wrw_ring_lds_base(
    const Conv1x1WrwRingPlan& p, int slot, int operand, int wave, int j) {
  return slot * p.stage_bytes + (operand ? p.chunk_rows * p.bn * 2 : 0) +
         conv1x1_wrw_ring_piece(wave, j);
}

// dw[N, K] bf16 from dy[R, N] and x[R, K] bf16 through part[splits, N, K]
// fp32, which needs no initialisation; every pointer 16-byte aligned.
void launch_conv1x1_wrw(const Conv1x1WrwPlan& p, const void* dy, const void* x,
                        float* part, void* dw, hipStream_t stream);
void launch_conv1x1_wrw_ring(const Conv1x1WrwRingPlan& p, const void* dy,
                             const void* x, float* part, void* dw,
                             hipStream_t stream);

// y[R, N] bf16 and part[splits, pstride] fp32 from x[R, K] and w[N, K] bf16;
// every pointer 16-byte aligned.
void launch_conv1x1_stats(const Conv1x1Plan& p, const void* x, const void* w,
                          void* y, float* part, hipStream_t stream);

// dx[R, K] = bf16(dy[R, N] * w[N, K] + skip[R, K]) for a plan of
// conv1x1_bwd_plan; skip may be null.  Every pointer 16-byte aligned.
void launch_conv1x1_bwd_data(const Conv1x1Plan& p, const void* dy,
                             const void* w, const void* skip, void* dx,
                             hipStream_t stream);

// The two above for a plan of conv1x1_tiled_plan / conv1x1_tiled_bwd_plan.
void launch_conv1x1_tiled_stats(const Conv1x1Plan& p, const void* x,
                                const void* w, void* y, float* part,
                                hipStream_t stream);
void launch_conv1x1_tiled_bwd_data(const Conv1x1Plan& p, const void* dy,
                                   const void* w, const void* skip, void* dx,
                                   hipStream_t stream);

}  // namespace cgx
