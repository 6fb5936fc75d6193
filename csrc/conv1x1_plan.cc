// Launch geometry of the 1x1 convolution with statistics: see conv1x1_plan.h.
#include "conv1x1_plan.h"

#include <algorithm>

namespace cgx {
namespace {

// The shapes at which the native kernel plus finalize beat MIOpen's forward
// plus bn_stats plus finalize in every run of an alternating measurement on
// MI355X (slowest native run faster than the fastest MIOpen run; table in
// benchmarks/RESULTS.md).  Measured at these row counts only, so only they go
// native; the five other stride-1 1x1 problems of ResNet-50 at batch 256
// (512->256, 1024->256, 1024->512, 512->2048, 2048->512), where W does not
// stay in LDS, lost and stay with MIOpen.
struct Measured {
  int k, n;
  int64_t rows;
  bool with_add = false;  // backward-data only
};
constexpr Measured kNative[] = {
    {64, 64, 802816},   {64, 256, 802816},  {256, 64, 802816},
    {256, 128, 802816}, {128, 512, 200704}, {512, 128, 200704},
    {256, 1024, 50176},
};

template <size_t N>
bool measured_faster(const Measured (&table)[N], int64_t rows, int64_t k,
                     int64_t n, bool with_add = false) {
  for (const Measured& m : table)
    if (m.k == k && m.n == n && m.rows == rows && m.with_add == with_add)
      return true;
  return false;
}

bool pow2_in(int64_t v, int64_t lo, int64_t hi) {
  return v >= lo && v <= hi && (v & (v - 1)) == 0;
}

// what all three kernels take
bool shape_ok(int64_t rows, int64_t k, int64_t n) {
  return pow2_in(k, 64, 2048) && pow2_in(n, 64, 2048) && rows >= 2 &&
         rows <= kBnMaxRows;
}

// `max_workgroups` > 0 caps the grid of `tiles` channel tiles
int64_t cap_splits(int64_t splits, int tiles, int64_t max_workgroups) {
  if (max_workgroups <= 0) return splits;
  max_workgroups = std::min<int64_t>(max_workgroups, 1 << 20);
  return std::min(splits, std::max<int64_t>(1, max_workgroups / tiles));
}

// The backward-data problems (dX K wide, dY N wide, with or without the skip
// gradient added) that met the same rule against MIOpen's backward-data plus,
// with a skip gradient, the bf16 add that follows it (benchmarks/RESULTS.md):
// the eight of ResNet-50's twelve at batch 256 whose W^T tile stays in LDS.
// 1024->512 and 2048->512 with the add, 256->1024 and 512->2048 without, lost.
constexpr Measured kNativeBwd[] = {
    {64, 64, 802816, true},    {256, 64, 802816, true},
    {256, 128, 802816, true},  {512, 128, 200704, true},
    {512, 256, 200704, true},  {1024, 256, 50176, true},
    {64, 256, 802816, false},  {128, 512, 200704, false},
};

// The tiles of a GEMM with p.k contracted and p.n produced; `stage_bytes` of
// LDS go to the waves' output strips.
void tile_geometry(Conv1x1Plan& p, int stage_bytes) {
  p.nt = std::min(p.n / 32, kConvMaxNt);
  p.bn = 32 * p.nt;
  p.ntiles = p.n / p.bn;
  p.kc = p.k == 64 ? 64 : 128;
  p.nchunks = p.k / p.kc;
  p.resident = p.bn * p.k * 2 <= kConvWLdsBytes;
  p.lds_bytes = p.bn * (p.resident ? p.k : p.kc) * 2 + stage_bytes;
  p.row_tiles = (int)((p.rows + kConvTileRows - 1) / kConvTileRows);
}

// as many workgroups per CU as LDS and the registers (`by_regs` waves per
// SIMD) allow
int64_t splits_by_occupancy(const Conv1x1Plan& p, int by_regs) {
  const int per_cu = std::max(1, std::min(kConvLdsBytes / p.lds_bytes, by_regs));
  return std::min<int64_t>(p.row_tiles,
                           std::max(1, kConvCus * per_cu / p.ntiles));
}

void set_grid(Conv1x1Plan& p, int64_t splits, int64_t max_workgroups) {
  p.splits = (int)cap_splits(splits, p.ntiles, max_workgroups);
  p.grid = p.ntiles * p.splits;
  p.tiles_per_split = (p.row_tiles + p.splits - 1) / p.splits;
}

// The backward-weights problems (K, N, rows) at which conv1x1_wrw plus its
// finalize met the same rule against MIOpen's workspace fill, igemm_wrw and
// cast (benchmarks/RESULTS.md): eleven of ResNet-50's twelve at batch 256.
// At 64->64 the ranges of the two overlap, and it stays stock.
constexpr Measured kNativeWrw[] = {
    {64, 256, 802816},  {256, 64, 802816},  {256, 128, 802816},
    {128, 512, 200704}, {512, 128, 200704}, {512, 256, 200704},
    {256, 1024, 50176}, {1024, 256, 50176}, {1024, 512, 50176},
    {512, 2048, 12544}, {2048, 512, 12544},
};

// The backward-weights problems at which conv1x1_wrw_ring met the same rule
// against conv1x1_wrw, both with the finalize (benchmarks/RESULTS.md,
// measured with benchmarks/conv1x1_wrw_ring_shapes.py): all nine of the twelve
// that have 128 channels on both sides.
constexpr Measured kNativeWrwRing[] = {
    {256, 128, 802816}, {128, 512, 200704}, {512, 128, 200704},
    {512, 256, 200704}, {256, 1024, 50176}, {1024, 256, 50176},
    {1024, 512, 50176}, {512, 2048, 12544}, {2048, 512, 12544},
};

// The tiled walk's own tables, by the same rule against the path each problem
// takes without it: the kernel of kNative / kNativeBwd where that lists the
// problem, else MIOpen's forward plus bn_stats, or its backward-data plus,
// with a skip gradient, the bf16 add (benchmarks/RESULTS.md, measured with
// benchmarks/conv1x1_tiled_shapes.py).  Measured at these row counts only.
// Forward: the five problems whose W tile does not stay in LDS; where it
// stays, the resident kernel's ranges overlap this walk's or lie below them.
constexpr Measured kNativeTiled[] = {
    {512, 256, 200704},  {1024, 256, 50176}, {1024, 512, 50176},
    {512, 2048, 12544},  {2048, 512, 12544},
};
// Backward-data: all eight problems MIOpen had kept at 14x14 and 7x7 and
// eight more that kNativeBwd does not list, sixteen of the twenty-four.
constexpr Measured kNativeTiledBwd[] = {
    {64, 64, 802816, false},    {64, 256, 802816, true},
    {256, 64, 802816, false},   {256, 128, 802816, false},
    {128, 512, 200704, true},   {512, 128, 200704, false},
    {512, 256, 200704, false},  {256, 1024, 50176, false},
    {256, 1024, 50176, true},   {1024, 256, 50176, false},
    {1024, 512, 50176, false},  {1024, 512, 50176, true},
    {512, 2048, 12544, false},  {512, 2048, 12544, true},
    {2048, 512, 12544, false},  {2048, 512, 12544, true},
};

// The geometry both tiled plans share: 256-row tiles of min(n, 128) produced
// channels, two [bn, 64] chunks of B and the strips in LDS, and the splits a
// multiple of 8 where there are more than 8 (conv1x1_tiled_split).
void tiled_geometry(Conv1x1Plan& p, int stage_bytes, int64_t splits_cap,
                    int64_t max_workgroups) {
  p.nt = std::min(p.n / 32, kTiledMaxNt);
  p.bn = 32 * p.nt;
  p.ntiles = p.n / p.bn;
  p.kc = kTiledKc;
  p.nchunks = p.k / p.kc;
  p.resident = false;
  p.lds_bytes = 2 * p.bn * p.kc * 2 + stage_bytes;
  p.row_tiles = (int)((p.rows + kTiledTileRows - 1) / kTiledTileRows);
  // the registers of a wave with eight accumulator tiles leave one wave per
  // SIMD, with four two
  int64_t splits =
      std::min(splits_by_occupancy(p, p.nt == 4 ? 1 : 2), splits_cap);
  // ... unless that makes the longest walk a tile longer
  const int64_t by8 = splits - splits % 8;
  if (splits > 8 &&
      (p.row_tiles + by8 - 1) / by8 == (p.row_tiles + splits - 1) / splits)
    splits = by8;
  set_grid(p, splits, max_workgroups);
}

}  // namespace

Conv1x1Plan conv1x1_tiled_plan(int64_t rows, int64_t k, int64_t n,
                               int64_t max_workgroups) {
  Conv1x1Plan p;
  p.rows = rows;
  p.eligible = shape_ok(rows, k, n);
  if (!p.eligible) return p;
  p.k = (int)k;
  p.n = (int)n;
  p.native = measured_faster(kNativeTiled, rows, k, n);
  // the partials within 5% of the output's bytes, as in conv1x1_plan
  tiled_geometry(p, kConvStageBytes, std::max<int64_t>(1, rows / 82),
                 max_workgroups);
  p.run = 32 * p.tiles_per_split;
  p.pstride = 2 * p.n + p.ntiles;
  p.partial_floats = (int64_t)p.splits * p.pstride;
  return p;
}

Conv1x1Plan conv1x1_tiled_bwd_plan(int64_t rows, int64_t k, int64_t n,
                                   bool with_add, int64_t max_workgroups) {
  Conv1x1Plan p;
  p.rows = rows;
  p.eligible = shape_ok(rows, k, n);
  if (!p.eligible) return p;
  p.k = (int)n;  // contracted: the width of dY
  p.n = (int)k;  // produced: the width of dX
  p.native = measured_faster(kNativeTiledBwd, rows, k, n, with_add);
  tiled_geometry(p, kConvBwdStageBytes, rows, max_workgroups);
  return p;
}

Conv1x1WrwPlan conv1x1_wrw_plan(int64_t rows, int64_t k, int64_t n,
                                int64_t max_workgroups) {
  Conv1x1WrwPlan p;
  p.rows = rows;
  p.eligible = shape_ok(rows, k, n);
  if (!p.eligible) return p;
  p.k = (int)k;
  p.n = (int)n;
  p.native = measured_faster(kNativeWrw, rows, k, n);
  p.chunk_rows = kWrwChunkRows;
  p.row_chunks = (int)((rows + kWrwChunkRows - 1) / kWrwChunkRows);
  // No more splits than keep the partials, 4*N*K bytes per split written and
  // read back once, within half of the 2*R*(N+K) bytes of the inputs.
  const int64_t cap = std::min<int64_t>(
      p.row_chunks, std::max<int64_t>(1, rows * (n + k) / (8 * n * k)));
  // The widest tile, which reads the inputs the fewest times; 256 x 256 would
  // leave one wave per SIMD.  Where the cap on the splits, not the rows, keeps
  // the grid below one workgroup per CU, more and smaller tiles fill it.
  p.bn = (int)std::min<int64_t>(n, 256);
  p.bk = (int)std::min<int64_t>(k, 256);
  if (p.bn == 256 && p.bk == 256) p.bn = 128;
  while (cap < p.row_chunks && std::max(p.bn, p.bk) > 128 &&
         (n / p.bn) * (k / p.bk) * cap < kConvCus)
    (p.bn >= p.bk ? p.bn : p.bk) /= 2;
  p.ntiles_n = p.n / p.bn;
  p.ntiles_k = p.k / p.bk;
  p.lds_bytes = kWrwChunkRows * (p.bn + p.bk) * 2;
  // four waves per SIMD with one 32x32 accumulator tile per wave, three with
  // two, two with four, one with eight
  const int acc_tiles = (p.bn / 64) * (p.bk / 64);
  const int by_regs =
      acc_tiles == 1 ? 4 : acc_tiles == 2 ? 3 : acc_tiles == 4 ? 2 : 1;
  const int per_cu = std::min(kConvLdsBytes / p.lds_bytes, by_regs);
  const int tiles = p.ntiles_n * p.ntiles_k;
  int64_t splits =
      std::min<int64_t>(cap, std::max(1, kConvCus * per_cu / tiles));
  if (splits > 8) splits -= splits % 8;  // conv1x1_wrw_split
  p.splits = (int)cap_splits(splits, tiles, max_workgroups);
  p.grid = tiles * p.splits;
  p.chunks_per_split = (p.row_chunks + p.splits - 1) / p.splits;
  p.partial_floats = (int64_t)p.splits * p.n * p.k;
  return p;
}

Conv1x1WrwRingPlan conv1x1_wrw_ring_plan(int64_t rows, int64_t k, int64_t n,
                                         int64_t max_workgroups) {
  Conv1x1WrwRingPlan p;
  p.rows = rows;
  p.eligible = shape_ok(rows, k, n) && k >= 128 && n >= 128;
  if (!p.eligible) return p;
  p.k = (int)k;
  p.n = (int)n;
  p.native = measured_faster(kNativeWrwRing, rows, k, n);
  p.chunk_rows = kWrwChunkRows;
  p.row_chunks = (int)((rows + kWrwChunkRows - 1) / kWrwChunkRows);
  p.bn = p.bk = kWrwRingTile;
  p.ntiles_n = p.n / p.bn;
  p.ntiles_k = p.k / p.bk;
  p.stage_bytes = p.chunk_rows * (p.bn + p.bk) * 2;
  p.stages = std::min(kWrwRingMaxStages, kConvLdsBytes / p.stage_bytes);
  p.lds_bytes = p.stages * p.stage_bytes;
  // one workgroup per CU: what keeps the loads in flight is the ring, not a
  // second workgroup, and the partials grow with the splits
  const int tiles = p.ntiles_n * p.ntiles_k;
  int64_t splits =
      std::min<int64_t>(p.row_chunks, std::max(1, kConvCus / tiles));
  if (splits > 8) splits -= splits % 8;  // conv1x1_wrw_split
  p.splits = (int)cap_splits(splits, tiles, max_workgroups);
  p.grid = tiles * p.splits;
  p.chunks_per_split = (p.row_chunks + p.splits - 1) / p.splits;
  p.partial_floats = (int64_t)p.splits * p.n * p.k;
  return p;
}

Conv1x1Plan conv1x1_plan(int64_t rows, int64_t k, int64_t n,
                         int64_t max_workgroups) {
  Conv1x1Plan p;
  p.rows = rows;
  p.eligible = shape_ok(rows, k, n);
  if (!p.eligible) return p;
  p.k = (int)k;
  p.n = (int)n;
  p.native = measured_faster(kNative, rows, k, n);
  tile_geometry(p, kConvStageBytes);
  // no more splits than keep a partial row per split (8*N bytes and the
  // counts) within 5% of the 2*R*N bytes of the output
  // one wave per SIMD with 8 MFMA tiles per wave, two with 4, three with 2
  const int by_regs = p.nt == 8 ? 1 : p.nt == 4 ? 2 : 3;
  set_grid(p,
           std::min(splits_by_occupancy(p, by_regs),
                    std::max<int64_t>(1, rows / 82)),
           max_workgroups);
  p.run = 16 * p.tiles_per_split;
  p.pstride = 2 * p.n + p.ntiles;
  p.partial_floats = (int64_t)p.splits * p.pstride;
  return p;
}

Conv1x1Plan conv1x1_bwd_plan(int64_t rows, int64_t k, int64_t n, bool with_add,
                             int64_t max_workgroups) {
  Conv1x1Plan p;
  p.rows = rows;
  p.eligible = shape_ok(rows, k, n);
  if (!p.eligible) return p;
  p.k = (int)n;  // contracted: the width of dY
  p.n = (int)k;  // produced: the width of dX
  p.native = measured_faster(kNativeBwd, rows, k, n, with_add);
  tile_geometry(p, kConvBwdStageBytes);
  // without the moments the kernel needs fewer registers than the forward:
  // two waves per SIMD with 8 MFMA tiles, three with 4, four with 2, and one
  // / two / two where W is staged chunk by chunk
  const int by_regs = p.resident ? (p.nt == 8 ? 2 : p.nt == 4 ? 3 : 4)
                                 : (p.nt == 8 ? 1 : 2);
  set_grid(p, splits_by_occupancy(p, by_regs), max_workgroups);
  return p;
}

}  // namespace cgx
