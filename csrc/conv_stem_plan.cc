// Launch geometry of the stem convolution: see conv_stem_plan.h.
#include "conv_stem_plan.h"

#include <algorithm>

namespace cgx {
namespace {

// The problems (batch, H, W) at which conv_stem_stats followed by
// bn_act_pool_forward with its partials beat MIOpen's forward followed by
// bn_act_pool_forward with a statistics pass in every run of an alternating
// measurement on MI355X: the slowest native pair faster than the fastest
// stock pair, in two processes (benchmarks/conv_stem_shapes.py, table in
// benchmarks/RESULTS.md).  Measured at this size only, so only it goes
// native.
struct MeasuredStem {
  int batch, h, w;
};
constexpr MeasuredStem kNativeStem[] = {
    {256, 224, 224},
};

unsigned magic_of(int d) {
  return (unsigned)(((uint64_t(1) << 32) + d - 1) / d);
}

}  // namespace

ConvStemPlan conv_stem_plan(int64_t batch, int64_t h, int64_t w,
                            int64_t max_workgroups) {
  ConvStemPlan p;
  const int64_t rows = batch * (h / 2) * (w / 2);
  p.eligible = batch >= 1 && batch <= kBnMaxRows && h >= 2 && h % 2 == 0 &&
               h <= kBnMaxRows && w >= 8 && w % 8 == 0 && w <= kConvStemMaxW &&
               rows >= 2 && rows <= kBnMaxRows;
  if (!p.eligible) return p;
  p.batch = (int)batch, p.h = (int)h, p.w = (int)w;
  for (const MeasuredStem& m : kNativeStem)
    p.native |= m.batch == batch && m.h == h && m.w == w;
  p.oh = p.h / 2, p.ow = p.w / 2;
  p.rows = (int)rows;
  p.nvec = 3 * p.w / 8 + 3;
  p.pitch = 16 * p.nvec;

  // the tallest band, up to 8 output rows, that a workgroup's threads stage
  // in kConvStemXVecs vectors each; one row always fits (kConvStemMaxW)
  p.band_rows = std::min(p.oh, kConvStemMaxBandRows);
  while ((2 * p.band_rows + 5) * p.nvec > kConvStemXVecs * kConvThreads)
    p.band_rows--;
  p.in_rows = 2 * p.band_rows + 5;
  p.xvecs = (p.in_rows * p.nvec + kConvThreads - 1) / kConvThreads;
  p.bands_per_image = (p.oh + p.band_rows - 1) / p.band_rows;
  p.bands = p.batch * p.bands_per_image;
  p.tiles_per_band = (p.band_rows * p.ow + kConvStemTile - 1) / kConvStemTile;

  int64_t splits = std::min<int64_t>(p.bands, kConvCus * kConvStemWgsPerCu);
  if (max_workgroups > 0) splits = std::min(splits, max_workgroups);
  p.splits = p.grid = (int)splits;
  p.bands_per_split = (p.bands + p.splits - 1) / p.splits;
  // a lane pushes 16 pixels of each tile its wave walks, every fourth tile
  p.run = 16 * ((p.tiles_per_band + 3) / 4) * p.bands_per_split;
  // two strips, which first hold the raw weight, and the waves' store stages
  const int weight_bytes = kConvStemN * kConvStemTaps * kConvStemTaps *
                           kConvStemC * 2;
  p.lds_bytes = std::max(2 * p.in_rows * p.pitch, weight_bytes) +
                kConvStageBytes;
  p.pstride = 2 * kConvStemN + 1;
  p.partial_floats = (int64_t)p.splits * p.pstride;
  p.magic_nvec = magic_of(p.nvec);
  p.magic_ow = magic_of(p.ow);
  return p;
}

namespace {

// The problems (batch, H, W) at which conv_stem_wrw with its finalize beat the
// stock weight gradient by the rule of kNativeStem
// (benchmarks/conv_stem_wrw_shapes.py, table in benchmarks/RESULTS.md).
constexpr MeasuredStem kNativeStemWrw[] = {
    {256, 224, 224},
};

}  // namespace

ConvStemWrwPlan conv_stem_wrw_plan(int64_t batch, int64_t h, int64_t w,
                                   int64_t max_workgroups) {
  ConvStemWrwPlan p;
  const int64_t rows = batch * (h / 2) * (w / 2);
  p.eligible = batch >= 1 && batch <= kBnMaxRows && h >= 2 && h % 2 == 0 &&
               h <= kBnMaxRows && w >= 16 && w % 16 == 0 &&
               w <= kConvStemWrwMaxW && rows >= 2 && rows <= kBnMaxRows &&
               max_workgroups >= 0;
  if (!p.eligible) return p;
  p.batch = (int)batch, p.h = (int)h, p.w = (int)w;
  for (const MeasuredStem& m : kNativeStemWrw)
    p.native |= m.batch == batch && m.h == h && m.w == w;
  p.oh = p.h / 2, p.ow = p.w / 2;
  p.gpr = p.ow / 8;
  p.units = p.ow / 4 + 2;
  p.plane = 8 * p.units;
  p.row_bytes = 6 * p.plane;

  // the tallest band whose two buffers fit in LDS and whose share per thread
  // fits the staging registers; one row always does (kConvStemWrwMaxW)
  auto fits = [&](int br) {
    const int dy = (br * p.ow + 15) / 16 * 16 * kConvStemN * 2;
    return 2 * (dy + (2 * br + 5) * p.row_bytes) <= kConvLdsBytes &&
           br * p.ow * 8 <= kConvStemWrwDyVecs * kConvThreads &&
           (2 * br + 5) * p.units <= kConvStemWrwXUnits * kConvThreads;
  };
  p.band_rows = 1;
  while (p.band_rows < p.oh && fits(p.band_rows + 1)) p.band_rows++;
  p.in_rows = 2 * p.band_rows + 5;
  p.groups = p.band_rows * p.gpr;
  p.steps = (p.groups + 1) / 2;
  p.dy_bytes = p.steps * 16 * kConvStemN * 2;
  p.buf_bytes = p.dy_bytes + p.in_rows * p.row_bytes;
  p.dyvecs = (p.groups * 64 + kConvThreads - 1) / kConvThreads;
  p.xunits = (p.in_rows * p.units + kConvThreads - 1) / kConvThreads;
  p.bands_per_image = (p.oh + p.band_rows - 1) / p.band_rows;
  p.bands = p.batch * p.bands_per_image;
  p.last_groups = (p.oh - (p.bands_per_image - 1) * p.band_rows) * p.gpr;
  p.last_steps = (p.last_groups + 1) / 2;

  // contiguous runs of bands_per_split bands, and no workgroup without one
  int64_t wgs = std::min<int64_t>(p.bands, kConvCus);
  if (max_workgroups > 0) wgs = std::min(wgs, max_workgroups);
  p.bands_per_split = (int)((p.bands + wgs - 1) / wgs);
  p.splits = p.grid = (p.bands + p.bands_per_split - 1) / p.bands_per_split;
  p.lds_bytes = std::max(2 * p.buf_bytes, kConvStemWrwSumBytes);
  p.partial_floats = (int64_t)p.splits * kConvStemN * kConvStemWrwCols;
  p.magic_units = magic_of(p.units);
  p.magic_gpr = magic_of(p.gpr);
  return p;
}

}  // namespace cgx
