// Launch geometry of the fused BatchNorm kernels: see bn_plan.h.
#include "bn_plan.h"

#include <algorithm>

namespace cgx {

BnPlan bn_plan(int64_t rows, int64_t channels) {
  BnPlan p;
  p.rows = rows;
  p.channels = (int)std::min<int64_t>(std::max<int64_t>(channels, 0), 1 << 30);
  const bool pow2 = channels > 0 && (channels & (channels - 1)) == 0;
  p.eligible = pow2 && channels >= 8 && channels <= 2048 && rows >= 2 &&
               rows <= kBnMaxRows;
  if (!p.eligible) return p;

  p.cgs = p.channels / 8;
  p.tc = std::min(p.cgs, kBnMaxTileCgs);
  p.ctiles = p.cgs / p.tc;
  p.rln = kBnThreads / p.tc;
  const int64_t row_blocks = (rows + p.rln - 1) / p.rln;
  // enough workgroups to fill the chip ...
  int64_t splits = std::min<int64_t>(row_blocks,
                                     std::max(1, kBnTargetWgs / p.ctiles));
  // ... while two fp32 partial rows per split (8*splits*C bytes) stay within
  // 5% of the 2*R*C bytes of the tensor
  splits = std::min(splits, std::max<int64_t>(1, rows / 80));
  p.splits = (int)splits;
  p.grid = p.ctiles * p.splits;
  p.rows_per_thread = (int)((row_blocks + splits - 1) / splits);
  p.partial_floats = (int64_t)p.splits * p.channels;
  return p;
}

BnPoolPlan bn_pool_plan(int64_t n, int64_t h, int64_t w, int64_t channels) {
  BnPoolPlan g;
  g.n = (int)n;
  g.h = (int)h;
  g.w = (int)w;
  g.oh = pool_out(g.h);
  g.ow = pool_out(g.w);
  g.cgs = (int)(channels / 8);
  g.threads = (int64_t)g.n * g.oh * g.ow * g.cgs;
  g.grid = (int)((g.threads + kBnThreads - 1) / kBnThreads);
  return g;
}

}  // namespace cgx
