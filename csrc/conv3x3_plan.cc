// Launch geometry of the 3x3 weight gradient, forwards and input gradients: see
// conv3x3_plan.h.
#include "conv3x3_plan.h"

#include <algorithm>
#include <array>

namespace cgx {
namespace {

// The problems (batch, H, W, C, N) at which conv3x3_wrw plus the finalize
// beat MIOpen's fill + igemm + cast in every run of an alternating
// measurement on MI355X: the slowest native run faster than the fastest stock
// run (benchmarks/conv3x3_wrw_shapes.py, table in benchmarks/RESULTS.md).
// Measured at these sizes only, so only they go native.  256->256 at 14x14
// and 512->512 at 7x7 of ResNet-50 at batch 256 did not meet the rule (their
// medians are within 5% of the stock path's either way) and stay stock.
struct Measured3x3 {
  int batch, h, w, c, n;
};
constexpr Measured3x3 kNativeWrw3x3[] = {
    {256, 56, 56, 64, 64},
    {256, 28, 28, 128, 128},
};

// The same rule for conv3x3_wrw_ring plus the finalize against the path the
// problem takes without it: conv3x3_wrw where the table above has it, the
// stock path elsewhere (benchmarks/conv3x3_wrw_ring_shapes.py).  All four met
// it, in two processes, with two stages and with three.
constexpr Measured3x3 kNativeWrw3x3Ring[] = {
    {256, 56, 56, 64, 64},
    {256, 28, 28, 128, 128},
    {256, 14, 14, 256, 256},
    {256, 7, 7, 512, 512},
};

// The same rule for conv3x3_stats followed by bn_act_forward with its partials
// against MIOpen's forward followed by bn_act_forward with a statistics pass
// (benchmarks/conv3x3_fwd_shapes.py).  All four bottleneck problems of
// ResNet-50 at batch 256 met it.
constexpr Measured3x3 kNativeFwd3x3[] = {
    {256, 56, 56, 64, 64},
    {256, 28, 28, 128, 128},
    {256, 14, 14, 256, 256},
    {256, 7, 7, 512, 512},
};

// The same rule for conv3x3_bwd_data against MIOpen's backward-data alone
// (benchmarks/conv3x3_bwd_shapes.py); here batch, H, W, C of dX, N of dY.
// All four met it as well.
constexpr Measured3x3 kNativeBwd3x3[] = {
    {256, 56, 56, 64, 64},
    {256, 28, 28, 128, 128},
    {256, 14, 14, 256, 256},
    {256, 7, 7, 512, 512},
};

// The same rule for conv3x3s2_stats followed by bn_act_forward with its
// partials against MIOpen's stride-2 forward followed by bn_act_forward with
// a statistics pass (benchmarks/conv3x3_s2_fwd_shapes.py); batch, H, W of the
// input.  Of the three strided problems of ResNet-50 at batch 256 only the
// deepest met it; 128->128 from 56x56 and 256->256 from 28x28 tie with the
// stock pair and stay stock.
constexpr Measured3x3 kNativeFwd3x3S2[] = {
    {256, 14, 14, 512, 512},
};

// The same rule for conv3x3s2_bwd_data against MIOpen's stride-2
// backward-data alone (benchmarks/conv3x3_s2_bwd_shapes.py); batch, H, W, C of
// dX, N of dY.  None of the three strided problems of ResNet-50 at batch 256
// met it in both processes: the native medians are 20 and 15 us below the
// stock ones at 128<-128 to 56x56 and 256<-256 to 28x28 and 3 us above at
// 512<-512 to 14x14, but each had a native run slower than a stock run in
// one process.  The table is empty and all three stay stock.
constexpr std::array<Measured3x3, 0> kNativeBwd3x3S2 = {};

// The same rule for conv3x3s2_wrw plus the finalize against MIOpen's stride-2
// fill + igemm + cast (benchmarks/conv3x3_s2_wrw_shapes.py); batch, H, W of
// the input.  All three strided problems of ResNet-50 at batch 256 met it, in
// two processes.
constexpr Measured3x3 kNativeWrw3x3S2[] = {
    {256, 56, 56, 128, 128},
    {256, 28, 28, 256, 256},
    {256, 14, 14, 512, 512},
};

bool pow2_in(int64_t v, int64_t lo, int64_t hi) {
  return v >= lo && v <= hi && (v & (v - 1)) == 0;
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

unsigned magic_of(int d) {
  return (unsigned)(((1u << kConv3x3MagicShift) + d - 1) / d);
}

int strip_dy_of(int rows, int pitch) { return round_up(rows * pitch, 16); }
// every index that a position below the rounded dY strip reaches with the
// last tap, offset 2*pitch + 2, in whole lines of the image
int strip_x_of(int rows, int pitch) {
  return round_up(strip_dy_of(rows, pitch) + 2 * pitch + 2, 4);
}

// whether chunks of `rows` rows pass through the staging registers
bool fits(int rows, int pitch, int bn, int bk) {
  return strip_dy_of(rows, pitch) * (bn / 8) <= kConv3x3DyVecs * kConvThreads &&
         strip_x_of(rows, pitch) * (bk / 8) <= kConv3x3XVecs * kConvThreads;
}

// The chunks for at most `limit` rows each: as many whole images as fit, or
// one image in the fewest chunks, of equal length but the last.
void set_chunks(Conv3x3WrwPlan& p, int limit) {
  const int whole = std::min((limit + 1) / (p.h + 1), p.batch);
  if (whole >= 2) {
    p.images = whole;
    p.group_rows = whole * (p.h + 1) - 1;
    p.chunks_per_image = 1;
    p.hr = p.group_rows;
  } else {
    p.images = 1;
    p.group_rows = p.h;
    p.chunks_per_image = (p.h + limit - 1) / limit;
    p.hr = (p.h + p.chunks_per_image - 1) / p.chunks_per_image;
  }
  const int groups = (p.batch + p.images - 1) / p.images;
  p.chunks = groups * p.chunks_per_image;
}

}  // namespace

Conv3x3WrwPlan conv3x3_wrw_plan(int64_t batch, int64_t h, int64_t w, int64_t c,
                                int64_t n, int64_t max_workgroups) {
  Conv3x3WrwPlan p;
  // 64 x 64 is the one tile: nine accumulator tiles per wave, 144 registers
  p.bn = p.bk = 64;
  p.eligible = pow2_in(c, 64, 512) && pow2_in(n, 64, 512) && batch >= 1 &&
               h >= 1 && w >= 1 && batch <= kBnMaxRows && h <= kBnMaxRows &&
               w <= kBnMaxRows && batch * h * w <= kBnMaxRows &&
               fits(1, (int)w + 1, p.bn, p.bk);
  if (!p.eligible) return p;
  p.batch = (int)batch, p.h = (int)h, p.w = (int)w, p.c = (int)c, p.n = (int)n;
  for (const Measured3x3& m : kNativeWrw3x3)
    p.native |= m.batch == batch && m.h == h && m.w == w && m.c == c && m.n == n;
  p.pitch = p.w + 1;
  p.ntiles_n = p.n / p.bn;
  p.ntiles_k = p.c / p.bk;
  const int tiles = p.ntiles_n * p.ntiles_k;

  // One workgroup per CU: the strips take most of LDS.  No more splits than
  // keep the partials, 4*N*9C bytes per split written and read back once,
  // within the bytes the workgroups read of the operands: 2*R*(N + C) once
  // per tile of the other operand's channels.
  const int64_t rows = batch * h * w;
  const int64_t operand_bytes =
      2 * rows * (n * p.ntiles_k + c * p.ntiles_n);
  const int64_t by_bytes = std::max<int64_t>(1, operand_bytes / (72 * n * c));
  int64_t splits = std::min<int64_t>(by_bytes, std::max(1, kConvCus / tiles));
  if (max_workgroups > 0)
    splits = std::min(splits, std::max<int64_t>(
                                  1, std::min<int64_t>(max_workgroups, 1 << 20) /
                                         tiles));

  // The longest chunk that fits.  With 64-wide tiles the bytes rule above
  // comes to one split per 1152 pixels (72*N*C bytes of partials against
  // 2*R*2*N*C/64 of operands) and a chunk holds at most 384 positions, so
  // every split has chunks without shortening them; the clamp below is for
  // the rounding at problems of a single chunk.
  int limit = 1;
  while (fits(limit + 1, p.pitch, p.bn, p.bk) &&
         limit + 1 <= (int)std::min<int64_t>(batch * (h + 1), 1 << 10))
    limit++;
  set_chunks(p, limit);
  splits = std::min<int64_t>(splits, p.chunks);
  if (splits > 8) splits -= splits % 8;  // conv3x3_wrw_split
  p.splits = (int)splits;
  p.grid = tiles * p.splits;
  p.chunks_per_split = (p.chunks + p.splits - 1) / p.splits;

  p.strip_dy = strip_dy_of(p.hr, p.pitch);
  p.strip_x = strip_x_of(p.hr, p.pitch);
  p.lds_bytes = (p.strip_dy * p.bn + p.strip_x * p.bk) * 2;
  p.partial_floats = (int64_t)p.splits * p.n * 9 * p.c;
  p.magic_pitch = magic_of(p.pitch);
  p.magic_h1 = magic_of(p.h + 1);
  return p;
}

namespace {

int ring_glds(int strip) { return (strip + 31) / 32; }
// The ring's dY strip is whole rounds of the fill, which costs no LDS and
// makes the number of 16-position steps even (the kernel alternates two sets
// of operand registers and has one path through a chunk) ...
int ring_strip_dy_of(int rows, int pitch) { return round_up(rows * pitch, 32); }
// ... and its X strip what that reaches
int ring_strip_x_of(int rows, int pitch) {
  return round_up(ring_strip_dy_of(rows, pitch) + 2 * pitch + 2, 4);
}

// whether chunks of `rows` rows fit a stage of a ring of `stages`
bool ring_fits(int rows, int pitch, int stages) {
  const int glds = ring_glds(ring_strip_dy_of(rows, pitch)) +
                   ring_glds(ring_strip_x_of(rows, pitch));
  return glds <= kConv3x3RingMaxGlds &&
         glds * 4096 * stages <= kConvLdsBytes;
}

}  // namespace

Conv3x3WrwRingPlan conv3x3_wrw_ring_plan(int64_t batch, int64_t h, int64_t w,
                                         int64_t c, int64_t n,
                                         int64_t max_workgroups, int stages) {
  Conv3x3WrwRingPlan p;
  p.bn = p.bk = 64;
  p.stages = stages == 0 ? kConv3x3RingStages : stages;
  p.eligible = (p.stages == 2 || p.stages == 3) && pow2_in(c, 64, 512) &&
               pow2_in(n, 64, 512) && batch >= 1 && h >= 1 && w >= 1 &&
               batch <= kBnMaxRows && h <= kBnMaxRows && w <= kBnMaxRows &&
               batch * h * w <= kBnMaxRows &&
               ring_fits(1, (int)w + 1, p.stages);
  if (!p.eligible) return p;
  p.batch = (int)batch, p.h = (int)h, p.w = (int)w, p.c = (int)c, p.n = (int)n;
  for (const Measured3x3& m : kNativeWrw3x3Ring)
    p.native |= m.batch == batch && m.h == h && m.w == w && m.c == c && m.n == n;
  p.pitch = p.w + 1;
  p.ntiles_n = p.n / p.bn;
  p.ntiles_k = p.c / p.bk;
  const int tiles = p.ntiles_n * p.ntiles_k;

  // conv3x3_wrw_plan's splits: one workgroup per CU, the partials within the
  // bytes of the operands, no more splits than chunks
  const int64_t rows = batch * h * w;
  const int64_t operand_bytes =
      2 * rows * (n * p.ntiles_k + c * p.ntiles_n);
  const int64_t by_bytes = std::max<int64_t>(1, operand_bytes / (72 * n * c));
  int64_t splits = std::min<int64_t>(by_bytes, std::max(1, kConvCus / tiles));
  if (max_workgroups > 0)
    splits = std::min(splits, std::max<int64_t>(
                                  1, std::min<int64_t>(max_workgroups, 1 << 20) /
                                         tiles));
  int limit = 1;
  while (ring_fits(limit + 1, p.pitch, p.stages) &&
         limit + 1 <= (int)std::min<int64_t>(batch * (h + 1), 1 << 10))
    limit++;
  set_chunks(p, limit);
  splits = std::min<int64_t>(splits, p.chunks);
  if (splits > 8) splits -= splits % 8;  // conv3x3_wrw_split
  p.splits = (int)splits;
  p.grid = tiles * p.splits;
  p.chunks_per_split = (p.chunks + p.splits - 1) / p.splits;

  p.strip_dy = ring_strip_dy_of(p.hr, p.pitch);
  p.strip_x = ring_strip_x_of(p.hr, p.pitch);
  p.dy_glds = ring_glds(p.strip_dy);
  p.x_glds = ring_glds(p.strip_x);
  p.stage_bytes = (p.dy_glds + p.x_glds) * 4096;
  p.lds_bytes = p.stages * p.stage_bytes;
  p.partial_floats = (int64_t)p.splits * p.n * 9 * p.c;
  p.magic_pitch = magic_of(p.pitch);
  p.magic_h1 = magic_of(p.h + 1);
  return p;
}

namespace {

// The stage of chunks of `rows` output rows; false where it is not within
// kConv3x3RingMaxGlds instructions a wave.
bool s2_wrw_stage(Conv3x3S2WrwPlan& p, int rows) {
  p.live = rows * p.pitch;
  p.strip_dy = ring_strip_dy_of(rows, p.pitch);
  int base = p.strip_dy, reach = 0;
  for (int plane = 3; plane >= 0; plane--) {
    const int top = (plane >> 1) * p.pitch + (plane & 1);  // the largest offset
    p.plane_base[plane] = base;
    p.plane_size[plane] = round_up(p.live + top, 4);
    reach = std::max(reach, base + top + p.strip_dy);
    base += p.plane_size[plane];
  }
  p.strip_x = base - p.strip_dy;
  p.stage_pos = round_up(std::max(base, reach), 32);
  p.glds = p.stage_pos / 32;
  p.stage_bytes = p.glds * 4096;
  p.lds_bytes = 2 * p.stage_bytes;
  return p.glds <= kConv3x3RingMaxGlds && p.lds_bytes <= kConvLdsBytes;
}

}  // namespace

Conv3x3S2WrwPlan conv3x3s2_wrw_plan(int64_t batch, int64_t h, int64_t w,
                                    int64_t c, int64_t n,
                                    int64_t max_workgroups) {
  Conv3x3S2WrwPlan p;
  p.bn = p.bk = 64;
  p.eligible = pow2_in(c, 64, 512) && pow2_in(n, 64, 512) && batch >= 1 &&
               h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 &&
               batch <= kBnMaxRows && h <= kBnMaxRows && w <= kBnMaxRows &&
               batch * h * w <= kBnMaxRows;
  if (p.eligible) {
    p.pitch = (int)w / 2 + 1;
    p.eligible = s2_wrw_stage(p, 1);
  }
  if (!p.eligible) return p;
  p.batch = (int)batch, p.h = (int)h, p.w = (int)w, p.c = (int)c, p.n = (int)n;
  p.ho = p.h / 2, p.wo = p.w / 2;
  for (const Measured3x3& m : kNativeWrw3x3S2)
    p.native |= m.batch == batch && m.h == h && m.w == w && m.c == c && m.n == n;
  p.ntiles_n = p.n / p.bn;
  p.ntiles_k = p.c / p.bk;
  const int tiles = p.ntiles_n * p.ntiles_k;

  // conv3x3_wrw_plan's splits, the operands being dY's R rows and X's 4R
  const int64_t rows = batch * p.ho * p.wo;
  const int64_t operand_bytes =
      2 * rows * (n * p.ntiles_k + 4 * c * p.ntiles_n);
  const int64_t by_bytes = std::max<int64_t>(1, operand_bytes / (72 * n * c));
  int64_t splits = std::min<int64_t>(by_bytes, std::max(1, kConvCus / tiles));
  if (max_workgroups > 0)
    splits = std::min(splits, std::max<int64_t>(
                                  1, std::min<int64_t>(max_workgroups, 1 << 20) /
                                         tiles));
  int limit = 1;
  while (limit + 1 <= (int)std::min<int64_t>(batch * (p.ho + 1), 1 << 10) &&
         s2_wrw_stage(p, limit + 1))
    limit++;
  // set_chunks on the output rows
  const int whole = std::min((limit + 1) / (p.ho + 1), p.batch);
  if (whole >= 2) {
    p.images = whole;
    p.group_rows = whole * (p.ho + 1) - 1;
    p.chunks_per_image = 1;
    p.hr = p.group_rows;
  } else {
    p.images = 1;
    p.group_rows = p.ho;
    p.chunks_per_image = (p.ho + limit - 1) / limit;
    p.hr = (p.ho + p.chunks_per_image - 1) / p.chunks_per_image;
  }
  p.chunks = (p.batch + p.images - 1) / p.images * p.chunks_per_image;
  s2_wrw_stage(p, p.hr);
  splits = std::min<int64_t>(splits, p.chunks);
  if (splits > 8) splits -= splits % 8;  // conv3x3_wrw_split
  p.splits = (int)splits;
  p.grid = tiles * p.splits;
  p.chunks_per_split = (p.chunks + p.splits - 1) / p.splits;
  p.partial_floats = (int64_t)p.splits * p.n * 9 * p.c;
  p.magic_pitch = magic_of(p.pitch);
  p.magic_h1 = magic_of(p.ho + 1);
  return p;
}

Conv3x3FwdPlan conv3x3_fwd_plan(int64_t batch, int64_t h, int64_t w, int64_t c,
                                int64_t n, int64_t max_workgroups) {
  Conv3x3FwdPlan p;
  p.bn = kConv3x3FwdBn;
  p.tile_rows = kConv3x3FwdTileRows;
  p.kc = kConv3x3FwdKc;
  const int64_t strip = p.tile_rows + 2 * w + 2;
  p.eligible = pow2_in(c, 64, 512) && pow2_in(n, 64, 512) && batch >= 1 &&
               h >= 1 && w >= 1 && batch <= kBnMaxRows && h <= kBnMaxRows &&
               w <= kBnMaxRows && batch * h * w <= kBnMaxRows &&
               batch * h * w >= 2 && strip <= 64 * kConv3x3FwdXVecs;
  if (!p.eligible) return p;
  p.batch = (int)batch, p.h = (int)h, p.w = (int)w, p.c = (int)c, p.n = (int)n;
  p.rows = (int)(batch * h * w);
  for (const Measured3x3& m : kNativeFwd3x3)
    p.native |= m.batch == batch && m.h == h && m.w == w && m.c == c && m.n == n;
  p.ntiles = p.n / p.bn;
  p.nchunks = p.c / p.kc;
  p.resident = p.nchunks == 2;
  p.row_tiles = (p.rows + p.tile_rows - 1) / p.tile_rows;
  p.strip_rows = (int)strip;
  p.xvecs = (p.strip_rows + 63) / 64;

  // one workgroup per CU: the buffers take most of LDS
  int64_t splits = std::min<int64_t>(p.row_tiles, std::max(1, kConvCus / p.ntiles));
  if (max_workgroups > 0)
    splits = std::min(splits, std::max<int64_t>(
                                  1, std::min<int64_t>(max_workgroups, 1 << 20) /
                                         p.ntiles));
  if (splits > 8) splits -= splits % 8;  // conv3x3_fwd_split
  p.splits = (int)splits;
  p.grid = p.ntiles * p.splits;
  p.tiles_per_split = (p.row_tiles + p.splits - 1) / p.splits;
  p.run = 32 * p.tiles_per_split;
  p.lds_bytes = 2 * kConv3x3FwdWBytes + 2 * p.xvecs * 64 * p.kc * 2 +
                kConvStageBytes;
  p.pstride = 2 * p.n + p.ntiles;
  p.partial_floats = (int64_t)p.splits * p.pstride;
  return p;
}

Conv3x3S2FwdPlan conv3x3s2_fwd_plan(int64_t batch, int64_t h, int64_t w,
                                    int64_t c, int64_t n,
                                    int64_t max_workgroups) {
  Conv3x3S2FwdPlan p;
  p.bn = kConv3x3FwdBn;
  p.tile_rows = kConv3x3S2TileRows;
  p.kc = kConv3x3FwdKc;
  const int64_t strip = 4 * p.tile_rows + w + 2;  // 2 * Wo of halo
  p.eligible = pow2_in(c, 64, 512) && pow2_in(n, 64, 512) && batch >= 1 &&
               h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && h <= 2048 &&
               batch <= kBnMaxRows && batch * h * w <= kBnMaxRows &&
               batch * h * w >= 8 && strip <= 64 * kConv3x3S2XVecs;
  if (!p.eligible) return p;
  p.batch = (int)batch, p.h = (int)h, p.w = (int)w, p.c = (int)c, p.n = (int)n;
  p.ho = p.h / 2, p.wo = p.w / 2;
  p.rows = p.batch * p.ho * p.wo;
  for (const Measured3x3& m : kNativeFwd3x3S2)
    p.native |= m.batch == batch && m.h == h && m.w == w && m.c == c && m.n == n;
  p.ntiles = p.n / p.bn;
  p.nchunks = p.c / p.kc;
  p.row_tiles = (p.rows + p.tile_rows - 1) / p.tile_rows;
  const int halo[4] = {0, 1, p.wo, p.wo + 1};
  for (int pl = 0, base = 0; pl < 4; pl++) {
    p.plane_base[pl] = base;
    p.plane_rows[pl] = p.tile_rows + halo[pl];
    base += p.plane_rows[pl];
  }
  p.strip_rows = (int)strip;
  p.xvecs = (p.strip_rows + 63) / 64;
  p.magic_wo = p.wo == 1 ? 0u : (unsigned)(((1ull << 32) + p.wo - 1) / p.wo);
  p.magic_ho = p.ho == 1 ? 0u : (unsigned)(((1ull << 32) + p.ho - 1) / p.ho);

  // conv3x3_fwd_plan's grid: one workgroup per CU
  int64_t splits = std::min<int64_t>(p.row_tiles, std::max(1, kConvCus / p.ntiles));
  if (max_workgroups > 0)
    splits = std::min(splits, std::max<int64_t>(
                                  1, std::min<int64_t>(max_workgroups, 1 << 20) /
                                         p.ntiles));
  if (splits > 8) splits -= splits % 8;  // conv3x3_fwd_split
  p.splits = (int)splits;
  p.grid = p.ntiles * p.splits;
  p.tiles_per_split = (p.row_tiles + p.splits - 1) / p.splits;
  p.run = 16 * p.tiles_per_split;
  p.lds_bytes = 2 * kConv3x3FwdWBytes + 2 * p.xvecs * 64 * p.kc * 2 +
                kConvStageBytes;
  p.pstride = 2 * p.n + p.ntiles;
  p.partial_floats = (int64_t)p.splits * p.pstride;
  return p;
}

Conv3x3FwdPlan conv3x3_bwd_plan(int64_t batch, int64_t h, int64_t w, int64_t c,
                                int64_t n, int64_t max_workgroups) {
  Conv3x3FwdPlan p = conv3x3_fwd_plan(batch, h, w, n, c, max_workgroups);
  p.native = false;
  p.pstride = 0;
  p.partial_floats = 0;
  if (!p.eligible) return p;
  for (const Measured3x3& m : kNativeBwd3x3)
    p.native |= m.batch == batch && m.h == h && m.w == w && m.c == c && m.n == n;
  return p;
}

Conv3x3S2BwdPlan conv3x3s2_bwd_plan(int64_t batch, int64_t h, int64_t w,
                                    int64_t c, int64_t n,
                                    int64_t max_workgroups) {
  Conv3x3S2BwdPlan p;
  p.bn = kConv3x3FwdBn;
  p.tile_rows = kConv3x3S2BwdTileRows;
  p.kc = kConv3x3FwdKc;
  const int64_t strip = p.tile_rows + w / 2 + 1;  // the last row's shift Wo + 1
  p.eligible = pow2_in(c, 64, 512) && pow2_in(n, 64, 512) && batch >= 1 &&
               h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && h <= 2048 &&
               batch <= kBnMaxRows && batch * h * w <= kBnMaxRows &&
               batch * h * w >= 8 && strip <= 64 * kConv3x3S2BwdXVecs;
  if (!p.eligible) return p;
  // the exchanged problem, as conv3x3_bwd_plan
  p.batch = (int)batch, p.h = (int)h, p.w = (int)w, p.c = (int)n, p.n = (int)c;
  p.ho = p.h / 2, p.wo = p.w / 2;
  p.rows = p.batch * p.ho * p.wo;
  for (const Measured3x3& m : kNativeBwd3x3S2)
    p.native |= m.batch == batch && m.h == h && m.w == w && m.c == c && m.n == n;
  p.ntiles = p.n / p.bn;
  p.nchunks = p.c / p.kc;
  p.row_tiles = (p.rows + p.tile_rows - 1) / p.tile_rows;
  p.strip_rows = (int)strip;
  p.xvecs = (p.strip_rows + 63) / 64;
  p.magic_wo = p.wo == 1 ? 0u : (unsigned)(((1ull << 32) + p.wo - 1) / p.wo);
  p.magic_ho = p.ho == 1 ? 0u : (unsigned)(((1ull << 32) + p.ho - 1) / p.ho);

  // conv3x3_fwd_plan's grid: one workgroup per CU
  int64_t splits = std::min<int64_t>(p.row_tiles, std::max(1, kConvCus / p.ntiles));
  if (max_workgroups > 0)
    splits = std::min(splits, std::max<int64_t>(
                                  1, std::min<int64_t>(max_workgroups, 1 << 20) /
                                         p.ntiles));
  if (splits > 8) splits -= splits % 8;  // conv3x3_fwd_split
  p.splits = (int)splits;
  p.grid = p.ntiles * p.splits;
  p.tiles_per_split = (p.row_tiles + p.splits - 1) / p.splits;
  p.lds_bytes = 2 * kConv3x3FwdWBytes + 2 * p.xvecs * 64 * p.kc * 2 +
                kConv3x3S2BwdStageBytes;
  return p;
}

}  // namespace cgx
