// Launch geometry of the stem convolution of a ResNet with the BatchNorm
// partials of its output (conv_stem_stats in conv_stem_kernels.hip):
// Conv2d(3, 64, 7, stride 2, padding 3) on channels_last bf16 tensors.
//
// Pure host arithmetic, like conv3x3_plan.h.  Y[R, 64] = A[R, K] * Wp[64, K]^T,
// R = B * H/2 * W/2 the output pixels in memory order.  In channels_last the
// 7 taps x 3 channels that one filter row takes from an input row are 21
// consecutive bf16 of that row, starting at element 6*ow - 9.  A filter row
// is padded to 24, so K = 7 * 24 = 168, rounded to 176: eleven 16-deep MFMA
// steps, or 22 operand groups of 8.  Group G = 3r + g is elements 8g .. 8g+7 of
// filter row r and never straddles two rows; group 21 is all pad.
//
// A workgroup walks bands: `band_rows` whole output rows of one image (the
// last band of an image may be short).  The strip of a band is a raw copy of
// its 2*band_rows + 5 input rows in LDS, a row of `pitch` bytes holding row
// element e at byte 2*(e + 9): 9 zero elements on the left for the windows
// that leave the image there, zeros on the right up to the pitch, and zero
// rows where the band's window leaves the image above or below.  The operand
// group G of band pixel (ohl, owl) is then the 16 bytes at
// (2*ohl + r)*pitch + 12*owl + 16*g, 4-byte aligned: no im2col image.  What
// a group reads beyond its filter row's 21 elements (the next pixel's data,
// against zero weights) is cleared in registers: conv_stem_keep.
//
// The grid is persistent: workgroup s walks bands s, s + splits, ... and
// writes one partial row [mean(64) | M2(64) | count].
#pragma once

#include <cstdint>

#include "conv1x1_plan.h"

namespace cgx {

constexpr int kConvStemC = 3, kConvStemN = 64, kConvStemTaps = 7;
constexpr int kConvStemRowK = 24;  // a filter row's 21 elements, padded
constexpr int kConvStemGroups = 22;  // operand groups of 8: K = 176
constexpr int kConvStemTile = 32;    // output pixels of a tile
constexpr int kConvStemMaxBandRows = 8;
// A thread stages a band through registers, at most this many 16-byte
// vectors of the strip.  A strip of one output row is 7 rows of 3W/8 + 3
// vectors, so this is what bounds the width: W <= 768 (LDS would allow more).
constexpr int kConvStemXVecs = 8;
constexpr int kConvStemMaxW = 768;
// resident workgroups per CU: two waves per SIMD, so that one wave's
// epilogue runs under the other's MFMAs (benchmarks/RESULTS.md)
constexpr int kConvStemWgsPerCu = 2;

struct ConvStemPlan {
  int batch = 0, h = 0, w = 0;
  bool eligible = false;
  bool native = false;  // measured faster than MIOpen + bn_stats
  int oh = 0, ow = 0;
  int rows = 0;       // R
  int band_rows = 0;  // output rows of a band
  int bands_per_image = 0, bands = 0;
  int tiles_per_band = 0;  // of a full band
  int in_rows = 0;         // strip rows: 2*band_rows + 5
  int nvec = 0;            // 16-byte vectors of a strip row: 3W/8 + 3
  int pitch = 0;           // bytes of a strip row
  int xvecs = 0;           // a thread's vectors of a strip
  int splits = 0;          // persistent workgroups
  int grid = 0;            // == splits: one tile of 64 channels
  int bands_per_split = 0;  // longest walk
  int run = 0;              // longest per-lane run of the moments
  int lds_bytes = 0;
  int pstride = 0;             // floats per partial row: 2*64 + 1
  int64_t partial_floats = 0;  // splits * pstride
  unsigned magic_nvec = 0, magic_ow = 0;  // conv_stem_div
};

// H even and >= 2, W a multiple of 8 (every input row 16-byte aligned) up to
// kConvStemMaxW, 2 <= B*(H/2)*(W/2) <= kBnMaxRows.  `max_workgroups` > 0 caps
// the grid.
ConvStemPlan conv_stem_plan(int64_t batch, int64_t h, int64_t w,
                            int64_t max_workgroups = 0);

// v / d for v * d < 2^32, magic = ceil(2^32 / d), d >= 2
__host__ __device__ inline int conv_stem_div(unsigned v, unsigned magic) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)__umulhi(v, magic);
#else
  return (int)(((uint64_t)v * magic) >> 32);
#endif
}

// Band -> its image, its first output row and its number of output rows.
struct ConvStemBand {
  int image, oh0, live;
};
__host__ __device__ inline ConvStemBand conv_stem_band(const ConvStemPlan& p,
                                                       int band) {
  const int image = band / p.bands_per_image;
  const int oh0 = (band - image * p.bands_per_image) * p.band_rows;
  const int left = p.oh - oh0;
  return ConvStemBand{image, oh0, left < p.band_rows ? left : p.band_rows};
}

// Where vector `idx` of a band's strip comes from: strip row rr = idx / nvec
// and vector j of that row hold the row elements 8j-9 .. 8j-2, that is the
// last element of the input row's vector j-2 and the first seven of its
// vector j-1.  `row` is the input row b*H + ih, or -1 for a zero row; `vec`
// the index of vector j-1 among the row's 3W/8 (-1: zeros), `elem` the row
// element 8j-9 (-1: zero).
struct ConvStemSrc {
  int rr, j, row, vec, elem;
};
__host__ __device__ inline ConvStemSrc conv_stem_src(const ConvStemPlan& p,
                                                     const ConvStemBand& b,
                                                     int idx) {
  ConvStemSrc s;
  s.rr = conv_stem_div((unsigned)idx, p.magic_nvec);
  s.j = idx - s.rr * p.nvec;
  const int ih = 2 * b.oh0 - 3 + s.rr;
  s.row = s.rr < p.in_rows && ih >= 0 && ih < p.h ? b.image * p.h + ih : -1;
  s.vec = s.row >= 0 && s.j >= 1 && s.j <= 3 * p.w / 8 ? s.j - 1 : -1;
  s.elem = s.row >= 0 && s.j >= 2 && 8 * s.j - 9 < 3 * p.w ? 8 * s.j - 9 : -1;
  return s;
}

// Byte of the strip at which group 0 of band pixel pl = ohl*OW + owl starts;
// group G = 3r + g is r*pitch + 16*g further on.
__host__ __device__ inline int conv_stem_operand(const ConvStemPlan& p,
                                                 int pl) {
  const int ohl = conv_stem_div((unsigned)pl, p.magic_ow);
  return 2 * ohl * p.pitch + 12 * (pl - ohl * p.ow);
}
__host__ __device__ inline int conv_stem_group_offset(const ConvStemPlan& p,
                                                      int group) {
  const int r = group / 3;
  return r * p.pitch + 16 * (group - 3 * r);
}
// The dwords of group G's operand that reach the MFMA, as four AND masks:
// elements 21 .. 23 of a filter row and all of group 21 are cleared.
__host__ __device__ inline unsigned conv_stem_keep(int group, int dword) {
  if (group >= kConvStemGroups - 1) return 0u;
  if (group % 3 != 2 || dword < 2) return ~0u;
  return dword == 2 ? 0xffffu : 0u;
}

// y[B, H/2, W/2, 64] bf16 and part[splits, pstride] fp32 from x[B, H, W, 3]
// and w[64, 7, 7, 3] bf16; every pointer 16-byte aligned.
void launch_conv_stem_stats(const ConvStemPlan& p, const void* x, const void* w,
                            void* y, float* part, hipStream_t stream);

// ---- weight gradient ----------------------------------------------------------
//
// dW[n][r][e] = sum over output pixels of dY[b, oh, ow, n] * X[b, 2oh+r-3][6ow-9+e]
// (conv_stem_wrw in conv_stem_kernels.hip), e = 3s + c the 21 elements that a
// filter row takes from an input row.  A GEMM with the output pixels as the
// contracted index: M the 64 channels of dY, N the 147 columns 21r + e, padded
// to 160.  A 16-deep MFMA step is two groups of eight consecutive ow of one
// output row, one per lane half; W % 16 == 0, so no group crosses a row.
//
// A band is `band_rows` output rows of one image (the last of an image may be
// short).  Its LDS buffer holds the band's pixels of dY as a wrw_cell<64> image
// and its 2*band_rows + 5 input rows de-interleaved: with the forward's nine
// zero elements on the left, strip position t = 6m + q goes to plane q, index
// m, so that the eight pixels of a group, six elements apart in the row, are
// eight consecutive bf16 of a plane.  A plane is stored from element -off(q),
// off = 2 for q < 3 and 3 for q >= 3: then the 24 elements of three input
// vectors fill exactly the four elements 4u .. 4u+3 of every plane (unit u),
// the first and the last unit of a plane are zeros, and the operand of column
// (r, e = 6a + q) for the group at (ohl, ow0) starts at element ow0 + a + off(q)
// of plane q of strip row 2*ohl + r.
//
// The grid is persistent: workgroup s walks the bands s*bands_per_split ..
// in order and writes one fp32 partial [64][160]; conv_stem_wrw_finalize adds
// the partials in a fixed order and rounds once.
constexpr int kConvStemWrwCols = 160;  // 147 columns, five 32-column tiles
constexpr int kConvStemWrwReal = 147;
// a thread's share of a band in registers: 16-byte vectors of dY, and units of
// three vectors of x
constexpr int kConvStemWrwDyVecs = 16, kConvStemWrwXUnits = 3;
// The widest W % 16 == 0 at which two buffers of a one-row band fit in LDS:
// 128 bytes of dY a pixel, OW rounded up to 16, and 7 rows of 6 planes of
// W + 16 bytes, 2 * 81408 bytes at 752.  Its share per thread fits as well.
constexpr int kConvStemWrwMaxW = 752;
// three waves' accumulator tiles, for the sum at the end of the walk
constexpr int kConvStemWrwSumBytes = 3 * kConvStemN * kConvStemWrwCols * 4;

struct ConvStemWrwPlan {
  int batch = 0, h = 0, w = 0;
  bool eligible = false;
  bool native = false;  // measured faster than the stock weight gradient
  int oh = 0, ow = 0;
  int band_rows = 0, bands_per_image = 0, bands = 0;
  int in_rows = 0;     // strip rows: 2*band_rows + 5
  int units = 0;       // 8-byte units of a plane: OW/4 + 2
  int plane = 0;       // bytes of a plane
  int row_bytes = 0;   // bytes of a strip row: 6 planes
  int dy_bytes = 0;    // the dY image, a whole number of 16-pixel steps
  int buf_bytes = 0;   // dy image + planes
  int dyvecs = 0, xunits = 0;  // a thread's share of a full band
  int gpr = 0;         // groups of an output row: OW/8
  int groups = 0, steps = 0;            // of a full band
  int last_groups = 0, last_steps = 0;  // of an image's last band
  int splits = 0, grid = 0, bands_per_split = 0;
  int lds_bytes = 0;
  int64_t partial_floats = 0;  // splits * 64 * 160
  unsigned magic_units = 0, magic_gpr = 0;  // conv_stem_div
};

// H even and >= 2, W a multiple of 16 up to kConvStemWrwMaxW,
// 2 <= B*(H/2)*(W/2) <= kBnMaxRows.  `max_workgroups` > 0 caps the grid.
ConvStemWrwPlan conv_stem_wrw_plan(int64_t batch, int64_t h, int64_t w,
                                   int64_t max_workgroups = 0);

// Band -> image, first output row, output rows (as conv_stem_band).
__host__ __device__ inline ConvStemBand conv_stem_wrw_band(
    const ConvStemWrwPlan& p, int band) {
  const int image = band / p.bands_per_image;
  const int oh0 = (band - image * p.bands_per_image) * p.band_rows;
  const int left = p.oh - oh0;
  return ConvStemBand{image, oh0, left < p.band_rows ? left : p.band_rows};
}

// The bands workgroup `split` walks: first .. end-1, never none.
__host__ __device__ inline int conv_stem_wrw_first(const ConvStemWrwPlan& p,
                                                   int split) {
  return split * p.bands_per_split;
}
__host__ __device__ inline int conv_stem_wrw_end(const ConvStemWrwPlan& p,
                                                 int split) {
  const int end = (split + 1) * p.bands_per_split;
  return end < p.bands ? end : p.bands;
}

// Column 21r + e of the GEMM -> where its operands start in the planes, apart
// from the group's own 2*ohl*row_bytes + 2*ow0: `byte` is 4-byte aligned and
// the operand starts `shift` bits into it.  Columns >= 147 have no operand.
struct ConvStemWrwCol {
  int byte, shift;
};
__host__ __device__ inline ConvStemWrwCol conv_stem_wrw_col(
    const ConvStemWrwPlan& p, int col) {
  const int r = col / 21, e = col - 21 * r;
  const int a = e / 6, q = e - 6 * a;
  const int at = a + (q < 3 ? 2 : 3);
  return ConvStemWrwCol{r * p.row_bytes + q * p.plane + 2 * (at & ~1),
                        16 * (at & 1)};
}

// dw[64, 7, 7, 3] bf16 from dy[B, H/2, W/2, 64] and x[B, H, W, 3] bf16, through
// part[splits, 64, 160] fp32; every pointer 16-byte aligned.
void launch_conv_stem_wrw(const ConvStemWrwPlan& p, const void* dy,
                          const void* x, float* part, void* dw,
                          hipStream_t stream);

}  // namespace cgx
