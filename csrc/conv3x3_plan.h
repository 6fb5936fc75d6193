// Launch geometry of the weight gradient of a 3x3 / stride 1 / padding 1
// convolution (conv3x3_wrw in conv3x3_kernels.hip) and, further down, of its
// forward with BatchNorm partials (conv3x3_stats) and of its input gradient
// (conv3x3_bwd_data); between them the stride-2 forward (conv3x3s2_stats),
// last the stride-2 input gradient (conv3x3s2_bwd_data), and after the ring
// the stride-2 weight gradient (conv3x3s2_wrw).
//
// Pure host arithmetic, like conv1x1_plan.h.  dW[n, c, r, s] = sum over b, h, w
// of dY[b, n, h, w] * X[b, c, h+r-1, w+s-1] on channels_last bf16 tensors is
// the GEMM dW[N, 9C] with column (3r+s)*C + c, contracted over the pixels.  A
// 256-thread workgroup owns a bn x bk tile of channels (its four waves 2 x 2)
// with all nine taps, and one of `splits` slices of the pixels.
//
// A chunk is `hr` rows of pitch P = W+1.  dY is staged in LDS as the strip of
// positions j = row*P + w with the pad w = W zero, X as rows -1 .. hr at index
// i = (row+1)*P + wx + 1 with column 0 zero, so that tap (r, s) pairs position
// j with index j + r*P + s: the taps share both strips and differ by an LDS
// offset.  The rows of a chunk are rows of a `group`: `images` whole images
// stacked with one zero row between them, group_rows = images*(H+1) - 1 rows.
// With images == 1 a group is one image, cut into chunks_per_image chunks of
// hr rows, the last one maybe short.  Where several images fit one chunk
// (7x7 and smaller) images > 1 and the group is the chunk: the rounding of a strip
// to 16 positions and the per-chunk barriers are paid once for all of them.
//
// Each workgroup writes its fp32 tile to part[split][N][9C]; the finalize of
// the 1x1 weight gradient sums the planes in a fixed order.
#pragma once

#include <cstdint>

#include "conv1x1_plan.h"

namespace cgx {

// A thread stages a chunk through registers, at most this many 16-byte
// vectors of dY and of X: strips of 384 and 512 positions at a 64-channel
// tile, 112 KiB of the 160 KiB of LDS.  With more of them the kernel spills
// to scratch; so this, not LDS, is what bounds hr and the image width
// (W <= 166, where one row is a chunk).
constexpr int kConv3x3DyVecs = 12;
constexpr int kConv3x3XVecs = 16;
// row = (j * magic) >> kConv3x3MagicShift is j / d for the j < 2^10 and
// d < 2^9 that occur, magic = ceil(2^20 / d)
constexpr int kConv3x3MagicShift = 20;

struct Conv3x3WrwPlan {
  int batch = 0, h = 0, w = 0, c = 0, n = 0;
  bool eligible = false;
  bool native = false;  // measured faster than MIOpen's fill + igemm + cast
  int bn = 0, bk = 0;   // the workgroup's tile of dW's channels
  int ntiles_n = 0, ntiles_k = 0;
  int pitch = 0;       // W + 1
  int images = 0;      // images of a group
  int group_rows = 0;  // images * (H + 1) - 1
  int hr = 0;          // rows of a chunk
  int chunks_per_image = 0;  // chunks of a group
  int chunks = 0;            // groups * chunks_per_image
  int strip_dy = 0, strip_x = 0;  // positions of the two LDS strips
  int splits = 0;  // workgroups per channel tile
  int grid = 0;    // ntiles_n * ntiles_k * splits
  int chunks_per_split = 0;  // longest walk
  int lds_bytes = 0;
  int64_t partial_floats = 0;  // splits * N * 9C
  unsigned magic_pitch = 0, magic_h1 = 0;  // for j / pitch and t / (H + 1)
};

// C and N powers of two in [64, 512], batch*H*W within kBnMaxRows, and W
// narrow enough for one row to be a chunk.  `max_workgroups` > 0 caps the
// grid.
Conv3x3WrwPlan conv3x3_wrw_plan(int64_t batch, int64_t h, int64_t w, int64_t c,
                                int64_t n, int64_t max_workgroups = 0);

// Workgroup -> (tile, split) as conv1x1_wrw_tile / _split: the workgroups of
// one slice 8 apart, on one XCD, wherever the splits divide by 8.  Split s
// walks chunks s, s + splits, ...
__host__ __device__ inline int conv3x3_wrw_tile(const Conv3x3WrwPlan& p,
                                                int wg) {
  const int tiles = p.ntiles_n * p.ntiles_k;
  return p.splits % 8 == 0 ? (wg / 8) % tiles : wg % tiles;
}
__host__ __device__ inline int conv3x3_wrw_split(const Conv3x3WrwPlan& p,
                                                 int wg) {
  const int tiles = p.ntiles_n * p.ntiles_k;
  return p.splits % 8 == 0 ? (wg / 8 / tiles) * 8 + wg % 8 : wg / tiles;
}

// Row t of group `group` as a row b*H + h of the tensors, or -1 where it is
// a zero row: before or after the group, between two images, past the batch.
__host__ __device__ inline int conv3x3_wrw_row(const Conv3x3WrwPlan& p,
                                               int group, int t) {
  if (t < 0 || t >= p.group_rows) return -1;
  int image = 0, h = t;
  if (p.images > 1) {
    image = (int)(((unsigned)t * p.magic_h1) >> kConv3x3MagicShift);
    h = t - image * (p.h + 1);
  }
  const int b = group * p.images + image;
  return h < p.h && b < p.batch ? b * p.h + h : -1;
}

// dw[N, 3, 3, C] bf16 (the memory of a channels_last [N, C, 3, 3]) from
// dy[B, H, W, N] and x[B, H, W, C] bf16 through part[splits, N, 9C] fp32,
// which needs no initialisation; every pointer 16-byte aligned.
void launch_conv3x3_wrw(const Conv3x3WrwPlan& p, const void* dy, const void* x,
                        float* part, void* dw, hipStream_t stream);

// ---- weight gradient through a ring of LDS stages (conv3x3_wrw_ring) ----------
//
// conv3x3_wrw with the chunks loaded straight into LDS, as conv1x1_wrw_ring:
// no staging registers, `stages` chunks in flight across the barriers.  The
// strips, the images, the walk and the partials are those above, so equal
// (tile, hr, images, splits) give equal bits.  A stage holds the dY image and
// behind it the X image, each rounded up to whole rounds of the four waves'
// global_load_lds_dwordx4 (4 KiB, 32 positions of a 64-channel image); the
// positions past a strip load zeros.  The stages share LDS, so a chunk is
// shorter than conv3x3_wrw's: at most 80 KiB with two stages, 52 KiB with
// three.  `native` is the ring's own measurement against the path the problem
// takes without it.
constexpr int kConv3x3RingStages = 2;  // the geometry kept (RESULTS.md)
// instructions of a wave per stage, both images: the registers that hold
// their source offsets, and 80 KiB
constexpr int kConv3x3RingMaxGlds = 20;

struct Conv3x3WrwRingPlan : Conv3x3WrwPlan {
  int stages = 0;
  int dy_glds = 0, x_glds = 0;  // instructions of a wave per stage and image
  int stage_bytes = 0;  // (dy_glds + x_glds) * 4096; lds_bytes = stages * it
};

// `stages` 0 is kConv3x3RingStages; 2 and 3 are built.
Conv3x3WrwRingPlan conv3x3_wrw_ring_plan(int64_t batch, int64_t h, int64_t w,
                                         int64_t c, int64_t n,
                                         int64_t max_workgroups = 0,
                                         int stages = 0);

// One global_load_lds_dwordx4 of a wave writes 1 KiB of LDS, lane l the 16
// bytes at 16*l.  Instruction j of `wave` fills bytes (4j + wave) * 1024 ..
// of the stage, dY's image first (j < dy_glds), so the wrw_cell permutation
// goes onto the address a lane loads from: position `pos` of the strip and
// 16-byte vector `vec` of its 64 channels are what the image holds at the
// lane's bytes.
struct Conv3x3RingSlot {
  bool is_x;
  int pos, vec;
};
__host__ __device__ inline Conv3x3RingSlot conv3x3_wrw_ring_slot(
    const Conv3x3WrwRingPlan& p, int wave, int j, int lane) {
  const bool is_x = j >= p.dy_glds;
  const WrwImageSlot s = conv1x1_wrw_image_slot(
      64, conv1x1_wrw_ring_piece(wave, is_x ? j - p.dy_glds : j) + 16 * lane);
  return {is_x, s.row, s.channel / 8};
}

// What position `pos` of a strip loads, whatever the chunk: the pixel
// relative to the chunk's first (conv3x3_wrw_ring_window) and a key that the
// chunk's window admits or not.  With one image per group the key is the row
// relative to the chunk's first, with several the image of the group.  A
// position that is zero on every chunk (pad column, rows past the chunk, the
// tail of the strip and of the stage, column 0 of X, the row between two
// images) has a key that no window admits.
constexpr int kConv3x3RingNever = -(1 << 20);
struct Conv3x3RingSrc {
  int pixel, key;
};
__host__ __device__ inline Conv3x3RingSrc conv3x3_wrw_ring_src(
    const Conv3x3WrwRingPlan& p, bool is_x, int pos) {
  const int x1 = is_x ? 1 : 0;
  const int rr = (int)(((unsigned)pos * p.magic_pitch) >> kConv3x3MagicShift);
  const int col = pos - rr * p.pitch - x1, t = rr - x1;
  if (pos >= (is_x ? p.strip_x : p.strip_dy) || rr >= p.hr + 2 * x1 ||
      col < 0 || col >= p.w)
    return {0, kConv3x3RingNever};
  if (p.images == 1) return {t * p.w + col, t};
  if (t < 0 || t >= p.group_rows) return {0, kConv3x3RingNever};
  const int image = (int)(((unsigned)t * p.magic_h1) >> kConv3x3MagicShift);
  const int h = t - image * (p.h + 1);
  if (h >= p.h) return {0, kConv3x3RingNever};
  return {(image * p.h + h) * p.w + col, image};
}
// The chunk's first pixel and the keys it admits: first <= key < first + count.
struct Conv3x3RingWindow {
  int pixel, first, count;
};
__host__ __device__ inline Conv3x3RingWindow conv3x3_wrw_ring_window(
    const Conv3x3WrwRingPlan& p, int chunk) {
  const int group = chunk / p.chunks_per_image;
  if (p.images > 1)
    return {group * p.images * p.h * p.w, 0, p.batch - group * p.images};
  const int t0 = (chunk - group * p.chunks_per_image) * p.hr;
  return {(group * p.h + t0) * p.w, -t0, p.h};
}

// As launch_conv3x3_wrw.  `zeros` is at least 16 bytes of zeros on the
// device, which the lanes of the zero positions load.
void launch_conv3x3_wrw_ring(const Conv3x3WrwRingPlan& p, const void* dy,
                             const void* x, const void* zeros, float* part,
                             void* dw, hipStream_t stream);

// ---- stride-2 weight gradient (conv3x3s2_wrw) ----------------------------------
//
// dW[n][(3r+s)*C + c] = sum over (b, oh, ow) of dY[b, oh, ow, n] *
// X[b, 2*oh + r - 1, 2*ow + s - 1, c] for the 3x3 / stride 2 / padding 1
// convolution of an image with even H and W, Ho = H/2, Wo = W/2: the tile, the
// splits, the walk over chunks and the partials of conv3x3_wrw, loaded as
// conv3x3_wrw_ring loads them.  A chunk is `hr` output rows of pitch
// P = Wo + 1 and dY the strip of positions j = row*P + ow, as above.  Four
// consecutive positions have inputs two pixels apart, so X is de-interleaved
// into four parity planes, plane 2*pr + pc holding input pixel
// (2*oh + pr, 2*ow + pc) of output pixel (row, ow) at index
//
//   i = (row + pr)*P + ow + pc
//
// A pr == 1 plane starts with the output row before the chunk (or a zero row)
// and a pc == 1 plane has a zero column 0; a pc == 0 plane has its zero
// column at ow == Wo, under dY's pad.  The pr == 0 planes have no halo row.
// Tap (r, s) pairs position j with index j + conv3x3s2_wrw_tap(p, 3r+s).offset
// of plane (r != 1, s != 1); the offset is 0 .. pr*P + pc.  With even sides
// only r == 0 at oh == 0 and s == 0 at ow == 0 leave the image and reach the
// zero row or column.  Every input pixel of a chunk's footprint is in exactly
// one plane slot.
//
// A stage is one wrw_cell<64> image of `stage_pos` positions: dY's strip
// (strip_dy, a multiple of 32, so the dY / X border is a border of
// instructions and the 16-position steps are even in number), then planes 3,
// 2, 1, 0, each the indices that a position below hr*P reaches, rounded to 4.
// The positions from hr*P to strip_dy hold zeros in dY and reach on into the
// next region of the stage; the stage ends no earlier than the last of them
// reaches.  Every byte of a stage is written on every chunk, so those zeros
// meet data of this chunk or zeros, never stale bytes.  Two 7x7 images with
// the zero row between them are 640 positions, 80 KiB, exactly.
struct Conv3x3S2WrwPlan : Conv3x3WrwPlan {  // h, w: the input's
  int ho = 0, wo = 0;
  int live = 0;  // hr * pitch: the positions past it are zeros on every chunk
  // plane 2*pr + pc: first position in the stage, and positions
  int plane_base[4] = {}, plane_size[4] = {};
  int stage_pos = 0;    // positions of a stage, a multiple of 32
  int glds = 0;         // instructions of a wave per stage: stage_pos / 32
  int stage_bytes = 0;  // glds * 4096; lds_bytes = 2 * stage_bytes
};

// C and N powers of two in [64, 512], H and W even, batch*H*W within
// kBnMaxRows and Wo narrow enough for one output row to be a stage
// (Wo <= 87).  `max_workgroups` > 0 caps the grid.  group_rows and hr are
// output rows; strip_x is the positions of the four planes together.
Conv3x3S2WrwPlan conv3x3s2_wrw_plan(int64_t batch, int64_t h, int64_t w,
                                    int64_t c, int64_t n,
                                    int64_t max_workgroups = 0);

// The plane and the offset from position j of tap = 3r + s.
struct Conv3x3S2WrwTap {
  int plane, offset;
};
__host__ __device__ inline Conv3x3S2WrwTap conv3x3s2_wrw_tap(
    const Conv3x3S2WrwPlan& p, int tap) {
  const int r = tap / 3, s = tap % 3, pr = r != 1, pc = s != 1;
  return {2 * pr + pc, (r == 2 ? p.pitch : 0) + (s == 2 ? 1 : 0)};
}

// What position `pos` of a stage loads, whatever the chunk, as
// conv3x3_wrw_ring_src: the tensor, the pixel relative to the chunk's first
// (of dY, or of X, conv3x3s2_wrw_window) and the key.  The key is the output
// row relative to the chunk's first, -1 for the halo row, or with several
// images the image of the group.
struct Conv3x3S2WrwSrc {
  bool is_x;
  int pixel, key;
};
__host__ __device__ inline Conv3x3S2WrwSrc conv3x3s2_wrw_src(
    const Conv3x3S2WrwPlan& p, int pos) {
  const bool is_x = pos >= p.strip_dy;
  int pr = 0, pc = 0, i = pos;
  if (is_x) {
    const int plane = (pos < p.plane_base[2]) + (pos < p.plane_base[1]) +
                      (pos < p.plane_base[0]);  // the planes lie 3, 2, 1, 0
    i = pos - p.plane_base[plane];
    if (pos >= p.stage_pos || i >= p.plane_size[plane])
      return {true, 0, kConv3x3RingNever};
    pr = plane >> 1, pc = plane & 1;
  }
  const int rr = (int)(((unsigned)i * p.magic_pitch) >> kConv3x3MagicShift);
  const int ow = i - rr * p.pitch - pc, t = rr - pr;
  if (t >= p.hr || ow < 0 || ow >= p.wo) return {is_x, 0, kConv3x3RingNever};
  int image = 0, oh = t, key = t;
  if (p.images > 1) {
    if (t < 0) return {is_x, 0, kConv3x3RingNever};
    image = (int)(((unsigned)t * p.magic_h1) >> kConv3x3MagicShift);
    oh = t - image * (p.ho + 1);
    if (oh >= p.ho) return {is_x, 0, kConv3x3RingNever};
    key = image;
  }
  if (!is_x) return {false, (image * p.ho + oh) * p.wo + ow, key};
  return {true, (image * p.h + 2 * oh + pr) * p.w + 2 * ow + pc, key};
}
// The chunk's first pixel of dY and of X and the keys it admits.
struct Conv3x3S2WrwWindow {
  int pixel_dy, pixel_x, first, count;
};
__host__ __device__ inline Conv3x3S2WrwWindow conv3x3s2_wrw_window(
    const Conv3x3S2WrwPlan& p, int chunk) {
  const int group = chunk / p.chunks_per_image;
  if (p.images > 1)
    return {group * p.images * p.ho * p.wo, group * p.images * p.h * p.w, 0,
            p.batch - group * p.images};
  const int t0 = (chunk - group * p.chunks_per_image) * p.hr;
  return {(group * p.ho + t0) * p.wo, (group * p.h + 2 * t0) * p.w, -t0, p.ho};
}
// The position of the stage that the 16 bytes of `lane` of instruction j of
// `wave` are (conv1x1_wrw_ring_piece), and their 16-byte vector of the 64
// channels.
__host__ __device__ inline Conv3x3RingSlot conv3x3s2_wrw_slot(int wave, int j,
                                                              int lane) {
  const WrwImageSlot s = conv1x1_wrw_image_slot(
      64, conv1x1_wrw_ring_piece(wave, j) + 16 * lane);
  return {false, s.row, s.channel / 8};
}

// As launch_conv3x3_wrw_ring, dy[B, Ho, Wo, N] and x[B, H, W, C].
void launch_conv3x3s2_wrw(const Conv3x3S2WrwPlan& p, const void* dy,
                          const void* x, const void* zeros, float* part,
                          void* dw, hipStream_t stream);

// ---- forward with BatchNorm partials (conv3x3_stats) -------------------------
//
// Y[R, N] = sum over the nine taps t of X_t[R, C] * W_t[N, C]^T, R = B*H*W the
// pixels in memory order.  The rows of the GEMM are the pixels themselves, not
// positions of a padded strip: a 256-thread workgroup owns 64 output channels
// and walks tiles of 256 consecutive pixels, whatever images they belong to
// (at 7x7 a tile holds more than five images), wave w rows 64*w .. 64*w+63 as
// two 32-row sub-tiles.  The strip of a tile is the pixels 256*t - (W+1) ..
// 256*t + 256 + W of one 32-channel chunk of X in LDS, so tap (r, s) of tile
// row m is strip index m + r*W + s: the nine taps share the strip and differ
// by an LDS offset.  The strip has no zero pads.  A neighbour that lies in
// another image row, another image or outside the tensor is a row of the
// strip like any other (outside the tensor: the nearest pixel inside), and
// the lane sets its operand to zero in registers: conv3x3_fwd_taps gives the
// pixel's nine validity bits.  So no tile row is a pad, every row below R is
// stored and pushed into the moments, and the count of a workgroup is the
// number of pixels it walked.
//
// The weight goes through LDS in [tap][64][32] chunks, one per chunk of the
// strip, both double-buffered.  At C == 64 the two chunks are the two buffers
// and stay (`resident`).  The grid, the walk, the moments and the partials are
// those of conv1x1_tiled_plan: `splits` persistent workgroups per channel
// tile, each writing one row [mean(N) | M2(N) | count(ntiles)].
constexpr int kConv3x3FwdTileRows = 256;
constexpr int kConv3x3FwdBn = 64;
constexpr int kConv3x3FwdKc = 32;
// bytes of one weight chunk, [9][64][32] bf16
constexpr int kConv3x3FwdWBytes = 9 * kConv3x3FwdBn * kConv3x3FwdKc * 2;
// a thread's share of a strip, in 16-byte vectors: 64 strip rows each
constexpr int kConv3x3FwdXVecs = 9;

struct Conv3x3FwdPlan {
  int batch = 0, h = 0, w = 0, c = 0, n = 0;
  int rows = 0;  // R
  bool eligible = false;
  bool native = false;  // measured faster than MIOpen + bn_stats
  int bn = 0;           // channels per workgroup
  int ntiles = 0;       // workgroups across N
  int tile_rows = 0;
  int kc = 0, nchunks = 0;  // channel chunk and C / kc
  bool resident = false;    // C == 64: the weight is staged once
  int row_tiles = 0;        // ceil(R / tile_rows)
  int strip_rows = 0;       // tile_rows + 2W + 2
  int xvecs = 0;            // ceil(strip_rows / 64); a buffer holds 64 * xvecs
  int splits = 0;           // persistent workgroups per channel tile
  int grid = 0;             // ntiles * splits
  int tiles_per_split = 0;  // longest walk
  int run = 0;              // per-lane run length: 32 * tiles_per_split
  int lds_bytes = 0;
  int pstride = 0;             // floats per partial row: 2*N + ntiles
  int64_t partial_floats = 0;  // splits * pstride
};

// C and N powers of two in [64, 512], 2 <= B*H*W <= kBnMaxRows, and W up to
// 159, where the two strip buffers fill what LDS the weight leaves.
// `max_workgroups` > 0 caps the grid.
Conv3x3FwdPlan conv3x3_fwd_plan(int64_t batch, int64_t h, int64_t w, int64_t c,
                                int64_t n, int64_t max_workgroups = 0);

// Workgroup -> (channel tile, split) as conv1x1_tiled_ntile / _split; split s
// walks row tiles s, s + splits, ...
__host__ __device__ inline int conv3x3_fwd_ntile(const Conv3x3FwdPlan& p,
                                                 int wg) {
  return p.splits % 8 == 0 ? (wg / 8) % p.ntiles : wg % p.ntiles;
}
__host__ __device__ inline int conv3x3_fwd_split(const Conv3x3FwdPlan& p,
                                                 int wg) {
  return p.splits % 8 == 0 ? (wg / 8 / p.ntiles) * 8 + wg % 8 : wg / p.ntiles;
}
// The pixel that index i of tile t's strip holds.
__host__ __device__ inline int conv3x3_fwd_strip_row(const Conv3x3FwdPlan& p,
                                                     int t, int i) {
  const int r = t * kConv3x3FwdTileRows - (p.w + 1) + i;
  return r < 0 ? 0 : r < p.rows ? r : p.rows - 1;
}
// The strip index that tap = 3r + s of tile row m reads.
__host__ __device__ inline int conv3x3_fwd_strip_index(const Conv3x3FwdPlan& p,
                                                       int m, int tap) {
  return m + (tap / 3) * p.w + tap % 3;
}
// Bit 3r + s is set where pixel `row` has a neighbour (h+r-1, w+s-1) in its
// own image.
__host__ __device__ inline unsigned conv3x3_fwd_taps(const Conv3x3FwdPlan& p,
                                                     int row) {
  const int line = row / p.w, w = row - line * p.w, h = line % p.h;
  const unsigned cols = (w > 0 ? 1u : 0u) | 2u | (w + 1 < p.w ? 4u : 0u);
  return (h > 0 ? cols : 0u) | cols << 3 | (h + 1 < p.h ? cols << 6 : 0u);
}

// y[B, H, W, N] bf16 and part[splits, pstride] fp32 from x[B, H, W, C] and
// w[N, 3, 3, C] bf16; every pointer 16-byte aligned.
void launch_conv3x3_stats(const Conv3x3FwdPlan& p, const void* x, const void* w,
                          void* y, float* part, hipStream_t stream);

// ---- stride-2 forward with BatchNorm partials (conv3x3s2_stats) --------------
//
// The same GEMM for a 3x3 / stride 2 / padding 1 convolution of an image with
// even H and W: R = B*Ho*Wo output pixels in memory order, Ho = H/2, Wo = W/2.
// Output pixel (oh, ow) and tap (r, s) read input (2*oh + r - 1, 2*ow + s - 1),
// so consecutive output pixels have neighbours two input pixels apart and one
// strip with an offset per tap no longer serves.  The strip of a tile is four
// parity planes instead: entry m = (b, oh, ow) of plane (pr, pc) holds input
// pixel (b, 2*oh + pr, 2*ow + pc).  r == 1 is the even row of oh, r == 2 the
// odd row of oh and r == 0 the odd row of oh - 1, columns alike, so tap (r, s)
// of tile row m is entry m - (r == 0)*Wo - (s == 0) of plane (r != 1, s != 1):
// the nine taps again differ by an LDS base and offset.  Plane (1, 1) serves
// four taps and has a halo of Wo + 1 entries before the tile, (1, 0) two taps
// and Wo, (0, 1) two taps and 1, (0, 0) the centre tap and none.  Every input
// pixel of a tile's footprint is in exactly one plane and is loaded once.
//
// There are no zero pads.  An entry outside the tensor holds the entry nearest
// inside, and with even H and W only r == 0 (needs oh > 0) and s == 0 (needs
// ow > 0) can leave the image: the lane clears those operands in registers.
//
// A tile is 128 output pixels, wave w rows 32*w .. 32*w+31 with all 64
// channels, and a stage one 32-channel chunk of it: 4*128 + 2*Wo + 2 entries
// of 64 bytes.  With the two [9][64][32] weight chunks (72 KiB) and the
// epilogue's stage (16 KiB) two strip buffers may take 36 KiB each, 576
// entries, nine vectors a thread: Wo <= 31, W <= 62.  A 256-pixel tile would
// need 68 KiB a buffer at Wo = 28 and not fit twice.  The weight is always
// streamed (C == 64 is two chunks); grid, walk, moments and partials are
// those of conv3x3_stats with 16 values per lane and tile.
constexpr int kConv3x3S2TileRows = 128;
// a thread's share of a strip, in 16-byte vectors: 64 entries each
constexpr int kConv3x3S2XVecs = 9;

struct Conv3x3S2FwdPlan : Conv3x3FwdPlan {  // h, w: the input's; rows: B*Ho*Wo
  int ho = 0, wo = 0;
  // plane 2*pr + pc: first entry in the strip, and entries (tile_rows + halo)
  int plane_base[4] = {}, plane_rows[4] = {};
  unsigned magic_wo = 0, magic_ho = 0;  // conv3x3s2_div; 0 where the divisor is 1
};

// C and N powers of two in [64, 512], H and W even, W <= 62, H <= 2048 (the
// divisions below), 2 <= B*Ho*Wo and B*H*W <= kBnMaxRows.  `max_workgroups`
// > 0 caps the grid.
Conv3x3S2FwdPlan conv3x3s2_fwd_plan(int64_t batch, int64_t h, int64_t w,
                                    int64_t c, int64_t n,
                                    int64_t max_workgroups = 0);

// v / d for v * d < 2^32 (v < 2^22 output rows, d <= 2^10), magic =
// ceil(2^32 / d), which is 2^32 and stored as 0 at d == 1
__host__ __device__ inline int conv3x3s2_div(int v, unsigned magic) {
  return magic == 0
             ? v
             : (int)(((unsigned long long)(unsigned)v * magic) >> 32);
}
// The input pixel (b*H + ih)*W + iw that entry e of tile t's strip holds.
__host__ __device__ inline int conv3x3s2_fwd_strip_pixel(
    const Conv3x3S2FwdPlan& p, int t, int e) {
  const int pl = (e >= p.plane_base[1]) + (e >= p.plane_base[2]) +
                 (e >= p.plane_base[3]);
  int m = t * kConv3x3S2TileRows - (p.plane_rows[pl] - kConv3x3S2TileRows) +
          (e - p.plane_base[pl]);
  m = m < 0 ? 0 : m < p.rows ? m : p.rows - 1;
  const int line = conv3x3s2_div(m, p.magic_wo), ow = m - line * p.wo;
  return (2 * line + (pl >> 1)) * p.w + 2 * ow + (pl & 1);
}
// The strip entry that tap = 3r + s of tile row m reads.
__host__ __device__ inline int conv3x3s2_fwd_strip_index(
    const Conv3x3S2FwdPlan& p, int m, int tap) {
  const int r = tap / 3, s = tap % 3, pl = 2 * (r != 1) + (s != 1);
  return p.plane_base[pl] + (p.plane_rows[pl] - kConv3x3S2TileRows) + m -
         (r == 0 ? p.wo : 0) - (s == 0 ? 1 : 0);
}
// Bit 3r + s is set where output pixel `row` has its neighbour
// (2*oh + r - 1, 2*ow + s - 1) in its own image.
__host__ __device__ inline unsigned conv3x3s2_fwd_taps(
    const Conv3x3S2FwdPlan& p, int row) {
  const int line = conv3x3s2_div(row, p.magic_wo), ow = row - line * p.wo;
  const int oh = line - conv3x3s2_div(line, p.magic_ho) * p.ho;
  const unsigned cols = (ow > 0 ? 1u : 0u) | 6u;
  return (oh > 0 ? cols : 0u) | cols << 3 | cols << 6;
}

// y[B, Ho, Wo, N] bf16 and part[splits, pstride] fp32 from x[B, H, W, C] and
// w[N, 3, 3, C] bf16; every pointer 16-byte aligned.
void launch_conv3x3s2_stats(const Conv3x3S2FwdPlan& p, const void* x,
                            const void* w, void* y, float* part,
                            hipStream_t stream);

// ---- input gradient (conv3x3_bwd_data) ----------------------------------------
//
// dX[R, C] = sum over the nine taps t of dY_t[R, N] * W_{8-t}[N, C]: the
// forward's GEMM with the roles of C and N exchanged, on the same strip with
// the same validity bits (H, W and the padding are the forward's).  So the
// plan is the forward's plan of the exchanged problem, and its fields keep
// the kernel's meaning: `c` is the contraction depth, the N of dY, and `n` the
// output width, the C of dX; `nchunks` and `resident` follow N, `ntiles` C.
// There are no partials: pstride and partial_floats are 0.  `native` comes
// from a table of its own.  Eligibility is the forward's.
Conv3x3FwdPlan conv3x3_bwd_plan(int64_t batch, int64_t h, int64_t w, int64_t c,
                                int64_t n, int64_t max_workgroups = 0);

// dx[B, H, W, C] bf16 from dy[B, H, W, N] and w[N, 3, 3, C] bf16, the
// convolution's own weight, read transposed; every pointer 16-byte aligned.
void launch_conv3x3_bwd_data(const Conv3x3FwdPlan& p, const void* dy,
                             const void* w, void* dx, hipStream_t stream);

// ---- stride-2 input gradient (conv3x3s2_bwd_data) -----------------------------
//
// dX[b, c, ih, iw] = sum over n, r, s of dY[b, n, oh, ow] * W[n, c, r, s] with
// 2*oh = ih + 1 - r and 2*ow = iw + 1 - s: the input gradient of the 3x3 /
// stride 2 / padding 1 convolution of an image with even H and W.  Written
// directly, without inserted zeros: with ih = 2a + ph, iw = 2b + pw the four
// pixels of the 2x2 cell of dY row m = (image, a, b) are four classes
// cls = 2*ph + pw, and a class sums the shifts k that are subsets of its bits,
// shift k being dY row m + (k & 1) + (k & 2 ? Wo : 0):
//
//   class 0   W(1,1) dY[m]
//   class 1   W(1,2) dY[m] + W(1,0) dY[m+1]
//   class 2   W(2,1) dY[m] + W(0,1) dY[m+Wo]
//   class 3   W(2,2) dY[m] + W(2,0) dY[m+1] + W(0,2) dY[m+Wo] + W(0,0) dY[m+Wo+1]
//
// Nine products per dY row, the convolution's real flops, into four
// accumulator sets.  The GEMM rows are the R = B*Ho*Wo rows of dY in memory
// order, a tile 128 of them, and its strip rows T*t .. T*t + T + Wo of one
// 32-deep chunk of dY's channels: the four shifts differ by an LDS offset.
// Shift bit 0 needs b + 1 < Wo and bit 1 needs a + 1 < Ho, two validity bits a
// row, and the lane clears the operand in registers; an entry past the tensor
// holds the last row and is only ever reached with its bit clear.  With even H
// and W every pixel of dX belongs to exactly one (row, class): each is
// written once, with no fill and no second pass.
//
// The plan keeps conv3x3_bwd_plan's meaning of the fields: `c` is the
// contraction depth, the N of dY, and `n` the output width, the C of dX; h
// and w are dX's, rows is R.  LDS holds the two [9][32 n][64 c] weight chunks
// of conv3x3_bwd_data (72 KiB), the whole rounded output of a tile, four
// classes of [128][64] bf16 (64 KiB), from which 128-byte runs go to dX, and
// two strip buffers in the 24 KiB that remain: three vectors a thread, 192
// entries, Wo <= 63.  So LDS, through the output stage, bounds the width:
// W <= 126.
constexpr int kConv3x3S2BwdTileRows = 128;
// a thread's share of a strip, in 16-byte vectors: 64 entries each
constexpr int kConv3x3S2BwdXVecs = 3;
// bytes of the output stage: [4 classes][128 rows][64 channels] bf16
constexpr int kConv3x3S2BwdStageBytes = 4 * kConv3x3S2BwdTileRows * 64 * 2;

struct Conv3x3S2BwdPlan : Conv3x3FwdPlan {
  int ho = 0, wo = 0;
  unsigned magic_wo = 0, magic_ho = 0;  // conv3x3s2_div
};

// C and N powers of two in [64, 512], H and W even, W <= 126, H <= 2048 (the
// divisions), 2 <= B*Ho*Wo and B*H*W <= kBnMaxRows.  `max_workgroups` > 0
// caps the grid.  `native` comes from a table of its own.
Conv3x3S2BwdPlan conv3x3s2_bwd_plan(int64_t batch, int64_t h, int64_t w,
                                    int64_t c, int64_t n,
                                    int64_t max_workgroups = 0);

// The dY row that entry i of tile t's strip holds.
__host__ __device__ inline int conv3x3s2_bwd_strip_row(
    const Conv3x3S2BwdPlan& p, int t, int i) {
  const int r = t * kConv3x3S2BwdTileRows + i;
  return r < p.rows ? r : p.rows - 1;
}
// The strip entry that shift k of tile row m reads.
__host__ __device__ inline int conv3x3s2_bwd_strip_index(
    const Conv3x3S2BwdPlan& p, int m, int k) {
  return m + (k & 1) + (k & 2 ? p.wo : 0);
}
// Bit 0 is set where dY row `row` has a right neighbour in its image row, bit
// 1 where it has a neighbour below in its image: shift k is valid where
// (bits & k) == k.
__host__ __device__ inline unsigned conv3x3s2_bwd_valid(
    const Conv3x3S2BwdPlan& p, int row) {
  const int line = conv3x3s2_div(row, p.magic_wo), b = row - line * p.wo;
  const int a = line - conv3x3s2_div(line, p.magic_ho) * p.ho;
  return (b + 1 < p.wo ? 1u : 0u) | (a + 1 < p.ho ? 2u : 0u);
}
// Term `term` of class cls: its shift k, the term-th subset of the class's
// bits in ascending order, and the weight tap 3r + s it multiplies; tap -1
// where the class has fewer terms.
struct Conv3x3S2BwdTerm {
  int tap, shift;
};
__host__ __device__ constexpr Conv3x3S2BwdTerm conv3x3s2_bwd_term(int cls,
                                                                  int term) {
  const int k = cls == 2 ? 2 * term : term;
  if (term < 0 || k > 3 || (k & cls) != k) return {-1, 0};
  const int r = cls & 2 ? (k & 2 ? 0 : 2) : 1;
  const int s = cls & 1 ? (k & 1 ? 0 : 2) : 1;
  return {3 * r + s, k};
}
// The pixel (image*H + ih)*W + iw of dX that class cls of dY row `row` is.
__host__ __device__ inline int conv3x3s2_bwd_pixel(const Conv3x3S2BwdPlan& p,
                                                   int row, int cls) {
  const int line = conv3x3s2_div(row, p.magic_wo), b = row - line * p.wo;
  return (2 * line + (cls >> 1)) * p.w + 2 * b + (cls & 1);
}

// dx[B, H, W, C] bf16 from dy[B, Ho, Wo, N] and w[N, 3, 3, C] bf16, the
// convolution's own weight, read transposed; every pointer 16-byte aligned.
void launch_conv3x3s2_bwd_data(const Conv3x3S2BwdPlan& p, const void* dy,
                               const void* w, void* dx, hipStream_t stream);

}  // namespace cgx
