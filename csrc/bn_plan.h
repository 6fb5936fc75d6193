// Launch geometry of the fused NHWC bf16 BatchNorm kernels (bn_kernels.hip).
//
// Pure host arithmetic, like plan.h: no HIP calls, no ATen.  A channels_last
// activation is a dense [R, C] bf16 matrix (R = N*H*W) of 16-byte vectors,
// 8 consecutive channels of one row each: C/8 "channel groups" per row.
//
// A 256-thread workgroup owns a tile of `tc` channel groups (at most 32, i.e.
// 512 contiguous bytes per row) and sweeps `rln` = 256/tc rows per iteration;
// `splits` workgroups share one channel tile and stride over the rows
// together.  A thread therefore keeps its channel group for the whole sweep
// and accumulates its 8 channels in registers.  Every reduction writes one
// fp32 partial row per (split, channel), merged in a fixed order by a
// finalize kernel, so `splits` is capped to keep the partials a few per cent
// of the tensor's bytes: with one tile over all of C = 2048 a full grid would
// need a partial row per 1-row workgroup iteration.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cgx {

constexpr int kBnThreads = 256;     // workgroup size of every sweep kernel
constexpr int kBnTargetWgs = 1024;  // 256 CUs x 4 resident workgroups
constexpr int kBnMaxTileCgs = 32;   // channel groups per tile (256 channels)
constexpr int kBnFinChannels = 4;   // channels per finalize workgroup

struct BnPlan {
  int64_t rows = 0;  // R
  int channels = 0;  // C
  bool eligible = false;
  int cgs = 0;              // channel groups per row, C/8
  int tc = 0;               // channel groups per tile
  int ctiles = 0;           // tiles across C
  int rln = 0;              // rows per workgroup iteration, 256/tc
  int splits = 0;           // workgroups striding over the rows of one tile
  int grid = 0;             // ctiles * splits
  int rows_per_thread = 0;  // longest per-thread run, ceil(R / (splits*rln))
  int64_t partial_floats = 0;  // one reduction's partial buffer: splits * C
};

// C a power of two in [8, 2048] (so 8*256 is a multiple of C) and
// 2 <= R <= 2^24: the unbiased running variance divides by R-1, and the
// kernels count rows in fp32, which is exact only up to 2^24.
constexpr int64_t kBnMaxRows = int64_t(1) << 24;
BnPlan bn_plan(int64_t rows, int64_t channels);

// Where thread `tid` of workgroup `wg` starts and how it steps: the sweep the
// kernels run and the one the CPU tests replay.
struct BnSweep {
  int cg;          // the thread's channel group, constant over the sweep
  int64_t row;     // first row
  int64_t stride;  // rows between iterations
};

__host__ __device__ inline BnSweep bn_sweep(const BnPlan& p, int wg, int tid) {
  const int ct = wg % p.ctiles, split = wg / p.ctiles;
  return BnSweep{ct * p.tc + tid % p.tc,
                 (int64_t)split * p.rln + tid / p.tc,
                 (int64_t)p.splits * p.rln};
}

// Vector index of (row, cg) in the [R, C/8] matrix of 16-byte vectors.
__host__ __device__ inline int64_t bn_vec(const BnPlan& p, int64_t row,
                                          int cg) {
  return row * p.cgs + cg;
}

// Where workgroup `wg` puts the 8 partials of channel group `cg` in a
// [splits, C] partial buffer.
__host__ __device__ inline int64_t bn_partial_offset(const BnPlan& p, int wg,
                                                     int cg) {
  return (int64_t)(wg / p.ctiles) * p.channels + (int64_t)cg * 8;
}

// Per-channel (count, mean, M2) partials as bn_stats_finalize merges them:
// partial s of channel c is mean[s*pstride + c], m2[s*pstride + c] with the
// count cnt[s*cstride + (c/8)/tc].  bn_stats writes [splits, C] arrays and one
// count per (split, channel tile); the 1x1 convolution (conv1x1_plan.h) writes
// one [mean | M2 | counts] row per persistent workgroup.
struct BnPartials {
  const float* mean = nullptr;
  const float* m2 = nullptr;
  const float* cnt = nullptr;
  int channels = 0;
  int splits = 0;   // partials per channel
  int tc = 0;       // channel groups that share one count
  int pstride = 0;  // floats between consecutive partials of a channel
  int cstride = 0;  // floats between consecutive counts of a channel tile
};

// Kernel launches (bn_kernels.hip), all on `stream`.  `part` holds
// 2*partial_floats + grid floats of workspace.  With `stats` set the
// statistics pass is skipped and those partials are finalized instead.
struct BnForwardArgs {
  const void* x;         // [R, C] bf16
  const void* identity;  // [R, C] bf16 or null
  const float* weight;
  const float* bias;
  float* running_mean;
  float* running_var;
  float momentum, eps;
  bool relu;
  void* out;      // [R, C] bf16
  float* mean;    // [C]
  float* invstd;  // [C]
  uint8_t* mask;  // [R*C/8], written iff relu
  float* part;
  const BnPartials* stats = nullptr;
};
void launch_bn_forward(const BnPlan& p, const BnForwardArgs& a,
                       hipStream_t stream);

struct BnBackwardArgs {
  const void* dy;  // [R, C] bf16
  const void* x;
  const float* mean;
  const float* invstd;
  const float* weight;
  const uint8_t* mask;  // null: no ReLU
  void* dx;             // [R, C] bf16
  void* didentity;      // [R, C] bf16 masked dy, or null
  float* dgamma;        // [C]
  float* dbeta;         // [C]
  float* part;
};
void launch_bn_backward(const BnPlan& p, const BnBackwardArgs& a,
                        hipStream_t stream);

// ---- residual join of two BatchNorms: relu(bn3(x3) + bn_d(xd)) -------------
//
// Same plan for both operands (same shape).  `part` holds two forward
// workspaces back to back (2 * (2*partial_floats + grid) floats); the backward
// uses its first 3*partial_floats.
struct BnOperand {
  const void* x;  // [R, C] bf16
  const float* weight;
  const float* bias;    // forward only
  float* running_mean;  // forward only
  float* running_var;   // forward only
  float momentum, eps;  // forward only
  float* mean;          // [C], written by the forward, read by the backward
  float* invstd;        // [C]
  void* dx;             // [R, C] bf16, backward only
  float* dgamma;        // [C], backward only
  float* dbeta;         // [C], backward only
  const BnPartials* stats = nullptr;  // forward only, as in BnForwardArgs
};
struct BnJoinArgs {
  BnOperand a, b;  // the block's bn3 and its downsample BatchNorm
  bool relu;
  void* out;        // forward: [R, C] bf16
  const void* dy;   // backward: [R, C] bf16
  uint8_t* mask;    // [R*C/8]; written by the forward, read by the backward
  float* part;
};
void launch_bn_join_forward(const BnPlan& p, const BnJoinArgs& a,
                            hipStream_t stream);
void launch_bn_join_backward(const BnPlan& p, const BnJoinArgs& a,
                             hipStream_t stream);

// ---- stem: BatchNorm + ReLU + 3x3 / stride 2 / pad 1 max-pool ---------------
//
// Along one axis of `in` pixels there are (in-1)/2 + 1 pooled positions;
// pooled position o looks at the input coordinates 2*o-1+k, k = 0..2, of
// which those in [0, in) exist.  Input coordinate i is covered by the pooled
// positions i/2 .. min((i+1)/2, out-1): one if i is even, two if it is odd
// and not cut off by the border.  A window position is kh*3+kw; kPoolNone
// marks a pooled element that passes no gradient (its value is <= 0).
constexpr int kPoolNone = 9;

struct BnPoolPlan {
  int n = 0, h = 0, w = 0;  // input pixels
  int oh = 0, ow = 0;       // pooled pixels
  int cgs = 0;              // channel groups per pixel
  int64_t threads = 0;      // forward: one per (pooled pixel, channel group)
  int grid = 0;             // forward workgroups of kBnThreads
};
BnPoolPlan bn_pool_plan(int64_t n, int64_t h, int64_t w, int64_t channels);

__host__ __device__ inline int pool_out(int in) { return (in - 1) / 2 + 1; }
__host__ __device__ inline int pool_in(int o, int k) { return 2 * o - 1 + k; }
__host__ __device__ inline int pool_cover_lo(int i) { return i / 2; }
__host__ __device__ inline int pool_cover_hi(int i, int out) {
  const int hi = (i + 1) / 2;
  return hi < out ? hi : out - 1;
}
// window position (along one axis) at which pooled position o sees input i
__host__ __device__ inline int pool_k(int i, int o) { return i - (2 * o - 1); }

struct BnPoolArgs {
  const void* x;  // [N, H, W, C] bf16
  const float* weight;
  const float* bias;
  float* running_mean;
  float* running_var;
  float momentum, eps;
  float* mean;
  float* invstd;
  void* out;        // forward: [N, OH, OW, C] bf16
  uint8_t* arg;     // [N, OH, OW, C] window position of the maximum
  const void* dy;   // backward: [N, OH, OW, C] bf16
  void* dx;         // backward: [N, H, W, C] bf16
  float* dgamma;
  float* dbeta;
  float* part;      // as for launch_bn_forward
};
void launch_bn_pool_forward(const BnPlan& p, const BnPoolPlan& g,
                            const BnPoolArgs& a, hipStream_t stream);
void launch_bn_pool_backward(const BnPlan& p, const BnPoolPlan& g,
                             const BnPoolArgs& a, hipStream_t stream);

}  // namespace cgx
