// The 3x3 / stride 1 / padding 1 convolution on channels_last bf16 tensors as
// implicit GEMMs: the weight gradient (conv3x3_wrw, first), the forward that
// also produces BatchNorm partials (conv3x3_stats, below it) and the input
// gradient (conv3x3_bwd_data), each with its own description; between
// the last two the forward of the 3x3 / stride 2 / padding 1 convolution
// (conv3x3s2_stats), last its input gradient (conv3x3s2_bwd_data), and after
// the ring its weight gradient (conv3x3s2_wrw).
// Geometry: conv3x3_plan.h.
//
// dW[n][(3r+s)*C + c] = sum over pixels of dY[b, h, w, n] * X[b, h+r-1, w+s-1, c].
// Both operands have the contracted index slow, so both MFMA operands are
// read transposed from LDS images as in conv1x1_wrw (wrw_image.h): dY^T is
// the A operand and X the B operand of v_mfma_f32_32x32x16_bf16.  What is new
// is that the nine taps share one staged copy of both:
//
//   dY strip  position j = row*P + w of the chunk's rows, P = W+1; the pad
//             w = W, the rows past the chunk and the positions up to the
//             next multiple of 16 are zeros
//   X strip   rows -1 .. hr of the chunk at index i = (row+1)*P + wx + 1;
//             column 0 is zero and serves as column W of the row before;
//             rows that are no image row (conv3x3_wrw_row) are zeros
//
// Tap (r, s) then pairs position j with index j + r*P + s: at w = 0, s = 0
// and at w = W-1, s = 2 that is a zero column of X, above the first and
// below the last row of an image a zero row, and at a pad of dY the dY factor
// is zero.  Every index that a position below strip_dy reaches, up to
// strip_dy + 2P + 1, is written on every chunk, so no product has a stale
// factor (0 * NaN is not 0).  The inner loop has no masks and no loads per
// tap: one A operand and nine B operands, at nine LDS offsets, feed nine MFMAs
// per 32x32 tile and 16-position step.
//
// Bank conflicts.  A transposed read takes, per 32-lane half, one 64-byte cell
// of four consecutive positions (conv1x1_wrw argues why these must sit in the
// four different 64-byte columns of a 256-byte line).  With the taps the four
// positions start anywhere, not at a multiple of four.  The swizzle still
// separates them.  The one instantiation is the 64 x 64 tile, so both images
// are wrw_cell<64>: the column is 2*(r & 1) + (u ^ ((r >> 1) & 1)) and the
// pair (r & 1, (r >> 1) & 1) takes all four values on four consecutive
// positions.  (A 128-wide image, which no instantiation has yet, would have
// column (u ^ r) & 3, and r & 3 takes four values likewise.)  A step moves
// every address by 16 positions and the second read of an operand by 4, which
// changes neither r & 3 nor the pair: a lane keeps one base address per tap
// and 32-channel tile, and the loop adds a multiple of the position stride.  Every address is a multiple of 8 and
// inside the image, and no divergent branch encloses the reads: EXEC is all
// ones.
//
// The global loads of the next chunk are issued before the MFMAs of the
// current one and wait in registers.  A load that is to give zeros is
// pointed at the first pixel and replaced, so nothing outside the two
// tensors is read.  Each workgroup stores its fp32 tile to its split's plane
// of `part`; conv1x1_wrw_finalize sums the planes in a fixed order and rounds
// once: no atomics, the same bits every run.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bn_moments.h"
#include "check.h"
#include "conv3x3_plan.h"
#include "conv_epilogue.h"
#include "wrw_image.h"

namespace cgx {
namespace {

constexpr int kT = kConvThreads;

// Thread tid's vectors of one strip of `chunk`: C channels from c0 of
// src[pixels, width].  IS_X: the strip starts a row and a column early.
template <int C, int NV, bool IS_X>
__device__ inline void conv3x3_load(uint4 (&v)[NV],
                                    const uint4* __restrict__ src,
                                    const Conv3x3WrwPlan& p, int chunk, int c0,
                                    int tid) {
  const int group = chunk / p.chunks_per_image;
  const int t0 = (chunk % p.chunks_per_image) * p.hr - (IS_X ? 1 : 0);
  const int strip = IS_X ? p.strip_x : p.strip_dy;
  const int width = IS_X ? p.c : p.n;
  const int rows = p.hr + (IS_X ? 2 : 0);
  const int nv = (strip * (C / 8) + kT - 1) / kT;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    if (i < nv) {  // uniform
      const int idx = tid + i * kT, j = idx / (C / 8), q = idx % (C / 8);
      const int rr = (int)(((unsigned)j * p.magic_pitch) >> kConv3x3MagicShift);
      const int col = j - rr * p.pitch - (IS_X ? 1 : 0);
      const int row = conv3x3_wrw_row(p, group, t0 + rr);
      const bool live = row >= 0 && rr < rows && col >= 0 && col < p.w;
      const int64_t pixel = live ? (int64_t)row * p.w + col : 0;
      const uint4 t = src[(pixel * width + c0) / 8 + q];
      v[i] = live ? t : make_uint4(0, 0, 0, 0);
    }
  }
}

// ... into the image: position j's 16-byte vector q, as wrw_store.
template <int C, int NV>
__device__ inline void conv3x3_store(char* img, const uint4 (&v)[NV], int strip,
                                     int tid) {
#pragma unroll
  for (int i = 0; i < NV; i++) {
    const int idx = tid + i * kT, j = idx / (C / 8), q = idx % (C / 8);
    if (j < strip)
      *reinterpret_cast<uint4*>(img + wrw_cell<C>(j, q >> 2) + 16 * (q & 3)) =
          v[i];
  }
}

template <int BN, int BK>
__global__ __launch_bounds__(kT) void conv3x3_wrw(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    float* __restrict__ part, Conv3x3WrwPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int MT = BN / 64, KT = BK / 64;  // 32x32 tiles of a wave, per tap
  // the registers a thread stages with hold the same bytes at every tile
  constexpr int DV = kConv3x3DyVecs, XV = kConv3x3XVecs;
  char* img_n = reinterpret_cast<char*>(lds);
  char* img_k = img_n + p.strip_dy * BN * 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int wn = wave >> 1, wk = wave & 1;
  const int tile = conv3x3_wrw_tile(p, blockIdx.x);
  const int split = conv3x3_wrw_split(p, blockIdx.x);
  const int n0 = (tile / p.ntiles_k) * BN, k0 = (tile % p.ntiles_k) * BK;

  // as conv1x1_wrw: lane 4q+pp of a 16-lane group supplies position 8h+q of
  // the step's first read; tap (r, s) shifts X by r*P + s positions
  const int q = (lane >> 2) & 3;
  const int in_cell = 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  int an[MT], ak[9][KT];
#pragma unroll
  for (int j = 0; j < MT; j++)
    an[j] = wrw_cell<BN>(8 * h + q, wn * MT + j) + in_cell;
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int j = 0; j < KT; j++)
      ak[tap][j] = wrw_cell<BK>(8 * h + q + (tap / 3) * p.pitch + tap % 3,
                                wk * KT + j) +
                   in_cell;

  f32x16 acc[9][MT][KT];
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int jm = 0; jm < MT; jm++)
#pragma unroll
      for (int jk = 0; jk < KT; jk++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[tap][jm][jk][e] = 0.f;

  uint4 vn[DV], vk[XV];
  int chunk = split;  // < p.chunks: no more splits than chunks
  conv3x3_load<BN, DV, false>(vn, dy, p, chunk, n0, tid);
  conv3x3_load<BK, XV, true>(vk, x, p, chunk, k0, tid);
  const int steps = p.strip_dy / 16;

  while (chunk < p.chunks) {
    __syncthreads();  // the previous chunk has been read
    conv3x3_store<BN, DV>(img_n, vn, p.strip_dy, tid);
    conv3x3_store<BK, XV>(img_k, vk, p.strip_x, tid);
    __syncthreads();
    chunk += p.splits;
    if (chunk < p.chunks) {
      conv3x3_load<BN, DV, false>(vn, dy, p, chunk, n0, tid);
      conv3x3_load<BK, XV, true>(vk, x, p, chunk, k0, tid);
    }
    // Two sets of operand registers: the reads of a step are issued before
    // the MFMAs of the step before it, so that no MFMA waits for LDS.
    bf16x8 a0[MT], b0[9][KT], a1[MT], b1[9][KT];
    auto read = [&](bf16x8 (&a)[MT], bf16x8 (&b)[9][KT], int s) {
#pragma unroll
      for (int j = 0; j < MT; j++) a[j] = wrw_operand<BN>(img_n, an[j], s);
#pragma unroll
      for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int j = 0; j < KT; j++)
          b[tap][j] = wrw_operand<BK>(img_k, ak[tap][j], s);
    };
    auto mma = [&](const bf16x8 (&a)[MT], const bf16x8 (&b)[9][KT]) {
#pragma unroll
      for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int jm = 0; jm < MT; jm++)
#pragma unroll
          for (int jk = 0; jk < KT; jk++)
            acc[tap][jm][jk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a[jm], b[tap][jk], acc[tap][jm][jk], 0, 0, 0);
    };
    read(a0, b0, 0);
    int s = 0;
    for (; s + 2 <= steps; s += 2) {
      read(a1, b1, s + 1);
      mma(a0, b0);
      if (s + 2 < steps) read(a0, b0, s + 2);
      mma(a1, b1);
    }
    if (s < steps) mma(a0, b0);  // an odd count's last step
  }

  // lane (c, h) holds dW[n][tap][k] for k = its column c and 16 rows n
  const int64_t ld = 9 * (int64_t)p.c;
  float* out = part + (int64_t)split * p.n * ld;
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int jm = 0; jm < MT; jm++)
#pragma unroll
      for (int jk = 0; jk < KT; jk++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int n = n0 + (wn * MT + jm) * 32 + acc_row(e, h);
          const int k = k0 + (wk * KT + jk) * 32 + c;
          out[n * ld + tap * p.c + k] = acc[tap][jm][jk][e];
        }
}

template <int BN, int BK>
void launch_wrw3x3(const Conv3x3WrwPlan& p, const void* dy, const void* x,
                   float* part, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv3x3_wrw<BN, BK>),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL((conv3x3_wrw<BN, BK>), dim3(p.grid), dim3(kT),
                     p.lds_bytes, stream, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x), part, p);
  CGX_HIP_CHECK(hipGetLastError());
}

// ---- weight gradient through a ring of LDS stages -----------------------------
//
// conv3x3_wrw with the chunks loaded straight into LDS (plan:
// conv3x3_wrw_ring_plan), as conv1x1_wrw_ring does it for the 1x1 weight
// gradient: the same images, read addresses and MFMA order, so the same bits
// at the same tile, hr, images and splits.  Per chunk:
//
//   s_waitcnt vmcnt(N)   the oldest stage of this wave has landed; N counts
//                        the instructions of the younger ones
//   s_barrier            ... and that of every wave
//   ds_read_b64_tr_b16, MFMAs
//   s_waitcnt lgkmcnt(0), s_barrier   every wave has read the stage
//   global_load_lds      chunk t + stages into the stage just freed
//
// Zeros.  Which position of a strip holds which pixel does not depend on the
// chunk, only whether it is live does (conv3x3_wrw_ring_src / _window): a
// lane keeps, per instruction, the byte offset of its 16 bytes from the
// chunk's first pixel and the key, and points a load whose key the chunk does
// not admit at `zeros`.  Every byte of a stage is written on every chunk and
// nothing outside the two tensors and `zeros` is read.
//
// Operand reads.  The compiler would put s_waitcnt vmcnt(0) in front of
// every LDS read it knows of while a global_load_lds is pending, so the reads
// are instructions of the kernel's own (ring_read_tr) and the kernel counts
// lgkmcnt itself.  A step has 20 reads and the counter ends at 15, so the
// reads run kRingAhead taps ahead of the MFMAs, not a step: before the MFMA
// of tap t the reads of tap t + kRingAhead are issued, of the next step
// where that is past tap 8 (with its A operand at tap 0), and the wait
// leaves exactly those in flight.  Nothing but source order and the
// sched_barrier(0) after each wait keeps the MFMAs behind the waits: after a
// change of toolchain read the .s again.

typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(1))) const void global_cvoid;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
constexpr int kRingAhead = 6;
static_assert(2 * kRingAhead + 2 <= 15 && kRingAhead < 9);

template <int N>
__device__ __forceinline__ void ring_wait_lgkmcnt() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
// s_waitcnt vmcnt(n) for a uniform n <= N
template <int N>
__device__ __forceinline__ void ring_wait_vmcnt(int n) {
  if (n >= N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
  else if constexpr (N > 0) ring_wait_vmcnt<N - 1>(n);
}
template <int OFF>
__device__ __forceinline__ u32x2 ring_read_tr(unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536);
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(v)
               : "v"(addr), "n"(OFF));
  return v;
}
// rows +0 .. +3 in elements 0 .. 3, rows +4 .. +7 in elements 4 .. 7
__device__ __forceinline__ bf16x8 ring_pair(const u32x2 (&v)[2]) {
  const unsigned w __attribute__((ext_vector_type(4))) = {v[0][0], v[0][1],
                                                          v[1][0], v[1][1]};
  return __builtin_bit_cast(bf16x8, w);
}
template <int I, int N, class F>
__device__ __forceinline__ void ring_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    ring_for<I + 1, N>(f);
  }
}

__global__ __launch_bounds__(kT) void conv3x3_wrw_ring(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    const uint4* __restrict__ zeros, float* __restrict__ part,
    Conv3x3WrwRingPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int C = 64;                  // both images
  constexpr int kStep = 16 * 2 * C;      // bytes of a 16-position step
  constexpr int kHi = 4 * 2 * C;         // ... and to an operand's second read
  constexpr int G = kConv3x3RingMaxGlds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  const int wn = wave >> 1, wk = wave & 1;
  const int tile = conv3x3_wrw_tile(p, blockIdx.x);
  const int split = conv3x3_wrw_split(p, blockIdx.x);
  const int n0 = (tile / p.ntiles_k) * C, k0 = (tile % p.ntiles_k) * C;

  // as conv3x3_wrw, from the start of a stage
  const int q = (lane >> 2) & 3;
  const int in_cell = 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  const int img_k = p.dy_glds * 4096;
  const unsigned an = wrw_cell<C>(8 * h + q, wn) + in_cell;
  unsigned ak[9];
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
    ak[tap] = img_k +
              wrw_cell<C>(8 * h + q + (tap / 3) * p.pitch + tap % 3, wk) +
              in_cell;

  f32x16 acc[9];
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[tap][e] = 0.f;

  // the lane's 16 bytes of instruction j of a stage: see above
  const int glds = p.dy_glds + p.x_glds;
  int off[G], key[G];
#pragma unroll
  for (int j = 0; j < G; j++) {
    off[j] = 0, key[j] = kConv3x3RingNever;
    if (j < glds) {  // uniform
      const Conv3x3RingSlot s = conv3x3_wrw_ring_slot(p, wave, j, lane);
      const Conv3x3RingSrc src = conv3x3_wrw_ring_src(p, s.is_x, s.pos);
      off[j] = (src.pixel * (s.is_x ? p.c : p.n) + s.vec * 8) * 2;
      key[j] = src.key;
    }
  }

  // the chunks split, split + splits, ... below p.chunks
  const int T = (p.chunks - split + p.splits - 1) / p.splits;
  const char* dy_b = reinterpret_cast<const char*>(dy) + n0 * 2;
  const char* x_b = reinterpret_cast<const char*>(x) + k0 * 2;
  auto issue = [&](int t, int slot) __attribute__((always_inline)) {
    const Conv3x3RingWindow win =
        conv3x3_wrw_ring_window(p, split + t * p.splits);
    const char* src_n = dy_b + (int64_t)win.pixel * p.n * 2;
    const char* src_k = x_b + (int64_t)win.pixel * p.c * 2;
    lds_char* dst =
        (lds_char*)reinterpret_cast<char*>(lds) + slot * p.stage_bytes +
        wave * 1024;
#pragma unroll
    for (int j = 0; j < G; j++)
      if (j < glds) {  // uniform
        const bool live = (unsigned)(key[j] - win.first) < (unsigned)win.count;
        const char* src = (j < p.dy_glds ? src_n : src_k) + off[j];
        __builtin_amdgcn_global_load_lds(
            (global_cvoid*)(live ? src : reinterpret_cast<const char*>(zeros)),
            dst + j * 4096, 16, 0, 0);
      }
  };

  // The 16-position steps of the stage at LDS address `stage`.
  const int steps_n = p.strip_dy / 16;
  auto steps = [&](unsigned stage) __attribute__((always_inline)) {
    u32x2 a[2][2], b[2][9][2];
    unsigned pa = stage + an, pb[9];
#pragma unroll
    for (int tap = 0; tap < 9; tap++) pb[tap] = stage + ak[tap];
    // the reads of tap TAP of this step (NEXT 0) or the one after it, into
    // register set SET
    auto read = [&](auto set_, auto tap_, auto next_)
                    __attribute__((always_inline)) {
      constexpr int SET = decltype(set_)::value, TAP = decltype(tap_)::value;
      constexpr int O = decltype(next_)::value * kStep;
      if constexpr (TAP == 0) {
        a[SET][0] = ring_read_tr<O>(pa);
        a[SET][1] = ring_read_tr<O + kHi>(pa);
      }
      b[SET][TAP][0] = ring_read_tr<O>(pb[TAP]);
      b[SET][TAP][1] = ring_read_tr<O + kHi>(pb[TAP]);
    };
    // one step from register set SET; LAST: no step follows
    auto step = [&](auto set_, auto last_) __attribute__((always_inline)) {
      constexpr int SET = decltype(set_)::value;
      constexpr bool LAST = decltype(last_)::value;
      ring_for<0, 9>([&](auto tap_) __attribute__((always_inline)) {
        constexpr int TAP = decltype(tap_)::value, AHEAD = TAP + kRingAhead;
        if constexpr (AHEAD < 9) {
          read(set_, std::integral_constant<int, AHEAD>{},
               std::integral_constant<int, 0>{});
          ring_wait_lgkmcnt<2 * kRingAhead>();
        } else if constexpr (!LAST) {
          read(std::integral_constant<int, SET ^ 1>{},
               std::integral_constant<int, AHEAD - 9>{},
               std::integral_constant<int, 1>{});
          ring_wait_lgkmcnt<2 * kRingAhead + 2>();  // with the A operand
        } else {
          ring_wait_lgkmcnt<2 * (8 - TAP)>();
        }
        __builtin_amdgcn_sched_barrier(0);
        acc[TAP] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            ring_pair(a[SET]), ring_pair(b[SET][TAP]), acc[TAP], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      });
      pa += kStep;
#pragma unroll
      for (int tap = 0; tap < 9; tap++) pb[tap] += kStep;
    };
    ring_for<0, kRingAhead>([&](auto tap_) __attribute__((always_inline)) {
      read(std::integral_constant<int, 0>{}, tap_,
           std::integral_constant<int, 0>{});
    });
    // an even count (the plan's strip_dy): one path, so that no accumulator
    // is copied where two would meet
    for (int s = 2; s < steps_n; s += 2) {
      step(std::integral_constant<int, 0>{}, std::false_type{});
      step(std::integral_constant<int, 1>{}, std::false_type{});
    }
    step(std::integral_constant<int, 0>{}, std::false_type{});
    step(std::integral_constant<int, 1>{}, std::true_type{});
  };

  for (int s = 0; s < p.stages; s++)
    if (s < T) issue(s, s);
  const unsigned ring_addr =
      (unsigned)(unsigned long)(lds_char*)reinterpret_cast<char*>(lds);
  int slot = 0;
  for (int t = 0; t < T; t++) {
    const int younger = T - 1 - t < p.stages - 1 ? T - 1 - t : p.stages - 1;
    ring_wait_vmcnt<2 * G>(younger * glds);
    __builtin_amdgcn_s_barrier();
    steps(ring_addr + slot * p.stage_bytes);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + p.stages < T) issue(t + p.stages, slot);
    slot = slot + 1 == p.stages ? 0 : slot + 1;
  }

  // as conv3x3_wrw
  const int64_t ld = 9 * (int64_t)p.c;
  float* out = part + (int64_t)split * p.n * ld;
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int n = n0 + wn * 32 + acc_row(e, h);
      const int k = k0 + wk * 32 + c;
      out[n * ld + tap * p.c + k] = acc[tap][e];
    }
}

void launch_wrw3x3_ring(const Conv3x3WrwRingPlan& p, const void* dy,
                        const void* x, const void* zeros, float* part,
                        hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv3x3_wrw_ring),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL(conv3x3_wrw_ring, dim3(p.grid), dim3(kT), p.lds_bytes,
                     stream, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x),
                     static_cast<const uint4*>(zeros), part, p);
  CGX_HIP_CHECK(hipGetLastError());
}

// ---- stride-2 weight gradient ---------------------------------------------------
//
// dW of the 3x3 / stride 2 / padding 1 convolution (plan: conv3x3s2_wrw_plan,
// which has the geometry): conv3x3_wrw_ring's tile, ring, waits and steps
// (ring_steps) on a stage that holds dY's strip and the four parity planes of
// X as one wrw_cell<64> image.  Tap (r, s) reads plane (r != 1, s != 1) at
// conv3x3s2_wrw_tap's offset from the position, so the nine B operands again
// differ by an LDS address only: no masks and no loads per tap.
//
// Fill.  The destination of an instruction is the wave's contiguous 1 KiB, so
// the de-interleaving, like the swizzle, is in the address a lane loads from:
// conv3x3s2_wrw_slot gives the stage position of its 16 bytes and
// conv3x3s2_wrw_src what that position holds on every chunk, two pixels apart
// along a row of a plane.  dY's strip is whole instructions, so which tensor
// an instruction reads is uniform.  A load whose key the chunk's window does
// not admit reads `zeros`.  A stage is at most 20 instructions a wave, X four
// times dY's: the 40 vectors a thread would stage through registers.
//
// Bank conflicts.  conv3x3_wrw's argument holds unchanged.  A transposed read
// takes four consecutive positions of the stage image, starting anywhere, and
// their columns are 2*(r & 1) + (u ^ ((r >> 1) & 1)): all four differ.  A
// plane's base is a multiple of four positions, 512 bytes, which moves a
// read by whole pairs of lines and leaves its columns as they are, and the
// tap offsets are what r*P + s was: any start.  A step adds 16 positions and
// an operand's second read 4, as there.
// conv3x3_wrw_ring's steps of one stage, an even number of them, for
// conv3x3s2_wrw: the A operand from LDS address pa, tap t's B operand from
// pb[t].  (conv3x3_wrw_ring keeps its own copy: calling this one changes its
// register allocation.)
__device__ __forceinline__ void ring_steps(f32x16 (&acc)[9], unsigned pa,
                                           unsigned (&pb)[9], int steps_n) {
  constexpr int kStep = 16 * 2 * 64;  // bytes of a 16-position step
  constexpr int kHi = 4 * 2 * 64;     // ... and to an operand's second read
  u32x2 a[2][2], b[2][9][2];
  // the reads of tap TAP of this step (NEXT 0) or the one after it, into
  // register set SET
  auto read = [&](auto set_, auto tap_, auto next_)
                  __attribute__((always_inline)) {
    constexpr int SET = decltype(set_)::value, TAP = decltype(tap_)::value;
    constexpr int O = decltype(next_)::value * kStep;
    if constexpr (TAP == 0) {
      a[SET][0] = ring_read_tr<O>(pa);
      a[SET][1] = ring_read_tr<O + kHi>(pa);
    }
    b[SET][TAP][0] = ring_read_tr<O>(pb[TAP]);
    b[SET][TAP][1] = ring_read_tr<O + kHi>(pb[TAP]);
  };
  // one step from register set SET; LAST: no step follows
  auto step = [&](auto set_, auto last_) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_)::value;
    constexpr bool LAST = decltype(last_)::value;
    ring_for<0, 9>([&](auto tap_) __attribute__((always_inline)) {
      constexpr int TAP = decltype(tap_)::value, AHEAD = TAP + kRingAhead;
      if constexpr (AHEAD < 9) {
        read(set_, std::integral_constant<int, AHEAD>{},
             std::integral_constant<int, 0>{});
        ring_wait_lgkmcnt<2 * kRingAhead>();
      } else if constexpr (!LAST) {
        read(std::integral_constant<int, SET ^ 1>{},
             std::integral_constant<int, AHEAD - 9>{},
             std::integral_constant<int, 1>{});
        ring_wait_lgkmcnt<2 * kRingAhead + 2>();  // with the A operand
      } else {
        ring_wait_lgkmcnt<2 * (8 - TAP)>();
      }
      __builtin_amdgcn_sched_barrier(0);
      acc[TAP] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          ring_pair(a[SET]), ring_pair(b[SET][TAP]), acc[TAP], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    });
    pa += kStep;
#pragma unroll
    for (int tap = 0; tap < 9; tap++) pb[tap] += kStep;
  };
  ring_for<0, kRingAhead>([&](auto tap_) __attribute__((always_inline)) {
    read(std::integral_constant<int, 0>{}, tap_,
         std::integral_constant<int, 0>{});
  });
  // an even count (the plan's strip_dy): one path, so that no accumulator
  // is copied where two would meet
  for (int s = 2; s < steps_n; s += 2) {
    step(std::integral_constant<int, 0>{}, std::false_type{});
    step(std::integral_constant<int, 1>{}, std::false_type{});
  }
  step(std::integral_constant<int, 0>{}, std::false_type{});
  step(std::integral_constant<int, 1>{}, std::true_type{});
}

__global__ __launch_bounds__(kT) void conv3x3s2_wrw(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    const uint4* __restrict__ zeros, float* __restrict__ part,
    Conv3x3S2WrwPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int C = 64;  // the image
  constexpr int G = kConv3x3RingMaxGlds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  const int wn = wave >> 1, wk = wave & 1;
  const int tile = conv3x3_wrw_tile(p, blockIdx.x);
  const int split = conv3x3_wrw_split(p, blockIdx.x);
  const int n0 = (tile / p.ntiles_k) * C, k0 = (tile % p.ntiles_k) * C;

  // as conv3x3_wrw_ring, from the start of a stage
  const int q = (lane >> 2) & 3;
  const int in_cell = 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  const unsigned an = wrw_cell<C>(8 * h + q, wn) + in_cell;
  unsigned ak[9];
#pragma unroll
  for (int tap = 0; tap < 9; tap++) {
    const Conv3x3S2WrwTap t = conv3x3s2_wrw_tap(p, tap);
    ak[tap] =
        wrw_cell<C>(p.plane_base[t.plane] + t.offset + 8 * h + q, wk) + in_cell;
  }

  f32x16 acc[9];
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[tap][e] = 0.f;

  // the lane's 16 bytes of instruction j of a stage: see above
  const int dy_glds = p.strip_dy / 32;
  int off[G], key[G];
#pragma unroll
  for (int j = 0; j < G; j++) {
    off[j] = 0, key[j] = kConv3x3RingNever;
    if (j < p.glds) {  // uniform
      const Conv3x3RingSlot s = conv3x3s2_wrw_slot(wave, j, lane);
      const Conv3x3S2WrwSrc src = conv3x3s2_wrw_src(p, s.pos);
      off[j] = (src.pixel * (src.is_x ? p.c : p.n) + s.vec * 8) * 2;
      key[j] = src.key;
    }
  }

  // the chunks split, split + splits, ... below p.chunks
  const int T = (p.chunks - split + p.splits - 1) / p.splits;
  const char* dy_b = reinterpret_cast<const char*>(dy) + n0 * 2;
  const char* x_b = reinterpret_cast<const char*>(x) + k0 * 2;
  auto issue = [&](int t, int slot) __attribute__((always_inline)) {
    const Conv3x3S2WrwWindow win =
        conv3x3s2_wrw_window(p, split + t * p.splits);
    const char* src_n = dy_b + (int64_t)win.pixel_dy * p.n * 2;
    const char* src_k = x_b + (int64_t)win.pixel_x * p.c * 2;
    lds_char* dst =
        (lds_char*)reinterpret_cast<char*>(lds) + slot * p.stage_bytes +
        wave * 1024;
#pragma unroll
    for (int j = 0; j < G; j++)
      if (j < p.glds) {  // uniform
        const bool live = (unsigned)(key[j] - win.first) < (unsigned)win.count;
        const char* src = (j < dy_glds ? src_n : src_k) + off[j];
        __builtin_amdgcn_global_load_lds(
            (global_cvoid*)(live ? src : reinterpret_cast<const char*>(zeros)),
            dst + j * 4096, 16, 0, 0);
      }
  };

  const int steps_n = p.strip_dy / 16;
  if (0 < T) issue(0, 0);
  if (1 < T) issue(1, 1);
  const unsigned ring_addr =
      (unsigned)(unsigned long)(lds_char*)reinterpret_cast<char*>(lds);
  for (int t = 0; t < T; t++) {
    const unsigned stage = ring_addr + (t & 1) * p.stage_bytes;
    ring_wait_vmcnt<G>(t + 1 < T ? p.glds : 0);
    __builtin_amdgcn_s_barrier();
    unsigned pb[9];
#pragma unroll
    for (int tap = 0; tap < 9; tap++) pb[tap] = stage + ak[tap];
    ring_steps(acc, stage + an, pb, steps_n);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 2 < T) issue(t + 2, t & 1);
  }

  // as conv3x3_wrw
  const int64_t ld = 9 * (int64_t)p.c;
  float* out = part + (int64_t)split * p.n * ld;
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int n = n0 + wn * 32 + acc_row(e, h);
      const int k = k0 + wk * 32 + c;
      out[n * ld + tap * p.c + k] = acc[tap][e];
    }
}

void launch_wrw3x3s2(const Conv3x3S2WrwPlan& p, const void* dy, const void* x,
                     const void* zeros, float* part, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv3x3s2_wrw),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL(conv3x3s2_wrw, dim3(p.grid), dim3(kT), p.lds_bytes,
                     stream, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x),
                     static_cast<const uint4*>(zeros), part, p);
  CGX_HIP_CHECK(hipGetLastError());
}

// ---- forward with BatchNorm partials ------------------------------------------
//
// y = conv2d(x, w, padding 1) and the partials of y for the BatchNorm that
// follows, as conv1x1_stats produces them.  Geometry: Conv3x3FwdPlan.
//
//   A   the strip of a tile, [64*xvecs pixels][32 channels], 64 bytes a pixel.
//       Lane (c, h) of a wave reads for tap (r, s) the 16 bytes of pixel
//       m + c + r*W + s, channels 8*(2k + h) .. +7 of 16-deep step k, and
//       clears them where the pixel's bit of conv3x3_fwd_taps is not set: a
//       select, so whatever the strip holds there never reaches a product
//   B   a weight chunk, [9 taps][64 channels][32 channels of X], the row of
//       (tap, n) at index 64*tap + n
//   C   a wave owns 64 rows x 64 channels, four accumulator tiles, so each
//       ds_read_b128 of A and each of B feeds two MFMAs; per 16-deep step and
//       tap that is four reads for four MFMAs, against ten for nine in
//       conv3x3_wrw
//
// Both images have 64-byte rows, fwd_slot: the 16 lanes that one pass of a
// ds_read_b128 serves read 16 consecutive rows j at one q, which start
// anywhere because the taps shift them.  Row j lies in the 64-byte column
// j & 3 of a 256-byte bank row and the XOR with (j >> 2) & 3 gives the four
// rows of a column four different 16-byte slots; j & 15 takes all 16 values
// on 16 consecutive rows, so the pass is conflict-free at every start.  The
// copies write whole rows from consecutive lanes.
//
// A stage is one 32-channel chunk of one tile: 72 MFMAs a wave.  A thread
// loads its share of the next stage, at most nine vectors of the strip and
// nine of the weight, into registers before the MFMAs of this one and writes
// them to the other buffers after them, so one barrier a stage orders both
// (gemm_walk_tiled).  The accumulators take 64 registers and the staged
// vectors 72: the kernel is far from the register bound of conv3x3_wrw.  Every
// accumulator is one chain over (chunk, tap, step) in ascending order, and
// the moments merge in a fixed tree: the same bits every run.

constexpr int kFwdWVecs = kConv3x3FwdWBytes / 16;  // of a weight chunk
constexpr int kFwdWShare = kFwdWVecs / kT;         // ... and of a thread
static_assert(kFwdWVecs % kT == 0 && kConv3x3FwdBn == 64 &&
              kConv3x3FwdKc == 32 && kConv3x3FwdTileRows == 4 * 64);

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 16-byte vector q of row j of an image with 64-byte rows
__device__ inline int fwd_slot(int j, int q) {
  return j * 4 + (q ^ ((j >> 2) & 3));
}

// vector q of channels n0 .. n0+63 of chunk kc of the weight's row (tap, n)
__device__ inline const uint4* fwd_w_src(const uint4* __restrict__ w,
                                         const Conv3x3FwdPlan& p, int n0,
                                         int kc, int idx) {
  const int q = idx & 3, row = idx >> 2, tap = row >> 6, n = row & 63;
  return w + ((int64_t)((n0 + n) * 9 + tap) * p.c + kc * kConv3x3FwdKc) / 8 + q;
}

// The same for conv3x3_bwd_data, whose plan has the roles exchanged (p.c is
// the N of dY, p.n the C of dX): vector idx of the [9 taps][32 n][64 c] chunk
// kc of the weight [N][3][3][C], channels c0 .. c0+63 of row (tap, n) ...
__device__ inline const uint4* bwd_w_src(const uint4* __restrict__ w,
                                         const Conv3x3FwdPlan& p, int c0,
                                         int kc, int idx) {
  const int q = idx & 7, row = idx >> 3, tap = row >> 5, n = row & 31;
  return w +
         ((int64_t)((kc * kConv3x3FwdKc + n) * 9 + tap) * p.n + c0) / 8 + q;
}
// ... and where it goes: row 32*tap + n of a 64-channel wrw_cell image
__device__ inline int bwd_w_slot(int idx) {
  return wrw_cell<64>(idx >> 3, (idx >> 2) & 1) / 16 + (idx & 3);
}

// A thread's share of one stage in registers (plain vectors: a uint4 member
// would keep the whole struct in scratch).  TR: the weight chunk of
// conv3x3_bwd_data.
template <bool RES, bool TR = false>
struct FwdStage {
  u32x4 wv[RES ? 1 : kFwdWShare], xv[kConv3x3FwdXVecs];
  __device__ __forceinline__ void load(const uint4* __restrict__ x,
                                       const uint4* __restrict__ w,
                                       const Conv3x3FwdPlan& p, int n0,
                                       int tile, int kc, int tid) {
    if (!RES) {
#pragma unroll
      for (int i = 0; i < kFwdWShare; i++)
        wv[i] = *reinterpret_cast<const u32x4*>(
            TR ? bwd_w_src(w, p, n0, kc, tid + i * kT)
               : fwd_w_src(w, p, n0, kc, tid + i * kT));
    }
#pragma unroll
    for (int i = 0; i < kConv3x3FwdXVecs; i++)
      if (i < p.xvecs) {  // uniform
        const int idx = tid + i * kT;
        const int64_t r = conv3x3_fwd_strip_row(p, tile, idx >> 2);
        xv[i] = *reinterpret_cast<const u32x4*>(
            x + (r * p.c + kc * kConv3x3FwdKc) / 8 + (idx & 3));
      }
  }
  __device__ __forceinline__ void store(uint4* wb, uint4* xb,
                                        const Conv3x3FwdPlan& p,
                                        int tid) const {
    if (!RES) {
#pragma unroll
      for (int i = 0; i < kFwdWShare; i++) {
        const int idx = tid + i * kT;
        *reinterpret_cast<u32x4*>(
            wb + (TR ? bwd_w_slot(idx) : fwd_slot(idx >> 2, idx & 3))) = wv[i];
      }
    }
#pragma unroll
    for (int i = 0; i < kConv3x3FwdXVecs; i++)
      if (i < p.xvecs) {
        const int idx = tid + i * kT;
        *reinterpret_cast<u32x4*>(xb + fwd_slot(idx >> 2, idx & 3)) = xv[i];
      }
  }
};

template <bool RES>
__global__ __launch_bounds__(kT) void conv3x3_stats(
    const uint4* __restrict__ x, const uint4* __restrict__ w,
    uint4* __restrict__ y, float* __restrict__ part, Conv3x3FwdPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = kConv3x3FwdBn, M = kConv3x3FwdTileRows;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int ntile = conv3x3_fwd_ntile(p, blockIdx.x);
  const int split = conv3x3_fwd_split(p, blockIdx.x);
  const int n0 = ntile * BN, nvec = p.n / 8;
  const int xbuf = p.xvecs * kT;  // vectors of a strip buffer
  uint4* wimg = lds;              // two weight chunks
  uint4* ximg = lds + 2 * kFwdWVecs;  // two strips
  uint4* stage = ximg + 2 * xbuf + wave * 256;  // [32 rows][64 channels]

  if (RES) {  // the two chunks are the two buffers, for good
    for (int idx = tid; idx < 2 * kFwdWVecs; idx += kT) {
      const int kc = idx / kFwdWVecs, v = idx % kFwdWVecs;
      wimg[kc * kFwdWVecs + fwd_slot(v >> 2, v & 3)] =
          *fwd_w_src(w, p, n0, kc, v);
    }
  }

  FwdStage<RES> st;
  int tile = split, kc = 0, buf = 0;  // split < row_tiles
  st.load(x, w, p, n0, tile, 0, tid);
  st.store(wimg, ximg, p, tid);

  // The lane's moments are those of v - pivot, pivot the first value the lane
  // pushes: a difference of two bf16 values, exact in fp32.  The roundings of
  // a run then scale with the spread of the values, not with their mean
  // (outputs near 100 with unit spread lose two digits of M2 otherwise), and
  // the pivot returns where the runs merge.
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
  f32x16 acc[2][2];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[s][j][e] = 0.f;
  unsigned valid[2] = {0, 0};

  while (tile < p.row_tiles) {
    // The next stage, of this tile or the first of the next, is loaded before
    // the MFMAs of this one.  All waves walk the same stages, so each
    // reaches every barrier.
    int nkc = kc + 1, ntl = tile;
    if (nkc == p.nchunks) nkc = 0, ntl = tile + p.splits;
    const bool more = ntl < p.row_tiles;
    if (more) st.load(x, w, p, n0, ntl, nkc, tid);
    // buffer `buf` is written, and the other one, read a stage ago, is free
    __syncthreads();
    if (kc == 0) {
#pragma unroll
      for (int s = 0; s < 2; s++)
        valid[s] = conv3x3_fwd_taps(p, tile * M + wave * 64 + s * 32 + c);
    }
    const uint4* wl = wimg + buf * kFwdWVecs;
    const uint4* xl = ximg + buf * xbuf;
    uint4 av[2][2], bv[2][2];  // the operands of this step and the next
    auto read = [&](int u) {
      const int tap = u >> 1, q = 2 * (u & 1) + h;
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int j = conv3x3_fwd_strip_index(p, wave * 64 + s * 32 + c, tap);
        const uint4 v = xl[fwd_slot(j, q)];
        const unsigned m = 0u - ((valid[s] >> tap) & 1u);
        av[u & 1][s] = make_uint4(v.x & m, v.y & m, v.z & m, v.w & m);
      }
#pragma unroll
      for (int j = 0; j < 2; j++)
        bv[u & 1][j] = wl[fwd_slot(tap * 64 + j * 32 + c, q)];
    };
    read(0);
#pragma unroll
    for (int u = 0; u < 18; u++) {
      if (u + 1 < 18) read(u + 1);
#pragma unroll
      for (int s = 0; s < 2; s++)
#pragma unroll
        for (int j = 0; j < 2; j++)
          acc[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(bf16x8, av[u & 1][s]),
              __builtin_bit_cast(bf16x8, bv[u & 1][j]), acc[s][j], 0, 0, 0);
    }
    // nothing that waits for the loads above may move up among the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    buf ^= 1;
    if (more) st.store(wimg + buf * kFwdWVecs, ximg + buf * xbuf, p, tid);

    if (nkc == 0) {
      // The tile is complete: round, push, store, as conv1x1_stats does
      // (stats_body in conv1x1_kernels.hip), one 32-row sub-tile at a time.
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int r0 = tile * M + wave * 64 + s * 32;
        const int live = p.rows - r0 < 32 ? p.rows - r0 : 32;  // may be <= 0
        unsigned pk[2][8];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int e = 0; e < 8; e++)
            pk[j][e] = fwd_pack_bf16(acc[s][j][2 * e], acc[s][j][2 * e + 1]);
        // the moments of the rounded values: what bn_apply will normalise
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
        fwd_store_subtile(pk, stage, y, r0, live, nvec, n0, lane);
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int e = 0; e < 16; e++) acc[s][j][e] = 0.f;
      }
    }
    kc = nkc, tile = ntl;
  }

  // The eight runs of every channel -> one partial, as a tree.  A merge
  // keeps the pivot of its first run (of the second where the first is
  // empty) and moves the other mean there: the difference of the pivots is
  // exact and the sum is of the size of the spread.  The pivot is added once,
  // at the end.
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
    row[n0 + tid] = pv[0] + m[0].mean[0];
    row[p.n + n0 + tid] = m[0].m2[0];
    if (tid == 0) row[2 * p.n + ntile] = m[0].n;
  }
}

template <bool RES>
void launch_fwd3x3(const Conv3x3FwdPlan& p, const void* x, const void* w,
                   void* y, float* part, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv3x3_stats<RES>),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL((conv3x3_stats<RES>), dim3(p.grid), dim3(kT), p.lds_bytes,
                     stream, static_cast<const uint4*>(x),
                     static_cast<const uint4*>(w), static_cast<uint4*>(y),
                     part, p);
  CGX_HIP_CHECK(hipGetLastError());
}

// ---- stride-2 forward with BatchNorm partials ---------------------------------
//
// y = conv2d(x, w, stride 2, padding 1) of an image with even sides, and the
// partials of y.  Geometry: Conv3x3S2FwdPlan.
//
//   A   the strip of a tile, four parity planes of one 32-channel chunk of X
//       behind one another, 64 bytes an entry in the fwd_slot layout.  Entry
//       e holds input pixel conv3x3s2_fwd_strip_pixel(e); a thread keeps the
//       addresses of its (at most nine) vectors of a tile, which do not depend
//       on the chunk, so the two divisions per vector are paid once a tile.
//       Lane (c, h) of wave w reads for tap (r, s) the 16 bytes of entry
//       conv3x3s2_fwd_strip_index(32*w + c, 3r + s): 16 consecutive entries
//       of one plane per pass, conflict-free at every start like the stride-1
//       strip, and clears them where conv3x3s2_fwd_taps has no bit
//   B   the weight chunk of conv3x3_stats, streamed: [9][64][32]
//   C   a wave owns 32 rows x 64 channels, two accumulator tiles: one read of
//       A and two of B feed two MFMAs per 16-deep step and tap
//
// A stage is one chunk of one tile, 36 MFMAs a wave, staged through registers
// behind the MFMAs of the stage before and ordered by one barrier, as in
// conv3x3_stats.  The epilogue, the per-lane pivot and the tree of the eight
// runs are conv3x3_stats' with one sub-tile per wave.

static_assert(kConv3x3S2TileRows == 4 * 32);

// The eight runs of every channel of a workgroup -> its partial row: the
// tree at the end of conv3x3_stats, which keeps its own copy so that its
// register allocation stays what RESULTS.md records.  `sc` is LDS that nobody
// reads any more.
__device__ __forceinline__ void fwd_merge_runs(float* sc, const Moments<2>& mo,
                                               const float (&pivot)[2],
                                               float* row, int n, int n0,
                                               int ntile, int tid) {
  constexpr int BN = kConv3x3FwdBn;
  const int wave = tid >> 6, c = tid & 31, h = (tid & 63) >> 5;
  __syncthreads();
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
    row[n0 + tid] = pv[0] + m[0].mean[0];
    row[n + n0 + tid] = m[0].m2[0];
    if (tid == 0) row[2 * n + ntile] = m[0].n;
  }
}

struct S2Stage {
  u32x4 wv[kFwdWShare], xv[kConv3x3S2XVecs];
  int src[kConv3x3S2XVecs];  // the thread's vectors of chunk 0 of the tile
  __device__ __forceinline__ void aim(const Conv3x3S2FwdPlan& p, int tile,
                                      int tid) {
#pragma unroll
    for (int i = 0; i < kConv3x3S2XVecs; i++)
      if (i < p.xvecs) {  // uniform
        const int idx = tid + i * kT;
        src[i] = conv3x3s2_fwd_strip_pixel(p, tile, idx >> 2) * (p.c / 8) +
                 (idx & 3);
      }
  }
  __device__ __forceinline__ void load(const uint4* __restrict__ x,
                                       const uint4* __restrict__ w,
                                       const Conv3x3S2FwdPlan& p, int n0,
                                       int kc, int tid) {
#pragma unroll
    for (int i = 0; i < kFwdWShare; i++)
      wv[i] = *reinterpret_cast<const u32x4*>(
          fwd_w_src(w, p, n0, kc, tid + i * kT));
#pragma unroll
    for (int i = 0; i < kConv3x3S2XVecs; i++)
      if (i < p.xvecs)
        xv[i] = *reinterpret_cast<const u32x4*>(
            x + src[i] + kc * (kConv3x3FwdKc / 8));
  }
  __device__ __forceinline__ void store(uint4* wb, uint4* xb,
                                        const Conv3x3S2FwdPlan& p,
                                        int tid) const {
#pragma unroll
    for (int i = 0; i < kFwdWShare; i++) {
      const int idx = tid + i * kT;
      *reinterpret_cast<u32x4*>(wb + fwd_slot(idx >> 2, idx & 3)) = wv[i];
    }
#pragma unroll
    for (int i = 0; i < kConv3x3S2XVecs; i++)
      if (i < p.xvecs) {
        const int idx = tid + i * kT;
        *reinterpret_cast<u32x4*>(xb + fwd_slot(idx >> 2, idx & 3)) = xv[i];
      }
  }
};

__global__ __launch_bounds__(kT) void conv3x3s2_stats(
    const uint4* __restrict__ x, const uint4* __restrict__ w,
    uint4* __restrict__ y, float* __restrict__ part, Conv3x3S2FwdPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = kConv3x3FwdBn, M = kConv3x3S2TileRows;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int ntile = conv3x3_fwd_ntile(p, blockIdx.x);
  const int split = conv3x3_fwd_split(p, blockIdx.x);
  const int n0 = ntile * BN, nvec = p.n / 8;
  const int xbuf = p.xvecs * kT;  // vectors of a strip buffer
  uint4* wimg = lds;              // two weight chunks
  uint4* ximg = lds + 2 * kFwdWVecs;  // two strips
  uint4* stage = ximg + 2 * xbuf + wave * 256;  // [32 rows][64 channels]

  S2Stage st;
  int tile = split, kc = 0, buf = 0;  // split < row_tiles
  st.aim(p, tile, tid);
  st.load(x, w, p, n0, 0, tid);
  st.store(wimg, ximg, p, tid);

  // the entry of each tap for the lane's row, the same on every tile
  int at[9];
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
    at[tap] = conv3x3s2_fwd_strip_index(p, wave * 32 + c, tap);

  Moments<2> mo;  // of v - pivot, as in conv3x3_stats
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
  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[j][e] = 0.f;
  unsigned valid = 0;

  while (tile < p.row_tiles) {
    int nkc = kc + 1, ntl = tile;
    if (nkc == p.nchunks) nkc = 0, ntl = tile + p.splits;
    const bool more = ntl < p.row_tiles;
    if (more) {
      if (nkc == 0) st.aim(p, ntl, tid);
      st.load(x, w, p, n0, nkc, tid);
    }
    // buffer `buf` is written, and the other one, read a stage ago, is free
    __syncthreads();
    if (kc == 0) valid = conv3x3s2_fwd_taps(p, tile * M + wave * 32 + c);
    const uint4* wl = wimg + buf * kFwdWVecs;
    const uint4* xl = ximg + buf * xbuf;
    uint4 av[2], bv[2][2];  // the operands of this step and the next
    auto read = [&](int u) {
      const int tap = u >> 1, q = 2 * (u & 1) + h;
      const uint4 v = xl[fwd_slot(at[tap], q)];
      const unsigned m = 0u - ((valid >> tap) & 1u);
      av[u & 1] = make_uint4(v.x & m, v.y & m, v.z & m, v.w & m);
#pragma unroll
      for (int j = 0; j < 2; j++)
        bv[u & 1][j] = wl[fwd_slot(tap * 64 + j * 32 + c, q)];
    };
    read(0);
#pragma unroll
    for (int u = 0; u < 18; u++) {
      if (u + 1 < 18) read(u + 1);
#pragma unroll
      for (int j = 0; j < 2; j++)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            __builtin_bit_cast(bf16x8, av[u & 1]),
            __builtin_bit_cast(bf16x8, bv[u & 1][j]), acc[j], 0, 0, 0);
    }
    // nothing that waits for the loads above may move up among the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    buf ^= 1;
    if (more) st.store(wimg + buf * kFwdWVecs, ximg + buf * xbuf, p, tid);

    if (nkc == 0) {  // the tile is complete: round, push, store
      const int r0 = tile * M + wave * 32;
      const int live = p.rows - r0 < 32 ? p.rows - r0 : 32;  // may be <= 0
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
      fwd_store_subtile(pk, stage, y, r0, live, nvec, n0, lane);
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.f;
    }
    kc = nkc, tile = ntl;
  }

  fwd_merge_runs(reinterpret_cast<float*>(lds), mo, pivot,
                 part + (int64_t)split * p.pstride, p.n, n0, ntile, tid);
}

void launch_fwd3x3s2(const Conv3x3S2FwdPlan& p, const void* x, const void* w,
                     void* y, float* part, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv3x3s2_stats),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL(conv3x3s2_stats, dim3(p.grid), dim3(kT), p.lds_bytes,
                     stream, static_cast<const uint4*>(x),
                     static_cast<const uint4*>(w), static_cast<uint4*>(y),
                     part, p);
  CGX_HIP_CHECK(hipGetLastError());
}

// ---- input gradient -----------------------------------------------------------
//
// dX[b, c, h, w] = sum over n, r, s of dY[b, n, h+1-r, w+1-s] * W[n, c, r, s]:
// the forward's GEMM with C and N exchanged, dX[R, C] = sum over taps t of
// dY_t[R, N] * W_{8-t}[N, C].  The plan is a Conv3x3FwdPlan of the exchanged
// problem (conv3x3_bwd_plan): p.c is the N of dY, p.n the C of dX.
//
//   A   the forward's strip, of dY: with r' = 2 - r, s' = 2 - s the factor of
//       W[., ., r, s] is the neighbour (h+r'-1, w+s'-1), strip tap
//       t = 3r' + s', cleared by the same bits of conv3x3_fwd_taps (H, W and
//       the padding are the forward's); the weight's tap is 8 - t
//   B   the weight stays [N][3][3][C], so the contracted index n is the slow
//       one of a chunk [9 taps][32 n][64 c]: 36 KiB like the forward's, copied
//       row by row (128 bytes) into a 64-channel wrw_cell image, row
//       32*tap + n, and read transposed as in conv1x1_wrw: two
//       ds_read_b64_tr_b16 per 32-channel tile and 16-deep step, each feeding
//       two MFMAs like the forward's ds_read_b128
//   C   as the forward, without moments
//
// Bank conflicts of B.  A transposed read takes per 32-lane half the cell
// (tile j) of the four rows n = 16k + 8h + 4i .. +3 of one tap, i the first or
// second read: the C == 64 case of conv1x1_wrw, rows 4m .. 4m+3 at a multiple
// of four, whose cells lie in the four 64-byte columns (2*(r & 1) + j) ^
// ((r >> 1) & 1) of their two 256-byte lines.  A tap moves the address by
// 4096 bytes, a step by 2048 and the second read by 512, all whole lines that
// leave r & 3 alone: one base address per tile, everything else an immediate
// offset.  The copy's 16-byte writes go out 16 lanes a pass, which are the 16
// vectors of rows 2v, 2v+1: one whole line, conflict-free under any
// permutation of its cells.  Every address is a multiple of 8 and inside the
// buffer, and the reads are in no divergent branch: EXEC is all ones.
//
// Staging, barriers and the order of every accumulator's chain over (chunk,
// tap, step) are the forward's: the same bits every run.
template <bool RES>
__global__ __launch_bounds__(kT) void conv3x3_bwd_data(
    const uint4* __restrict__ dy, const uint4* __restrict__ w,
    uint4* __restrict__ dx, Conv3x3FwdPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = kConv3x3FwdBn, M = kConv3x3FwdTileRows;
  constexpr int kTapBytes = kConv3x3FwdKc * BN * 2;  // [32 n][64 c]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int c0 = conv3x3_fwd_ntile(p, blockIdx.x) * BN;  // of dX's channels
  const int split = conv3x3_fwd_split(p, blockIdx.x);
  const int nvec = p.n / 8;
  const int xbuf = p.xvecs * kT;      // vectors of a strip buffer
  uint4* wimg = lds;                  // two weight chunks
  uint4* ximg = lds + 2 * kFwdWVecs;  // two strips
  uint4* stage = ximg + 2 * xbuf + wave * 256;  // [32 rows][64 channels]

  if (RES) {  // the two chunks are the two buffers, for good
    for (int idx = tid; idx < 2 * kFwdWVecs; idx += kT) {
      const int kc = idx / kFwdWVecs, v = idx % kFwdWVecs;
      wimg[kc * kFwdWVecs + bwd_w_slot(v)] = *bwd_w_src(w, p, c0, kc, v);
    }
  }

  FwdStage<RES, true> st;
  int tile = split, kc = 0, buf = 0;  // split < row_tiles
  st.load(dy, w, p, c0, tile, 0, tid);
  st.store(wimg, ximg, p, tid);

  // as conv1x1_wrw: lane 4q+pp of a 16-lane group supplies row 8h+q of the
  // step's first read, channels 4pp .. 4pp+3 of its half of tile j's cell
  int bb[2];
#pragma unroll
  for (int j = 0; j < 2; j++)
    bb[j] = wrw_cell<BN>(8 * h + ((lane >> 2) & 3), j) +
            32 * ((lane >> 4) & 1) + 8 * (lane & 3);

  f32x16 acc[2][2];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[s][j][e] = 0.f;
  unsigned valid[2] = {0, 0};

  while (tile < p.row_tiles) {
    // as conv3x3_stats: the next stage is loaded before the MFMAs of this one
    int nkc = kc + 1, ntl = tile;
    if (nkc == p.nchunks) nkc = 0, ntl = tile + p.splits;
    const bool more = ntl < p.row_tiles;
    if (more) st.load(dy, w, p, c0, ntl, nkc, tid);
    // buffer `buf` is written, and the other one, read a stage ago, is free
    __syncthreads();
    if (kc == 0) {
#pragma unroll
      for (int s = 0; s < 2; s++)
        valid[s] = conv3x3_fwd_taps(p, tile * M + wave * 64 + s * 32 + c);
    }
    char* wl = reinterpret_cast<char*>(wimg + buf * kFwdWVecs);
    const uint4* xl = ximg + buf * xbuf;
    uint4 av[2][2];  // the operands of this step and the next
    bf16x8 bv[2][2];
    auto read = [&](int u) {
      const int tap = u >> 1, q = 2 * (u & 1) + h;
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int j = conv3x3_fwd_strip_index(p, wave * 64 + s * 32 + c, tap);
        const uint4 v = xl[fwd_slot(j, q)];
        const unsigned m = 0u - ((valid[s] >> tap) & 1u);
        av[u & 1][s] = make_uint4(v.x & m, v.y & m, v.z & m, v.w & m);
      }
#pragma unroll
      for (int j = 0; j < 2; j++)  // the mirrored tap
        bv[u & 1][j] = wrw_operand<BN>(wl + (8 - tap) * kTapBytes, bb[j], u & 1);
    };
    read(0);
#pragma unroll
    for (int u = 0; u < 18; u++) {
      if (u + 1 < 18) read(u + 1);
#pragma unroll
      for (int s = 0; s < 2; s++)
#pragma unroll
        for (int j = 0; j < 2; j++)
          acc[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(bf16x8, av[u & 1][s]), bv[u & 1][j],
              acc[s][j], 0, 0, 0);
    }
    // nothing that waits for the loads above may move up among the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    buf ^= 1;
    if (more) st.store(wimg + buf * kFwdWVecs, ximg + buf * xbuf, p, tid);

    if (nkc == 0) {  // the tile is complete: round once and store
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int r0 = tile * M + wave * 64 + s * 32;
        const int live = p.rows - r0 < 32 ? p.rows - r0 : 32;  // may be <= 0
        unsigned pk[2][8];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int e = 0; e < 8; e++)
            pk[j][e] = fwd_pack_bf16(acc[s][j][2 * e], acc[s][j][2 * e + 1]);
        fwd_store_subtile(pk, stage, dx, r0, live, nvec, c0, lane);
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int e = 0; e < 16; e++) acc[s][j][e] = 0.f;
      }
    }
    kc = nkc, tile = ntl;
  }
}

template <bool RES>
void launch_bwd3x3(const Conv3x3FwdPlan& p, const void* dy, const void* w,
                   void* dx, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv3x3_bwd_data<RES>),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL((conv3x3_bwd_data<RES>), dim3(p.grid), dim3(kT),
                     p.lds_bytes, stream, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(w), static_cast<uint4*>(dx), p);
  CGX_HIP_CHECK(hipGetLastError());
}

// ---- stride-2 input gradient --------------------------------------------------
//
// The input gradient of conv2d(x, w, stride 2, padding 1) of an image with
// even sides, written directly: no zeros are inserted into dY and no MFMA
// multiplies one.  Geometry and the four classes: Conv3x3S2BwdPlan.
//
//   A   the strip of a tile, rows 128*t .. 128*t + 128 + Wo of one 32-channel
//       chunk of dY, 64 bytes an entry in the fwd_slot layout, no parity
//       planes and no halo before the tile.  Lane (c, h) reads for shift k the
//       16 bytes of entry m + c + (k & 1) + (k & 2 ? Wo : 0): 16 consecutive
//       entries a pass, conflict-free at every start like the forwards'
//       strips, and clears them where conv3x3s2_bwd_valid lacks a bit of k
//   B   the [9 taps][32 n][64 c] chunk of conv3x3_bwd_data, unmirrored: class
//       cls and shift k multiply tap conv3x3s2_bwd_term; read transposed with
//       the same base address, the tap an immediate offset
//   C   the four waves are 2 x 2 over a 128-row x 64-channel tile: a wave owns
//       64 rows x 32 channels x four classes, 128 fp32 accumulators.  Per
//       16-deep step it reads eight A operands (two sub-tiles x four shifts)
//       and nine B operands for 18 MFMAs: 272 bytes of LDS a lane, against
//       432 in conv3x3s2_stats and 288 in conv3x3_stats
//
// A stage is one chunk of one tile, 36 MFMAs a wave, staged through registers
// behind the MFMAs of the stage before and ordered by one barrier, as in
// conv3x3_stats; the weight is always streamed.  Every accumulator is one
// chain over (chunk, step, term) in a fixed order: the same bits every run.
//
// Epilogue.  Row m of class (ph, pw) is dX pixel (2*line + ph)*W + 2b + pw,
// line = m / Wo: consecutive rows are two pixels apart and the classes of a
// row are a 2x2 cell, so no wave holds a run of pixels.  All four waves round
// their accumulators into one image [4 classes][128 rows][64 channels] of
// LDS, in the swizzle of fwd_store_subtile, and after a barrier the 256
// threads write it out as 128-byte runs, one per pixel and channel tile,
// eight lanes a run.  A thread serves four rows of the tile (the same for
// every class), so a tile costs it four divisions.  The image is written
// again only in the next tile's epilogue, at least two stage barriers later.

static_assert(kConv3x3S2BwdTileRows == 2 * 64 &&
              kConv3x3S2BwdStageBytes == 4 * kConv3x3S2BwdTileRows * 128);

// the (class, term) pairs in the order a step issues them: no class twice in a
// row, so that consecutive MFMAs do not wait for one another's result
constexpr int kS2BwdOrder[9][2] = {{3, 0}, {1, 0}, {3, 1}, {2, 0}, {3, 2},
                                   {1, 1}, {3, 3}, {2, 1}, {0, 0}};

struct S2BwdStage {
  u32x4 wv[kFwdWShare], xv[kConv3x3S2BwdXVecs];
  __device__ __forceinline__ void load(const uint4* __restrict__ dy,
                                       const uint4* __restrict__ w,
                                       const Conv3x3S2BwdPlan& p, int c0,
                                       int tile, int kc, int tid) {
#pragma unroll
    for (int i = 0; i < kFwdWShare; i++)
      wv[i] = *reinterpret_cast<const u32x4*>(
          bwd_w_src(w, p, c0, kc, tid + i * kT));
#pragma unroll
    for (int i = 0; i < kConv3x3S2BwdXVecs; i++)
      if (i < p.xvecs) {  // uniform
        const int idx = tid + i * kT;
        const int64_t r = conv3x3s2_bwd_strip_row(p, tile, idx >> 2);
        xv[i] = *reinterpret_cast<const u32x4*>(
            dy + (r * p.c + kc * kConv3x3FwdKc) / 8 + (idx & 3));
      }
  }
  __device__ __forceinline__ void store(uint4* wb, uint4* xb,
                                        const Conv3x3S2BwdPlan& p,
                                        int tid) const {
#pragma unroll
    for (int i = 0; i < kFwdWShare; i++)
      *reinterpret_cast<u32x4*>(wb + bwd_w_slot(tid + i * kT)) = wv[i];
#pragma unroll
    for (int i = 0; i < kConv3x3S2BwdXVecs; i++)
      if (i < p.xvecs) {
        const int idx = tid + i * kT;
        *reinterpret_cast<u32x4*>(xb + fwd_slot(idx >> 2, idx & 3)) = xv[i];
      }
  }
};

__global__ __launch_bounds__(kT) void conv3x3s2_bwd_data(
    const uint4* __restrict__ dy, const uint4* __restrict__ w,
    uint4* __restrict__ dx, Conv3x3S2BwdPlan p) {
  extern __shared__ uint4 lds[];
  constexpr int BN = kConv3x3FwdBn, M = kConv3x3S2BwdTileRows;
  constexpr int kTapBytes = kConv3x3FwdKc * BN * 2;  // [32 n][64 c]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;  // the wave's rows and channels
  const int c0 = conv3x3_fwd_ntile(p, blockIdx.x) * BN;  // of dX's channels
  const int split = conv3x3_fwd_split(p, blockIdx.x);
  const int nvec = p.n / 8;
  const int xbuf = p.xvecs * kT;      // vectors of a strip buffer
  uint4* wimg = lds;                  // two weight chunks
  uint4* ximg = lds + 2 * kFwdWVecs;  // two strips
  uint4* stage = ximg + 2 * xbuf;     // [4 classes][128 rows][64 channels]

  S2BwdStage st;
  int tile = split, kc = 0, buf = 0;  // split < row_tiles
  st.load(dy, w, p, c0, tile, 0, tid);
  st.store(wimg, ximg, p, tid);

  // the lane's B base, as conv3x3_bwd_data, for the wave's 32 channels ...
  const int bb = wrw_cell<BN>(8 * h + ((lane >> 2) & 3), wc) +
                 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  // ... and the strip entry of each shift for its row of each sub-tile, the
  // same on every tile
  int at[2][4];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int k = 0; k < 4; k++)
      at[s][k] = conv3x3s2_bwd_strip_index(p, wr * 64 + s * 32 + c, k);

  f32x16 acc[4][2];  // [class][sub-tile]
#pragma unroll
  for (int cls = 0; cls < 4; cls++)
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[cls][s][e] = 0.f;
  unsigned valid[2] = {0, 0};

  while (tile < p.row_tiles) {
    // as conv3x3_stats: the next stage is loaded before the MFMAs of this one
    int nkc = kc + 1, ntl = tile;
    if (nkc == p.nchunks) nkc = 0, ntl = tile + p.splits;
    const bool more = ntl < p.row_tiles;
    if (more) st.load(dy, w, p, c0, ntl, nkc, tid);
    // buffer `buf` is written, and the other one, read a stage ago, is free
    __syncthreads();
    if (kc == 0) {
#pragma unroll
      for (int s = 0; s < 2; s++)
        valid[s] = conv3x3s2_bwd_valid(p, tile * M + wr * 64 + s * 32 + c);
    }
    char* wl = reinterpret_cast<char*>(wimg + buf * kFwdWVecs);
    const uint4* xl = ximg + buf * xbuf;
    uint4 av[2][2][4];  // [step][sub-tile][shift]
    bf16x8 bv[2];       // the B operand of this unit and the next
    auto read_a = [&](int step, int i) {  // operand i = 4*s + k of a step
      const int s = i >> 2, k = i & 3;
      const uint4 v = xl[fwd_slot(at[s][k], 2 * step + h)];
      const unsigned m = (valid[s] & k) == (unsigned)k ? ~0u : 0u;
      av[step][s][k] = make_uint4(v.x & m, v.y & m, v.z & m, v.w & m);
    };
    auto read_b = [&](int u) {  // unit u = 9*step + position in the order
      const int step = u / 9, i = u % 9;
      const int tap =
          conv3x3s2_bwd_term(kS2BwdOrder[i][0], kS2BwdOrder[i][1]).tap;
      bv[u & 1] = wrw_operand<BN>(wl + tap * kTapBytes, bb, step);
    };
#pragma unroll
    for (int i = 0; i < 8; i++) read_a(0, i);
    read_b(0);
#pragma unroll
    for (int u = 0; u < 18; u++) {
      if (u + 1 < 18) read_b(u + 1);
      if (u < 8) read_a(1, u);  // the second step's A behind the first's MFMAs
      const int step = u / 9, i = u % 9, cls = kS2BwdOrder[i][0];
      const int k = conv3x3s2_bwd_term(cls, kS2BwdOrder[i][1]).shift;
#pragma unroll
      for (int s = 0; s < 2; s++)
        acc[cls][s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            __builtin_bit_cast(bf16x8, av[step][s][k]), bv[u & 1], acc[cls][s],
            0, 0, 0);
    }
    // nothing that waits for the loads above may move up among the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    buf ^= 1;
    if (more) st.store(wimg + buf * kFwdWVecs, ximg + buf * xbuf, p, tid);

    if (nkc == 0) {  // the tile is complete: round once, gather, store
      unsigned* stage32 = reinterpret_cast<unsigned*>(stage);
      const int odd = c & 1;
#pragma unroll
      for (int cls = 0; cls < 4; cls++)
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
          for (int e = 0; e < 8; e++) {
            // as fwd_store_subtile: lanes c and c^1 trade words, so that the
            // even lane writes channels (c, c+1) of row 2e and the odd one
            // channels (c-1, c) of row 2e+1
            const unsigned own =
                fwd_pack_bf16(acc[cls][s][2 * e], acc[cls][s][2 * e + 1]);
            const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(
                0, (int)own, 0xB1, 0xf, 0xf, false);  // quad_perm [1, 0, 3, 2]
            const unsigned word = odd ? (other >> 16) | (own & 0xffff0000u)
                                      : (own & 0xffffu) | (other << 16);
            const int row =
                cls * M + wr * 64 + s * 32 + acc_row(2 * e, h) + odd;
            stage32[row * 32 + ((wc * 16 + (c >> 1)) ^ ((row & 1) << 4))] = word;
            acc[cls][s][2 * e] = 0.f, acc[cls][s][2 * e + 1] = 0.f;
          }
      // the thread's four rows of the tile: their cells' first pixels
      int pix[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int row = tile * M + j * 32 + (tid >> 3);
        pix[j] = row < p.rows ? conv3x3s2_bwd_pixel(p, row, 0) : -1;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 16; u++) {
        const int idx = u * kT + tid, row = idx >> 3, q = idx & 7;
        const int cls = u >> 2, px = pix[u & 3];
        const uint4 v = stage[row * 8 + (q ^ ((row & 1) << 2))];
        if (px >= 0)
          dx[(int64_t)(px + (cls >> 1) * p.w + (cls & 1)) * nvec + c0 / 8 + q] =
              v;
      }
    }
    kc = nkc, tile = ntl;
  }
}

void launch_bwd3x3s2(const Conv3x3S2BwdPlan& p, const void* dy, const void* w,
                     void* dx, hipStream_t stream) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv3x3s2_bwd_data),
      hipFuncAttributeMaxDynamicSharedMemorySize, kConvLdsBytes);
  CGX_HIP_CHECK(attr);
  hipLaunchKernelGGL(conv3x3s2_bwd_data, dim3(p.grid), dim3(kT), p.lds_bytes,
                     stream, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(w), static_cast<uint4*>(dx), p);
  CGX_HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_conv3x3s2_bwd_data(const Conv3x3S2BwdPlan& p, const void* dy,
                               const void* w, void* dx, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv3x3s2_bwd_data: shape is not eligible");
  TORCH_CHECK(p.bn == kConv3x3FwdBn && p.kc == kConv3x3FwdKc &&
                  p.tile_rows == kConv3x3S2BwdTileRows &&
                  p.xvecs <= kConv3x3S2BwdXVecs &&
                  p.strip_rows == p.tile_rows + p.wo + 1 &&
                  p.strip_rows <= 64 * p.xvecs && p.nchunks >= 2 &&
                  p.splits <= p.row_tiles && p.lds_bytes <= kConvLdsBytes,
              "conv3x3s2_bwd_data: plan and kernel disagree");
  launch_bwd3x3s2(p, dy, w, dx, stream);
}

void launch_conv3x3_bwd_data(const Conv3x3FwdPlan& p, const void* dy,
                             const void* w, void* dx, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv3x3_bwd_data: shape is not eligible");
  TORCH_CHECK(p.bn == kConv3x3FwdBn && p.kc == kConv3x3FwdKc &&
                  p.xvecs <= kConv3x3FwdXVecs &&
                  p.strip_rows <= 64 * p.xvecs && p.splits <= p.row_tiles &&
                  p.resident == (p.nchunks == 2) &&
                  p.lds_bytes <= kConvLdsBytes,
              "conv3x3_bwd_data: plan and kernel disagree");
  if (p.resident) launch_bwd3x3<true>(p, dy, w, dx, stream);
  else launch_bwd3x3<false>(p, dy, w, dx, stream);
}

void launch_conv3x3_stats(const Conv3x3FwdPlan& p, const void* x, const void* w,
                          void* y, float* part, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv3x3_stats: shape is not eligible");
  TORCH_CHECK(p.bn == kConv3x3FwdBn && p.kc == kConv3x3FwdKc &&
                  p.xvecs <= kConv3x3FwdXVecs &&
                  p.strip_rows <= 64 * p.xvecs && p.splits <= p.row_tiles &&
                  p.resident == (p.nchunks == 2) &&
                  p.lds_bytes <= kConvLdsBytes,
              "conv3x3_stats: plan and kernel disagree");
  if (p.resident) launch_fwd3x3<true>(p, x, w, y, part, stream);
  else launch_fwd3x3<false>(p, x, w, y, part, stream);
}

void launch_conv3x3s2_stats(const Conv3x3S2FwdPlan& p, const void* x,
                            const void* w, void* y, float* part,
                            hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv3x3s2_stats: shape is not eligible");
  TORCH_CHECK(p.bn == kConv3x3FwdBn && p.kc == kConv3x3FwdKc &&
                  p.tile_rows == kConv3x3S2TileRows &&
                  p.xvecs <= kConv3x3S2XVecs && p.strip_rows <= 64 * p.xvecs &&
                  p.plane_base[3] + p.plane_rows[3] == p.strip_rows &&
                  p.splits <= p.row_tiles && p.lds_bytes <= kConvLdsBytes,
              "conv3x3s2_stats: plan and kernel disagree");
  launch_fwd3x3s2(p, x, w, y, part, stream);
}

void launch_conv3x3_wrw(const Conv3x3WrwPlan& p, const void* dy, const void* x,
                        float* part, void* dw, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv3x3_wrw: shape is not eligible");
  TORCH_CHECK(p.bn == 64 && p.bk == 64 && p.lds_bytes <= kConvLdsBytes &&
                  p.splits <= p.chunks,
              "conv3x3_wrw: plan and kernel disagree");
  launch_wrw3x3<64, 64>(p, dy, x, part, stream);
  launch_wrw_finalize(part, dw, p.splits, (int64_t)p.n * 9 * p.c, stream);
}

void launch_conv3x3_wrw_ring(const Conv3x3WrwRingPlan& p, const void* dy,
                             const void* x, const void* zeros, float* part,
                             void* dw, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv3x3_wrw_ring: shape is not eligible");
  const int glds = p.dy_glds + p.x_glds;
  TORCH_CHECK(p.bn == 64 && p.bk == 64 && p.stages >= 2 && p.stages <= 3 &&
                  glds <= kConv3x3RingMaxGlds &&
                  p.strip_dy <= 32 * p.dy_glds && p.strip_x <= 32 * p.x_glds &&
                  p.strip_dy % 32 == 0 && p.stage_bytes == glds * 4096 &&
                  p.lds_bytes == p.stages * p.stage_bytes &&
                  p.lds_bytes <= kConvLdsBytes && p.splits <= p.chunks &&
                  zeros != nullptr,
              "conv3x3_wrw_ring: plan and kernel disagree");
  launch_wrw3x3_ring(p, dy, x, zeros, part, stream);
  launch_wrw_finalize(part, dw, p.splits, (int64_t)p.n * 9 * p.c, stream);
}

void launch_conv3x3s2_wrw(const Conv3x3S2WrwPlan& p, const void* dy,
                          const void* x, const void* zeros, float* part,
                          void* dw, hipStream_t stream) {
  TORCH_CHECK(p.eligible, "conv3x3s2_wrw: shape is not eligible");
  const int last = p.plane_base[0] + p.plane_size[0];
  TORCH_CHECK(p.bn == 64 && p.bk == 64 && p.glds <= kConv3x3RingMaxGlds &&
                  p.strip_dy % 32 == 0 && p.live <= p.strip_dy &&
                  p.plane_base[3] == p.strip_dy && last <= p.stage_pos &&
                  p.plane_base[0] + p.strip_dy <= p.stage_pos &&
                  p.stage_pos == 32 * p.glds &&
                  p.stage_bytes == p.glds * 4096 &&
                  p.lds_bytes == 2 * p.stage_bytes &&
                  p.lds_bytes <= kConvLdsBytes && p.splits <= p.chunks &&
                  zeros != nullptr,
              "conv3x3s2_wrw: plan and kernel disagree");
  launch_wrw3x3s2(p, dy, x, zeros, part, stream);
  launch_wrw_finalize(part, dw, p.splits, (int64_t)p.n * 9 * p.c, stream);
}

}  // namespace cgx
