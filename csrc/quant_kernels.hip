// CDNA4 (gfx950) max-min quantization kernels for the cgx backend.
//
// The host router (compress.h route_quantize/route_dequantize) decides which
// kernel serves which slice; launch() at the end of this file dispatches a
// routed group.  The family is REGISTER-ISOLATED: the register allocator
// sizes a kernel for its worst path, so each hot path is its own launch and
// is kept at the allocation it was measured with (benchmarks/RESULTS.md).
//
//  pinned (hot) kernels
//    k_quantize_fast  QuantRun: one wave per bucket, bucket % 8 == 0 and
//                     <= 2048, so every lane's packs stay in registers
//                     between the min/max reduction and the encode (single
//                     HBM read); compile-time groups per lane; 16-bit
//                     dtypes reduce with packed v_pk_min/max.
//    k_quantize_sub   QuantSub: power-of-two buckets < 512 pack
//                     64/(bucket/8) buckets per wave with segmented DPP
//                     reductions.
//    k_dequant_fast   bucket % 8 == 0, u32-indexable: one 16-byte store per
//                     thread per iteration, incremental bucket index,
//                     compile-time alignment/accumulate flags.
//  generic (cold) kernels, one body each
//    k_quantize       error feedback, unaligned input, bucket > 2048,
//                     partial buckets (kFlagTailOnly) and, with
//                     ENCODE=false, the meta pass of bucket % 8 != 0.
//    k_pack_generic   the pack pass of bucket % 8 != 0.
//    k_dequant        bucket % 8 != 0, slices of 2^31 or more elements and
//                     ragged tails (kFlagTailOnly): decode_unit.
//    k_residual_q/_d  raw skip_incomplete tails;  k_add  y += x.
//
//  * the numeric spec lives once: slice_geom (compress.h) for the wire
//    layout, quant_level/encode_pack for encode, decode_raw/accum_raw for
//    decode; every kernel inlines these.
//  * memory-bound workload: 16-byte loads/stores wherever the base is
//    16B-aligned, and no integer division in a hot loop.
//  * min/max reductions are DPP row operations (seg_minmax), not shuffles.
//  * stochastic rounding via a stateless splitmix64 hash per pack (no RNG
//    state buffers, deterministic given the per-launch seed; the hash key is
//    the GLOBAL pack index, so the kernel split is byte-transparent);
//    optional error-feedback residual update fused into the encode.
//
// Wire-format parity with the reference implementation is defined by
// torch_cgx_amd/ops/golden.py (see reference
// src/common/compression/cuda_compression_operations.cu:68-96,219-285).
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <type_traits>

#include "compress.h"
#include "config.h"

namespace cgx {
namespace {

constexpr float kEps = 1e-10f;
constexpr int kThreads = 256;  // 4 waves
constexpr int kWave = 64;
constexpr int kMaxBlocks = 4096;  // 256 CU * 8 blocks/CU * 2

// One splitmix64-style hash per 8-value pack; each element draws 8 bits of
// uniform randomness ([0,1) in steps of 1/256: a fraction f rounds up with
// probability floor(256 f)/256, so the rounding bias per element lies in
// (-1/256, 0] of a quantization unit, -1/512 on average -- negligible vs. the
// unit-sized quantization error).  torch_cgx_amd/ops/golden.py models the
// hash (pack_rand_words / stochastic_rand); tests/test_gpu_stochastic.py
// holds every kernel to it byte for byte.
__device__ __forceinline__ uint64_t rand_pack(uint64_t seed, uint64_t key) {
  uint64_t z = seed + key * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The random word of one pack: keyed by the slice's index in its launch
// group and the pack's index in the slice (0 when rounding is deterministic).
__device__ __forceinline__ uint64_t pack_rand(uint64_t seed, int stochastic,
                                              int slice_idx, int64_t pack) {
  return stochastic
             ? rand_pack(seed, (static_cast<uint64_t>(slice_idx) << 44) |
                                   static_cast<uint64_t>(pack))
             : 0;
}

__device__ __forceinline__ float rand_lane(uint64_t pack_rand, int j) {
  return static_cast<float>((pack_rand >> (8 * j)) & 0xFF) * (1.0f / 256.0f);
}

// Min/max reduction over aligned segments of L lanes (a power of two; L = 64
// is the whole wave) via DPP row operations (register path, ~2 cycles/step)
// instead of __shfl_xor, which hipcc lowers to six dependent ds_bpermute_b32
// (LDS latency) per value.  Ladder: row_shr 1/2/4/8, row_bcast 15/31,
// truncated at L; the segment's last lane then holds its result, which is
// handed to every lane by readlane 63 (L = 64) or one ds_bpermute.
template <int CTRL, bool MAX>
__device__ __forceinline__ float dpp_step(float v) {
  const int ident = __builtin_bit_cast(int, MAX ? -INFINITY : INFINITY);
  const float t = __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(ident, __builtin_bit_cast(int, v),
                                         CTRL, 0xf, 0xf, false));
  return MAX ? fmaxf(v, t) : fminf(v, t);
}

template <int L, bool MAX>
__device__ __forceinline__ float dpp_ladder(float v) {
  if constexpr (L >= 2) v = dpp_step<0x111, MAX>(v);   // row_shr:1
  if constexpr (L >= 4) v = dpp_step<0x112, MAX>(v);   // row_shr:2
  if constexpr (L >= 8) v = dpp_step<0x114, MAX>(v);   // row_shr:4
  if constexpr (L >= 16) v = dpp_step<0x118, MAX>(v);  // row_shr:8
  if constexpr (L >= 32) v = dpp_step<0x142, MAX>(v);  // row_bcast:15
  if constexpr (L >= 64) v = dpp_step<0x143, MAX>(v);  // row_bcast:31
  return v;
}

// The statement order below (for the whole wave: min ladder, readlane, max
// ladder, readlane) is the one the pinned kernels were measured with.
template <int L>
__device__ __forceinline__ void seg_minmax(float& vmin, float& vmax,
                                           int lane) {
  if constexpr (L == kWave) {
    const int imin = __builtin_bit_cast(int, dpp_ladder<L, false>(vmin));
    vmin = __builtin_bit_cast(float, __builtin_amdgcn_readlane(imin, 63));
    const int imax = __builtin_bit_cast(int, dpp_ladder<L, true>(vmax));
    vmax = __builtin_bit_cast(float, __builtin_amdgcn_readlane(imax, 63));
  } else if constexpr (L > 1) {
    const int imin = __builtin_bit_cast(int, dpp_ladder<L, false>(vmin));
    const int imax = __builtin_bit_cast(int, dpp_ladder<L, true>(vmax));
    const int src = ((lane / L) * L + (L - 1)) * 4;
    vmin = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, imin));
    vmax = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, imax));
  }
}

template <typename To, typename From>
__device__ __forceinline__ To bitcast(From f) {
  static_assert(sizeof(To) == sizeof(From));
  To t;
  __builtin_memcpy(&t, &f, sizeof(To));
  return t;
}

template <typename T>
struct RawOf;
template <>
struct RawOf<float> {
  using type = uint32_t;
};
template <>
struct RawOf<__half> {
  using type = uint16_t;
};
template <>
struct RawOf<__hip_bfloat16> {
  using type = uint16_t;
};

// All element math runs on raw bit patterns + fp32; conversions below are the
// only dtype-specific pieces.  T-precision ops (decode mul/add, accumulate)
// are expressed as fp32 ops + round-to-T, which is bitwise identical to
// native T arithmetic because products/sums of two T values are exact in
// fp32 for all of {fp32, fp16, bf16}.
template <typename T>
__device__ __forceinline__ float raw2f(uint32_t r);
template <>
__device__ __forceinline__ float raw2f<float>(uint32_t r) {
  return bitcast<float>(r);
}
template <>
__device__ __forceinline__ float raw2f<__half>(uint32_t r) {
  return __half2float(bitcast<__half>(static_cast<uint16_t>(r)));
}
template <>
__device__ __forceinline__ float raw2f<__hip_bfloat16>(uint32_t r) {
  return __bfloat162float(bitcast<__hip_bfloat16>(static_cast<uint16_t>(r)));
}

template <typename T>
__device__ __forceinline__ uint32_t f2raw(float f);
template <>
__device__ __forceinline__ uint32_t f2raw<float>(float f) {
  return bitcast<uint32_t>(f);
}
template <>
__device__ __forceinline__ uint32_t f2raw<__half>(float f) {
  return bitcast<uint16_t>(__float2half(f));
}
template <>
__device__ __forceinline__ uint32_t f2raw<__hip_bfloat16>(float f) {
  return bitcast<uint16_t>(__float2bfloat16(f));
}

// ---------------------------------------------------------------------------
// The numeric spec, one copy each (docs/DESIGN.md "Numerics").
// ---------------------------------------------------------------------------
// 8 levels fit a uint32 when BITS <= 4: halves the shift/or cost
template <int BITS>
using pack_acc_t =
    typename std::conditional<(BITS <= 4), uint32_t, uint64_t>::type;

// Quantization level of one element; rnd is 0.5 (deterministic) or uniform
// in [0,1) (stochastic).
template <typename T>
__device__ __forceinline__ uint32_t quant_level(uint32_t raw, float minf,
                                                float rinv, float rnd,
                                                float divisor) {
  const float dd = (raw2f<T>(raw) - minf) * rinv + rnd;
  return static_cast<uint32_t>(fminf(floorf(dd), divisor));
}

template <int BITS, typename Acc>
__device__ __forceinline__ Acc level_bits(uint32_t level, int j) {
  return static_cast<Acc>(level & ((1u << BITS) - 1)) << (j * BITS);
}

// Encode one full pack: 8 raw values -> packed word.  pr is the pack's
// random word (rand_pack), read only when stochastic.
template <typename T, int BITS, typename Acc = pack_acc_t<BITS>>
__device__ __forceinline__ Acc encode_pack(const uint32_t (&r)[8], float minf,
                                           float rinv, float divisor,
                                           uint64_t pr, int stochastic) {
  Acc value = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const float rnd = stochastic ? rand_lane(pr, j) : 0.5f;
    value |= level_bits<BITS, Acc>(
        quant_level<T>(r[j], minf, rinv, rnd, divisor), j);
  }
  return value;
}

// Partial pack (first m <= 8 values); also returns the levels, which the
// error-feedback residual needs.
template <typename T, int BITS>
__device__ __forceinline__ uint64_t encode_pack(const uint32_t (&r)[8], int m,
                                                float minf, float rinv,
                                                float divisor, uint64_t pr,
                                                int stochastic,
                                                uint32_t (&lv)[8]) {
  uint64_t value = 0;
  for (int j = 0; j < m; j++) {
    const float rnd = stochastic ? rand_lane(pr, j) : 0.5f;
    lv[j] = quant_level<T>(r[j], minf, rinv, rnd, divisor);
    value |= level_bits<BITS, uint64_t>(lv[j], j);
  }
  return value;
}

template <int BITS>
__device__ __forceinline__ uint32_t pack_level(uint64_t value, int j) {
  return static_cast<uint32_t>((value >> (j * BITS)) & ((1u << BITS) - 1));
}

// Decode: round(unit*lvl) then round(min + product), both to T.
template <typename T>
__device__ __forceinline__ uint32_t decode_raw(uint32_t unit_raw,
                                               uint32_t min_raw,
                                               uint32_t lvl) {
  const uint32_t prod =
      f2raw<T>(raw2f<T>(unit_raw) * static_cast<float>(lvl));
  return f2raw<T>(raw2f<T>(min_raw) + raw2f<T>(prod));
}

// T-precision accumulate in source order; the first source of a non-adding
// decode just lands.
template <typename T>
__device__ __forceinline__ void accum_raw(uint32_t& acc, bool first,
                                          uint32_t dec) {
  if (first) {
    acc = dec;
  } else {
    acc = f2raw<T>(raw2f<T>(acc) + raw2f<T>(dec));
  }
}

// Slice owning work unit b: largest i with cum[i] <= b.
__device__ __forceinline__ int find_slice(const int64_t* __restrict__ cum,
                                          int nslices, int64_t b) {
  int lo = 0, hi = nslices;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

template <typename T>
__device__ __forceinline__ SliceGeom geom_of(int64_t n, int32_t bucket,
                                             int32_t flags, int bits) {
  return slice_geom(n, bucket, bits, sizeof(T),
                    (flags & kFlagSkipIncomplete) != 0);
}

// Packed-pair min/max for 16-bit dtypes (v_pk_min/max_f16|bf16): phase A of
// the fp16/bf16 quantize was 87% VALU-busy with per-element convert+min+max;
// packed ops process 2 elements per instruction without unpacking.
template <typename T>
struct Pk2Elem;
template <>
struct Pk2Elem<__half> {
  using type = _Float16;
  static constexpr uint32_t kInf = 0x7C00u;
};
template <>
struct Pk2Elem<__hip_bfloat16> {
  using type = __bf16;
  static constexpr uint32_t kInf = 0x7F80u;
};
template <typename T>
struct Pk2 {
  using P = typename Pk2Elem<T>::type __attribute__((ext_vector_type(2)));
  static constexpr uint32_t kInf = Pk2Elem<T>::kInf * 0x10001u;  // +inf, +inf
  static constexpr uint32_t kNInf = kInf | 0x80008000u;          // -inf, -inf
  static __device__ __forceinline__ P min(P a, P b) {
    return __builtin_elementwise_min(a, b);
  }
  static __device__ __forceinline__ P max(P a, P b) {
    return __builtin_elementwise_max(a, b);
  }
  static __device__ __forceinline__ float lo(P v) {
    return static_cast<float>(v[0]);
  }
  static __device__ __forceinline__ float hi(P v) {
    return static_cast<float>(v[1]);
  }
};

using v4u = uint32_t __attribute__((ext_vector_type(4)));

// Compile-time-aligned 16-byte load/store (a runtime alignment flag compiles
// into per-dword flat accesses inside a hot loop).
template <bool AL16>
__device__ __forceinline__ void load16B(const void* p, uint32_t (&r)[4]) {
  if constexpr (AL16) {
    const v4u a = *reinterpret_cast<const v4u*>(
        __builtin_assume_aligned(p, 16));
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
  } else {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = q[j];
  }
}

template <bool AL16>
__device__ __forceinline__ void store16B(void* p, const uint32_t (&r)[4]) {
  if constexpr (AL16) {
    v4u a;
    a.x = r[0]; a.y = r[1]; a.z = r[2]; a.w = r[3];
    *reinterpret_cast<v4u*>(__builtin_assume_aligned(p, 16)) = a;
  } else {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = r[j];
  }
}

// First m >= 1 of N raw values at p (the rest repeat the first, so a min/max
// over all N needs no mask), for the generic kernels
// and QuantSub: 16-byte accesses when all N are there and p is 16B-aligned,
// element accesses otherwise -- a 16-bit base that is only 2-byte aligned
// must not be touched with 32-bit accesses.  N * sizeof(T) is 16 or 32.
// (Plain int4 accesses: through load16B<true> every k_quantize_sub
// instantiation compiles to other code than it was measured with.)
template <typename T, int N>
__device__ __forceinline__ void load_vec(const T* p, bool aligned16, int m,
                                         uint32_t (&r)[N]) {
  constexpr int E = 16 / sizeof(T);
  if (m == N && aligned16) {
#pragma unroll
    for (int c = 0; c < N; c += E) {
      const int4 a = *reinterpret_cast<const int4*>(p + c);
      const uint32_t w[4] = {static_cast<uint32_t>(a.x),
                             static_cast<uint32_t>(a.y),
                             static_cast<uint32_t>(a.z),
                             static_cast<uint32_t>(a.w)};
#pragma unroll
      for (int j = 0; j < E; j++) {
        if constexpr (sizeof(T) == 4) r[c + j] = w[j];
        else r[c + j] = (w[j >> 1] >> ((j & 1) * 16)) & 0xFFFF;
      }
    }
    return;
  }
  const auto* q = reinterpret_cast<const typename RawOf<T>::type*>(p);
  if (m == N) {
#pragma unroll
    for (int j = 0; j < N; j++) r[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < N; j++) r[j] = q[j < m ? j : 0];
  }
}

template <typename T, int N>
__device__ __forceinline__ void store_vec(T* p, bool aligned16, int m,
                                          const uint32_t (&r)[N]) {
  constexpr int E = 16 / sizeof(T);
  if (m == N && aligned16) {
#pragma unroll
    for (int c = 0; c < N; c += E) {
      int w[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if constexpr (sizeof(T) == 4) w[j] = r[c + j];
        else w[j] = r[c + 2 * j] | (r[c + 2 * j + 1] << 16);
      }
      *reinterpret_cast<int4*>(p + c) = int4{w[0], w[1], w[2], w[3]};
    }
    return;
  }
  using R = typename RawOf<T>::type;
  R* q = reinterpret_cast<R*>(p);
#pragma unroll
  for (int j = 0; j < N; j++) {
    if (j < m) q[j] = static_cast<R>(r[j]);
  }
}

// Write the low `nb` bytes of v to p (little-endian), widest aligned stores.
__device__ __forceinline__ void store_bytes(uint8_t* p, uint64_t v, int nb) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (nb == 8 && (a & 7) == 0) {
    *reinterpret_cast<uint64_t*>(p) = v;
    return;
  }
  if (nb == 4 && (a & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = static_cast<uint32_t>(v);
    return;
  }
  if (nb == 2 && (a & 1) == 0) {
    *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(v);
    return;
  }
  for (int i = 0; i < nb; i++) p[i] = static_cast<uint8_t>(v >> (8 * i));
}

__device__ __forceinline__ uint64_t load_bytes(const uint8_t* p, int nb) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (nb == 8) {
    if ((a & 7) == 0) return *reinterpret_cast<const uint64_t*>(p);
    if ((a & 3) == 0) {
      const uint32_t lo = reinterpret_cast<const uint32_t*>(p)[0];
      const uint32_t hi = reinterpret_cast<const uint32_t*>(p)[1];
      return static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
    }
  }
  if (nb == 4) {
    if ((a & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
    if ((a & 1) == 0) {
      const uint16_t lo = reinterpret_cast<const uint16_t*>(p)[0];
      const uint16_t hi = reinterpret_cast<const uint16_t*>(p)[1];
      return static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 16);
    }
  }
  if (nb == 2 && (a & 1) == 0) return *reinterpret_cast<const uint16_t*>(p);
  uint64_t v = 0;
  for (int i = 0; i < nb; i++) v |= static_cast<uint64_t>(p[i]) << (8 * i);
  return v;
}

// Register-resident quantize of a RUN of full buckets (bucket % 8 == 0, 16B
// aligned, no error feedback) with a COMPILE-TIME groups-per-lane count G.
// Two design points vs the round-1 per-bucket fast path:
//  * G is a template parameter, so the stash loops fully unroll (the
//    runtime-trip form compiled into s_set_gpr_idx register-indexed access);
//  * the wave pipelines bucket i+1's HBM loads under bucket i's
//    reduce+encode (two stash banks, statically unrolled 2x steady state) —
//    the PMC profile showed SQ_WAIT_ANY ~17x SQ_BUSY on the serial
//    load->reduce->encode chain.
// 16-bit dtypes stash the RAW dwords (w[G][4], half the registers) and run
// packed v_pk_min/max on them; elements are extracted at encode time.
template <typename T, int BITS, int G>
struct QuantRun {
  using R = typename RawOf<T>::type;
  static constexpr int kWords = sizeof(T) == 4 ? 8 : 4;
  struct Stash {
    uint32_t w[G][kWords];
  };

  const T* __restrict__ base;
  R* __restrict__ meta;
  uint8_t* __restrict__ packed;
  int lane;
  int ngroups;  // per bucket
  float divisor;
  uint64_t seed;
  int stochastic;
  int slice_idx;

  __device__ __forceinline__ void load(Stash& s, int64_t lb) const {
    const T* in = base + lb * (int64_t)(ngroups * 8);
#pragma unroll
    for (int k = 0; k < G; k++) {
      const int g = lane + k * kWave;
      if (g >= ngroups) continue;  // buckets < 512: extra lanes idle
      const int4 a = *reinterpret_cast<const int4*>(
          __builtin_assume_aligned(in + g * 8, 16));
      if constexpr (sizeof(T) == 4) {
        const int4 b = *reinterpret_cast<const int4*>(
            __builtin_assume_aligned(in + g * 8 + 4, 16));
        s.w[k][0] = a.x; s.w[k][1] = a.y; s.w[k][2] = a.z; s.w[k][3] = a.w;
        s.w[k][4] = b.x; s.w[k][5] = b.y; s.w[k][6] = b.z; s.w[k][7] = b.w;
      } else {
        s.w[k][0] = a.x; s.w[k][1] = a.y; s.w[k][2] = a.z; s.w[k][3] = a.w;
      }
    }
  }

  __device__ __forceinline__ uint32_t elem(const Stash& s, int k,
                                           int j) const {
    if constexpr (sizeof(T) == 4) {
      return s.w[k][j];
    } else {
      return (s.w[k][j >> 1] >> ((j & 1) * 16)) & 0xFFFF;
    }
  }

  __device__ __forceinline__ void encode(const Stash& s, int64_t lb) const {
    float lmin = INFINITY, lmax = -INFINITY;
    if constexpr (sizeof(T) == 2) {
      using PK = Pk2<T>;
      typename PK::P pmin = bitcast<typename PK::P>(PK::kInf);
      typename PK::P pmax = bitcast<typename PK::P>(PK::kNInf);
#pragma unroll
      for (int k = 0; k < G; k++) {
        const int g = lane + k * kWave;
        if (g >= ngroups) continue;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const auto v = bitcast<typename PK::P>(s.w[k][q]);
          pmin = PK::min(pmin, v);
          pmax = PK::max(pmax, v);
        }
      }
      lmin = fminf(PK::lo(pmin), PK::hi(pmin));
      lmax = fmaxf(PK::lo(pmax), PK::hi(pmax));
    } else {
#pragma unroll
      for (int k = 0; k < G; k++) {
        const int g = lane + k * kWave;
        if (g >= ngroups) continue;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float f = raw2f<T>(s.w[k][j]);
          lmin = fminf(lmin, f);
          lmax = fmaxf(lmax, f);
        }
      }
    }
    seg_minmax<kWave>(lmin, lmax, lane);
    const uint32_t unit_raw = f2raw<T>((lmax - lmin) / divisor);
    const float unitf = raw2f<T>(unit_raw);
    const float minf = lmin;
    if (lane == 0) {
      meta[2 * lb] = static_cast<R>(unit_raw);
      meta[2 * lb + 1] = static_cast<R>(f2raw<T>(lmin));
    }
    const bool live = unitf >= kEps;
    const float rinv = live ? 1.0f / unitf : 0.0f;
    const int64_t gbase = lb * (int64_t)ngroups;
#pragma unroll
    for (int k = 0; k < G; k++) {
      const int g = lane + k * kWave;
      if (g >= ngroups) continue;
      pack_acc_t<BITS> value = 0;
      if (live) {
        uint32_t r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = elem(s, k, j);
        value = encode_pack<T, BITS>(
            r, minf, rinv, divisor,
            pack_rand(seed, stochastic, slice_idx, gbase + g), stochastic);
      }
      store_bytes(packed + (gbase + g) * BITS, static_cast<uint64_t>(value),
                  BITS);
    }
  }

  // count buckets at lb0, lb0+nw, ...  Single stash bank (used by the
  // MAXGT>=2 kernel variants, where a second bank costs occupancy — the
  // two-bank pipeline was measured and rejected twice, see RESULTS.md).
  __device__ __forceinline__ void run(int64_t lb0, int64_t count,
                                      int64_t nw) const {
    Stash A;
    for (int64_t i = 0; i < count; i++) {
      load(A, lb0 + i * nw);
      encode(A, lb0 + i * nw);
    }
  }

};

// Sub-wave quantize for SMALL buckets (bucket/8 = L lanes per bucket, a
// power of two < 64): the wave-per-bucket layout leaves (64-L) lanes idle
// and serializes 64/L x more buckets per wave; here the wave processes
// W = 64/L buckets at once, reducing each L-lane segment with the DPP
// ladder truncated at L (seg_minmax<L>).  Bucket 256 measured 1.3-2.4 TB/s
// on the wave-per-bucket path; this recovers most of the bucket-1024 rate.
template <typename T, int BITS, int L>
struct QuantSub {
  using R = typename RawOf<T>::type;
  const T* __restrict__ base;
  R* __restrict__ meta;
  uint8_t* __restrict__ packed;
  int lane;
  float divisor;
  uint64_t seed;
  int stochastic;
  int slice_idx;

  // buckets lb0, lb0+nw, ..., count of them; W = 64/L per wave iteration
  __device__ void run(int64_t lb0, int64_t count, int64_t nw) const {
    constexpr int W = kWave / L;
    const int s = lane / L;   // my segment = which of the W buckets
    const int li = lane % L;  // my 8-elem group within the bucket
    for (int64_t i = 0; i < count; i += W) {
      const bool active = (i + s) < count;
      const int64_t lb = lb0 + (i + s) * nw;
      uint32_t r[8];
      float lmin = INFINITY, lmax = -INFINITY;
      if (active) {
        const T* in = base + lb * (int64_t)(L * 8) + li * 8;
        load_vec<T, 8>(in, true, 8, r);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float f = raw2f<T>(r[j]);
          lmin = fminf(lmin, f);
          lmax = fmaxf(lmax, f);
        }
      }
      seg_minmax<L>(lmin, lmax, lane);
      if (!active) continue;
      const uint32_t unit_raw = f2raw<T>((lmax - lmin) / divisor);
      const float unitf = raw2f<T>(unit_raw);
      const float minf = lmin;
      if (li == 0) {
        meta[2 * lb] = static_cast<R>(unit_raw);
        meta[2 * lb + 1] = static_cast<R>(f2raw<T>(lmin));
      }
      const int64_t g = lb * L + li;  // global group index in the slice
      pack_acc_t<BITS> value = 0;
      if (unitf >= kEps) {
        // encode_pack's loop written out from the same primitives: going
        // through the helper shifts the 16-bit instantiations' register
        // allocation (107 -> 102 VGPR), and this kernel is kept at the
        // allocation it was measured with
        const float rinv = 1.0f / unitf;
        const uint64_t pr = pack_rand(seed, stochastic, slice_idx, g);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float rnd = stochastic ? rand_lane(pr, j) : 0.5f;
          value |= level_bits<BITS, pack_acc_t<BITS>>(
              quant_level<T>(r[j], minf, rinv, rnd, divisor), j);
        }
      }
      store_bytes(packed + g * BITS, static_cast<uint64_t>(value), BITS);
    }
  }
};

// Lean fast-path kernel (see compress.h LaunchKind kFast): only the
// QuantRun register path is instantiated, so the register allocator is not
// forced to the generic/EF paths' footprint (k_quantize<T,BITS,true> runs
// at 4 waves/SIMD; this kernel at 5-8).
template <typename T, int BITS, int MAXGT>
__global__ __launch_bounds__(kThreads) void k_quantize_fast(
    const QuantDesc* __restrict__ descs, const int64_t* __restrict__ cum,
    int nslices, int64_t total_buckets, uint64_t seed, int stochastic) {
  using R = typename RawOf<T>::type;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wid = static_cast<int64_t>(blockIdx.x) * (kThreads / kWave) +
                      (threadIdx.x / kWave);
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (kThreads / kWave);
  constexpr float divisor = static_cast<float>((1 << BITS) - 1);
  int64_t b = wid;
  while (b < total_buckets) {
    const int lo = find_slice(cum, nslices, b);
    const QuantDesc d = descs[lo];
    const int64_t meta_bytes =
        geom_of<T>(d.n, d.bucket, d.flags, BITS).meta_bytes;
    const int64_t nb_full = cum[lo + 1] - cum[lo];
    const int64_t lb = b - cum[lo];
    const int ngroups = d.bucket >> 3;
    const int64_t count = (nb_full - lb + nw - 1) / nw;
#define CGX_QRUNF(GV)                                                      \
  do {                                                                     \
    QuantRun<T, BITS, GV> qr{reinterpret_cast<const T*>(d.in),             \
                             reinterpret_cast<R*>(d.out),                  \
                             d.out + meta_bytes,                           \
                             lane,    ngroups, divisor,                    \
                             seed,    stochastic, lo};                     \
    qr.run(lb, count, nw);                                                 \
  } while (0)
    if constexpr (MAXGT <= 2) {
      // all buckets <= 1024: half the stash registers -> higher occupancy.
      // (A two-bank pipelined run was retried here after the lean-kernel
      // split: VGPR 53 -> 94, quantize 0.072 -> 0.077 ms — the second bank
      // still costs more occupancy than its prefetch hides.  Rejected.)
      if (((ngroups + kWave - 1) >> 6) <= 1) CGX_QRUNF(1);
      else CGX_QRUNF(2);
    } else {
      switch ((ngroups + kWave - 1) >> 6) {
        case 1: CGX_QRUNF(1); break;
        case 2: CGX_QRUNF(2); break;
        case 3: CGX_QRUNF(3); break;
        default: CGX_QRUNF(4); break;
      }
    }
#undef CGX_QRUNF
    b += count * nw;
  }
}

// Dedicated small-bucket kernel: ONLY QuantSub is instantiated (folding it
// into k_quantize_fast measured VGPR 53 -> 107/143, regressing the large
// buckets -- the same register-allocation coupling the lean split fixed).
template <typename T, int BITS>
__global__ __launch_bounds__(kThreads) void k_quantize_sub(
    const QuantDesc* __restrict__ descs, const int64_t* __restrict__ cum,
    int nslices, int64_t total_buckets, uint64_t seed, int stochastic) {
  using R = typename RawOf<T>::type;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wid = static_cast<int64_t>(blockIdx.x) * (kThreads / kWave) +
                      (threadIdx.x / kWave);
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (kThreads / kWave);
  constexpr float divisor = static_cast<float>((1 << BITS) - 1);
  int64_t b = wid;
  while (b < total_buckets) {
    const int lo = find_slice(cum, nslices, b);
    const QuantDesc d = descs[lo];
    const int64_t meta_bytes =
        geom_of<T>(d.n, d.bucket, d.flags, BITS).meta_bytes;
    const int64_t nb_full = cum[lo + 1] - cum[lo];
    const int64_t lb = b - cum[lo];
    const int ngroups = d.bucket >> 3;
    const int64_t count = (nb_full - lb + nw - 1) / nw;
#define CGX_QSUB(LV)                                                       \
  do {                                                                     \
    QuantSub<T, BITS, LV> q{reinterpret_cast<const T*>(d.in),              \
                            reinterpret_cast<R*>(d.out),                   \
                            d.out + meta_bytes,                            \
                            lane, divisor, seed, stochastic, lo};          \
    q.run(lb, count, nw);                                                  \
  } while (0)
    switch (ngroups) {
      case 1: CGX_QSUB(1); break;
      case 2: CGX_QSUB(2); break;
      case 4: CGX_QSUB(4); break;
      case 8: CGX_QSUB(8); break;
      case 16: CGX_QSUB(16); break;
      default: CGX_QSUB(32); break;
    }
#undef CGX_QSUB
    b += count * nw;
  }
}

// First m values of pack g of a bucket as the quantizer sees them: x, plus
// the error-feedback residual when there is one, rounded to T (the rest
// repeat the first).
template <typename T>
__device__ __forceinline__ void load_pack(const T* in, const T* fbp,
                                          bool al16, bool al16_fb, int g,
                                          int m, uint32_t (&r)[8]) {
  load_vec<T, 8>(in + g * 8, al16, m, r);
  if (fbp) {
    uint32_t f[8];
    load_vec<T, 8>(fbp + g * 8, al16_fb, m, f);
#pragma unroll
    for (int j = 0; j < 8; j++)
      r[j] = f2raw<T>(raw2f<T>(r[j]) + raw2f<T>(f[j]));
  }
}

// ---------------------------------------------------------------------------
// Quantize: one wave per bucket.  ENCODE=true requires bucket % 8 == 0 for
// every slice (host guarantees); ENCODE=false computes meta only (the
// arbitrary-bucket path then packs with k_pack_generic).
// ---------------------------------------------------------------------------
template <typename T, int BITS, bool ENCODE>
__global__ __launch_bounds__(kThreads) void k_quantize(
    const QuantDesc* __restrict__ descs, const int64_t* __restrict__ cum,
    int nslices, int64_t total_buckets, uint64_t seed, int stochastic) {
  using R = typename RawOf<T>::type;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wid =
      static_cast<int64_t>(blockIdx.x) * (kThreads / kWave) + (threadIdx.x / kWave);
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (kThreads / kWave);
  constexpr float divisor = static_cast<float>((1 << BITS) - 1);
  constexpr int MAXG = 4;  // register-stashed packs per lane (bucket <= 2048)

  for (int64_t b = wid; b < total_buckets; b += nw) {
    const int lo = find_slice(cum, nslices, b);
    const QuantDesc d = descs[lo];
    const SliceGeom sg = geom_of<T>(d.n, d.bucket, d.flags, BITS);
    const int64_t nq = sg.nq;
    // kFlagTailOnly: the full buckets were handled by the fast/sub kernel;
    // this desc's single cum entry maps to the trailing partial bucket
    const int64_t lb =
        b - cum[lo] + ((d.flags & kFlagTailOnly) ? d.n / d.bucket : 0);
    const int64_t bstart = lb * static_cast<int64_t>(d.bucket);
    const int cur = static_cast<int>(min(static_cast<int64_t>(d.bucket), nq - bstart));
    const T* in = reinterpret_cast<const T*>(d.in) + bstart;
    const bool al16 = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    const int ngroups = (cur + 7) >> 3;

    // fb alignment is independent of the input's (the engine rebases the
    // phase-2 feedback base by a partition offset), so probe it separately
    T* const fbp = d.fb ? reinterpret_cast<T*>(d.fb) + bstart : nullptr;
    const bool al16_fb = (reinterpret_cast<uintptr_t>(fbp) & 15) == 0;
    uint32_t stash[MAXG][8];
    float lmin = INFINITY, lmax = -INFINITY;
    for (int g = lane, gi = 0; g < ngroups; g += kWave, gi++) {
      uint32_t r[8];
      const int m = min(8, cur - g * 8);
      load_pack<T>(in, fbp, al16, al16_fb, g, m, r);
      if (gi < MAXG) {
#pragma unroll
        for (int j = 0; j < 8; j++) stash[gi][j] = r[j];
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {  // r[j >= m] repeats r[0]
        const float f = raw2f<T>(r[j]);
        lmin = fminf(lmin, f);
        lmax = fmaxf(lmax, f);
      }
    }
    seg_minmax<kWave>(lmin, lmax, lane);
    const uint32_t unit_raw = f2raw<T>((lmax - lmin) / divisor);
    const float unitf = raw2f<T>(unit_raw);
    const float minf = lmin;
    R* meta = reinterpret_cast<R*>(d.out);
    if (lane == 0) {
      meta[2 * lb] = static_cast<R>(unit_raw);
      meta[2 * lb + 1] = static_cast<R>(f2raw<T>(lmin));
    }

    if constexpr (ENCODE) {
      uint8_t* packed = d.out + sg.meta_bytes;
      const int64_t gbase = bstart >> 3;
      const bool live = unitf >= kEps;
      const float rinv = 1.0f / unitf;  // hoisted: fp32 div is 1/4 VALU rate
      for (int g = lane, gi = 0; g < ngroups; g += kWave, gi++) {
        uint32_t r[8];
        const int m = min(8, cur - g * 8);
        if (gi < MAXG) {
#pragma unroll
          for (int j = 0; j < 8; j++) r[j] = stash[gi][j];
        } else {
          load_pack<T>(in, fbp, al16, al16_fb, g, m, r);
        }
        uint64_t value = 0;
        uint32_t lv[8] = {};
        if (live) {
          value = encode_pack<T, BITS>(
              r, m, minf, rinv, divisor,
              pack_rand(seed, stochastic, lo, gbase + g), stochastic, lv);
        }
        if (fbp) {
          // residual: (x+fb) - decode(level), rounded to T per the spec
          R* f = reinterpret_cast<R*>(fbp) + g * 8;
          for (int j = 0; j < m; j++) {
            const uint32_t dec =
                decode_raw<T>(unit_raw, f2raw<T>(minf), lv[j]);
            f[j] = static_cast<R>(
                f2raw<T>(raw2f<T>(r[j]) - raw2f<T>(dec)));
          }
        }
        const int64_t gb = (gbase + g) * BITS;
        const int nbytes = static_cast<int>(
            min(static_cast<int64_t>(BITS), sg.packed_bytes - gb));
        store_bytes(packed + gb, value, nbytes);
      }
    }
  }
}

// Generic pack phase for bucket % 8 != 0 (meta already computed): grid-stride
// threads over packs, per-element bucket lookup.
template <typename T, int BITS>
__global__ __launch_bounds__(kThreads) void k_pack_generic(
    const QuantDesc* __restrict__ descs, int nslices, uint64_t seed,
    int stochastic) {
  using R = typename RawOf<T>::type;
  const int64_t t0 =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  constexpr float divisor = static_cast<float>((1 << BITS) - 1);
  for (int s = 0; s < nslices; s++) {
    const QuantDesc d = descs[s];
    const SliceGeom sg = geom_of<T>(d.n, d.bucket, d.flags, BITS);
    const int64_t nq = sg.nq;
    const int64_t ngroups = (nq + 7) >> 3;
    const R* meta = reinterpret_cast<const R*>(d.out);
    uint8_t* packed = d.out + sg.meta_bytes;
    const R* in = reinterpret_cast<const R*>(d.in);
    const bool small = d.n < (int64_t(1) << 31);
    for (int64_t g = t0; g < ngroups; g += stride) {
      const int m = static_cast<int>(min(static_cast<int64_t>(8), nq - g * 8));
      uint64_t value = 0;
      const uint64_t pr = pack_rand(seed, stochastic, s, g);
      for (int j = 0; j < m; j++) {
        const int64_t eidx = g * 8 + j;
        const int64_t bk =
            small ? static_cast<int64_t>(static_cast<uint32_t>(eidx) /
                                         static_cast<uint32_t>(d.bucket))
                  : eidx / d.bucket;
        const float unitf = raw2f<T>(meta[2 * bk]);
        if (unitf < kEps) continue;
        const float minf = raw2f<T>(meta[2 * bk + 1]);
        const float rnd = stochastic ? rand_lane(pr, j) : 0.5f;
        value |= level_bits<BITS, uint64_t>(
            quant_level<T>(in[eidx], minf, 1.0f / unitf, rnd, divisor), j);
      }
      const int64_t gb = g * BITS;
      const int nbytes = static_cast<int>(
          min(static_cast<int64_t>(BITS), sg.packed_bytes - gb));
      store_bytes(packed + gb, value, nbytes);
    }
  }
}

// Load a (unit, min) meta pair with ONE aligned load (pairs are naturally
// 2*sizeof(R)-aligned: the slice base is 8-byte aligned).
template <typename R>
__device__ __forceinline__ void load_meta_pair(const R* meta, int64_t bk,
                                               uint32_t& unit_raw,
                                               uint32_t& min_raw) {
  if constexpr (sizeof(R) == 4) {
    const uint64_t p = *reinterpret_cast<const uint64_t*>(meta + 2 * bk);
    unit_raw = static_cast<uint32_t>(p);
    min_raw = static_cast<uint32_t>(p >> 32);
  } else {
    const uint32_t p = *reinterpret_cast<const uint32_t*>(meta + 2 * bk);
    unit_raw = p & 0xFFFF;
    min_raw = p >> 16;
  }
}

// Branch-free packed loads for the hot BITS values.  The compressed stream
// base is always 8-byte aligned (align8 slice sizes + 2*sizeof(R)*nb meta),
// so the typed loads below are aligned by construction.
// half: 4 elements (fp32 path; h selects the half-pack).
template <int BITS>
__device__ __forceinline__ uint64_t load_pack_half(
    const uint8_t* __restrict__ src, int64_t g, int h) {
  if constexpr (BITS == 1) {
    return static_cast<uint64_t>(src[g]) >> (h * 4);
  } else if constexpr (BITS == 2) {
    return src[g * 2 + h];
  } else if constexpr (BITS == 4) {
    return *reinterpret_cast<const uint16_t*>(src + g * 4 + h * 2);
  } else if constexpr (BITS == 8) {
    return *reinterpret_cast<const uint32_t*>(src + g * 8 + h * 4);
  } else if constexpr ((BITS & 1) == 0) {
    return load_bytes(src + g * BITS + h * (BITS / 2), BITS / 2);
  } else {
    return load_bytes(src + g * BITS, BITS) >> (h * 4 * BITS);
  }
}

// full: 8 elements (16-bit dtype path).
template <int BITS>
__device__ __forceinline__ uint64_t load_pack_full(
    const uint8_t* __restrict__ src, int64_t g) {
  if constexpr (BITS == 1) {
    return src[g];
  } else if constexpr (BITS == 2) {
    return *reinterpret_cast<const uint16_t*>(src + g * 2);
  } else if constexpr (BITS == 4) {
    return *reinterpret_cast<const uint32_t*>(src + g * 4);
  } else if constexpr (BITS == 8) {
    return *reinterpret_cast<const uint64_t*>(src + g * 8);
  } else {
    return load_bytes(src + g * BITS, BITS);
  }
}

// Incremental bucket-index tracker: replaces the per-iteration integer
// division (a ~40-instruction software sequence that dominated the round-1
// hot loop) with one uniform quotient add + carry per iteration.  Valid
// while indexes fit in u32 (`small` slices) and the per-iteration step is
// uniform.
struct BkTrack {
  uint32_t bk, rem, q, r, div;
  __device__ __forceinline__ void init(uint32_t x, uint32_t step,
                                       uint32_t d) {
    div = d;
    bk = x / d;
    rem = x % d;
    q = step / d;
    r = step % d;
  }
  __device__ __forceinline__ void advance() {
    bk += q;
    rem += r;
    if (rem >= div) {
      rem -= div;
      bk += 1;
    }
  }
};

// fp32 fast path: bucket % 8 == 0, u32-indexable slice.  4 elems/lane, two
// independent chains, no division, no per-access branches.  (U=4 in the
// lean kernel: VGPR 56->106 for a wash — the fifth occupancy-vs-ILP
// datapoint on this kernel family, all negative.)
template <int BITS, bool AL16, bool HAVE>
__device__ void deq_f32_fast(const DequantDesc& d,
                             const uint8_t* __restrict__ in0,
                             int64_t meta_bytes, int64_t full_subs,
                             uint32_t B4, int64_t t0, int64_t stride) {
  constexpr int U = 2;
  BkTrack bk[U];
#pragma unroll
  for (int u = 0; u < U; u++)
    bk[u].init(static_cast<uint32_t>(t0 + u * stride),
               static_cast<uint32_t>(U * stride), B4);
  int64_t w = t0;
  for (; w + (U - 1) * stride < full_subs; w += U * stride) {
    uint32_t v[U][4];
    float* outp[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      outp[u] = reinterpret_cast<float*>(d.out) + (w + u * stride) * 4;
      if constexpr (HAVE) load16B<AL16>(outp[u], v[u]);
    }
    for (int sidx = 0; sidx < d.nsrc; sidx++) {
      const uint8_t* __restrict__ src = in0 + sidx * d.src_stride;
      const float* __restrict__ meta =
          reinterpret_cast<const float*>(src - meta_bytes);
      uint64_t value[U];
      uint32_t ur[U], mr[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int64_t ws = w + u * stride;
        value[u] = load_pack_half<BITS>(src, ws >> 1,
                                        static_cast<int>(ws & 1));
        load_meta_pair<uint32_t>(reinterpret_cast<const uint32_t*>(meta),
                                 bk[u].bk, ur[u], mr[u]);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          accum_raw<float>(
              v[u][j], !HAVE && sidx == 0,
              decode_raw<float>(ur[u], mr[u], pack_level<BITS>(value[u], j)));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      store16B<AL16>(outp[u], v[u]);
      bk[u].advance();
    }
  }
  // at most one trailing sub per thread
  for (; w < full_subs; w += stride) {
    uint32_t v[4];
    float* outp = reinterpret_cast<float*>(d.out) + w * 4;
    if constexpr (HAVE) load16B<AL16>(outp, v);
    const uint32_t bkw = static_cast<uint32_t>(w) / B4;
    for (int sidx = 0; sidx < d.nsrc; sidx++) {
      const uint8_t* __restrict__ src = in0 + sidx * d.src_stride;
      const uint32_t* __restrict__ meta =
          reinterpret_cast<const uint32_t*>(src - meta_bytes);
      const uint64_t value =
          load_pack_half<BITS>(src, w >> 1, static_cast<int>(w & 1));
      uint32_t ur, mr;
      load_meta_pair<uint32_t>(meta, bkw, ur, mr);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        accum_raw<float>(
            v[j], !HAVE && sidx == 0,
            decode_raw<float>(ur, mr, pack_level<BITS>(value, j)));
      }
    }
    store16B<AL16>(outp, v);
  }
}

// 16-bit fast path: 8 elems/lane (one int4 store), incremental bucket index.
template <typename T, int BITS, bool AL16, bool HAVE>
__device__ void deq_16_fast(const DequantDesc& d,
                            const uint8_t* __restrict__ in0,
                            int64_t meta_bytes, int64_t full_groups,
                            uint32_t B8, int64_t t0, int64_t stride) {
  using R = typename RawOf<T>::type;
  BkTrack bk;
  bk.init(static_cast<uint32_t>(t0), static_cast<uint32_t>(stride), B8);
  for (int64_t g = t0; g < full_groups; g += stride) {
    uint32_t w4[4];
    T* outp = reinterpret_cast<T*>(d.out) + g * 8;
    uint32_t v[8];
    if constexpr (HAVE) {
      if constexpr (AL16) {
        load16B<true>(outp, w4);
#pragma unroll
        for (int j = 0; j < 8; j++)
          v[j] = (w4[j >> 1] >> ((j & 1) * 16)) & 0xFFFF;
      } else {
        // 2-byte-aligned output: element loads (u32 would be misaligned)
        const R* q = reinterpret_cast<const R*>(outp);
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = q[j];
      }
    }
    for (int sidx = 0; sidx < d.nsrc; sidx++) {
      const uint8_t* __restrict__ src = in0 + sidx * d.src_stride;
      const R* __restrict__ meta = reinterpret_cast<const R*>(src - meta_bytes);
      const uint64_t value = load_pack_full<BITS>(src, g);
      uint32_t ur, mr;
      load_meta_pair<R>(meta, bk.bk, ur, mr);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        accum_raw<T>(v[j], !HAVE && sidx == 0,
                     decode_raw<T>(ur, mr, pack_level<BITS>(value, j)));
      }
    }
    if constexpr (AL16) {
#pragma unroll
      for (int j = 0; j < 4; j++) w4[j] = v[2 * j] | (v[2 * j + 1] << 16);
      store16B<true>(outp, w4);
    } else {
      R* q = reinterpret_cast<R*>(outp);
#pragma unroll
      for (int j = 0; j < 8; j++) q[j] = static_cast<R>(v[j]);
    }
    bk.advance();
  }
}

// Lean dequantize kernel: only the branch-free fast paths (bucket%8==0,
// u32-indexable slices) are instantiated, so the register allocator does
// not have to cover the generic/tail paths; ragged tails re-enter k_dequant
// with kFlagTailOnly.
template <typename T, int BITS>
__global__ __launch_bounds__(kThreads) void k_dequant_fast(
    const DequantDesc* __restrict__ descs, int nslices) {
  using R = typename RawOf<T>::type;
  const int64_t t0 =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int si = 0; si < nslices; si++) {
    const DequantDesc d = descs[si];
    // slice_geom's nq / meta_bytes written out: through the helper the
    // per-slice scalar prologue compiles differently (11 instructions
    // shorter, other SGPR numbering through the whole kernel), and this
    // kernel is kept instruction-identical to the code it was measured with
    const bool skip = (d.flags & kFlagSkipIncomplete) != 0;
    const int64_t nq =
        skip ? (d.n / d.bucket) * static_cast<int64_t>(d.bucket) : d.n;
    const int64_t nb_slice =
        skip ? d.n / d.bucket : (d.n + d.bucket - 1) / d.bucket;
    const int64_t meta_bytes = 2 * sizeof(R) * nb_slice;
    const bool al16 = (reinterpret_cast<uintptr_t>(d.out) & 15) == 0;
    const uint8_t* const in0 = d.in + meta_bytes;
    const bool have = d.add != 0;
    if constexpr (sizeof(T) == 4) {
      const int64_t full_subs = nq >> 2;
      const uint32_t B4 = static_cast<uint32_t>(d.bucket >> 2);
      if (al16) {
        if (have)
          deq_f32_fast<BITS, true, true>(d, in0, meta_bytes, full_subs, B4,
                                         t0, stride);
        else
          deq_f32_fast<BITS, true, false>(d, in0, meta_bytes, full_subs, B4,
                                          t0, stride);
      } else {
        if (have)
          deq_f32_fast<BITS, false, true>(d, in0, meta_bytes, full_subs, B4,
                                          t0, stride);
        else
          deq_f32_fast<BITS, false, false>(d, in0, meta_bytes, full_subs, B4,
                                           t0, stride);
      }
    } else {
      const int64_t full_groups = nq >> 3;
      const uint32_t B8 = static_cast<uint32_t>(d.bucket >> 3);
      if (al16) {
        if (have)
          deq_16_fast<T, BITS, true, true>(d, in0, meta_bytes, full_groups,
                                           B8, t0, stride);
        else
          deq_16_fast<T, BITS, true, false>(d, in0, meta_bytes, full_groups,
                                            B8, t0, stride);
      } else {
        if (have)
          deq_16_fast<T, BITS, false, true>(d, in0, meta_bytes, full_groups,
                                            B8, t0, stride);
        else
          deq_16_fast<T, BITS, false, false>(d, in0, meta_bytes, full_groups,
                                             B8, t0, stride);
      }
    }
  }
}

// Decode the first m elements (all E for a full unit) of unit w of a slice:
// E = 16 / sizeof(T) elements, so a full unit is one 16-byte store and lies
// inside one pack.  The d.nsrc streams are summed in T precision in stream
// order (matching the CPU simulation's per-source sequential accumulate), on
// top of the existing output when d.add.  Any bucket size: the bucket index
// is divided out once per unit and stepped per element.
template <typename T, int BITS>
__device__ __forceinline__ void decode_unit(const DequantDesc& d,
                                            const SliceGeom& sg, bool al16,
                                            int64_t w, int m) {
  using R = typename RawOf<T>::type;
  constexpr int E = 16 / sizeof(T);
  const int64_t e0 = w * E;
  const int64_t gb = (e0 >> 3) * BITS;  // byte offset of the unit's pack
  const int shift = static_cast<int>(e0 & 7) * BITS;
  const int nbytes = static_cast<int>(
      min(static_cast<int64_t>(BITS), sg.packed_bytes - gb));
  const int64_t bk0 = e0 / d.bucket;
  const int rem0 = static_cast<int>(e0 - bk0 * d.bucket);
  const bool have = d.add != 0;
  T* outp = reinterpret_cast<T*>(d.out) + e0;
  uint32_t v[E];
  if (have) load_vec<T, E>(outp, al16, m, v);
  for (int sidx = 0; sidx < d.nsrc; sidx++) {
    const R* meta = reinterpret_cast<const R*>(d.in + sidx * d.src_stride);
    const uint64_t value =
        load_bytes(d.in + sidx * d.src_stride + sg.meta_bytes + gb, nbytes) >>
        shift;
    int64_t bk = bk0;
    int rem = rem0;
    uint32_t ur, mr;
    load_meta_pair<R>(meta, bk, ur, mr);
#pragma unroll
    for (int j = 0; j < E; j++) {
      if (j >= m) break;
      if (j > 0 && ++rem == d.bucket) {  // crossed into the next bucket
        rem = 0;
        load_meta_pair<R>(meta, ++bk, ur, mr);
      }
      accum_raw<T>(v[j], !have && sidx == 0,
                   decode_raw<T>(ur, mr, pack_level<BITS>(value, j)));
    }
  }
  store_vec<T, E>(outp, al16, m, v);
}

// Generic dequantize (+ multi-source accumulate): grid-stride threads over
// full units, then thread 0 decodes the ragged remainder.  kFlagTailOnly:
// k_dequant_fast already decoded the full units.
template <typename T, int BITS>
__global__ __launch_bounds__(kThreads) void k_dequant(
    const DequantDesc* __restrict__ descs, int nslices) {
  constexpr int E = 16 / sizeof(T);
  const int64_t t0 =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int si = 0; si < nslices; si++) {
    const DequantDesc d = descs[si];
    const SliceGeom sg = geom_of<T>(d.n, d.bucket, d.flags, BITS);
    const bool al16 = (reinterpret_cast<uintptr_t>(d.out) & 15) == 0;
    const int64_t full_units = sg.nq / E;
    if (!(d.flags & kFlagTailOnly)) {
      for (int64_t w = t0; w < full_units; w += stride)
        decode_unit<T, BITS>(d, sg, al16, w, E);
    }
    const int mtail = static_cast<int>(sg.nq - full_units * E);
    if (mtail > 0 && t0 == 0)
      decode_unit<T, BITS>(d, sg, al16, full_units, mtail);
  }
}

// skip_incomplete residual handling: the trailing partial bucket travels as
// raw T values after the aligned packed region (reference
// MaxMinQuantizer::Compress/DecompressBuffer, compressor.cc:332-341,384-400).
template <typename T>
__global__ __launch_bounds__(kThreads) void k_residual_q(
    const QuantDesc* __restrict__ descs, int nslices, int bits) {
  using R = typename RawOf<T>::type;
  const int64_t t0 =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int s = 0; s < nslices; s++) {
    const QuantDesc d = descs[s];
    if (!(d.flags & kFlagSkipIncomplete)) continue;
    const SliceGeom sg = geom_of<T>(d.n, d.bucket, d.flags, bits);
    const int64_t nq = sg.nq;
    const int64_t r = sg.resid;
    if (r == 0) continue;
    const R* src = reinterpret_cast<const R*>(d.in) + nq;
    R* dst = reinterpret_cast<R*>(d.out + sg.resid_off);
    if (d.fb) {
      // error feedback: the raw residual tail carries x+fb exactly, so the
      // new residual is zero
      R* f = reinterpret_cast<R*>(d.fb) + nq;
      for (int64_t i = t0; i < r; i += stride) {
        dst[i] = static_cast<R>(
            f2raw<T>(raw2f<T>(src[i]) + raw2f<T>(f[i])));
        f[i] = 0;
      }
    } else {
      for (int64_t i = t0; i < r; i += stride) dst[i] = src[i];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_residual_d(
    const DequantDesc* __restrict__ descs, int nslices, int bits) {
  using R = typename RawOf<T>::type;
  const int64_t t0 =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int s = 0; s < nslices; s++) {
    const DequantDesc d = descs[s];
    if (!(d.flags & kFlagSkipIncomplete)) continue;
    const SliceGeom sg = geom_of<T>(d.n, d.bucket, d.flags, bits);
    const int64_t r = sg.resid;
    if (r == 0) continue;
    R* outp = reinterpret_cast<R*>(d.out) + sg.nq;
    for (int64_t i = t0; i < r; i += stride) {
      uint32_t v = 0;
      if (d.add) v = outp[i];
      for (int src = 0; src < d.nsrc; src++) {
        const R* rp = reinterpret_cast<const R*>(d.in + src * d.src_stride +
                                                 sg.resid_off);
        accum_raw<T>(v, !d.add && src == 0, rp[i]);
      }
      outp[i] = static_cast<R>(v);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_add(const T* __restrict__ x,
                                                  T* __restrict__ y,
                                                  int64_t n) {
  const int64_t t0 =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  using R = typename RawOf<T>::type;
  const R* xr = reinterpret_cast<const R*>(x);
  R* yr = reinterpret_cast<R*>(y);
  for (int64_t i = t0; i < n; i += stride) {
    yr[i] = static_cast<R>(f2raw<T>(raw2f<T>(xr[i]) + raw2f<T>(yr[i])));
  }
}

inline int max_blocks() {
  // CGX_MAX_BLOCKS: experimentation knob for grid-size sweeps (default
  // kMaxBlocks = 4096, i.e. 2 resident workgroup generations on 256 CUs)
  const int x = env_max_blocks();
  return x > 0 ? x : kMaxBlocks;
}

inline int grid_for(int64_t work, int per_block) {
  const int64_t blocks = (work + per_block - 1) / per_block;
  const int64_t cap = max_blocks();
  return static_cast<int>(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

#define CGX_DISPATCH_BITS(BITS_VAL, ...)                        \
  switch (BITS_VAL) {                                           \
    case 1: { constexpr int BITS = 1; __VA_ARGS__; break; }     \
    case 2: { constexpr int BITS = 2; __VA_ARGS__; break; }     \
    case 3: { constexpr int BITS = 3; __VA_ARGS__; break; }     \
    case 4: { constexpr int BITS = 4; __VA_ARGS__; break; }     \
    case 5: { constexpr int BITS = 5; __VA_ARGS__; break; }     \
    case 6: { constexpr int BITS = 6; __VA_ARGS__; break; }     \
    case 7: { constexpr int BITS = 7; __VA_ARGS__; break; }     \
    case 8: { constexpr int BITS = 8; __VA_ARGS__; break; }     \
    default:                                                    \
      printf("cgx: invalid bits %d\n", BITS_VAL);               \
      abort();                                                  \
  }

#define CGX_DISPATCH_T(DT, ...)                                       \
  switch (DT) {                                                       \
    case DType::F32: { using T = float; __VA_ARGS__; break; }         \
    case DType::F16: { using T = __half; __VA_ARGS__; break; }        \
    case DType::BF16: { using T = __hip_bfloat16; __VA_ARGS__; break; } \
  }

}  // namespace

void launch(const QuantGroup& g, const QuantDesc* descs, const int64_t* cum,
            DType dt, uint64_t seed, bool stochastic, hipStream_t stream) {
  const int nslices = static_cast<int>(g.descs.size());
  if (nslices <= 0) return;
  const int64_t total_buckets = g.cum.back();
  const dim3 grid(grid_for(std::max<int64_t>(total_buckets, 1),
                           kThreads / kWave));
  const dim3 block(kThreads);
  const int stoch = stochastic;
#define CGX_QUANT(...)                                                   \
  hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, stream, descs, cum,  \
                     nslices, total_buckets, seed, stoch)
  CGX_DISPATCH_T(dt, CGX_DISPATCH_BITS(g.bits, {
    if (total_buckets > 0) {
      switch (g.kind) {
        case kFast:
          if (g.max_gpl <= 2) CGX_QUANT(k_quantize_fast<T, BITS, 2>);
          else CGX_QUANT(k_quantize_fast<T, BITS, 4>);
          break;
        case kSub: CGX_QUANT(k_quantize_sub<T, BITS>); break;
        case kGeneric: CGX_QUANT(k_quantize<T, BITS, true>); break;
        default:  // kTwoPass: meta pass, then the arbitrary-bucket pack pass
          CGX_QUANT(k_quantize<T, BITS, false>);
          hipLaunchKernelGGL((k_pack_generic<T, BITS>), grid, block, 0,
                             stream, descs, nslices, seed, stoch);
      }
    }
    if (g.any_residual) {
      hipLaunchKernelGGL((k_residual_q<T>), dim3(32), block, 0, stream, descs,
                         nslices, g.bits);
    }
  }));
#undef CGX_QUANT
}

void launch(const DequantGroup& g, const DequantDesc* descs, DType dt,
            hipStream_t stream) {
  const int nslices = static_cast<int>(g.descs.size());
  if (nslices <= 0) return;
  const dim3 grid(grid_for(std::max<int64_t>(g.total_groups, 1), kThreads));
  const dim3 block(kThreads);
  CGX_DISPATCH_T(dt, CGX_DISPATCH_BITS(g.bits, {
    if (g.total_groups > 0) {
      if (g.kind == kFast) {
        hipLaunchKernelGGL((k_dequant_fast<T, BITS>), grid, block, 0, stream,
                           descs, nslices);
      } else {
        hipLaunchKernelGGL((k_dequant<T, BITS>), grid, block, 0, stream,
                           descs, nslices);
      }
    }
    if (g.any_residual) {
      hipLaunchKernelGGL((k_residual_d<T>), dim3(32), block, 0, stream, descs,
                         nslices, g.bits);
    }
  }));
}

void launch_add(const void* x, void* y, int64_t n, DType dt,
                hipStream_t stream) {
  if (n <= 0) return;
  const int grid = grid_for(n, kThreads);
  CGX_DISPATCH_T(dt, {
    hipLaunchKernelGGL((k_add<T>), dim3(grid), dim3(kThreads), 0, stream,
                       reinterpret_cast<const T*>(x), reinterpret_cast<T*>(y),
                       n);
  });
}

}  // namespace cgx
