// Host-side API of the CDNA4 max-min quantization kernels.
//
// Wire format (see torch_cgx_amd/ops/golden.py, the single source of truth;
// parity with reference cuda_compression_operations.cu:68-96,219-285):
// per slice: [2*num_buckets values of T, interleaved (unit, min)]
//            [ceil(n*bits/8) packed bytes, groups of 8 values little-endian]
// total size align8-padded (buffer_size()).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace cgx {

enum class DType : int { F32 = 0, F16 = 1, BF16 = 2 };

inline int elem_size(DType d) { return d == DType::F32 ? 4 : 2; }

__host__ __device__ inline int64_t align8(int64_t x) {
  return (x + 7) / 8 * 8;
}

// Wire layout of one n-element slice; the one place it is computed, for
// buffer_size(), the router and every kernel.
// skip_incomplete: the trailing partial bucket is stored as raw T values
// after the aligned packed region instead of being quantized.
struct SliceGeom {
  int64_t nq;            // quantized elements (== n unless skip_incomplete)
  int64_t nb;            // buckets with a (unit, min) pair
  int64_t meta_bytes;    // 2 * nb * esize; the packed region starts here
  int64_t packed_bytes;  // ceil(nq * bits / 8): bytes the packs occupy
  int64_t resid_off;     // byte offset of the raw residual tail
  int64_t resid;         // raw residual elements (n - nq)
};

__host__ __device__ inline SliceGeom slice_geom(int64_t n, int bucket,
                                                int bits, int esize,
                                                bool skip_incomplete) {
  SliceGeom g;
  g.nq = skip_incomplete ? (n / bucket) * static_cast<int64_t>(bucket) : n;
  g.nb = skip_incomplete ? n / bucket : (n + bucket - 1) / bucket;
  g.meta_bytes = 2 * static_cast<int64_t>(esize) * g.nb;
  g.packed_bytes = (g.nq * bits + 7) / 8;
  g.resid_off = g.meta_bytes + align8(g.packed_bytes);
  g.resid = n - g.nq;
  return g;
}

// Compressed byte size of an n-element slice (golden.buffer_size parity).
inline int64_t buffer_size(int64_t n, DType dt, int bits, int bucket_size,
                           bool skip_incomplete = false) {
  if (n == 0) return 0;
  const SliceGeom g =
      slice_geom(n, bucket_size, bits, elem_size(dt), skip_incomplete);
  return g.resid_off + g.resid * elem_size(dt);
}

constexpr int32_t kFlagSkipIncomplete = 1;
// The slice's full buckets (quantize) or full 4/8-element units (dequant)
// were already handled by the lean fast kernel; this generic-kernel desc
// covers only the trailing partial bucket / ragged tail.
constexpr int32_t kFlagTailOnly = 2;

// One quantize work item: compress `n` elems at `in` into `out` bytes.
// fb (optional): error-feedback residual of the same length/dtype as `in`;
// the encoded value is in[i]+fb[i] (rounded to T) and fb is updated in place
// to the new residual.  Wire format is unchanged.  (The reference carried
// this plumbing but never enabled it, cuda_compression_operations.cu:713.)
struct QuantDesc {
  const void* in;
  uint8_t* out;
  void* fb;
  int64_t n;
  int32_t bucket;
  int32_t flags;  // kFlagSkipIncomplete | kFlagTailOnly
};

// One dequantize work item: decode `n` elems from `nsrc` compressed streams
// (at in + s*src_stride for s < nsrc), summing them in T precision in stream
// order, then write into `out` (add=1: accumulate into existing values).
struct DequantDesc {
  const uint8_t* in;
  void* out;
  int64_t n;
  int64_t src_stride;
  int32_t bucket;
  int32_t nsrc;
  int32_t add;
  int32_t flags;  // kFlagSkipIncomplete | kFlagTailOnly
};

// ---------------------------------------------------------------------------
// Router: the one place that decides which kernel serves which slice.
//
// The kernel family is split into register-isolated launches (see
// quant_kernels.hip); route_quantize/route_dequantize sort a list of slices
// into launch groups, in ascending (bits, kind) order, slices in input order
// inside a group.  Pure host code: no HIP calls.  The caller copies
// descs (and, for quantize, cum) to the device and hands them to launch().
// ---------------------------------------------------------------------------
enum LaunchKind : int {
  // quantize: bucket % 8 == 0, bucket <= 2048 (the register stash), 16B
  //   aligned input, no error feedback, n >= bucket.  cum counts FULL
  //   buckets; a partial last bucket re-enters kGeneric with kFlagTailOnly
  //   (unless skip_incomplete, where it travels raw).
  // dequant: bucket % 8 == 0 and nq < 2^31 (u32 indexing; per-thread
  //   indices are 4/8-element units).  A ragged tail (nq % 4 for fp32,
  //   nq % 8 for 16-bit) re-enters kGeneric with kFlagTailOnly.
  kFast = 0,
  // everything else with bucket % 8 == 0: error feedback, unaligned input,
  // n < bucket, bucket > 2048, tails.  cum counts ceil-buckets (1 per tail).
  kGeneric = 1,
  // quantize only, bucket % 8 != 0: meta pass + generic pack pass.
  kTwoPass = 2,
  // quantize only: kFast's preconditions and bucket/8 a power of two < 64;
  // the wave packs 64/(bucket/8) buckets per iteration.
  kSub = 3,
};

struct QuantSlice {
  const void* in;
  uint8_t* out;
  void* fb;  // error-feedback residual for this slice, or nullptr
  int64_t n;
  int bits;
  int bucket;
  bool skip_incomplete;
};

struct DequantSlice {
  const uint8_t* in;
  void* out;
  int64_t n;
  int bits;
  int bucket;
  bool skip_incomplete;
};

struct QuantGroup {
  int bits;
  int kind;
  std::vector<QuantDesc> descs;
  // exclusive prefix over per-desc bucket counts, trailing total
  std::vector<int64_t> cum;
  // a slice carries kFlagSkipIncomplete with a non-empty raw residual tail
  // (adds one small copy pass)
  bool any_residual = false;
  // kFast: max over slices of ceil((bucket/8)/64); <= 2 selects the
  // half-stash kernel variant (higher occupancy for buckets <= 1024)
  int max_gpl = 1;
};

struct DequantGroup {
  int bits;
  int kind;
  std::vector<DequantDesc> descs;
  int64_t total_groups = 0;  // 8-element groups of work: sizes the grid
  bool any_residual = false;
};

// Slices with n <= 0 are dropped.
std::vector<QuantGroup> route_quantize(const std::vector<QuantSlice>& slices);
std::vector<DequantGroup> route_dequantize(
    const std::vector<DequantSlice>& slices, DType dt, int64_t src_stride,
    int nsrc, bool add);

// Launch one group; `descs`/`cum` are the DEVICE copies of g.descs/g.cum.
// The stochastic hash key is (index in group << 44) | pack index.
void launch(const QuantGroup& g, const QuantDesc* descs, const int64_t* cum,
            DType dt, uint64_t seed, bool stochastic, hipStream_t stream);
void launch(const DequantGroup& g, const DequantDesc* descs, DType dt,
            hipStream_t stream);

// y[i] += x[i] elementwise (T precision), n elements.
void launch_add(const void* x, void* y, int64_t n, DType dt,
                hipStream_t stream);

}  // namespace cgx
