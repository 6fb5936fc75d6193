// Compression engine: the streams, events and staging that execute the
// compressed Scatter-Reduce-AllGather / Ring allreduce over RCCL/xGMI.  What
// is reduced where is decided by pure host code: the layer registry
// (registry.h), the env config (config.h) and chunk planning (plan.h).
//
// This is the MI355X-native equivalent of the reference's
// mpi_allreduce_operations + compressor + reducer stack
// (/root/reference/src/mpi_allreduce_operations.cc,
//  src/common/scatter_reduce_allgather.cc, src/common/compressor.cc):
// one RCCL communicator bootstrapped from the c10d Store replaces the
// MPI/SHM/NCCL communicator trio; grouped ncclSend/ncclRecv drive all 7 xGMI
// links concurrently; batched descriptor-driven kernels replace per-layer
// kernel launches.
#pragma once

#include <ATen/ATen.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "check.h"
#include "compress.h"
#include "config.h"
#include "phase_timer.h"
#include "plan.h"
#include "registry.h"
#include "transport.h"

namespace cgx {

// Pinned-host + device descriptor upload arena with an event-guarded ring so
// batches can be queued back-to-back without host/device races.
class DescRing {
 public:
  ~DescRing();
  // Acquire a slot of >= bytes; returns host pointer to fill.
  void* acquire(size_t bytes);
  // Async-copy the filled slot to device, record the guard event on stream,
  // advance the ring; returns the DEVICE pointer for kernel args.
  void* commit(size_t bytes, hipStream_t stream);

 private:
  static constexpr int kSlots = 16;
  struct Slot {
    void* host = nullptr;
    void* dev = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool ev_recorded = false;
  };
  Slot slots_[kSlots];
  int cur_ = 0;
};

class Engine {
 public:
  // is_cross: this engine drives the cross-node stage of the hierarchical
  // path and selects its reduction algorithm from CGX_CROSS_REDUCTION_TYPE
  // (default Ring) instead of CGX_INNER_REDUCTION_TYPE (default SRA).
  Engine(int rank, int size, bool is_cross = false);
  ~Engine();

  // SUM-allreduce of a flat fp32/fp16/bf16 CUDA tensor: registered (or
  // default-config) layers are quantized and reduced via SRA over RCCL;
  // non-compressible layers go through fused ncclAllReduce.
  //
  // Three-stream pipeline: quantize runs on the caller's side stream `qs`,
  // p2p/collective traffic on comm_stream_, decode(+re-quantize) on
  // deq_stream_, chained by events.  Because `qs` never waits on the other
  // two, the NEXT bucket's quantize overlaps this bucket's xGMI traffic
  // (the reference serialized everything on one side stream).  Returns the
  // stream carrying the final operation (record the Work end event there).
  // `forced`: pre-resolved layer info (hierarchical mode resolves the
  // registry ONCE per bucket and passes it to both the intra and cross
  // engines -- each engine consuming a registry cursor step would
  // desynchronize leader vs non-leader ranks when bucket totals repeat).
  hipStream_t allreduce(at::Tensor bucket, Transport* tr, hipStream_t qs,
                        const Registry::BucketInfo* forced = nullptr,
                        bool forced_match = false);

  hipStream_t comm_stream() const { return comm_stream_; }
  hipStream_t deq_stream() const { return deq_stream_; }

  // Compressed broadcast (reference Reducer::Broadcast parity,
  // reducer.cc:96-160): root quantizes with the default env config, the
  // compressed bytes travel once over the wire, everyone decodes.  Falls
  // back to plain ncclBroadcast when compression is off.  Used by the
  // hierarchical intra-node broadcast when CGX_INTRA_COMPRESS=1 (default,
  // matching the reference, mpi_allreduce_operations.cc:134).
  hipStream_t broadcast(at::Tensor t, int root, Transport* tr,
                        hipStream_t qs);

 private:
  // Double-buffered staging so chunk c+1's quantize (on qs) can start while
  // chunk c's traffic/decode (on comm/deq streams) still reads its slot.
  struct StagingSlot {
    at::Tensor buf;
    hipEvent_t done_ev = nullptr;  // recorded on deq stream at chunk end
    bool recorded = false;
  };

  // fb_key: stable identity of this (bucket, chunk) for the error-feedback
  // residual store — (bucket_idx << 20 | chunk ordinal) when the registry
  // matched, else a pointer-derived fallback key.
  void sra_chunk(const std::vector<LayerView>& views, DType dt,
                 Transport* tr, hipStream_t qs, const EngineConfig& cfg,
                 int64_t fb_key);
  void ring_chunk(const std::vector<LayerView>& views, DType dt,
                  Transport* tr, hipStream_t stream,
                  const EngineConfig& cfg);
  // Brute-force debug reduction (CGX_DEBUG_ALL_TO_ALL_REDUCTION parity,
  // reference scatter_reduce_allgather.cc:269-306): every rank quantizes its
  // ENTIRE chunk once, sends it to all peers, and every rank decodes the
  // same ws compressed streams — no partitioning, ws× the wire traffic, but
  // removes the partition/offset machinery from the fault surface.  Ranks
  // accumulate in different orders (self first), so at ws>2 results agree
  // to fp rounding, not bitwise.
  void a2a_chunk(const std::vector<LayerView>& views, DType dt,
                 Transport* tr, hipStream_t qs, const EngineConfig& cfg);
  uint8_t* staging(int64_t bytes, hipStream_t user);     // single-stream path
  uint8_t* slot_bytes(StagingSlot& slot, int64_t bytes); // pipelined path
  void chain(hipStream_t from, hipStream_t to);  // event: `to` waits `from`
  hipEvent_t next_ev();

  // Launch one quantize "job list": the router (compress.h) sorts the slices
  // into launch groups, each consuming one seed.
  // fb_base (optional): error-feedback buffer indexed by slice fb_off minus
  // fb_rebase elements (phase 2 buffers cover only this rank's partition, so
  // its slices rebase by the partition start — computed host-side per slice,
  // never by out-of-bounds pointer arithmetic).
  void run_quantize(const std::vector<Slice>& slices, uint8_t* out_base,
                    DType dt, hipStream_t stream, bool stochastic,
                    char* fb_base = nullptr, int64_t fb_rebase = 0);
  // Persistent error-feedback residuals keyed by (chunk identity, phase).
  // Bounded: on cap overflow the store resets (residuals are a convergence
  // aid, losing them once is benign; unbounded growth is not).
  at::Tensor& feedback_buf(int64_t key, int phase, int64_t numel,
                           at::ScalarType st);
  std::map<std::pair<int64_t, int>, at::Tensor> fb_bufs_;
  void run_dequant(const std::vector<Slice>& slices, const uint8_t* in_base,
                   int64_t src_stride, int nsrc, bool add, DType dt,
                   hipStream_t stream);

  int rank_, size_;
  bool is_cross_ = false;
  PhaseTimer timer_;  // CGX_TIMINGS=1: per-phase timing of SRA chunks
  at::Tensor staging_;
  StagingSlot slots_[2];
  int slot_cur_ = 0;
  hipStream_t comm_stream_ = nullptr;
  hipStream_t deq_stream_ = nullptr;
  static constexpr int kEvents = 16;
  hipEvent_t evs_[kEvents] = {};
  int ev_cur_ = 0;
  DescRing ring_;
  uint64_t seed_;
};

// fp32/fp16/bf16: the dtypes the kernels compress (dtype_of throws on others)
bool is_compressible(at::ScalarType st);
DType dtype_of(at::ScalarType st);
DType dtype_of(const at::Tensor& t);
at::ScalarType scalar_type_of(DType dt);
ncclDataType_t nccl_dtype(const at::Tensor& t);

}  // namespace cgx
