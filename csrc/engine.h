// Compression engine: layer registry, fusion chunking, rank partitioning and
// the compressed Scatter-Reduce-AllGather allreduce over RCCL/xGMI.
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

#include "transport.h"

#include <cstdint>
#include <map>
#include <mutex>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "compress.h"

namespace cgx {

#define CGX_HIP_CHECK(cmd)                                              \
  do {                                                                  \
    hipError_t e_ = (cmd);                                              \
    TORCH_CHECK(e_ == hipSuccess, "cgx HIP error: ", hipGetErrorString(e_)); \
  } while (0)

#define CGX_NCCL_CHECK(cmd)                                              \
  do {                                                                   \
    ncclResult_t r_ = (cmd);                                             \
    TORCH_CHECK(r_ == ncclSuccess, "cgx RCCL error: ", ncclGetErrorString(r_)); \
  } while (0)

struct LayerConfig {
  int bits = 32;
  int bucket_size = 512;
};

// Process-global layer registry (parity with the reference's static
// MPIAllReduce_Operation::RegisterLayer / Compressor config registry,
// mpi_allreduce_operations.h:37-49, compressor.h:93-107).
class Registry {
 public:
  struct BucketInfo {
    int idx = -1;
    std::vector<int64_t> numels;
    std::vector<LayerConfig> cfgs;
    int64_t total = 0;
  };

  static Registry& get();

  void register_layer(int bucket_idx, int layer_idx, int64_t numel, int bits,
                      int bucket_size);
  void set_bits(int bucket_idx, int layer_idx, int bits);
  void set_bucket_size(int bucket_idx, int layer_idx, int bucket_size);
  void clear();
  bool empty();

  // Match the next allreduce call (of `numel` total elements) to a
  // registered bucket, cycling through registration order (the reference's
  // modulo-cursor, extractLayers, mpi_allreduce_operations.cc:257-285 —
  // hardened twice over: a bucket only matches if its total numel agrees,
  // and once a flat-bucket storage pointer `key` has matched a bucket, the
  // pointer is bound to it so later calls resolve by identity even when two
  // buckets share a total but differ in layer layout (DDP reuses its flat
  // gradient buffers, so the pointer is stable until a bucket rebuild — at
  // which point the total check unbinds it and the cursor re-learns).
  // Returns a copy (thread safety) or nullopt-like empty BucketInfo.
  bool next(int64_t numel, const void* key, BucketInfo* out);
  std::vector<BucketInfo> snapshot();

 private:
  std::mutex mu_;
  std::vector<BucketInfo> order_;
  std::unordered_map<int, size_t> by_idx_;
  std::unordered_map<const void*, size_t> bound_;
  size_t cursor_ = 0;
};

// A contiguous compressible piece of the flat bucket tensor.
struct LayerView {
  char* data;
  int64_t numel;
  int bits;
  int bucket_size;
};

struct EngineConfig {
  int64_t fusion_bytes = 64ll << 20;
  int64_t min_elems = 16;
  int default_bits = 32;
  int default_bucket = 512;
  bool stochastic = true;
  bool ring = false;        // CGX_INNER_REDUCTION_TYPE=Ring (default SRA)
  bool cross_ring = true;   // CGX_CROSS_REDUCTION_TYPE (default Ring, like
                            // the reference's cross-node default,
                            // mpi_allreduce_operations.cc:96-115)
  bool debug_a2a = false;   // CGX_DEBUG_ALL_TO_ALL_REDUCTION: brute-force
                            // all-to-all fallback for fault isolation
  double fake_ratio = 1.0;  // CGX_COMPRESSION_FAKE_RATIO (bandwidth expt)
  bool skip_incomplete = false;  // CGX_COMPRESSION_SKIP_INCOMPLETE_BUCKETS
  bool dummy = false;  // CGX_DEBUG_DUMMY_COMPRESSION: force uncompressed
  bool intra_compress = true;  // CGX_INTRA_COMPRESS
  bool error_feedback = false;  // CGX_ERROR_FEEDBACK (needs bucket%8==0)
  static EngineConfig from_env();  // re-read every bucket like the reference
};

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

  // Mirror of the partition walk (reference Quantizer::GetSizesAndOffsets,
  // compressor.cc:265-299); exposed for tests via bindings.
  static void partition(int64_t num_elements, int world_size,
                        const std::vector<int64_t>& layer_numels, int esize,
                        std::vector<int64_t>* offsets,
                        std::vector<int64_t>* sizes);

 private:
  struct Slice {  // one layer piece inside one rank chunk
    char* data;
    int64_t n;
    int bits;
    int bucket;
    int64_t comp_off;  // byte offset of this slice in the chunk's comp stream
    bool skip_incomplete = false;
    int64_t fb_off = 0;  // element offset in the chunk's error-feedback buf
  };

  // Double-buffered staging so chunk c+1's quantize (on qs) can start while
  // chunk c's traffic/decode (on comm/deq streams) still reads its slot.
  struct StagingSlot {
    at::Tensor buf;
    hipEvent_t done_ev = nullptr;  // recorded on deq stream at chunk end
    bool recorded = false;
  };

  struct ChunkPlan {
    std::vector<std::vector<Slice>> rs;  // per-rank slice lists
    std::vector<int64_t> comp;           // per-rank compressed bytes
    std::vector<int64_t> offs, szs;
    int64_t n = 0;
  };
  ChunkPlan plan(const std::vector<LayerView>& views, DType dt,
                 bool skip_incomplete);

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

  // CGX_TIMINGS=1: per-phase GPU timing of each SRA chunk (quantize /
  // round-1 comm / decode+requantize / round-2 comm / final decode),
  // aggregated and printed every 50 chunks (the reference had no
  // timers at all).
  struct PhaseTimer {
    static constexpr int kRing = 4;
    static constexpr int kEv = 6;
    hipEvent_t ev[kRing][kEv] = {};
    bool pending[kRing] = {};
    int cur = 0;
    double sum_ms[kEv - 1] = {};
    int64_t count = 0;
    bool inited = false;
  };
  PhaseTimer timer_;
  void timer_begin(hipStream_t qs, bool enabled);
  void timer_mark(int idx, hipStream_t stream);  // idx 1..5
  void timer_finish();
  void timer_drain();  // destructor: flush in-flight slots + final print
  void timer_collect(int slot);  // fold one finished slot into the sums
  void timer_print(const char* suffix) const;  // the five-phase line
  bool timing_ = false;
  int timer_slot_ = -1;

  int rank_, size_;
  bool is_cross_ = false;
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

DType dtype_of(at::ScalarType st);
DType dtype_of(const at::Tensor& t);
at::ScalarType scalar_type_of(DType dt);
ncclDataType_t nccl_dtype(const at::Tensor& t);

}  // namespace cgx
