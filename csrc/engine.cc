// Implementation of the compression engine (see engine.h).
#include "engine.h"

#include <ATen/hip/impl/HIPCachingAllocatorMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/util/Exception.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <optional>

namespace cgx {

// ---------------------------------------------------------------------------
// DescRing
// ---------------------------------------------------------------------------
DescRing::~DescRing() {
  for (auto& s : slots_) {
    if (s.host) (void)hipHostFree(s.host);
    if (s.dev) (void)hipFree(s.dev);
    if (s.ev) (void)hipEventDestroy(s.ev);
  }
}

void* DescRing::acquire(size_t bytes) {
  Slot& s = slots_[cur_];
  if (!s.ev) CGX_HIP_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  if (s.ev_recorded) CGX_HIP_CHECK(hipEventSynchronize(s.ev));
  if (s.cap < bytes) {
    if (s.host) CGX_HIP_CHECK(hipHostFree(s.host));
    if (s.dev) CGX_HIP_CHECK(hipFree(s.dev));
    size_t cap = 4096;
    while (cap < bytes) cap *= 2;
    CGX_HIP_CHECK(hipHostMalloc(&s.host, cap));
    CGX_HIP_CHECK(hipMalloc(&s.dev, cap));
    s.cap = cap;
  }
  return s.host;
}

void* DescRing::commit(size_t bytes, hipStream_t stream) {
  Slot& s = slots_[cur_];
  CGX_HIP_CHECK(
      hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, stream));
  CGX_HIP_CHECK(hipEventRecord(s.ev, stream));
  s.ev_recorded = true;
  void* dev = s.dev;
  cur_ = (cur_ + 1) % kSlots;
  return dev;
}

// ---------------------------------------------------------------------------
// dtype maps
// ---------------------------------------------------------------------------
// the one list of dtypes the kernels compress
static std::optional<DType> compressed_dtype(at::ScalarType st) {
  switch (st) {
    case at::kFloat: return DType::F32;
    case at::kHalf: return DType::F16;
    case at::kBFloat16: return DType::BF16;
    default: return std::nullopt;
  }
}

bool is_compressible(at::ScalarType st) {
  return compressed_dtype(st).has_value();
}

DType dtype_of(at::ScalarType st) {
  const auto dt = compressed_dtype(st);
  TORCH_CHECK(dt, "cgx: unsupported compression dtype ", st);
  return *dt;
}

DType dtype_of(const at::Tensor& t) { return dtype_of(t.scalar_type()); }

at::ScalarType scalar_type_of(DType dt) {
  switch (dt) {
    case DType::F32: return at::kFloat;
    case DType::F16: return at::kHalf;
    case DType::BF16: return at::kBFloat16;
  }
  TORCH_CHECK(false, "cgx: invalid DType ", (int)dt);
}

ncclDataType_t nccl_dtype(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return ncclFloat32;
    case at::kDouble: return ncclFloat64;
    case at::kHalf: return ncclFloat16;
    case at::kBFloat16: return ncclBfloat16;
    case at::kInt: return ncclInt32;
    case at::kLong: return ncclInt64;
    case at::kChar: return ncclInt8;
    case at::kByte: return ncclUint8;
    case at::kBool: return ncclUint8;
    default:
      TORCH_CHECK(false, "cgx: unsupported dtype for RCCL ", t.scalar_type());
  }
}

// ---------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------
Engine::Engine(int rank, int size, bool is_cross)
    : rank_(rank), size_(size), is_cross_(is_cross), timer_(rank) {
  seed_ = 0x9E3779B97F4A7C15ull ^ (0xD1B54A32D192ED03ull * (uint64_t)(rank + 1));
  // constructed under the backend's device guard (lazyInit)
  int least = 0, greatest = 0;
  CGX_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  CGX_HIP_CHECK(hipStreamCreateWithPriority(&comm_stream_,
                                            hipStreamNonBlocking, greatest));
  CGX_HIP_CHECK(hipStreamCreateWithPriority(&deq_stream_,
                                            hipStreamNonBlocking, greatest));
  for (auto& e : evs_)
    CGX_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& s : slots_)
    CGX_HIP_CHECK(hipEventCreateWithFlags(&s.done_ev, hipEventDisableTiming));
}

Engine::~Engine() {
  timer_.drain();
  for (auto& s : slots_)
    if (s.done_ev) (void)hipEventDestroy(s.done_ev);
  for (auto& e : evs_)
    if (e) (void)hipEventDestroy(e);
  if (comm_stream_) (void)hipStreamDestroy(comm_stream_);
  if (deq_stream_) (void)hipStreamDestroy(deq_stream_);
}

hipEvent_t Engine::next_ev() {
  hipEvent_t e = evs_[ev_cur_];
  ev_cur_ = (ev_cur_ + 1) % kEvents;
  return e;
}

void Engine::chain(hipStream_t from, hipStream_t to) {
  hipEvent_t e = next_ev();
  CGX_HIP_CHECK(hipEventRecord(e, from));
  CGX_HIP_CHECK(hipStreamWaitEvent(to, e, 0));
}

// Grow `buf` to at least `bytes` (power-of-two capacity).  The old buffer
// may still be read by work queued on `streams`; the caching allocator
// defers its reuse until those streams pass.
static uint8_t* grow(at::Tensor& buf, int64_t bytes,
                     std::initializer_list<hipStream_t> streams) {
  if (bytes <= 0) bytes = 1;
  if (!buf.defined() || buf.numel() < bytes) {
    if (buf.defined()) {
      for (hipStream_t s : streams) {
        if (!s) continue;
        c10::hip::HIPCachingAllocatorMasqueradingAsCUDA::
            recordStreamMasqueradingAsCUDA(
                buf.storage().data_ptr(),
                c10::hip::getStreamFromExternalMasqueradingAsCUDA(
                    s, buf.device().index()));
      }
    }
    int64_t cap = 1 << 20;
    while (cap < bytes) cap *= 2;
    buf = at::empty({cap},
                    at::TensorOptions().dtype(at::kByte).device(at::kCUDA));
  }
  return buf.data_ptr<uint8_t>();
}

uint8_t* Engine::staging(int64_t bytes, hipStream_t user) {
  return grow(staging_, bytes, {user, comm_stream_, deq_stream_});
}

uint8_t* Engine::slot_bytes(StagingSlot& slot, int64_t bytes) {
  return grow(slot.buf, bytes, {comm_stream_, deq_stream_});
}

at::Tensor& Engine::feedback_buf(int64_t key, int phase, int64_t numel,
                                 at::ScalarType st) {
  // bounded: residuals are a convergence aid; resetting them once (on a cap
  // overflow that only a pathological caller can trigger) is benign,
  // unbounded growth is not
  constexpr size_t kMaxEntries = 4096;
  if (fb_bufs_.size() >= kMaxEntries) {
    TORCH_WARN_ONCE("cgx: error-feedback store exceeded ", kMaxEntries,
                    " entries; resetting residuals");
    fb_bufs_.clear();
  }
  auto k = std::make_pair(key, phase);
  auto it = fb_bufs_.find(k);
  if (it != fb_bufs_.end() &&
      (it->second.numel() < numel || it->second.scalar_type() != st)) {
    fb_bufs_.erase(it);  // chunk grew or dtype changed: restart residual
    it = fb_bufs_.end();
  }
  if (it == fb_bufs_.end()) {
    auto t = at::zeros({numel}, at::TensorOptions().dtype(st).device(
                                    at::kCUDA));
    it = fb_bufs_.emplace(k, std::move(t)).first;
  }
  return it->second;
}

void Engine::run_quantize(const std::vector<Slice>& slices, uint8_t* out_base,
                          DType dt, hipStream_t stream, bool stochastic,
                          char* fb_base, int64_t fb_rebase) {
  std::vector<QuantSlice> qs;
  qs.reserve(slices.size());
  for (const auto& s : slices) {
    if (s.n <= 0) continue;
    void* fb =
        fb_base ? fb_base + (s.fb_off - fb_rebase) * elem_size(dt) : nullptr;
    TORCH_CHECK(!fb_base || s.fb_off >= fb_rebase,
                "cgx: error-feedback slice offset below buffer base");
    TORCH_CHECK(!fb || s.bucket % 8 == 0,
                "cgx: CGX_ERROR_FEEDBACK requires bucket_size % 8 == 0");
    qs.push_back(QuantSlice{s.data, out_base + s.comp_off, fb, s.n, s.bits,
                            s.bucket, s.skip_incomplete});
  }
  for (const QuantGroup& g : route_quantize(qs)) {
    const size_t desc_bytes = sizeof(QuantDesc) * g.descs.size();
    const size_t cum_bytes = sizeof(int64_t) * g.cum.size();
    char* host = (char*)ring_.acquire(desc_bytes + cum_bytes);
    std::memcpy(host, g.descs.data(), desc_bytes);
    std::memcpy(host + desc_bytes, g.cum.data(), cum_bytes);
    char* dev = (char*)ring_.commit(desc_bytes + cum_bytes, stream);
    launch(g, reinterpret_cast<const QuantDesc*>(dev),
           reinterpret_cast<const int64_t*>(dev + desc_bytes), dt, seed_++,
           stochastic, stream);
  }
}

void Engine::run_dequant(const std::vector<Slice>& slices,
                         const uint8_t* in_base, int64_t src_stride, int nsrc,
                         bool add, DType dt, hipStream_t stream) {
  std::vector<DequantSlice> ds;
  ds.reserve(slices.size());
  for (const auto& s : slices)
    ds.push_back(DequantSlice{in_base + s.comp_off, s.data, s.n, s.bits,
                              s.bucket, s.skip_incomplete});
  for (const DequantGroup& g :
       route_dequantize(ds, dt, src_stride, nsrc, add)) {
    const size_t desc_bytes = sizeof(DequantDesc) * g.descs.size();
    void* host = ring_.acquire(desc_bytes);
    std::memcpy(host, g.descs.data(), desc_bytes);
    launch(g, static_cast<const DequantDesc*>(ring_.commit(desc_bytes, stream)),
           dt, stream);
  }
}

void Engine::sra_chunk(const std::vector<LayerView>& views, DType dt,
                       Transport* tr, hipStream_t qs,
                       const EngineConfig& cfg, int64_t fb_key) {
  const int ws = size_;
  const ChunkPlan pl = plan_chunk(views, dt, ws, cfg.skip_incomplete);
  if (pl.n == 0) return;
  auto& rs = pl.rs;
  auto& comp = pl.comp;
  const int64_t mycomp = comp[rank_];
  // every peer's compressed stream back to back, in rank order: the layout
  // of send1 (round 1) and of recv2 (round 2)
  const ChunkPlan::Packed peers = pl.pack(/*skip_rank=*/rank_);
  const std::vector<int64_t>& peer_off = peers.off;
  const int64_t send1_total = peers.total;
  const int64_t recv1_total = (int64_t)(ws - 1) * mycomp;

  StagingSlot& sslot = slots_[slot_cur_];
  slot_cur_ ^= 1;
  if (sslot.recorded) {
    // don't overwrite staging another chunk's comm/decode still reads
    CGX_HIP_CHECK(hipStreamWaitEvent(qs, sslot.done_ev, 0));
  }
  uint8_t* base =
      slot_bytes(sslot, send1_total + recv1_total + mycomp + send1_total);
  uint8_t* send1 = base;
  uint8_t* recv1 = send1 + send1_total;
  uint8_t* send2 = recv1 + recv1_total;
  uint8_t* recv2 = send2 + mycomp;

  // round 1 quantize of every peer chunk, on the quantize stream
  {
    char* fb1 = nullptr;
    if (cfg.error_feedback) {
      at::Tensor& t =
          feedback_buf(fb_key, /*phase=*/1, pl.n, scalar_type_of(dt));
      fb1 = static_cast<char*>(t.data_ptr());
    }
    run_quantize(peers.slices, send1, dt, qs, cfg.stochastic, fb1);
  }
  timer_.mark(1, qs);

  // round 1 exchange on the comm stream (grouped p2p drives all xGMI links)
  chain(qs, comm_stream_);
  {
    std::vector<Transport::Op> sends, recvs;
    for (int p = 0; p < ws; p++) {
      if (p == rank_) continue;
      sends.push_back(Transport::Op{send1 + peer_off[p], comp[p], p});
      recvs.push_back(Transport::Op{
          recv1 + (int64_t)recv_slot(p, rank_) * mycomp, mycomp, p});
    }
    tr->exchange(sends, recvs, comm_stream_);
  }
  timer_.mark(2, comm_stream_);

  // decode-accumulate + self-quantize on the deq stream
  chain(comm_stream_, deq_stream_);
  if (mycomp > 0) {
    run_dequant(rs[rank_], recv1, mycomp, ws - 1, /*add=*/true, dt,
                deq_stream_);
    // self-quantize the reduced chunk; the same bytes go to every peer and
    // through my own decode so all ranks end bit-identical
    char* fb2 = nullptr;
    int64_t fb2_rebase = 0;
    if (cfg.error_feedback && pl.szs[rank_] > 0) {
      at::Tensor& t = feedback_buf(fb_key, /*phase=*/2, pl.szs[rank_],
                                   scalar_type_of(dt));
      // slice fb_off is in chunk element space; the phase-2 buffer covers
      // only this rank's partition, so rebase by its start (host-side per
      // slice — no out-of-range pointer arithmetic)
      fb2 = static_cast<char*>(t.data_ptr());
      fb2_rebase = pl.offs[rank_];
    }
    run_quantize(rs[rank_], send2, dt, deq_stream_, cfg.stochastic, fb2,
                 fb2_rebase);
  }
  timer_.mark(3, deq_stream_);

  // round 2 exchange on the comm stream
  chain(deq_stream_, comm_stream_);
  {
    std::vector<Transport::Op> sends, recvs;
    for (int p = 0; p < ws; p++) {
      if (p == rank_) continue;
      sends.push_back(Transport::Op{send2, mycomp, p});
      recvs.push_back(Transport::Op{recv2 + peer_off[p], comp[p], p});
    }
    tr->exchange(sends, recvs, comm_stream_);
  }
  timer_.mark(4, comm_stream_);

  // final decode: own chunk from send2, peers' chunks from recv2
  chain(comm_stream_, deq_stream_);
  if (mycomp > 0)
    run_dequant(rs[rank_], send2, 0, 1, /*add=*/false, dt, deq_stream_);
  run_dequant(peers.slices, recv2, 0, 1, /*add=*/false, dt, deq_stream_);
  timer_.mark(5, deq_stream_);
  timer_.finish();
  CGX_HIP_CHECK(hipEventRecord(sslot.done_ev, deq_stream_));
  sslot.recorded = true;
}

void Engine::ring_chunk(const std::vector<LayerView>& views, DType dt,
                        Transport* tr, hipStream_t stream,
                        const EngineConfig& cfg) {
  // Compressed ring allreduce (reference MPI_Allreduce_Ring semantics,
  // ring.cc:139-226): ws-1 reduce-scatter steps with per-hop requantize of
  // the running partial sum, then ws-1 allgather steps FORWARDING the
  // once-quantized reduced segments, final batch decompress.
  TORCH_CHECK(!cfg.error_feedback,
              "cgx: CGX_ERROR_FEEDBACK is not supported with Ring reduction "
              "(the ring requantizes running partial sums, which have no "
              "stable per-step residual); use SRA or disable error feedback");
  const int ws = size_;
  const ChunkPlan pl = plan_chunk(views, dt, ws, cfg.skip_incomplete);
  if (pl.n == 0) return;
  auto& rs = pl.rs;
  auto& comp = pl.comp;
  const int next = (rank_ + 1) % ws;
  const int prev = (rank_ + ws - 1) % ws;

  // every rank's reduced segment back to back: the allgather buffer
  const ChunkPlan::Packed all = pl.pack();
  const std::vector<int64_t>& seg_off = all.off;
  const int64_t seg_total = all.total;
  const int64_t maxc = *std::max_element(comp.begin(), comp.end());
  uint8_t* base = staging(seg_total + 2 * maxc, stream);
  uint8_t* segs = base;
  uint8_t* tmp_send = base + seg_total;
  uint8_t* tmp_recv = tmp_send + maxc;

  // reduce-scatter: accumulate into local chunks hop by hop
  for (int s = 0; s < ws - 1; s++) {
    const int send_c = (rank_ - s + ws) % ws;
    const int recv_c = (rank_ - s - 1 + ws) % ws;
    if (comp[send_c] > 0)
      run_quantize(rs[send_c], tmp_send, dt, stream, cfg.stochastic);
    tr->exchange({Transport::Op{tmp_send, comp[send_c], next}},
                 {Transport::Op{tmp_recv, comp[recv_c], prev}}, stream);
    if (comp[recv_c] > 0)
      run_dequant(rs[recv_c], tmp_recv, 0, 1, /*add=*/true, dt, stream);
  }

  // own fully-reduced chunk after ws-1 hops
  const int own = (rank_ + 1) % ws;
  if (comp[own] > 0)
    run_quantize(rs[own], segs + seg_off[own], dt, stream, cfg.stochastic);

  // allgather: forward the quantized reduced segments around the ring
  for (int s = 0; s < ws - 1; s++) {
    const int send_c = (own - s + ws) % ws;
    const int recv_c = (own - s - 1 + ws) % ws;
    tr->exchange({Transport::Op{segs + seg_off[send_c], comp[send_c], next}},
                 {Transport::Op{segs + seg_off[recv_c], comp[recv_c], prev}},
                 stream);
  }

  // final decode of every segment (own included, for bit-identical results)
  run_dequant(all.slices, segs, 0, 1, /*add=*/false, dt, stream);
}

void Engine::a2a_chunk(const std::vector<LayerView>& views, DType dt,
                       Transport* tr, hipStream_t qs,
                       const EngineConfig& cfg) {
  // Debug brute-force reduction (reference AllReduceAlltoAllCompressed,
  // scatter_reduce_allgather.cc:269-306): every rank quantizes its ENTIRE
  // chunk once and sends it to every peer; every rank then decodes the same
  // ws compressed streams (self first, then peers in rank order).  Each
  // rank's data is quantized exactly once, but the per-rank ACCUMULATION
  // order differs (self-first), so at ws>2 results agree to fp rounding,
  // not bitwise — same as the reference's arrival-order accumulate.  ws x
  // the wire bytes of SRA, but no partitioning machinery in the fault
  // surface.
  TORCH_CHECK(!cfg.error_feedback,
              "cgx: CGX_DEBUG_ALL_TO_ALL_REDUCTION does not support "
              "CGX_ERROR_FEEDBACK");
  const int ws = size_;
  // the whole chunk as one rank's share: one slice per view
  const ChunkPlan pl = plan_chunk(views, dt, /*ws=*/1, cfg.skip_incomplete);
  if (pl.n == 0) return;
  const std::vector<Slice>& sl = pl.rs[0];
  const int64_t C = pl.comp[0];
  uint8_t* base = staging(C * ws, qs);
  uint8_t* send = base;          // own compressed stream
  uint8_t* recv = base + C;      // ws-1 peer streams, stride C
  run_quantize(sl, send, dt, qs, cfg.stochastic);
  chain(qs, comm_stream_);
  {
    std::vector<Transport::Op> sends, recvs;
    for (int p = 0; p < ws; p++) {
      if (p == rank_) continue;
      sends.push_back(Transport::Op{send, C, p});
      recvs.push_back(
          Transport::Op{recv + (int64_t)recv_slot(p, rank_) * C, C, p});
    }
    tr->exchange(sends, recvs, comm_stream_);
  }
  chain(comm_stream_, deq_stream_);
  run_dequant(sl, send, 0, 1, /*add=*/false, dt, deq_stream_);
  if (ws > 1)
    run_dequant(sl, recv, C, ws - 1, /*add=*/true, dt, deq_stream_);
  // the shared staging() buffer is reused by the next chunk's quantize on
  // qs: fence it behind this chunk's decode
  chain(deq_stream_, qs);
}

hipStream_t Engine::broadcast(at::Tensor t, int root, Transport* tr,
                              hipStream_t qs) {
  const EngineConfig cfg = EngineConfig::from_env();
  const int64_t n = t.numel();
  const bool compress = !cfg.dummy && cfg.intra_compress &&
                        cfg.default_bits <= 8 && n > cfg.min_elems &&
                        is_compressible(t.scalar_type());
  if (!compress || size_ <= 1) {
    if (size_ > 1) {
      tr->broadcast(t.data_ptr(), n, (int)t.element_size(), nccl_dtype(t),
                    root, qs);
    }
    return qs;
  }
  const DType dt = dtype_of(t);
  const int64_t bytes =
      buffer_size(n, dt, cfg.default_bits, cfg.default_bucket,
                  cfg.skip_incomplete);
  uint8_t* buf = staging(bytes, qs);
  std::vector<Slice> sl{Slice{static_cast<char*>(t.data_ptr()), n,
                              cfg.default_bits, cfg.default_bucket, 0,
                              cfg.skip_incomplete}};
  if (rank_ == root) {
    run_quantize(sl, buf, dt, qs, cfg.stochastic);
  }
  tr->broadcast(buf, bytes, 1, ncclUint8, root, qs);
  // every rank (root included) decodes the same bytes -> bit-identical
  run_dequant(sl, buf, 0, 1, /*add=*/false, dt, qs);
  return qs;
}

hipStream_t Engine::allreduce(at::Tensor bucket, Transport* tr,
                              hipStream_t qs,
                              const Registry::BucketInfo* forced,
                              bool forced_match) {
  if (size_ <= 1) return qs;
  TORCH_CHECK(bucket.is_contiguous(), "cgx: bucket must be contiguous");
  EngineConfig cfg = EngineConfig::from_env();
  if (is_cross_) cfg.ring = cfg.cross_ring;
  const DType dt = dtype_of(bucket);
  const int es = elem_size(dt);
  char* base = static_cast<char*>(bucket.data_ptr());
  const int64_t numel = bucket.numel();

  Registry::BucketInfo info;
  bool matched;
  if (forced) {
    matched = forced_match;
    if (matched) info = *forced;
  } else {
    matched = Registry::get().next(numel, bucket.data_ptr(), &info);
  }
  std::vector<LayerView> views;
  if (matched) {
    int64_t off = 0;
    for (size_t i = 0; i < info.numels.size(); i++) {
      views.push_back(LayerView{base + off * es, info.numels[i],
                                info.cfgs[i].bits, info.cfgs[i].bucket_size});
      off += info.numels[i];
    }
  } else {
    views.push_back(LayerView{base, numel, cfg.default_bits,
                              cfg.default_bucket});
  }

  const BucketPlan bp = plan_bucket(views, cfg, es);

  if (!bp.uncomp.empty()) {
    const ncclDataType_t ndt = nccl_dtype(bucket);
    chain(qs, comm_stream_);
    std::vector<std::pair<void*, int64_t>> bufs;
    for (auto& [ptr, cnt] : bp.uncomp) bufs.emplace_back(ptr, cnt);
    tr->allreduce_sum_group(bufs, ndt, comm_stream_);
  }

  for (size_t ci = 0; ci < bp.chunks.size(); ci++) {
    const std::vector<LayerView>& vs = bp.chunks[ci];
    // error-feedback residual identity for this (bucket, chunk): registry
    // bucket index + chunk ordinal when matched; pointer-derived negative
    // fallback key otherwise (DDP flat buffers are pointer-stable)
    const int64_t fb_key =
        matched ? (((int64_t)info.idx << 20) | (int64_t)ci)
                : -(int64_t)(reinterpret_cast<uintptr_t>(vs[0].data) >> 3);
    timer_.begin(qs, env_timings() && !cfg.ring);
    if (cfg.debug_a2a) {
      a2a_chunk(vs, dt, tr, qs, cfg);
    } else if (cfg.ring && size_ > 2) {
      // ring is hop-serial and runs on one stream (qs).  Its NCCL ops must
      // be ordered behind any uncompressed ncclAllReduce group queued on
      // comm_stream_ above: unordered concurrent ops on one communicator
      // are UB in NCCL/RCCL.
      chain(comm_stream_, qs);
      ring_chunk(vs, dt, tr, qs, cfg);
      chain(qs, deq_stream_);             // keep completion on deq stream
    } else {
      sra_chunk(vs, dt, tr, qs, cfg, fb_key);
    }
  }

  // completion stream: all compressed chunks end on deq_stream_, and each
  // chained through comm_stream_, where the uncompressed group ran first
  if (!bp.chunks.empty()) return deq_stream_;
  if (!bp.uncomp.empty()) return comm_stream_;
  return qs;
}

}  // namespace cgx
