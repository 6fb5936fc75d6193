// Python bindings for torch_cgx_amd._C.
//
// Surface parity with the reference pybind module
// (/root/reference/src/ProcessGroupCGX.cc:852-857): register_layer,
// set_quantization_bits, set_quantization_bucket_size (the reference's
// set_quantization_bucket_size mistakenly called SetQBits — fixed here),
// plus the ProcessGroupCGX class for the Python-side backend creator and
// direct kernel entry points used by the GPU tests.
#include <torch/extension.h>

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/csrc/utils/pybind.h>

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <functional>
#include <thread>
#include <tuple>

#include "backend.h"
#include "bn_plan.h"
#include "collectives.h"
#include "conv1x1_plan.h"
#include "reducer.h"

namespace cgx {
namespace {

// Rank-thread harness of the loopback seams: one quantize stream and one
// thread per rank, GIL released.  A rank that throws stores its error and
// calls `abort` (poison the hubs so no peer blocks in join); the first error
// is rethrown once every thread has joined and the device has drained.
void run_rank_threads(int ws, int dev,
                      const std::function<void(int, hipStream_t)>& body,
                      const std::function<void()>& abort) {
  std::vector<hipStream_t> qs(ws, nullptr);
  for (auto& s : qs)
    CGX_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  std::vector<std::exception_ptr> errs(ws);
  {
    py::gil_scoped_release nogil;
    std::vector<std::thread> th;
    for (int r = 0; r < ws; r++) {
      th.emplace_back([&, r] {
        try {
          c10::hip::HIPGuardMasqueradingAsCUDA g(dev);
          body(r, qs[r]);
        } catch (...) {
          errs[r] = std::current_exception();
          abort();  // unblock peers so join() cannot hang
        }
      });
    }
    for (auto& t : th) t.join();
  }
  (void)hipDeviceSynchronize();  // loopback events/copies fully retired
  for (auto s : qs)
    if (s) (void)hipStreamDestroy(s);
  for (int r = 0; r < ws; r++)
    if (errs[r]) std::rethrow_exception(errs[r]);
}

// N ranks inside one process: a Reducer per rank over loopback transports
// (device-to-device copies with full stream/event fencing) -- the production
// engines with their own streams, staging and events, composed by the
// production Reducer.  local_size == 0 builds the flat stage only (one world
// hub); otherwise ws = n_nodes * local_size and every rank also gets an intra
// stage on its node's hub, each node leader a cross stage on the leaders'
// hub, like the backend's lazyInit.
struct LoopbackWorld {
  std::vector<std::unique_ptr<LoopbackHub>> hubs;
  std::vector<std::unique_ptr<LoopbackTransport>> trs;
  std::vector<Reducer> ranks;

  LoopbackWorld(int ws, int local_size) {
    ranks.resize(ws);
    LoopbackHub* world = hub(ws);
    for (int r = 0; r < ws; r++) ranks[r].flat.emplace(r, ws, tr(world, r));
    if (local_size == 0) return;
    const int nodes = ws / local_size;
    LoopbackHub* cross = hub(nodes);
    for (int nd = 0; nd < nodes; nd++) {
      LoopbackHub* intra = hub(local_size);
      for (int lr = 0; lr < local_size; lr++) {
        Reducer& red = ranks[nd * local_size + lr];
        red.intra.emplace(lr, local_size, tr(intra, lr));
        red.leader = lr == 0;
        if (red.leader)
          red.cross.emplace(nd, nodes, tr(cross, nd), /*is_cross=*/true);
      }
    }
  }
  // poison every hub so no peer of a failed rank blocks
  void abort() {
    for (auto& h : hubs) h->abort();
  }

 private:
  LoopbackHub* hub(int world) {
    hubs.push_back(std::make_unique<LoopbackHub>(world));
    return hubs.back().get();
  }
  Transport* tr(LoopbackHub* h, int rank) {
    trs.push_back(std::make_unique<LoopbackTransport>(h, rank));
    return trs.back().get();
  }
};

// Run body(rank's Reducer, quantize stream, rank) -> completion stream on one
// thread per rank of a LoopbackWorld over `tensors` (tensors[r] is rank r's),
// then drain every stream the rank used.  This is the hardware test seam the
// multi-rank paths run under `pytest -m gpu` with a single MI355X: RCCL
// itself refuses two ranks on one device.
void run_loopback(
    const std::vector<at::Tensor>& tensors, int local_size,
    const std::function<hipStream_t(Reducer&, hipStream_t, int)>& body) {
  const int ws = (int)tensors.size();
  TORCH_CHECK(ws >= 2, "loopback: need >= 2 per-rank tensors");
  TORCH_CHECK(local_size == 0 || (ws % local_size == 0 && ws / local_size >= 2),
              "loopback: hierarchical world must be n_nodes*local_size with "
              ">= 2 nodes");
  for (const auto& t : tensors) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(),
                "loopback: CUDA contiguous tensors required");
    TORCH_CHECK(t.device() == tensors[0].device() &&
                    t.numel() == tensors[0].numel() &&
                    t.scalar_type() == tensors[0].scalar_type(),
                "loopback: tensors must match in device/numel/dtype");
  }
  const int dev = tensors[0].device().index();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  LoopbackWorld world(ws, local_size);
  run_rank_threads(
      ws, dev,
      [&](int r, hipStream_t qs) {
        hipStream_t fin = body(world.ranks[r], qs, r);
        CGX_HIP_CHECK(hipStreamSynchronize(fin));
        CGX_HIP_CHECK(hipStreamSynchronize(qs));
        world.ranks[r].for_each_stream(
            [](hipStream_t s) { CGX_HIP_CHECK(hipStreamSynchronize(s)); });
      },
      [&] { world.abort(); });
}

// The rank threads share one layer registry, so the harness takes its one
// cursor step per bucket up front and forces the result into every rank.
struct Resolved {
  explicit Resolved(int64_t numel)
      : matched(Registry::get().next(numel, nullptr, &info)) {}
  Registry::BucketInfo info;
  bool matched;
};

void py_loopback_allreduce(std::vector<at::Tensor> buckets) {
  const Resolved reg(buckets.empty() ? 0 : buckets[0].numel());
  run_loopback(buckets, /*local_size=*/0,
               [&](Reducer& red, hipStream_t qs, int r) {
                 return red.allreduce(buckets[r], qs, &reg.info, reg.matched);
               });
}

// Multiple allreduce steps on PERSISTENT engines (one set of engines for
// all steps, like a training run): steps[s][r] is rank r's bucket at step
// s, reduced in place.  This is what lets error-feedback residuals carry
// across steps on hardware.
void py_loopback_allreduce_multi(
    std::vector<std::vector<at::Tensor>> steps) {
  TORCH_CHECK(!steps.empty(), "loopback_allreduce_multi: no steps");
  const int ws = (int)steps[0].size();
  const int64_t numel = steps[0][0].numel();
  for (auto& st : steps) {
    TORCH_CHECK((int)st.size() == ws && st[0].numel() == numel,
                "loopback_allreduce_multi: ragged steps");
  }
  const Resolved reg(numel);
  run_loopback(steps[0], /*local_size=*/0,
               [&](Reducer& red, hipStream_t qs, int r) {
                 hipStream_t fin = qs;
                 for (auto& st : steps)
                   fin = red.allreduce(st[r], qs, &reg.info, reg.matched);
                 return fin;
               });
}

void py_loopback_broadcast(std::vector<at::Tensor> tensors, int64_t root) {
  run_loopback(tensors, /*local_size=*/0,
               [&](Reducer& red, hipStream_t qs, int r) {
                 return red.flat->engine->broadcast(tensors[r], (int)root,
                                                    red.flat->tr, qs);
               });
}

// The multi-node allreduce on one GPU: ws = n_nodes * local_size ranks run
// Reducer::allreduce, the call ProcessGroupCGX makes per bucket -- the
// hierarchical flow, or the flat one under CGX_INTRA_BROADCAST=0.
void py_loopback_hierarchical(std::vector<at::Tensor> buckets,
                              int64_t local_size) {
  TORCH_CHECK(local_size >= 1, "loopback_hierarchical: local_size >= 1");
  const Resolved reg(buckets.empty() ? 0 : buckets[0].numel());
  run_loopback(buckets, (int)local_size,
               [&](Reducer& red, hipStream_t qs, int r) {
                 return red.allreduce(buckets[r], qs, &reg.info, reg.matched);
               });
}

// The backend's p2p collectives (collectives.h) with real peers on one GPU:
// rank r runs the function ProcessGroupCGX runs, over a loopback transport,
// on inputs[r] / outputs[r], the tensor lists its backend method would get
// (alltoall_base: one tensor each; the non-root side of gather/scatter: none).
void py_loopback_collective(
    const std::string& name, std::vector<std::vector<at::Tensor>> inputs,
    std::vector<std::vector<at::Tensor>> outputs, int64_t root,
    std::vector<std::vector<int64_t>> in_splits,
    std::vector<std::vector<int64_t>> out_splits) {
  const int ws = (int)inputs.size();
  TORCH_CHECK(ws >= 1 && (int)outputs.size() == ws && root >= 0 && root < ws,
              "loopback_collective: one input and one output list per rank "
              "and a root among them");
  TORCH_CHECK((in_splits.empty() || (int)in_splits.size() == ws) &&
                  (out_splits.empty() || (int)out_splits.size() == ws),
              "loopback_collective: splits are per rank, or empty");
  in_splits.resize(ws);
  out_splits.resize(ws);
  // per name: the list lengths of rank r, and the call it makes
  std::function<size_t(int)> n_in, n_out;
  std::function<void(Transport*, int, hipStream_t)> call;
  const auto one = [](int) { return (size_t)1; };
  const auto all = [ws](int) { return (size_t)ws; };
  const auto at_root = [ws, root](int r) { return r == root ? (size_t)ws : 0; };
  if (name == "allgather") {
    n_in = one; n_out = all;
    call = [&](Transport* tr, int r, hipStream_t s) {
      coll::allgather(tr, r, ws, inputs[r][0], outputs[r], s);
    };
  } else if (name == "gather") {
    n_in = one; n_out = at_root;
    call = [&](Transport* tr, int r, hipStream_t s) {
      coll::gather(tr, r, ws, (int)root, inputs[r][0], outputs[r], s);
    };
  } else if (name == "scatter") {
    n_in = at_root; n_out = one;
    call = [&](Transport* tr, int r, hipStream_t s) {
      coll::scatter(tr, r, ws, (int)root, inputs[r], outputs[r][0], s);
    };
  } else if (name == "alltoall") {
    n_in = all; n_out = all;
    call = [&](Transport* tr, int r, hipStream_t s) {
      coll::alltoall(tr, r, ws, inputs[r], outputs[r], s);
    };
  } else if (name == "alltoall_base") {
    n_in = one; n_out = one;
    call = [&](Transport* tr, int r, hipStream_t s) {
      coll::alltoall_base(tr, r, ws, inputs[r][0], outputs[r][0], in_splits[r],
                          out_splits[r], s);
    };
  } else {
    TORCH_CHECK(false, "loopback_collective: unknown collective '", name, "'");
  }
  c10::optional<at::Device> device;
  for (int r = 0; r < ws; r++) {
    TORCH_CHECK(inputs[r].size() == n_in(r) && outputs[r].size() == n_out(r),
                "loopback_collective: rank ", r, " of ", name, " takes ",
                n_in(r), " input and ", n_out(r), " output tensors");
    for (const auto* ts : {&inputs[r], &outputs[r]})
      for (const at::Tensor& t : *ts) {
        TORCH_CHECK(t.is_cuda() && t.is_contiguous(),
                    "loopback_collective: CUDA contiguous tensors required");
        if (!device) device = t.device();
        TORCH_CHECK(t.device() == *device,
                    "loopback_collective: tensors must share one device");
      }
  }
  const int dev = device->index();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  // the rank streams do not order behind the caller's: drain its work first
  CGX_HIP_CHECK(hipStreamSynchronize(
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev).stream()));
  LoopbackHub hub(ws);
  std::vector<LoopbackTransport> trs;
  for (int r = 0; r < ws; r++) trs.emplace_back(&hub, r);
  run_rank_threads(
      ws, dev,
      [&](int r, hipStream_t s) {
        call(&trs[r], r, s);
        CGX_HIP_CHECK(hipStreamSynchronize(s));
      },
      [&] { hub.abort(); });
}

// Copy a routed group's descs (followed by cum, if any) to the device.
template <typename Desc>
at::Tensor upload(const std::vector<Desc>& descs,
                  const std::vector<int64_t>& cum, at::Device device) {
  const size_t desc_bytes = sizeof(Desc) * descs.size();
  const size_t cum_bytes = sizeof(int64_t) * cum.size();
  std::vector<char> host(desc_bytes + cum_bytes);
  std::memcpy(host.data(), descs.data(), desc_bytes);
  std::memcpy(host.data() + desc_bytes, cum.data(), cum_bytes);
  return at::from_blob(host.data(), {(int64_t)host.size()},
                       at::TensorOptions().dtype(at::kByte))
      .to(device);
}

// Route one slice's decode and launch every group on the current stream.
void dequantize_slice(const at::Tensor& comp, at::Tensor& out, int64_t bits,
                      int64_t bucket_size, bool skip_incomplete,
                      int64_t src_stride, int nsrc, bool add) {
  const DType dt = dtype_of(out);
  auto stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(out.device().index());
  const std::vector<DequantSlice> slices{
      DequantSlice{comp.data_ptr<uint8_t>(), out.data_ptr(), out.numel(),
                   (int)bits, (int)bucket_size, skip_incomplete}};
  for (const DequantGroup& g :
       route_dequantize(slices, dt, src_stride, nsrc, add)) {
    auto dev = upload(g.descs, {}, out.device());
    launch(g, static_cast<const DequantDesc*>(dev.data_ptr()), dt,
           stream.stream());
  }
}

// Zero-filled buffer for the compressed form of x.
at::Tensor compressed_buffer(const at::Tensor& x, int64_t bits,
                             int64_t bucket_size, bool skip_incomplete) {
  const int64_t bytes = buffer_size(x.numel(), dtype_of(x), (int)bits,
                                    (int)bucket_size, skip_incomplete);
  return at::zeros({std::max<int64_t>(bytes, 1)},
                   at::TensorOptions().dtype(at::kByte).device(x.device()));
}

// Route `slices` and launch every group on the current stream; group k (in
// routed order) runs with seed + k * seed_step.
void launch_quantize(const std::vector<QuantSlice>& slices, DType dt,
                     uint64_t seed, uint64_t seed_step, bool stochastic,
                     at::Device device) {
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(device.index());
  uint64_t k = 0;
  for (const QuantGroup& g : route_quantize(slices)) {
    auto dev = upload(g.descs, g.cum, device);
    const char* devp = static_cast<const char*>(dev.data_ptr());
    launch(g, reinterpret_cast<const QuantDesc*>(devp),
           reinterpret_cast<const int64_t*>(devp +
                                            sizeof(QuantDesc) * g.descs.size()),
           dt, seed + (k++) * seed_step, stochastic, stream.stream());
  }
}

// Compress a 1-D CUDA tensor; returns the uint8 compressed buffer
// (zero-filled alignment padding so byte comparisons are well-defined).
at::Tensor py_quantize(at::Tensor x, int64_t bits, int64_t bucket_size,
                       bool stochastic, int64_t seed, bool skip_incomplete,
                       c10::optional<at::Tensor> feedback) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "quantize: CUDA contiguous");
  TORCH_CHECK(bits >= 1 && bits <= 8, "quantize: bits in [1,8]");
  TORCH_CHECK(bucket_size >= 1, "quantize: bucket_size >= 1");
  void* fbp = nullptr;
  if (feedback.has_value()) {
    TORCH_CHECK(feedback->is_cuda() && feedback->is_contiguous() &&
                    feedback->numel() == x.numel() &&
                    feedback->scalar_type() == x.scalar_type(),
                "quantize: feedback must match x");
    TORCH_CHECK(bucket_size % 8 == 0,
                "quantize: error feedback requires bucket_size % 8 == 0");
    fbp = feedback->data_ptr();
  }
  const DType dt = dtype_of(x);
  const int64_t n = x.numel();
  auto out = compressed_buffer(x, bits, bucket_size, skip_incomplete);
  launch_quantize({QuantSlice{x.data_ptr(), out.data_ptr<uint8_t>(), fbp, n,
                              (int)bits, (int)bucket_size, skip_incomplete}},
                  dt, (uint64_t)seed, /*seed_step=*/0, stochastic, x.device());
  return out;
}

// Test seam for the slice index of the stochastic hash key: compress several
// 1-D CUDA tensors of one dtype with ONE route_quantize call, so a launch
// group holds more than one slice, and give group k (in routed order) the
// seed `seed + k`, as Engine::run_quantize does with seed_++.  Returns one
// compressed buffer per tensor.
std::vector<at::Tensor> py_quantize_slices(std::vector<at::Tensor> xs,
                                           std::vector<int64_t> bits,
                                           std::vector<int64_t> bucket_sizes,
                                           bool stochastic, int64_t seed,
                                           bool skip_incomplete) {
  TORCH_CHECK(!xs.empty() && bits.size() == xs.size() &&
                  bucket_sizes.size() == xs.size(),
              "quantize_slices: one bits and one bucket_size per tensor");
  std::vector<QuantSlice> slices;
  std::vector<at::Tensor> outs;
  for (size_t i = 0; i < xs.size(); i++) {
    const at::Tensor& x = xs[i];
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 1 &&
                    x.numel() > 0 && x.device() == xs[0].device() &&
                    x.scalar_type() == xs[0].scalar_type(),
                "quantize_slices: non-empty 1-D contiguous CUDA tensors of "
                "one dtype on one device");
    TORCH_CHECK(bits[i] >= 1 && bits[i] <= 8, "quantize_slices: bits in [1,8]");
    TORCH_CHECK(bucket_sizes[i] >= 1, "quantize_slices: bucket_size >= 1");
    outs.push_back(
        compressed_buffer(x, bits[i], bucket_sizes[i], skip_incomplete));
    slices.push_back(QuantSlice{x.data_ptr(), outs[i].data_ptr<uint8_t>(),
                                nullptr, x.numel(), (int)bits[i],
                                (int)bucket_sizes[i], skip_incomplete});
  }
  launch_quantize(slices, dtype_of(xs[0]), (uint64_t)seed, /*seed_step=*/1,
                  stochastic, xs[0].device());
  return outs;
}

// Decompress `comp` into `out` (1-D CUDA tensor of n elements); add=True
// accumulates in T precision.
void py_dequantize(at::Tensor comp, at::Tensor out, int64_t bits,
                   int64_t bucket_size, bool add, bool skip_incomplete) {
  TORCH_CHECK(comp.is_cuda() && out.is_cuda() && out.is_contiguous());
  dequantize_slice(comp, out, bits, bucket_size, skip_incomplete,
                   /*src_stride=*/0, /*nsrc=*/1, add);
}

// Multi-source decode-and-sum: comp is [nsrc, stride] uint8; decodes each
// row's stream and accumulates in T precision (the engine's round-1 path).
void py_dequantize_multi(at::Tensor comp, at::Tensor out, int64_t bits,
                         int64_t bucket_size, bool add) {
  TORCH_CHECK(comp.is_cuda() && comp.dim() == 2 && comp.is_contiguous());
  TORCH_CHECK(out.is_cuda() && out.is_contiguous());
  dequantize_slice(comp, out, bits, bucket_size, /*skip_incomplete=*/false,
                   comp.stride(0), (int)comp.size(0), add);
}

int64_t py_buffer_size(int64_t n, at::ScalarType st, int64_t bits,
                       int64_t bucket_size, bool skip_incomplete) {
  return buffer_size(n, dtype_of(st), (int)bits, (int)bucket_size,
                     skip_incomplete);
}

// Test seams for the router (compress.h): pure host code, pointers travel
// as ints, so the routing policy is testable without a GPU.
// slices: [(in, out, fb, n, bits, bucket, skip_incomplete)] ->
// [(bits, kind, [(in, out, fb, n, bucket, flags)], cum, any_residual,
//   max_gpl)]
py::list py_route_quantize(
    const std::vector<std::tuple<uint64_t, uint64_t, uint64_t, int64_t, int,
                                 int, bool>>& slices) {
  std::vector<QuantSlice> qs;
  for (const auto& [in, out, fb, n, bits, bucket, skip] : slices)
    qs.push_back(QuantSlice{reinterpret_cast<const void*>(in),
                            reinterpret_cast<uint8_t*>(out),
                            reinterpret_cast<void*>(fb), n, bits, bucket,
                            skip});
  py::list groups;
  for (const QuantGroup& g : route_quantize(qs)) {
    py::list descs;
    for (const QuantDesc& d : g.descs)
      descs.append(py::make_tuple(reinterpret_cast<uint64_t>(d.in),
                                  reinterpret_cast<uint64_t>(d.out),
                                  reinterpret_cast<uint64_t>(d.fb), d.n,
                                  d.bucket, d.flags));
    groups.append(py::make_tuple(g.bits, g.kind, descs, g.cum, g.any_residual,
                                 g.max_gpl));
  }
  return groups;
}

// slices: [(in, out, n, bits, bucket, skip_incomplete)] ->
// [(bits, kind, [(in, out, n, src_stride, bucket, nsrc, add, flags)],
//   total_groups, any_residual)]
py::list py_route_dequantize(
    const std::vector<std::tuple<uint64_t, uint64_t, int64_t, int, int,
                                 bool>>& slices,
    at::ScalarType st, int64_t src_stride, int nsrc, bool add) {
  std::vector<DequantSlice> ds;
  for (const auto& [in, out, n, bits, bucket, skip] : slices)
    ds.push_back(DequantSlice{reinterpret_cast<const uint8_t*>(in),
                              reinterpret_cast<void*>(out), n, bits, bucket,
                              skip});
  py::list groups;
  for (const DequantGroup& g :
       route_dequantize(ds, dtype_of(st), src_stride, nsrc, add)) {
    py::list descs;
    for (const DequantDesc& d : g.descs)
      descs.append(py::make_tuple(reinterpret_cast<uint64_t>(d.in),
                                  reinterpret_cast<uint64_t>(d.out), d.n,
                                  d.src_stride, d.bucket, d.nsrc, d.add,
                                  d.flags));
    groups.append(py::make_tuple(g.bits, g.kind, descs, g.total_groups,
                                 g.any_residual));
  }
  return groups;
}

std::pair<std::vector<int64_t>, std::vector<int64_t>> py_partition(
    int64_t num_elements, int64_t world_size,
    std::vector<int64_t> layer_numels, int64_t esize) {
  std::vector<int64_t> offs, szs;
  partition(num_elements, (int)world_size, layer_numels, (int)esize, &offs,
            &szs);
  return {offs, szs};
}

// Test seams for chunk planning (plan.h): pure host code.  Pointers travel
// as ints with base 0, so every `data` is a byte offset into the bucket.
// (byte_off, numel, bits, bucket)
using PyView = std::tuple<uint64_t, int64_t, int, int>;
std::vector<LayerView> to_views(const std::vector<PyView>& views) {
  std::vector<LayerView> out;
  for (const auto& [off, numel, bits, bucket] : views)
    out.push_back(LayerView{reinterpret_cast<char*>(off), numel, bits, bucket});
  return out;
}

// -> (uncomp [(byte_off, count)], chunks [[(byte_off, numel, bits, bucket)]])
py::tuple py_plan_bucket(const std::vector<int64_t>& layer_numels,
                         const std::vector<std::pair<int, int>>& layer_cfgs,
                         at::ScalarType st, int64_t fusion_bytes,
                         int64_t min_elems, double fake_ratio, bool dummy) {
  TORCH_CHECK(layer_numels.size() == layer_cfgs.size(),
              "plan_bucket: one (bits, bucket_size) per layer");
  const int es = elem_size(dtype_of(st));
  EngineConfig cfg;
  cfg.fusion_bytes = fusion_bytes;
  cfg.min_elems = min_elems;
  cfg.fake_ratio = fake_ratio;
  cfg.dummy = dummy;
  std::vector<LayerView> views;
  int64_t off = 0;
  for (size_t i = 0; i < layer_numels.size(); i++) {
    views.push_back(LayerView{reinterpret_cast<char*>(off * es),
                              layer_numels[i], layer_cfgs[i].first,
                              layer_cfgs[i].second});
    off += layer_numels[i];
  }
  const BucketPlan bp = plan_bucket(views, cfg, es);
  py::list uncomp, chunks;
  for (const auto& [ptr, cnt] : bp.uncomp)
    uncomp.append(py::make_tuple(reinterpret_cast<uint64_t>(ptr), cnt));
  for (const auto& chunk : bp.chunks) {
    py::list vs;
    for (const LayerView& v : chunk)
      vs.append(py::make_tuple(reinterpret_cast<uint64_t>(v.data), v.numel,
                               v.bits, v.bucket_size));
    chunks.append(vs);
  }
  return py::make_tuple(uncomp, chunks);
}

// views: [(byte_off, numel, bits, bucket)] ->
// (offs, szs, comp, rs [[(byte_off, n, bits, bucket, comp_off, skip, fb_off)]])
py::tuple py_plan_chunk(const std::vector<PyView>& views, at::ScalarType st,
                        int ws, bool skip_incomplete) {
  TORCH_CHECK(ws >= 1, "plan_chunk: ws >= 1");
  const ChunkPlan pl =
      plan_chunk(to_views(views), dtype_of(st), ws, skip_incomplete);
  py::list rs;
  for (const auto& slices : pl.rs) {
    py::list r;
    for (const Slice& s : slices)
      r.append(py::make_tuple(reinterpret_cast<uint64_t>(s.data), s.n, s.bits,
                              s.bucket, s.comp_off, s.skip_incomplete,
                              s.fb_off));
    rs.append(r);
  }
  return py::make_tuple(pl.offs, pl.szs, pl.comp, rs);
}

// ---- fused BatchNorm (bn_plan.h, bn_kernels.hip) ---------------------------

// What the kernels index: a dense channels_last bf16 CUDA tensor whose first
// byte is 16-byte aligned.
bool bn_tensor_ok(const at::Tensor& t) {
  return t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.dim() == 4 &&
         t.numel() > 0 && t.is_contiguous(at::MemoryFormat::ChannelsLast) &&
         reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

BnPlan bn_plan_of(const at::Tensor& t) {
  return bn_plan(t.numel() / t.size(1), t.size(1));
}

bool py_bn_eligible(const at::Tensor& x) {
  return bn_tensor_ok(x) && bn_plan_of(x).eligible;
}

float* bn_channel_vec(const at::Tensor& t, int64_t c, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.numel() == c,
              "bn_act: ", what, " must be a contiguous fp32 CUDA vector of ",
              c, " elements");
  return t.data_ptr<float>();
}

// Partials a 1x1 convolution left for the BatchNorm of `x` (conv1x1_stats):
// [splits, 2*C + ntiles] fp32.
BnPartials bn_external_partials(const at::Tensor& part, const at::Tensor& x) {
  const int64_t c = x.size(1);
  TORCH_CHECK(part.is_cuda() && part.device() == x.device() &&
                  part.scalar_type() == at::kFloat && part.dim() == 2 &&
                  part.is_contiguous() && part.size(0) >= 1 &&
                  part.size(1) > 2 * c,
              "bn_act: part must be the [splits, 2*C + ntiles] fp32 partials "
              "of conv1x1_stats");
  const int64_t ntiles = part.size(1) - 2 * c;
  TORCH_CHECK(c % (8 * ntiles) == 0, "bn_act: part has a bad count column");
  return conv1x1_partials(part.data_ptr<float>(), (int)c, (int)part.size(0),
                          (int)ntiles);
}

at::Tensor bn_workspace(const BnPlan& p, const at::Tensor& like) {
  return at::empty({2 * p.partial_floats + p.grid},
                   like.options().dtype(at::kFloat));
}

// -> (out, mean, invstd, mask | None); running statistics updated in place
std::tuple<at::Tensor, at::Tensor, at::Tensor, c10::optional<at::Tensor>>
py_bn_act_forward(const at::Tensor& x, const c10::optional<at::Tensor>& identity,
                  const at::Tensor& weight, const at::Tensor& bias,
                  at::Tensor running_mean, at::Tensor running_var,
                  double momentum, double eps, bool relu,
                  const c10::optional<at::Tensor>& stats_part) {
  TORCH_CHECK(py_bn_eligible(x), "bn_act_forward: input is not eligible");
  const BnPlan p = bn_plan_of(x);
  const int64_t c = p.channels;
  if (identity.has_value())
    TORCH_CHECK(bn_tensor_ok(*identity) && identity->sizes() == x.sizes() &&
                    identity->device() == x.device(),
                "bn_act_forward: identity must match the input");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device().index());
  auto out = at::empty(x.sizes(), x.options(), at::MemoryFormat::ChannelsLast);
  auto stats = x.options().dtype(at::kFloat);
  auto mean = at::empty({c}, stats), invstd = at::empty({c}, stats);
  c10::optional<at::Tensor> mask;
  if (relu) mask = at::empty({x.numel() / 8}, x.options().dtype(at::kByte));
  auto part = bn_workspace(p, x);
  BnForwardArgs a;
  a.x = x.data_ptr();
  a.identity = identity.has_value() ? identity->data_ptr() : nullptr;
  a.weight = bn_channel_vec(weight, c, "weight");
  a.bias = bn_channel_vec(bias, c, "bias");
  a.running_mean = bn_channel_vec(running_mean, c, "running_mean");
  a.running_var = bn_channel_vec(running_var, c, "running_var");
  a.momentum = (float)momentum;
  a.eps = (float)eps;
  a.relu = relu;
  a.out = out.data_ptr();
  a.mean = mean.data_ptr<float>();
  a.invstd = invstd.data_ptr<float>();
  a.mask = relu ? mask->data_ptr<uint8_t>() : nullptr;
  a.part = part.data_ptr<float>();
  BnPartials ext;
  if (stats_part.has_value()) {
    ext = bn_external_partials(*stats_part, x);
    a.stats = &ext;
  }
  launch_bn_forward(
      p, a, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(
                x.device().index()).stream());
  return {out, mean, invstd, mask};
}

// -> (dx, dgamma, dbeta, didentity | None).  Without a mask the identity
// branch's gradient is dy itself and is returned as such.
std::tuple<at::Tensor, at::Tensor, at::Tensor, c10::optional<at::Tensor>>
py_bn_act_backward(at::Tensor dy, const at::Tensor& x, const at::Tensor& mean,
                   const at::Tensor& invstd, const at::Tensor& weight,
                   const c10::optional<at::Tensor>& mask, bool has_identity) {
  TORCH_CHECK(py_bn_eligible(x), "bn_act_backward: input is not eligible");
  const BnPlan p = bn_plan_of(x);
  const int64_t c = p.channels;
  TORCH_CHECK(dy.is_cuda() && dy.device() == x.device() &&
                  dy.scalar_type() == at::kBFloat16 && dy.sizes() == x.sizes(),
              "bn_act_backward: dy must match the input");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device().index());
  if (!bn_tensor_ok(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  if (!bn_tensor_ok(dy)) dy = dy.clone(at::MemoryFormat::ChannelsLast);
  if (mask.has_value())
    TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == at::kByte &&
                    mask->is_contiguous() && mask->numel() == x.numel() / 8,
                "bn_act_backward: mask must hold one bit per element");
  auto dx = at::empty(x.sizes(), x.options(), at::MemoryFormat::ChannelsLast);
  auto stats = x.options().dtype(at::kFloat);
  auto dgamma = at::empty({c}, stats), dbeta = at::empty({c}, stats);
  c10::optional<at::Tensor> didentity;
  if (has_identity)
    didentity = mask.has_value()
                    ? at::empty(x.sizes(), x.options(),
                                at::MemoryFormat::ChannelsLast)
                    : dy;
  auto part = bn_workspace(p, x);
  BnBackwardArgs a;
  a.dy = dy.data_ptr();
  a.x = x.data_ptr();
  a.mean = bn_channel_vec(mean, c, "mean");
  a.invstd = bn_channel_vec(invstd, c, "invstd");
  a.weight = bn_channel_vec(weight, c, "weight");
  a.mask = mask.has_value() ? mask->data_ptr<uint8_t>() : nullptr;
  a.dx = dx.data_ptr();
  a.didentity =
      has_identity && mask.has_value() ? didentity->data_ptr() : nullptr;
  a.dgamma = dgamma.data_ptr<float>();
  a.dbeta = dbeta.data_ptr<float>();
  a.part = part.data_ptr<float>();
  launch_bn_backward(
      p, a, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(
                x.device().index()).stream());
  return {dx, dgamma, dbeta, didentity};
}

hipStream_t bn_stream(const at::Tensor& x) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(x.device().index())
      .stream();
}

// dy as the kernels index it: dense channels_last, 16-byte aligned
at::Tensor bn_dense_dy(at::Tensor dy) {
  if (!bn_tensor_ok(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  if (!bn_tensor_ok(dy)) dy = dy.clone(at::MemoryFormat::ChannelsLast);
  return dy;
}

// relu(bn3(x3) + bn_d(xd)) -> (out, mean3, invstd3, meand, invstdd,
// mask | None); both pairs of running statistics updated in place
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
           c10::optional<at::Tensor>>
py_bn_act2_forward(const at::Tensor& x3, const at::Tensor& xd,
                   const at::Tensor& weight3, const at::Tensor& bias3,
                   at::Tensor running_mean3, at::Tensor running_var3,
                   double momentum3, double eps3, const at::Tensor& weightd,
                   const at::Tensor& biasd, at::Tensor running_meand,
                   at::Tensor running_vard, double momentumd, double epsd,
                   bool relu, const c10::optional<at::Tensor>& stats_part3,
                   const c10::optional<at::Tensor>& stats_partd) {
  TORCH_CHECK(py_bn_eligible(x3), "bn_act2_forward: input is not eligible");
  TORCH_CHECK(bn_tensor_ok(xd) && xd.sizes() == x3.sizes() &&
                  xd.device() == x3.device(),
              "bn_act2_forward: both inputs must have the same shape");
  const BnPlan p = bn_plan_of(x3);
  const int64_t c = p.channels;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x3.device().index());
  auto out = at::empty(x3.sizes(), x3.options(), at::MemoryFormat::ChannelsLast);
  auto stats = x3.options().dtype(at::kFloat);
  auto mean3 = at::empty({c}, stats), invstd3 = at::empty({c}, stats);
  auto meand = at::empty({c}, stats), invstdd = at::empty({c}, stats);
  c10::optional<at::Tensor> mask;
  if (relu) mask = at::empty({x3.numel() / 8}, x3.options().dtype(at::kByte));
  auto part = at::empty({2 * (2 * p.partial_floats + p.grid)}, stats);
  BnJoinArgs j{};
  j.a.x = x3.data_ptr();
  j.a.weight = bn_channel_vec(weight3, c, "weight");
  j.a.bias = bn_channel_vec(bias3, c, "bias");
  j.a.running_mean = bn_channel_vec(running_mean3, c, "running_mean");
  j.a.running_var = bn_channel_vec(running_var3, c, "running_var");
  j.a.momentum = (float)momentum3;
  j.a.eps = (float)eps3;
  j.a.mean = mean3.data_ptr<float>();
  j.a.invstd = invstd3.data_ptr<float>();
  j.b.x = xd.data_ptr();
  j.b.weight = bn_channel_vec(weightd, c, "identity weight");
  j.b.bias = bn_channel_vec(biasd, c, "identity bias");
  j.b.running_mean = bn_channel_vec(running_meand, c, "identity running_mean");
  j.b.running_var = bn_channel_vec(running_vard, c, "identity running_var");
  j.b.momentum = (float)momentumd;
  j.b.eps = (float)epsd;
  j.b.mean = meand.data_ptr<float>();
  j.b.invstd = invstdd.data_ptr<float>();
  j.relu = relu;
  j.out = out.data_ptr();
  j.mask = relu ? mask->data_ptr<uint8_t>() : nullptr;
  j.part = part.data_ptr<float>();
  BnPartials ext3, extd;
  if (stats_part3.has_value()) {
    ext3 = bn_external_partials(*stats_part3, x3);
    j.a.stats = &ext3;
  }
  if (stats_partd.has_value()) {
    extd = bn_external_partials(*stats_partd, xd);
    j.b.stats = &extd;
  }
  launch_bn_join_forward(p, j, bn_stream(x3));
  return {out, mean3, invstd3, meand, invstdd, mask};
}

// -> (dx3, dxd, dgamma3, dbeta3, dgammad, dbetad)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
           at::Tensor>
py_bn_act2_backward(at::Tensor dy, const at::Tensor& x3, const at::Tensor& xd,
                    const at::Tensor& mean3, const at::Tensor& invstd3,
                    const at::Tensor& weight3, const at::Tensor& meand,
                    const at::Tensor& invstdd, const at::Tensor& weightd,
                    const c10::optional<at::Tensor>& mask) {
  TORCH_CHECK(py_bn_eligible(x3), "bn_act2_backward: input is not eligible");
  TORCH_CHECK(bn_tensor_ok(xd) && xd.sizes() == x3.sizes() &&
                  xd.device() == x3.device(),
              "bn_act2_backward: both inputs must have the same shape");
  const BnPlan p = bn_plan_of(x3);
  const int64_t c = p.channels;
  TORCH_CHECK(dy.is_cuda() && dy.device() == x3.device() &&
                  dy.scalar_type() == at::kBFloat16 && dy.sizes() == x3.sizes(),
              "bn_act2_backward: dy must match the input");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x3.device().index());
  dy = bn_dense_dy(dy);
  if (mask.has_value())
    TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == at::kByte &&
                    mask->is_contiguous() && mask->numel() == x3.numel() / 8,
                "bn_act2_backward: mask must hold one bit per element");
  auto dx3 = at::empty(x3.sizes(), x3.options(), at::MemoryFormat::ChannelsLast);
  auto dxd = at::empty(x3.sizes(), x3.options(), at::MemoryFormat::ChannelsLast);
  auto stats = x3.options().dtype(at::kFloat);
  auto dgamma3 = at::empty({c}, stats), dbeta3 = at::empty({c}, stats);
  auto dgammad = at::empty({c}, stats), dbetad = at::empty({c}, stats);
  auto part = at::empty({3 * p.partial_floats}, stats);
  BnJoinArgs j{};
  j.a.x = x3.data_ptr();
  j.a.mean = bn_channel_vec(mean3, c, "mean");
  j.a.invstd = bn_channel_vec(invstd3, c, "invstd");
  j.a.weight = bn_channel_vec(weight3, c, "weight");
  j.a.dx = dx3.data_ptr();
  j.a.dgamma = dgamma3.data_ptr<float>();
  j.a.dbeta = dbeta3.data_ptr<float>();
  j.b.x = xd.data_ptr();
  j.b.mean = bn_channel_vec(meand, c, "identity mean");
  j.b.invstd = bn_channel_vec(invstdd, c, "identity invstd");
  j.b.weight = bn_channel_vec(weightd, c, "identity weight");
  j.b.dx = dxd.data_ptr();
  j.b.dgamma = dgammad.data_ptr<float>();
  j.b.dbeta = dbetad.data_ptr<float>();
  j.dy = dy.data_ptr();
  j.mask = mask.has_value() ? mask->data_ptr<uint8_t>() : nullptr;
  j.part = part.data_ptr<float>();
  launch_bn_join_backward(p, j, bn_stream(x3));
  return {dx3, dxd, dgamma3, dbeta3, dgammad, dbetad};
}

BnPoolPlan bn_pool_plan_of(const at::Tensor& x) {
  return bn_pool_plan(x.size(0), x.size(2), x.size(3), x.size(1));
}

// maxpool3x3/2/1(relu(bn(x))) -> (pooled, mean, invstd, arg); arg holds one
// byte per pooled element: the window position of its maximum
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
py_bn_act_pool_forward(const at::Tensor& x, const at::Tensor& weight,
                       const at::Tensor& bias, at::Tensor running_mean,
                       at::Tensor running_var, double momentum, double eps) {
  TORCH_CHECK(py_bn_eligible(x), "bn_act_pool_forward: input is not eligible");
  const BnPlan p = bn_plan_of(x);
  const BnPoolPlan g = bn_pool_plan_of(x);
  const int64_t c = p.channels;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device().index());
  auto out = at::empty({x.size(0), c, g.oh, g.ow}, x.options(),
                       at::MemoryFormat::ChannelsLast);
  auto arg = at::empty({x.size(0), c, g.oh, g.ow},
                       x.options().dtype(at::kByte),
                       at::MemoryFormat::ChannelsLast);
  auto stats = x.options().dtype(at::kFloat);
  auto mean = at::empty({c}, stats), invstd = at::empty({c}, stats);
  auto part = bn_workspace(p, x);
  BnPoolArgs a{};
  a.x = x.data_ptr();
  a.weight = bn_channel_vec(weight, c, "weight");
  a.bias = bn_channel_vec(bias, c, "bias");
  a.running_mean = bn_channel_vec(running_mean, c, "running_mean");
  a.running_var = bn_channel_vec(running_var, c, "running_var");
  a.momentum = (float)momentum;
  a.eps = (float)eps;
  a.mean = mean.data_ptr<float>();
  a.invstd = invstd.data_ptr<float>();
  a.out = out.data_ptr();
  a.arg = arg.data_ptr<uint8_t>();
  a.part = part.data_ptr<float>();
  launch_bn_pool_forward(p, g, a, bn_stream(x));
  return {out, mean, invstd, arg};
}

// -> (dx, dgamma, dbeta)
std::tuple<at::Tensor, at::Tensor, at::Tensor>
py_bn_act_pool_backward(at::Tensor dy, const at::Tensor& x,
                        const at::Tensor& mean, const at::Tensor& invstd,
                        const at::Tensor& weight, const at::Tensor& arg) {
  TORCH_CHECK(py_bn_eligible(x), "bn_act_pool_backward: input is not eligible");
  const BnPlan p = bn_plan_of(x);
  const BnPoolPlan g = bn_pool_plan_of(x);
  const int64_t c = p.channels;
  const std::vector<int64_t> pooled = {x.size(0), c, g.oh, g.ow};
  TORCH_CHECK(dy.is_cuda() && dy.device() == x.device() &&
                  dy.scalar_type() == at::kBFloat16 && dy.sizes() == at::IntArrayRef(pooled),
              "bn_act_pool_backward: dy must have the pooled shape");
  TORCH_CHECK(arg.is_cuda() && arg.device() == x.device() &&
                  arg.scalar_type() == at::kByte && arg.sizes() == at::IntArrayRef(pooled) &&
                  arg.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  reinterpret_cast<uintptr_t>(arg.data_ptr()) % 8 == 0,
              "bn_act_pool_backward: arg must be the forward's");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device().index());
  dy = bn_dense_dy(dy);
  auto dx = at::empty(x.sizes(), x.options(), at::MemoryFormat::ChannelsLast);
  auto stats = x.options().dtype(at::kFloat);
  auto dgamma = at::empty({c}, stats), dbeta = at::empty({c}, stats);
  auto part = bn_workspace(p, x);
  BnPoolArgs a{};
  a.x = x.data_ptr();
  a.mean = bn_channel_vec(mean, c, "mean");
  a.invstd = bn_channel_vec(invstd, c, "invstd");
  a.weight = bn_channel_vec(weight, c, "weight");
  a.arg = arg.data_ptr<uint8_t>();
  a.dy = dy.data_ptr();
  a.dx = dx.data_ptr();
  a.dgamma = dgamma.data_ptr<float>();
  a.dbeta = dbeta.data_ptr<float>();
  a.part = part.data_ptr<float>();
  launch_bn_pool_backward(p, g, a, bn_stream(x));
  return {dx, dgamma, dbeta};
}

// Test seam: the pooling geometry the stem kernels use, for one h x w image.
// -> (windows [oh*ow, 9], covers [h*w, 4, 2]): row o of `windows` holds the
// input pixel (ih*w + iw) each window position of pooled pixel o reads, -1
// for padding; row i of `covers` holds the (pooled pixel, window position)
// pairs the backward visits for input pixel i, in that order, -1 beyond them.
std::tuple<at::Tensor, at::Tensor> py_bn_pool_geometry(int64_t h, int64_t w) {
  TORCH_CHECK(h >= 1 && w >= 1 && h * w <= kBnMaxRows, "bn_pool_geometry: bad");
  const BnPoolPlan g = bn_pool_plan(1, h, w, 8);
  auto opt = at::TensorOptions().dtype(at::kLong);
  auto windows = at::full({(int64_t)g.oh * g.ow, 9}, -1, opt);
  auto covers = at::full({h * w, 4, 2}, -1, opt);
  int64_t* wi = windows.data_ptr<int64_t>();
  int64_t* co = covers.data_ptr<int64_t>();
  for (int oh = 0; oh < g.oh; oh++)
    for (int ow = 0; ow < g.ow; ow++)
      for (int k = 0; k < 9; k++) {
        const int ih = pool_in(oh, k / 3), iw = pool_in(ow, k % 3);
        if (ih >= 0 && ih < g.h && iw >= 0 && iw < g.w)
          wi[((int64_t)oh * g.ow + ow) * 9 + k] = (int64_t)ih * g.w + iw;
      }
  for (int ih = 0; ih < g.h; ih++)
    for (int iw = 0; iw < g.w; iw++) {
      int n = 0;
      for (int oh = pool_cover_lo(ih); oh <= pool_cover_hi(ih, g.oh); oh++)
        for (int ow = pool_cover_lo(iw); ow <= pool_cover_hi(iw, g.ow); ow++) {
          int64_t* e = co + (((int64_t)ih * g.w + iw) * 4 + n++) * 2;
          e[0] = (int64_t)oh * g.ow + ow;
          e[1] = pool_k(ih, oh) * 3 + pool_k(iw, ow);
        }
    }
  return {windows, covers};
}

py::dict py_bn_plan(int64_t rows, int64_t channels) {
  const BnPlan p = bn_plan(rows, channels);
  py::dict d;
  d["eligible"] = p.eligible;
  d["threads"] = kBnThreads;
  d["cgs"] = p.cgs;
  d["tile_cgs"] = p.tc;
  d["ctiles"] = p.ctiles;
  d["rows_per_iter"] = p.rln;
  d["splits"] = p.splits;
  d["grid"] = p.grid;
  d["rows_per_thread"] = p.rows_per_thread;
  d["partial_floats"] = p.partial_floats;
  return d;
}

// Test seam: replay the kernels' sweep on the host.  Row t of the result is
// thread t % 256 of workgroup t / 256: the vector indices it visits in order,
// -1 once it has run out of rows.
at::Tensor py_bn_sweep_indices(int64_t rows, int64_t channels) {
  const BnPlan p = bn_plan(rows, channels);
  TORCH_CHECK(p.eligible, "bn_sweep_indices: shape is not eligible");
  auto out = at::full({(int64_t)p.grid * kBnThreads, p.rows_per_thread + 1},
                      -1, at::TensorOptions().dtype(at::kLong));
  int64_t* o = out.data_ptr<int64_t>();
  const int64_t width = p.rows_per_thread + 1;
  for (int wg = 0; wg < p.grid; wg++)
    for (int tid = 0; tid < kBnThreads; tid++) {
      const BnSweep sw = bn_sweep(p, wg, tid);
      int64_t k = 0;
      for (int64_t r = sw.row; r < p.rows; r += sw.stride, k++) {
        TORCH_CHECK(k < width, "bn_sweep_indices: run longer than planned");
        o[((int64_t)wg * kBnThreads + tid) * width + k] = bn_vec(p, r, sw.cg);
      }
    }
  return out;
}

// Test seam: the partial-buffer offsets workgroup `wg` writes (per reduction),
// as the kernels compute them.
std::vector<int64_t> py_bn_partial_offsets(int64_t rows, int64_t channels,
                                           int wg) {
  const BnPlan p = bn_plan(rows, channels);
  TORCH_CHECK(p.eligible && wg >= 0 && wg < p.grid, "bn_partial_offsets: bad");
  std::vector<int64_t> offs;
  for (int tid = 0; tid < p.tc; tid++) {
    const BnSweep sw = bn_sweep(p, wg, tid);
    const int64_t o = bn_partial_offset(p, wg, sw.cg);
    for (int j = 0; j < 8; j++) offs.push_back(o + j);
  }
  return offs;
}

// ---- 1x1 convolution with statistics (conv1x1_plan.h) ----------------------

// R of a channels_last activation
int64_t rows_of(const at::Tensor& t) { return t.numel() / t.size(1); }

// A dense, 16-byte aligned bf16 [N, K, 1, 1] weight on the device of `like`.
bool conv_weight_ok(const at::Tensor& weight, const at::Tensor& like) {
  return weight.is_cuda() && weight.device() == like.device() &&
         weight.scalar_type() == at::kBFloat16 && weight.dim() == 4 &&
         weight.size(2) == 1 && weight.size(3) == 1 &&
         weight.is_contiguous() &&
         reinterpret_cast<uintptr_t>(weight.data_ptr()) % 16 == 0;
}

// What the kernel takes: a bf16 channels_last activation as for the BatchNorm
// kernels and the convolution's weight, K wide.
bool py_conv1x1_eligible(const at::Tensor& x, const at::Tensor& weight) {
  return bn_tensor_ok(x) && conv_weight_ok(weight, x) &&
         weight.size(1) == x.size(1) &&
         conv1x1_plan(rows_of(x), x.size(1), weight.size(0)).eligible;
}

// conv2d(x, weight) for a 1x1 / stride 1 convolution -> (y, part); part holds
// the BatchNorm partials of y for bn_act_forward / bn_act2_forward
std::tuple<at::Tensor, at::Tensor> py_conv1x1_stats(const at::Tensor& x,
                                                    const at::Tensor& weight,
                                                    int64_t max_workgroups) {
  TORCH_CHECK(max_workgroups >= 0, "conv1x1_stats: max_workgroups >= 0");
  TORCH_CHECK(py_conv1x1_eligible(x, weight),
              "conv1x1_stats: input or weight is not eligible");
  const Conv1x1Plan p =
      conv1x1_plan(rows_of(x), x.size(1), weight.size(0), max_workgroups);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device().index());
  auto y = at::empty({x.size(0), p.n, x.size(2), x.size(3)}, x.options(),
                     at::MemoryFormat::ChannelsLast);
  auto part = at::empty({p.splits, p.pstride}, x.options().dtype(at::kFloat));
  launch_conv1x1_stats(p, x.data_ptr(), weight.data_ptr(), y.data_ptr(),
                       part.data_ptr<float>(), bn_stream(x));
  return {y, part};
}

// The keys the forward's and the backward-data plan share.  For the backward
// tile_channels / ntiles are over dX's K channels, k_chunk(s) over dY's N.
py::dict conv1x1_plan_dict(const Conv1x1Plan& p) {
  py::dict d;
  d["eligible"] = p.eligible;
  d["native"] = p.native;
  d["threads"] = kConvThreads;
  d["tile_rows"] = kConvTileRows;
  d["mfma_tiles"] = p.nt;
  d["tile_channels"] = p.bn;
  d["ntiles"] = p.ntiles;
  d["k_chunk"] = p.kc;
  d["k_chunks"] = p.nchunks;
  d["resident"] = p.resident;
  d["row_tiles"] = p.row_tiles;
  d["splits"] = p.splits;
  d["grid"] = p.grid;
  d["tiles_per_split"] = p.tiles_per_split;
  d["lds_bytes"] = p.lds_bytes;
  return d;
}

py::dict py_conv1x1_plan(int64_t rows, int64_t k, int64_t n,
                         int64_t max_workgroups) {
  const Conv1x1Plan p = conv1x1_plan(rows, k, n, max_workgroups);
  py::dict d = conv1x1_plan_dict(p);
  d["run"] = p.run;
  d["partial_stride"] = p.pstride;
  d["partial_floats"] = p.partial_floats;
  return d;
}

// Test seam: replay the kernel's tile walk on the host.  Entry [wg, i] holds
// (row0, row1, n0, n1) of the i-th tile of workgroup wg: the rows it stores
// and counts and its channels; -1 once it has run out of tiles.
at::Tensor conv1x1_walk_of(const Conv1x1Plan& p) {
  auto out = at::full({p.grid, p.tiles_per_split, 4}, -1,
                      at::TensorOptions().dtype(at::kLong));
  int64_t* o = out.data_ptr<int64_t>();
  for (int wg = 0; wg < p.grid; wg++) {
    const int split = conv1x1_split(p, wg), nt = conv1x1_ntile(p, wg);
    for (int i = 0; i < p.tiles_per_split; i++) {
      const int t = conv1x1_tile(p, split, i);
      if (t >= p.row_tiles) break;
      int64_t* e = o + ((int64_t)wg * p.tiles_per_split + i) * 4;
      e[0] = (int64_t)t * kConvTileRows;
      e[1] = std::min<int64_t>(e[0] + kConvTileRows, p.rows);
      e[2] = (int64_t)nt * p.bn;
      e[3] = e[2] + p.bn;
    }
  }
  return out;
}

at::Tensor py_conv1x1_walk(int64_t rows, int64_t k, int64_t n,
                           int64_t max_workgroups) {
  const Conv1x1Plan p = conv1x1_plan(rows, k, n, max_workgroups);
  TORCH_CHECK(p.eligible, "conv1x1_walk: shape is not eligible");
  return conv1x1_walk_of(p);
}

// ---- 1x1 convolution backward-data with the skip gradient added ------------

// dy as the BatchNorm kernels take it, the convolution's dense bf16
// [N, K, 1, 1] weight, and a skip gradient, if any, of dX's shape and layout.
bool py_conv1x1_bwd_eligible(const at::Tensor& dy, const at::Tensor& weight,
                             const c10::optional<at::Tensor>& skip) {
  if (!(bn_tensor_ok(dy) && conv_weight_ok(weight, dy) &&
        weight.size(0) == dy.size(1) &&
        conv1x1_bwd_plan(rows_of(dy), weight.size(1), weight.size(0),
                         skip.has_value())
            .eligible))
    return false;
  if (!skip.has_value()) return true;
  const at::Tensor& s = *skip;
  return s.dim() == 4 && s.size(0) == dy.size(0) &&
         s.size(1) == weight.size(1) && s.size(2) == dy.size(2) &&
         s.size(3) == dy.size(3) && s.device() == dy.device() &&
         bn_tensor_ok(s);
}

// Gradient of conv2d(x, weight) for x, plus `skip`: (dy, weight, skip) -> dx
at::Tensor py_conv1x1_bwd_data(const at::Tensor& dy, const at::Tensor& weight,
                               const c10::optional<at::Tensor>& skip,
                               int64_t max_workgroups) {
  TORCH_CHECK(max_workgroups >= 0, "conv1x1_bwd_data: max_workgroups >= 0");
  TORCH_CHECK(py_conv1x1_bwd_eligible(dy, weight, skip),
              "conv1x1_bwd_data: dy, weight or skip is not eligible");
  const Conv1x1Plan p =
      conv1x1_bwd_plan(rows_of(dy), weight.size(1), weight.size(0),
                       skip.has_value(), max_workgroups);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dy.device().index());
  auto dx = at::empty({dy.size(0), p.n, dy.size(2), dy.size(3)}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  launch_conv1x1_bwd_data(p, dy.data_ptr(), weight.data_ptr(),
                          skip.has_value() ? skip->data_ptr() : nullptr,
                          dx.data_ptr(), bn_stream(dy));
  return dx;
}

py::dict py_conv1x1_bwd_plan(int64_t rows, int64_t k, int64_t n, bool with_add,
                             int64_t max_workgroups) {
  return conv1x1_plan_dict(
      conv1x1_bwd_plan(rows, k, n, with_add, max_workgroups));
}

at::Tensor py_conv1x1_bwd_walk(int64_t rows, int64_t k, int64_t n,
                               bool with_add, int64_t max_workgroups) {
  const Conv1x1Plan p =
      conv1x1_bwd_plan(rows, k, n, with_add, max_workgroups);
  TORCH_CHECK(p.eligible, "conv1x1_bwd_walk: shape is not eligible");
  return conv1x1_walk_of(p);
}

// ---- the tiled walk of both (conv1x1_tiled_plan) ---------------------------

std::tuple<at::Tensor, at::Tensor> py_conv1x1_tiled_stats(
    const at::Tensor& x, const at::Tensor& weight, int64_t max_workgroups) {
  TORCH_CHECK(max_workgroups >= 0, "conv1x1_tiled_stats: max_workgroups >= 0");
  TORCH_CHECK(py_conv1x1_eligible(x, weight),
              "conv1x1_tiled_stats: input or weight is not eligible");
  const Conv1x1Plan p = conv1x1_tiled_plan(rows_of(x), x.size(1),
                                           weight.size(0), max_workgroups);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device().index());
  auto y = at::empty({x.size(0), p.n, x.size(2), x.size(3)}, x.options(),
                     at::MemoryFormat::ChannelsLast);
  auto part = at::empty({p.splits, p.pstride}, x.options().dtype(at::kFloat));
  launch_conv1x1_tiled_stats(p, x.data_ptr(), weight.data_ptr(), y.data_ptr(),
                             part.data_ptr<float>(), bn_stream(x));
  return {y, part};
}

at::Tensor py_conv1x1_tiled_bwd_data(const at::Tensor& dy,
                                     const at::Tensor& weight,
                                     const c10::optional<at::Tensor>& skip,
                                     int64_t max_workgroups) {
  TORCH_CHECK(max_workgroups >= 0,
              "conv1x1_tiled_bwd_data: max_workgroups >= 0");
  TORCH_CHECK(py_conv1x1_bwd_eligible(dy, weight, skip),
              "conv1x1_tiled_bwd_data: dy, weight or skip is not eligible");
  const Conv1x1Plan p =
      conv1x1_tiled_bwd_plan(rows_of(dy), weight.size(1), weight.size(0),
                             skip.has_value(), max_workgroups);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dy.device().index());
  auto dx = at::empty({dy.size(0), p.n, dy.size(2), dy.size(3)}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  launch_conv1x1_tiled_bwd_data(p, dy.data_ptr(), weight.data_ptr(),
                                skip.has_value() ? skip->data_ptr() : nullptr,
                                dx.data_ptr(), bn_stream(dy));
  return dx;
}

py::dict conv1x1_tiled_plan_dict(const Conv1x1Plan& p) {
  py::dict d = conv1x1_plan_dict(p);
  d["tile_rows"] = kTiledTileRows;
  return d;
}

py::dict py_conv1x1_tiled_plan(int64_t rows, int64_t k, int64_t n,
                               int64_t max_workgroups) {
  const Conv1x1Plan p = conv1x1_tiled_plan(rows, k, n, max_workgroups);
  py::dict d = conv1x1_tiled_plan_dict(p);
  d["run"] = p.run;
  d["partial_stride"] = p.pstride;
  d["partial_floats"] = p.partial_floats;
  return d;
}

py::dict py_conv1x1_tiled_bwd_plan(int64_t rows, int64_t k, int64_t n,
                                   bool with_add, int64_t max_workgroups) {
  return conv1x1_tiled_plan_dict(
      conv1x1_tiled_bwd_plan(rows, k, n, with_add, max_workgroups));
}

// Test seam: conv1x1_walk_of for the tiled walk's 256-row tiles and its
// workgroup order.
at::Tensor conv1x1_tiled_walk_of(const Conv1x1Plan& p) {
  TORCH_CHECK(p.eligible, "conv1x1_tiled_walk: shape is not eligible");
  auto out = at::full({p.grid, p.tiles_per_split, 4}, -1,
                      at::TensorOptions().dtype(at::kLong));
  int64_t* o = out.data_ptr<int64_t>();
  for (int wg = 0; wg < p.grid; wg++) {
    const int split = conv1x1_tiled_split(p, wg);
    const int nt = conv1x1_tiled_ntile(p, wg);
    for (int i = 0; i < p.tiles_per_split; i++) {
      const int t = conv1x1_tile(p, split, i);
      if (t >= p.row_tiles) break;
      int64_t* e = o + ((int64_t)wg * p.tiles_per_split + i) * 4;
      e[0] = (int64_t)t * kTiledTileRows;
      e[1] = std::min<int64_t>(e[0] + kTiledTileRows, p.rows);
      e[2] = (int64_t)nt * p.bn;
      e[3] = e[2] + p.bn;
    }
  }
  return out;
}

at::Tensor py_conv1x1_tiled_walk(int64_t rows, int64_t k, int64_t n,
                                 int64_t max_workgroups) {
  return conv1x1_tiled_walk_of(conv1x1_tiled_plan(rows, k, n, max_workgroups));
}

at::Tensor py_conv1x1_tiled_bwd_walk(int64_t rows, int64_t k, int64_t n,
                                     bool with_add, int64_t max_workgroups) {
  return conv1x1_tiled_walk_of(
      conv1x1_tiled_bwd_plan(rows, k, n, with_add, max_workgroups));
}

// ---- 1x1 convolution backward-weights --------------------------------------

// dy and x as the BatchNorm kernels take them, of one batch and image size.
bool py_conv1x1_wrw_eligible(const at::Tensor& dy, const at::Tensor& x) {
  return bn_tensor_ok(dy) && bn_tensor_ok(x) && x.device() == dy.device() &&
         x.size(0) == dy.size(0) && x.size(2) == dy.size(2) &&
         x.size(3) == dy.size(3) &&
         conv1x1_wrw_plan(rows_of(dy), x.size(1), dy.size(1)).eligible;
}

// Gradient of conv2d(x, weight) for the [N, K, 1, 1] weight: (dy, x) -> dw
at::Tensor py_conv1x1_wrw(const at::Tensor& dy, const at::Tensor& x,
                          int64_t max_workgroups) {
  TORCH_CHECK(max_workgroups >= 0, "conv1x1_wrw: max_workgroups >= 0");
  TORCH_CHECK(py_conv1x1_wrw_eligible(dy, x),
              "conv1x1_wrw: dy or x is not eligible");
  const Conv1x1WrwPlan p =
      conv1x1_wrw_plan(rows_of(dy), x.size(1), dy.size(1), max_workgroups);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dy.device().index());
  // the layout the stock weight gradient has: channels_last, which for a
  // 1x1 filter is the same dense [N, K] memory
  auto dw = at::empty({p.n, p.k, 1, 1}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  auto part = at::empty({p.splits, p.n, p.k}, dy.options().dtype(at::kFloat));
  launch_conv1x1_wrw(p, dy.data_ptr(), x.data_ptr(), part.data_ptr<float>(),
                     dw.data_ptr(), bn_stream(dy));
  return dw;
}

py::dict py_conv1x1_wrw_plan(int64_t rows, int64_t k, int64_t n,
                             int64_t max_workgroups) {
  const Conv1x1WrwPlan p = conv1x1_wrw_plan(rows, k, n, max_workgroups);
  py::dict d;
  d["eligible"] = p.eligible;
  d["native"] = p.native;
  d["threads"] = kConvThreads;
  d["bn"] = p.bn;
  d["bk"] = p.bk;
  d["ntiles_n"] = p.ntiles_n;
  d["ntiles_k"] = p.ntiles_k;
  d["chunk_rows"] = p.chunk_rows;
  d["row_chunks"] = p.row_chunks;
  d["splits"] = p.splits;
  d["grid"] = p.grid;
  d["chunks_per_split"] = p.chunks_per_split;
  d["lds_bytes"] = p.lds_bytes;
  d["partial_floats"] = p.partial_floats;
  return d;
}

// Test seam: the kernel's walk replayed on the host.  Entry [wg, i] holds
// (n0, k0, split, row0, row1) of the i-th chunk of workgroup wg: the corner
// of its tile of dW, the plane of the partials it writes and the rows it
// sums; -1 once it has run out of chunks.
at::Tensor py_conv1x1_wrw_walk(int64_t rows, int64_t k, int64_t n,
                               int64_t max_workgroups) {
  const Conv1x1WrwPlan p = conv1x1_wrw_plan(rows, k, n, max_workgroups);
  TORCH_CHECK(p.eligible, "conv1x1_wrw_walk: shape is not eligible");
  auto out = at::full({p.grid, p.chunks_per_split, 5}, -1,
                      at::TensorOptions().dtype(at::kLong));
  int64_t* o = out.data_ptr<int64_t>();
  for (int wg = 0; wg < p.grid; wg++) {
    const int tile = conv1x1_wrw_tile(p, wg), split = conv1x1_wrw_split(p, wg);
    for (int i = 0; i < p.chunks_per_split; i++) {
      const int ch = conv1x1_wrw_chunk(p, split, i);
      if (ch >= p.row_chunks) break;
      int64_t* e = o + ((int64_t)wg * p.chunks_per_split + i) * 5;
      e[0] = (int64_t)(tile / p.ntiles_k) * p.bn;
      e[1] = (int64_t)(tile % p.ntiles_k) * p.bk;
      e[2] = split;
      e[3] = (int64_t)ch * p.chunk_rows;
      e[4] = std::min<int64_t>(e[3] + p.chunk_rows, p.rows);
    }
  }
  return out;
}

// ---- 1x1 convolution backward-weights, ring ---------------------------------

bool py_conv1x1_wrw_ring_eligible(const at::Tensor& dy, const at::Tensor& x) {
  return py_conv1x1_wrw_eligible(dy, x) &&
         conv1x1_wrw_ring_plan(rows_of(dy), x.size(1), dy.size(1)).eligible;
}

// as py_conv1x1_wrw, by conv1x1_wrw_ring
at::Tensor py_conv1x1_wrw_ring(const at::Tensor& dy, const at::Tensor& x,
                               int64_t max_workgroups) {
  TORCH_CHECK(max_workgroups >= 0, "conv1x1_wrw_ring: max_workgroups >= 0");
  TORCH_CHECK(py_conv1x1_wrw_ring_eligible(dy, x),
              "conv1x1_wrw_ring: dy or x is not eligible");
  const Conv1x1WrwRingPlan p = conv1x1_wrw_ring_plan(
      rows_of(dy), x.size(1), dy.size(1), max_workgroups);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dy.device().index());
  auto dw = at::empty({p.n, p.k, 1, 1}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  auto part = at::empty({p.splits, p.n, p.k}, dy.options().dtype(at::kFloat));
  launch_conv1x1_wrw_ring(p, dy.data_ptr(), x.data_ptr(),
                          part.data_ptr<float>(), dw.data_ptr(),
                          bn_stream(dy));
  return dw;
}

py::dict py_conv1x1_wrw_ring_plan(int64_t rows, int64_t k, int64_t n,
                                  int64_t max_workgroups) {
  const Conv1x1WrwRingPlan p =
      conv1x1_wrw_ring_plan(rows, k, n, max_workgroups);
  py::dict d;
  d["eligible"] = p.eligible;
  d["native"] = p.native;
  d["threads"] = kConvThreads;
  d["bn"] = p.bn;
  d["bk"] = p.bk;
  d["ntiles_n"] = p.ntiles_n;
  d["ntiles_k"] = p.ntiles_k;
  d["chunk_rows"] = p.chunk_rows;
  d["row_chunks"] = p.row_chunks;
  d["stages"] = p.stages;
  d["stage_bytes"] = p.stage_bytes;
  d["splits"] = p.splits;
  d["grid"] = p.grid;
  d["chunks_per_split"] = p.chunks_per_split;
  d["lds_bytes"] = p.lds_bytes;
  d["partial_floats"] = p.partial_floats;
  return d;
}

// Test seams.  The walk as py_conv1x1_wrw_walk ...
at::Tensor py_conv1x1_wrw_ring_walk(int64_t rows, int64_t k, int64_t n,
                                    int64_t max_workgroups) {
  const Conv1x1WrwRingPlan p =
      conv1x1_wrw_ring_plan(rows, k, n, max_workgroups);
  TORCH_CHECK(p.eligible, "conv1x1_wrw_ring_walk: shape is not eligible");
  auto out = at::full({p.grid, p.chunks_per_split, 5}, -1,
                      at::TensorOptions().dtype(at::kLong));
  int64_t* o = out.data_ptr<int64_t>();
  for (int wg = 0; wg < p.grid; wg++) {
    const int tile = conv1x1_wrw_tile(p, wg), split = conv1x1_wrw_split(p, wg);
    for (int i = 0; i < p.chunks_per_split; i++) {
      const int ch = conv1x1_wrw_chunk(p, split, i);
      if (ch >= p.row_chunks) break;
      int64_t* e = o + ((int64_t)wg * p.chunks_per_split + i) * 5;
      e[0] = (int64_t)(tile / p.ntiles_k) * p.bn;
      e[1] = (int64_t)(tile % p.ntiles_k) * p.bk;
      e[2] = split;
      e[3] = (int64_t)ch * p.chunk_rows;
      e[4] = std::min<int64_t>(e[3] + p.chunk_rows, p.rows);
    }
  }
  return out;
}

// ... and the fill of one stage replayed on the host.  Entry [operand, wave,
// j, lane] holds (LDS byte, row of the stage, first channel of the tile) of
// the 16 bytes that lane `lane` of instruction j of `wave` moves for dY
// (operand 0) or X (operand 1) into stage `slot`; -1 where the operand has
// fewer instructions than the other.
at::Tensor py_conv1x1_wrw_ring_fill(int64_t rows, int64_t k, int64_t n,
                                    int64_t slot) {
  const Conv1x1WrwRingPlan p = conv1x1_wrw_ring_plan(rows, k, n);
  TORCH_CHECK(p.eligible, "conv1x1_wrw_ring_fill: shape is not eligible");
  TORCH_CHECK(slot >= 0 && slot < p.stages, "conv1x1_wrw_ring_fill: slot");
  const int waves = kConvThreads / 64;
  const int most = p.chunk_rows * std::max(p.bn, p.bk) / 2048;
  auto out = at::full({2, waves, most, 64, 3}, -1,
                      at::TensorOptions().dtype(at::kLong));
  int64_t* o = out.data_ptr<int64_t>();
  for (int op = 0; op < 2; op++) {
    const int c = op ? p.bk : p.bn;
    for (int wave = 0; wave < waves; wave++)
      for (int j = 0; j < p.chunk_rows * c / 2048; j++)
        for (int lane = 0; lane < 64; lane++) {
          const WrwImageSlot s = conv1x1_wrw_image_slot(
              c, conv1x1_wrw_ring_piece(wave, j) + 16 * lane);
          int64_t* e = o + ((((int64_t)op * waves + wave) * most + j) * 64 +
                            lane) * 3;
          e[0] = conv1x1_wrw_ring_lds_base(p, (int)slot, op, wave, j) +
                 16 * lane;
          e[1] = s.row;
          e[2] = s.channel;
        }
  }
  return out;
}

void py_register_layer(int64_t bucket_idx, int64_t layer_idx, int64_t numel,
                       int64_t bits, int64_t bucket_size) {
  Registry::get().register_layer((int)bucket_idx, (int)layer_idx, numel,
                                 (int)bits, (int)bucket_size);
}

void py_set_bits(int64_t bucket_idx, int64_t layer_idx, int64_t bits) {
  Registry::get().set_bits((int)bucket_idx, (int)layer_idx, (int)bits);
}

void py_set_bucket(int64_t bucket_idx, int64_t layer_idx,
                   int64_t bucket_size) {
  Registry::get().set_bucket_size((int)bucket_idx, (int)layer_idx,
                                  (int)bucket_size);
}

}  // namespace
}  // namespace cgx

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  py::class_<cgx::ProcessGroupCGX,
             c10::intrusive_ptr<cgx::ProcessGroupCGX>, c10d::Backend>(
      m, "ProcessGroupCGX")
      .def(py::init<c10::intrusive_ptr<c10d::Store>, int, int,
                    c10::intrusive_ptr<c10d::Backend>>(),
           py::arg("store"), py::arg("rank"), py::arg("size"),
           py::arg("cpu_delegate") = nullptr);

  m.def("register_layer", &cgx::py_register_layer, py::arg("bucket_idx"),
        py::arg("layer_idx"), py::arg("layer_numel"), py::arg("bits"),
        py::arg("bucket_size"));
  m.def("set_quantization_bits", &cgx::py_set_bits);
  m.def("set_quantization_bucket_size", &cgx::py_set_bucket);
  m.def("clear_registry", [] { cgx::Registry::get().clear(); });
  m.def("registry_match",
        [](int64_t numel, int64_t key) {
          // test seam for Registry::next: key is an opaque bucket-storage
          // identity (the engine passes the flat tensor's data_ptr)
          cgx::Registry::BucketInfo info;
          const bool ok = cgx::Registry::get().next(
              numel, reinterpret_cast<const void*>(key), &info);
          return py::make_tuple(ok, ok ? info.idx : -1);
        },
        py::arg("numel"), py::arg("key") = 0);
  m.def("registry_snapshot", [] {
    // [(bucket_idx, [numels], [(bits, bucket_size)])] in registration order
    py::list out;
    auto& reg = cgx::Registry::get();
    for (const auto& b : reg.snapshot()) {
      py::list numels, cfgs;
      for (auto n : b.numels) numels.append(n);
      for (const auto& c : b.cfgs)
        cfgs.append(py::make_tuple(c.bits, c.bucket_size));
      out.append(py::make_tuple(b.idx, numels, cfgs));
    }
    return out;
  });

  m.def("parse_engine_config", [] {
    // test seam: the env-derived engine configuration, as each Engine
    // re-reads it per bucket (inner_ring/cross_ring select the reduction
    // algorithm for the intra-node vs cross-node engine independently)
    auto c = cgx::EngineConfig::from_env();
    py::dict d;
    d["fusion_bytes"] = c.fusion_bytes;
    d["min_elems"] = c.min_elems;
    d["default_bits"] = c.default_bits;
    d["default_bucket"] = c.default_bucket;
    d["stochastic"] = c.stochastic;
    d["inner_ring"] = c.ring;
    d["cross_ring"] = c.cross_ring;
    d["debug_a2a"] = c.debug_a2a;
    d["fake_ratio"] = c.fake_ratio;
    d["skip_incomplete"] = c.skip_incomplete;
    d["dummy"] = c.dummy;
    d["intra_compress"] = c.intra_compress;
    d["intra_broadcast"] = c.intra_broadcast;
    d["error_feedback"] = c.error_feedback;
    return d;
  });
  m.def("env_flag", &cgx::env_flag, py::arg("name"),
        py::arg("default") = false,
        "Test seam: the textual boolean parser (only \"0\" is false).");
  m.def("env_int", &cgx::env_int, py::arg("name"), py::arg("default"),
        "Test seam: the numeric parser behind the `!= 0` booleans.");
  m.def("loopback_allreduce", &cgx::py_loopback_allreduce, py::arg("buckets"),
        "Run Reducer::allreduce (flat) at world_size=len(buckets) on one GPU "
        "via the loopback transport; buckets[r] is rank r's flat bucket "
        "tensor, reduced in place.");
  m.def("loopback_broadcast", &cgx::py_loopback_broadcast, py::arg("tensors"),
        py::arg("root") = 0,
        "Run the production Engine::broadcast at world_size=len(tensors) on "
        "one GPU via the loopback transport.");
  m.def("loopback_allreduce_multi", &cgx::py_loopback_allreduce_multi,
        py::arg("steps"),
        "Multiple allreduce steps on persistent engines (steps[s][r] = rank "
        "r's bucket at step s, reduced in place); error-feedback residuals "
        "carry across steps.");
  m.def("loopback_hierarchical", &cgx::py_loopback_hierarchical,
        py::arg("buckets"), py::arg("local_size"),
        "Run Reducer::allreduce, the backend's per-bucket call, for "
        "n_nodes*local_size ranks on one GPU via loopback transports: intra "
        "allreduce -> leader cross reduction -> intra broadcast, or the "
        "flat path under CGX_INTRA_BROADCAST=0.");
  m.def("loopback_collective", &cgx::py_loopback_collective, py::arg("name"),
        py::arg("inputs"), py::arg("outputs"), py::arg("root") = 0,
        py::arg("in_splits") = std::vector<std::vector<int64_t>>{},
        py::arg("out_splits") = std::vector<std::vector<int64_t>>{},
        "Run one of the backend's p2p collectives (allgather, gather, "
        "scatter, alltoall, alltoall_base) at world_size=len(inputs) on one "
        "GPU via the loopback transport; inputs[r] / outputs[r] are rank r's "
        "tensor lists, in_splits[r] / out_splits[r] its alltoall_base splits.");
  m.def("quantize", &cgx::py_quantize, py::arg("x"), py::arg("bits"),
        py::arg("bucket_size"), py::arg("stochastic") = false,
        py::arg("seed") = 0, py::arg("skip_incomplete") = false,
        py::arg("feedback") = py::none());
  m.def("quantize_slices", &cgx::py_quantize_slices, py::arg("xs"),
        py::arg("bits"), py::arg("bucket_sizes"), py::arg("stochastic"),
        py::arg("seed"), py::arg("skip_incomplete") = false,
        "Test seam: compress several 1-D CUDA tensors through one "
        "route_quantize call; launch group k runs with seed + k.");
  m.def("dequantize", &cgx::py_dequantize, py::arg("comp"), py::arg("out"),
        py::arg("bits"), py::arg("bucket_size"), py::arg("add") = false,
        py::arg("skip_incomplete") = false);
  m.def("dequantize_multi", &cgx::py_dequantize_multi, py::arg("comp"),
        py::arg("out"), py::arg("bits"), py::arg("bucket_size"),
        py::arg("add") = false);
  m.def("compute_topology",
        [](const c10::intrusive_ptr<c10d::Store>& store, int rank, int size,
           const std::string& hostname) {
          auto t = cgx::compute_topology(store, rank, size, hostname);
          return std::make_tuple(t.node_id, t.local_rank, t.local_size,
                                 t.n_nodes, t.uniform);
        },
        "Exchange hostnames through the store -> (node_id, local_rank, "
        "local_size, n_nodes, uniform)");
  m.def("buffer_size", &cgx::py_buffer_size, py::arg("n"), py::arg("dtype"),
        py::arg("bits"), py::arg("bucket_size"),
        py::arg("skip_incomplete") = false);
  m.def("partition", &cgx::py_partition);
  m.def("plan_bucket", &cgx::py_plan_bucket, py::arg("layer_numels"),
        py::arg("layer_cfgs"), py::arg("dtype"), py::arg("fusion_bytes"),
        py::arg("min_elems"), py::arg("fake_ratio") = 1.0,
        py::arg("dummy") = false,
        "Test seam: the bucket plan for layers laid out back to back from "
        "byte offset 0 -> (uncomp [(byte_off, count)], chunks [[(byte_off, "
        "numel, bits, bucket)]]).");
  m.def("plan_chunk", &cgx::py_plan_chunk, py::arg("views"), py::arg("dtype"),
        py::arg("ws"), py::arg("skip_incomplete") = false,
        "Test seam: the rank plan of one chunk [(byte_off, numel, bits, "
        "bucket)] -> (offs, szs, comp, rs [[(byte_off, n, bits, bucket, "
        "comp_off, skip_incomplete, fb_off)]]).");
  m.def("route_quantize", &cgx::py_route_quantize, py::arg("slices"),
        "Test seam: the launch router's quantize plan for "
        "[(in, out, fb, n, bits, bucket, skip_incomplete)] (pointers as "
        "ints) -> [(bits, kind, descs, cum, any_residual, max_gpl)].");
  m.def("route_dequantize", &cgx::py_route_dequantize, py::arg("slices"),
        py::arg("dtype"), py::arg("src_stride") = 0, py::arg("nsrc") = 1,
        py::arg("add") = false,
        "Test seam: the launch router's dequantize plan for "
        "[(in, out, n, bits, bucket, skip_incomplete)] -> "
        "[(bits, kind, descs, total_groups, any_residual)].");
  m.def("bn_act_forward", &cgx::py_bn_act_forward, py::arg("x"),
        py::arg("identity"), py::arg("weight"), py::arg("bias"),
        py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"),
        py::arg("eps"), py::arg("relu"), py::arg("part") = py::none(),
        "Training-mode BatchNorm2d of a channels_last bf16 tensor, fused with "
        "an optional residual add and ReLU -> (out, mean, invstd, mask | "
        "None); updates the running statistics in place.  With `part`, the "
        "partials conv1x1_stats returned with x, the statistics pass over x "
        "is skipped.");
  m.def("bn_act_backward", &cgx::py_bn_act_backward, py::arg("dy"),
        py::arg("x"), py::arg("mean"), py::arg("invstd"), py::arg("weight"),
        py::arg("mask"), py::arg("has_identity"),
        "Backward of bn_act_forward -> (dx, dgamma, dbeta, didentity | None).");
  m.def("bn_act2_forward", &cgx::py_bn_act2_forward, py::arg("x3"),
        py::arg("xd"), py::arg("weight3"), py::arg("bias3"),
        py::arg("running_mean3"), py::arg("running_var3"),
        py::arg("momentum3"), py::arg("eps3"), py::arg("weightd"),
        py::arg("biasd"), py::arg("running_meand"), py::arg("running_vard"),
        py::arg("momentumd"), py::arg("epsd"), py::arg("relu"),
        py::arg("part3") = py::none(), py::arg("partd") = py::none(),
        "relu(bn3(x3) + bn_d(xd)) with both BatchNorms in training mode: "
        "(x3, xd, weight3, bias3, running_mean3, running_var3, momentum3, "
        "eps3, weightd, biasd, running_meand, running_vard, momentumd, epsd, "
        "relu, part3=None, partd=None) -> (out, mean3, invstd3, meand, "
        "invstdd, mask | None); part3 / partd as `part` of bn_act_forward.");
  m.def("conv1x1_stats", &cgx::py_conv1x1_stats, py::arg("x"),
        py::arg("weight"), py::arg("max_workgroups") = 0,
        "conv2d(x, weight) of a 1x1 / stride 1 / no-bias convolution on a "
        "channels_last bf16 tensor -> (y, part); part holds the per-channel "
        "(count, mean, M2) partials of y.  max_workgroups > 0 caps the "
        "persistent grid.");
  m.def("conv1x1_eligible", &cgx::py_conv1x1_eligible, py::arg("x"),
        py::arg("weight"),
        "True where conv1x1_stats takes (x, weight): CUDA, bf16, dense "
        "channels_last input, [N, K, 1, 1] weight, and a shape conv1x1_plan "
        "calls eligible.");
  m.def("conv1x1_plan", &cgx::py_conv1x1_plan, py::arg("rows"), py::arg("k"),
        py::arg("n"), py::arg("max_workgroups") = 0,
        "The launch geometry of conv1x1_stats for [rows, k] x [n, k], and "
        "`native`: whether the model uses it at this shape.");
  m.def("conv1x1_walk", &cgx::py_conv1x1_walk, py::arg("rows"), py::arg("k"),
        py::arg("n"), py::arg("max_workgroups") = 0,
        "Test seam: [grid, tiles_per_split, 4] int64, (row0, row1, n0, n1) "
        "of every tile each workgroup visits (-1: none).");
  m.def("conv1x1_bwd_data", &cgx::py_conv1x1_bwd_data, py::arg("dy"),
        py::arg("weight"), py::arg("skip") = py::none(),
        py::arg("max_workgroups") = 0,
        "Input gradient of conv2d(x, weight) for a 1x1 / stride 1 convolution "
        "on channels_last bf16 tensors, plus `skip` (a bf16 channels_last "
        "tensor of dx's shape) where given: dx = bf16(dy * W + skip), rounded "
        "once.  `skip` is not written.");
  m.def("conv1x1_bwd_eligible", &cgx::py_conv1x1_bwd_eligible, py::arg("dy"),
        py::arg("weight"), py::arg("skip") = py::none(),
        "True where conv1x1_bwd_data takes (dy, weight, skip).");
  m.def("conv1x1_bwd_plan", &cgx::py_conv1x1_bwd_plan, py::arg("rows"),
        py::arg("k"), py::arg("n"), py::arg("with_add") = false,
        py::arg("max_workgroups") = 0,
        "The launch geometry of conv1x1_bwd_data for dx [rows, k] from dy "
        "[rows, n], and `native`: whether the model uses it for this problem.");
  m.def("conv1x1_bwd_walk", &cgx::py_conv1x1_bwd_walk, py::arg("rows"),
        py::arg("k"), py::arg("n"), py::arg("with_add") = false,
        py::arg("max_workgroups") = 0,
        "Test seam: conv1x1_walk for the plan of conv1x1_bwd_plan; channels "
        "are dx's.");
  m.def("conv1x1_tiled_stats", &cgx::py_conv1x1_tiled_stats, py::arg("x"),
        py::arg("weight"), py::arg("max_workgroups") = 0,
        "conv1x1_stats by the tiled walk (256-row tiles, B double-buffered in "
        "LDS chunk by chunk): the same y bit for bit, partials of the same "
        "layout.  Takes what conv1x1_eligible admits.");
  m.def("conv1x1_tiled_bwd_data", &cgx::py_conv1x1_tiled_bwd_data,
        py::arg("dy"), py::arg("weight"), py::arg("skip") = py::none(),
        py::arg("max_workgroups") = 0,
        "conv1x1_bwd_data by the tiled walk: the same dx bit for bit.  Takes "
        "what conv1x1_bwd_eligible admits.");
  m.def("conv1x1_tiled_plan", &cgx::py_conv1x1_tiled_plan, py::arg("rows"),
        py::arg("k"), py::arg("n"), py::arg("max_workgroups") = 0,
        "The launch geometry of conv1x1_tiled_stats, with the keys of "
        "conv1x1_plan, and `native`: whether the model uses it at this shape.");
  m.def("conv1x1_tiled_bwd_plan", &cgx::py_conv1x1_tiled_bwd_plan,
        py::arg("rows"), py::arg("k"), py::arg("n"),
        py::arg("with_add") = false, py::arg("max_workgroups") = 0,
        "The launch geometry of conv1x1_tiled_bwd_data, with the keys of "
        "conv1x1_bwd_plan.");
  m.def("conv1x1_tiled_walk", &cgx::py_conv1x1_tiled_walk, py::arg("rows"),
        py::arg("k"), py::arg("n"), py::arg("max_workgroups") = 0,
        "Test seam: conv1x1_walk for the plan of conv1x1_tiled_plan.");
  m.def("conv1x1_tiled_bwd_walk", &cgx::py_conv1x1_tiled_bwd_walk,
        py::arg("rows"), py::arg("k"), py::arg("n"),
        py::arg("with_add") = false, py::arg("max_workgroups") = 0,
        "Test seam: conv1x1_walk for the plan of conv1x1_tiled_bwd_plan; "
        "channels are dx's.");
  m.def("conv1x1_wrw", &cgx::py_conv1x1_wrw, py::arg("dy"), py::arg("x"),
        py::arg("max_workgroups") = 0,
        "Weight gradient of conv2d(x, weight) for a 1x1 / stride 1 convolution "
        "on channels_last bf16 tensors: dw[n, k] = bf16(sum_r dy[r, n] * "
        "x[r, k]) as [N, K, 1, 1], accumulated in fp32 in a fixed order and "
        "rounded once.");
  m.def("conv1x1_wrw_ring", &cgx::py_conv1x1_wrw_ring, py::arg("dy"),
        py::arg("x"), py::arg("max_workgroups") = 0,
        "conv1x1_wrw by the kernel that loads the chunks straight into a "
        "ring of LDS stages; K and N at least 128.");
  m.def("conv1x1_wrw_ring_eligible", &cgx::py_conv1x1_wrw_ring_eligible,
        py::arg("dy"), py::arg("x"),
        "True where conv1x1_wrw_ring takes (dy, x).");
  m.def("conv1x1_wrw_ring_plan", &cgx::py_conv1x1_wrw_ring_plan,
        py::arg("rows"), py::arg("k"), py::arg("n"),
        py::arg("max_workgroups") = 0,
        "The launch geometry of conv1x1_wrw_ring.");
  m.def("conv1x1_wrw_ring_walk", &cgx::py_conv1x1_wrw_ring_walk,
        py::arg("rows"), py::arg("k"), py::arg("n"),
        py::arg("max_workgroups") = 0,
        "Test seam: conv1x1_wrw_walk for conv1x1_wrw_ring.");
  m.def("conv1x1_wrw_ring_fill", &cgx::py_conv1x1_wrw_ring_fill,
        py::arg("rows"), py::arg("k"), py::arg("n"), py::arg("slot") = 0,
        "Test seam: (LDS byte, row, channel) of every lane of every load "
        "that fills one stage of the ring.");
  m.def("conv1x1_wrw_image_slot",
        [](int c, int p) {
          const cgx::WrwImageSlot s = cgx::conv1x1_wrw_image_slot(c, p);
          return py::make_tuple(s.row, s.channel);
        },
        py::arg("c"), py::arg("p"),
        "Test seam: (row, first channel) at byte p of the LDS image of a "
        "[64, c] chunk.");
  m.def("conv1x1_wrw_ring_piece", &cgx::conv1x1_wrw_ring_piece,
        py::arg("wave"), py::arg("j"),
        "Test seam: the image byte at which load j of a wave lands.");
  m.def("conv1x1_wrw_eligible", &cgx::py_conv1x1_wrw_eligible, py::arg("dy"),
        py::arg("x"), "True where conv1x1_wrw takes (dy, x).");
  m.def("conv1x1_wrw_plan", &cgx::py_conv1x1_wrw_plan, py::arg("rows"),
        py::arg("k"), py::arg("n"), py::arg("max_workgroups") = 0,
        "The launch geometry of conv1x1_wrw for dw [n, k] from dy [rows, n] "
        "and x [rows, k], and `native`: whether the model uses it for this "
        "problem.");
  m.def("conv1x1_wrw_walk", &cgx::py_conv1x1_wrw_walk, py::arg("rows"),
        py::arg("k"), py::arg("n"), py::arg("max_workgroups") = 0,
        "Test seam: [grid, chunks_per_split, 5] int64, (n0, k0, split, row0, "
        "row1) of every row chunk each workgroup visits (-1: none).");
  m.def("bn_act2_backward", &cgx::py_bn_act2_backward,
        "Backward of bn_act2_forward: (dy, x3, xd, mean3, invstd3, weight3, "
        "meand, invstdd, weightd, mask) -> (dx3, dxd, dgamma3, dbeta3, "
        "dgammad, dbetad).");
  m.def("bn_act_pool_forward", &cgx::py_bn_act_pool_forward, py::arg("x"),
        py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        "max_pool2d(relu(bn(x)), 3, 2, 1) in training mode -> (pooled, mean, "
        "invstd, arg); arg is one byte per pooled element.");
  m.def("bn_act_pool_backward", &cgx::py_bn_act_pool_backward, py::arg("dy"),
        py::arg("x"), py::arg("mean"), py::arg("invstd"), py::arg("weight"),
        py::arg("arg"),
        "Backward of bn_act_pool_forward -> (dx, dgamma, dbeta).");
  m.def("bn_pool_geometry", &cgx::py_bn_pool_geometry, py::arg("h"),
        py::arg("w"),
        "Test seam: (windows [oh*ow, 9], covers [h*w, 4, 2]) of the stem's "
        "3x3/2/1 pooling as the kernels index it.");
  m.def("bn_eligible", &cgx::py_bn_eligible, py::arg("x"),
        "True where the fused BatchNorm kernels take `x`: CUDA, bf16, dense "
        "channels_last, and a shape bn_plan calls eligible.");
  m.def("bn_plan", &cgx::py_bn_plan, py::arg("rows"), py::arg("channels"),
        "Test seam: the launch geometry of the fused BatchNorm kernels for a "
        "[rows, channels] activation.");
  m.def("bn_sweep_indices", &cgx::py_bn_sweep_indices, py::arg("rows"),
        py::arg("channels"),
        "Test seam: [grid*threads, rows_per_thread+1] int64, the 16-byte "
        "vector indices every thread visits (-1: none).");
  m.def("bn_partial_offsets", &cgx::py_bn_partial_offsets, py::arg("rows"),
        py::arg("channels"), py::arg("wg"),
        "Test seam: the partial-buffer floats workgroup `wg` writes.");
  m.attr("FLAG_SKIP_INCOMPLETE") = cgx::kFlagSkipIncomplete;
  m.attr("FLAG_TAIL_ONLY") = cgx::kFlagTailOnly;
  m.attr("KIND_FAST") = (int)cgx::kFast;
  m.attr("KIND_GENERIC") = (int)cgx::kGeneric;
  m.attr("KIND_TWO_PASS") = (int)cgx::kTwoPass;
  m.attr("KIND_SUB") = (int)cgx::kSub;
}
