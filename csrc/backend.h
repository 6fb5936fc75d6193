// ProcessGroupCGX: a modern c10d::Backend for the "cgx" torch.distributed
// backend name.
//
// MI355X-native re-design of the reference ProcessGroupCGX
// (/root/reference/src/ProcessGroupCGX.{h,cc}): instead of an MPI-backed
// worker thread consuming a queue of blocking WorkEntries, every collective
// is enqueued from the calling thread onto a dedicated high-priority HIP side
// stream (RCCL calls are stream-ordered and non-blocking, so no thread is
// needed); the c10d Store replaces MPI for rendezvous (the reference ignores
// the store and requires mpirun, README.md:66-67); CPU tensors delegate to an
// internal gloo backend (the reference used CUDA-aware MPI for those).
//
// fp32/fp16/bf16 SUM allreduce of CUDA tensors routes through the
// compression Engine (engine.h); everything else is RCCL passthrough.
#pragma once

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <rccl/rccl.h>
#include <torch/csrc/distributed/c10d/Backend.hpp>
#include <torch/csrc/distributed/c10d/Store.hpp>
#include <torch/csrc/distributed/c10d/Types.hpp>
#include <torch/csrc/distributed/c10d/Work.hpp>

#include <memory>
#include <deque>
#include <mutex>
#include <optional>
#include <vector>

#include "reducer.h"

namespace cgx {

class WorkCGX : public c10d::Work {
 public:
  WorkCGX(int rank, c10d::OpType op, at::Device device,
          std::vector<at::Tensor> outputs,
          const char* profiling_title = "cgx");
  ~WorkCGX() override;

  // record the completion event on `stream` and mark the future completed
  // (caller must have `stream` current so the future captures CUDA context)
  void recordEnd(const c10::hip::HIPStreamMasqueradingAsCUDA& stream);

  bool isCompleted() override;
  bool isSuccess() const override;
  bool wait(std::chrono::milliseconds timeout) override;
  void synchronize() override;
  c10::intrusive_ptr<c10::ivalue::Future> getFuture() override;

 private:
  at::Device device_;
  hipEvent_t ev_ = nullptr;
  bool recorded_ = false;
  std::vector<at::Tensor> outputs_;
  c10::intrusive_ptr<c10::ivalue::Future> future_;
};

// Rank topology computed by exchanging hostnames through the c10d Store
// (replaces the reference's MPI_Comm_split_type node detection,
// mpi_context.cc:25-35).
struct Topology {
  int node_id = 0;      // index of this rank's node (order of first rank)
  int local_rank = 0;   // rank within the node
  int local_size = 1;   // ranks on this node
  int n_nodes = 1;
  bool uniform = true;  // every node has the same local_size
};

Topology compute_topology(const c10::intrusive_ptr<c10d::Store>& store,
                          int rank, int size, const std::string& hostname);

class ProcessGroupCGX : public c10d::Backend {
 public:
  ProcessGroupCGX(c10::intrusive_ptr<c10d::Store> store, int rank, int size,
                  c10::intrusive_ptr<c10d::Backend> cpu_delegate);
  ~ProcessGroupCGX() override;

  const std::string getBackendName() const override { return "cgx"; }

  c10::intrusive_ptr<c10d::Work> allreduce(
      std::vector<at::Tensor>& tensors,
      const c10d::AllreduceOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> allreduce_coalesced(
      std::vector<at::Tensor>& tensors,
      const c10d::AllreduceCoalescedOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> broadcast(
      std::vector<at::Tensor>& tensors,
      const c10d::BroadcastOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> reduce(std::vector<at::Tensor>& tensors,
                                        const c10d::ReduceOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> allgather(
      std::vector<std::vector<at::Tensor>>& outputs,
      std::vector<at::Tensor>& inputs,
      const c10d::AllgatherOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> _allgather_base(
      at::Tensor& output, at::Tensor& input,
      const c10d::AllgatherOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> gather(
      std::vector<std::vector<at::Tensor>>& outputs,
      std::vector<at::Tensor>& inputs,
      const c10d::GatherOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> scatter(
      std::vector<at::Tensor>& outputs,
      std::vector<std::vector<at::Tensor>>& inputs,
      const c10d::ScatterOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> reduce_scatter(
      std::vector<at::Tensor>& outputs,
      std::vector<std::vector<at::Tensor>>& inputs,
      const c10d::ReduceScatterOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> _reduce_scatter_base(
      at::Tensor& output, at::Tensor& input,
      const c10d::ReduceScatterOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> alltoall_base(
      at::Tensor& output, at::Tensor& input,
      std::vector<int64_t>& outputSplitSizes,
      std::vector<int64_t>& inputSplitSizes,
      const c10d::AllToAllOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> alltoall(
      std::vector<at::Tensor>& outputs, std::vector<at::Tensor>& inputs,
      const c10d::AllToAllOptions& opts) override;
  c10::intrusive_ptr<c10d::Work> send(std::vector<at::Tensor>& tensors,
                                      int dstRank, int tag) override;
  c10::intrusive_ptr<c10d::Work> recv(std::vector<at::Tensor>& tensors,
                                      int srcRank, int tag) override;
  c10::intrusive_ptr<c10d::Work> recvAnysource(
      std::vector<at::Tensor>& tensors, int tag) override;
  c10::intrusive_ptr<c10d::Work> barrier(
      const c10d::BarrierOptions& opts) override;

 private:
  void lazyInit(at::Device device);

  // Prologue and epilogue of every GPU collective (under mu_): lazyInit,
  // async-error check of every live communicator, fork stream_ behind the
  // caller's current stream, fn(stream_) -> the stream the op completes on,
  // then keep `outputs` alive on the streams that touch them and return the
  // Work whose end event sits on that stream.  `path` selects the
  // passthrough/compressed differences; see the definition.
  enum class Path { kPassthrough, kCompressed };
  template <typename Fn>
  c10::intrusive_ptr<c10d::Work> enqueue(Path path,
                                         std::vector<at::Tensor> outputs,
                                         at::Device device, c10d::OpType op,
                                         const char* title, Fn&& fn);

  // RCCL passthrough: enqueue fn(stream_) behind the current stream and all
  // engine traffic; returns the event-backed Work.  Caller holds no lock.
  template <typename Fn>
  c10::intrusive_ptr<c10d::Work> collective(std::vector<at::Tensor> outputs,
                                            at::Device device,
                                            c10d::OpType op, Fn&& fn);

  // the CPU (gloo) delegate; CPU tensors cannot be served without one
  c10d::Backend& cpu_delegate() const {
    TORCH_CHECK(cpu_, "cgx: no CPU delegate backend available");
    return *cpu_;
  }

  c10::intrusive_ptr<c10d::Store> store_;
  c10::intrusive_ptr<c10d::Backend> cpu_;
  // CGX_P2P_ANYSOURCE: in-flight gloo source announcements (fire-and-forget)
  std::mutex ann_mu_;
  std::deque<c10::intrusive_ptr<c10d::Work>> pending_ann_;
  int device_index_ = -1;
  // Communicators (created in lazyInit, destroyed here) and the transports
  // over them.  intra/cross exist in hierarchical (multi-node) mode only.
  Topology topo_;
  ncclComm_t comm_ = nullptr;
  ncclComm_t intra_comm_ = nullptr;
  ncclComm_t cross_comm_ = nullptr;
  std::unique_ptr<RcclTransport> tr_, intra_tr_, cross_tr_;
  // the compression engines over those transports, filled by lazyInit
  std::unique_ptr<Reducer> reducer_;
  std::optional<c10::hip::HIPStreamMasqueradingAsCUDA> stream_;
  hipEvent_t start_ev_ = nullptr;
  std::mutex mu_;
};

}  // namespace cgx
