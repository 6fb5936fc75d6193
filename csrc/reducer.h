// Reducer: how engines compose into one compressed allreduce.  The only
// place that knows the flat-or-hierarchical decision; shared by
// ProcessGroupCGX (over RCCL) and the one-GPU loopback harnesses
// (bindings.cc), so the tests run the flow production runs.
#pragma once

#include <memory>
#include <optional>

#include "engine.h"
#include "transport.h"

namespace cgx {

class Reducer {
 public:
  // One engine and the transport it speaks through (not owned).
  struct Stage {
    Stage(int rank, int size, Transport* tr, bool is_cross = false)
        : engine(std::make_unique<Engine>(rank, size, is_cross)), tr(tr) {}
    std::unique_ptr<Engine> engine;
    Transport* tr;
  };

  std::optional<Stage> flat;   // all ranks
  std::optional<Stage> intra;  // ranks of this node; absent on a single node
  std::optional<Stage> cross;  // same local rank on every node
  bool leader = false;         // local rank 0: runs the cross stage

  bool hierarchical() const { return intra.has_value(); }

  // SUM-allreduce `t` in place, quantizing on `qs`; returns the stream
  // carrying the final operation.  Hierarchical (when the intra stage exists
  // and CGX_INTRA_BROADCAST is not 0, reference
  // mpi_allreduce_operations.cc:160-183): intra-node allreduce, cross-node
  // allreduce on the leader, intra-node broadcast from the leader.  Else the
  // flat engine.  Either way the layer registry advances exactly one cursor
  // step per bucket; `forced` replaces that step with the caller's own
  // (Engine::allreduce has the semantics).
  hipStream_t allreduce(at::Tensor t, hipStream_t qs,
                        const Registry::BucketInfo* forced = nullptr,
                        bool forced_match = false);

  // fn(stream) for the comm and deq stream of every live stage
  template <typename Fn>
  void for_each_stream(Fn&& fn) const {
    for (const auto* s : {&flat, &intra, &cross}) {
      if (!*s) continue;
      fn((*s)->engine->comm_stream());
      fn((*s)->engine->deq_stream());
    }
  }
};

}  // namespace cgx
