// Implementation of Reducer (see reducer.h).
#include "reducer.h"

namespace cgx {

hipStream_t Reducer::allreduce(at::Tensor t, hipStream_t qs,
                               const Registry::BucketInfo* forced,
                               bool forced_match) {
  if (!intra || !EngineConfig::from_env().intra_broadcast)
    return flat->engine->allreduce(t, flat->tr, qs, forced, forced_match);
  // The registry is consulted exactly ONCE per bucket so the cursor stays in
  // lockstep on every rank (leaders run two engine passes).
  Registry::BucketInfo info;
  if (!forced) {
    forced_match = Registry::get().next(t.numel(), t.data_ptr(), &info);
    forced = &info;
  }
  hipStream_t fin =
      intra->engine->allreduce(t, intra->tr, qs, forced, forced_match);
  if (leader)
    fin = cross->engine->allreduce(t, cross->tr, fin, forced, forced_match);
  return intra->engine->broadcast(t, /*root=*/0, intra->tr, fin);
}

}  // namespace cgx
