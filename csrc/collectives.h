// The p2p collectives (allgather, gather, scatter, alltoall, alltoall_base)
// as compositions of one grouped Transport::exchange plus a self copy.
//
// Stateless free functions over a Transport*, this rank and the world size:
// ProcessGroupCGX runs them over its RcclTransport, the loopback test seam
// (`_C.loopback_collective`) runs the same functions with real peers on one
// GPU.  Everything is queued on the one stream passed in.
#pragma once

#include <ATen/ATen.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "transport.h"

namespace cgx {
namespace coll {

// A byte range on the device; bytes == 0 is an empty slot.
struct Buf {
  void* ptr = nullptr;
  int64_t bytes = 0;
};

// The whole tensor as a slot.  Rejects (nccl_dtype) the dtypes RCCL cannot
// carry; the byte transport itself would take anything.
Buf buf_of(const at::Tensor& t);

// send[p] goes to peer p, recv[p] is filled by peer p (one slot per rank;
// empty slots are skipped): one exchange of every non-self slot, then
// recv[rank] = send[rank] as a device-to-device copy on the same stream.
void exchange_slots(Transport* tr, int rank, const std::vector<Buf>& send,
                    const std::vector<Buf>& recv, hipStream_t stream);

void allgather(Transport* tr, int rank, int size, const at::Tensor& in,
               const std::vector<at::Tensor>& outs, hipStream_t stream);
// `outs` is read on the root only, `ins` of scatter likewise.
void gather(Transport* tr, int rank, int size, int root, const at::Tensor& in,
            const std::vector<at::Tensor>& outs, hipStream_t stream);
void scatter(Transport* tr, int rank, int size, int root,
             const std::vector<at::Tensor>& ins, const at::Tensor& out,
             hipStream_t stream);
void alltoall(Transport* tr, int rank, int size,
              const std::vector<at::Tensor>& ins,
              const std::vector<at::Tensor>& outs, hipStream_t stream);
// Splits are in dim-0 rows; both empty means an even division by `size`.
void alltoall_base(Transport* tr, int rank, int size, const at::Tensor& in,
                   const at::Tensor& out, std::vector<int64_t> isplit,
                   std::vector<int64_t> osplit, hipStream_t stream);

}  // namespace coll
}  // namespace cgx
