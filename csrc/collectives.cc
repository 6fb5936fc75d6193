// Implementation of the p2p collectives (see collectives.h).
#include "collectives.h"

#include "check.h"
#include "engine.h"

namespace cgx {
namespace coll {

Buf buf_of(const at::Tensor& t) {
  (void)nccl_dtype(t);
  return Buf{t.data_ptr(), (int64_t)t.nbytes()};
}

namespace {

std::vector<Buf> bufs_of(const std::vector<at::Tensor>& ts, int size) {
  TORCH_CHECK((int)ts.size() == size, "cgx: expected one tensor per rank (",
              size, "), got ", ts.size());
  std::vector<Buf> bufs;
  for (const auto& t : ts) bufs.push_back(buf_of(t));
  return bufs;
}

// `size` empty slots but for slot `p`
std::vector<Buf> only(int size, int p, Buf b) {
  TORCH_CHECK(p >= 0 && p < size, "cgx: bad root rank ", p);
  std::vector<Buf> bufs(size);
  bufs[p] = b;
  return bufs;
}

}  // namespace

void exchange_slots(Transport* tr, int rank, const std::vector<Buf>& send,
                    const std::vector<Buf>& recv, hipStream_t stream) {
  const int size = (int)send.size();
  TORCH_CHECK(recv.size() == send.size() && rank >= 0 && rank < size,
              "cgx: exchange_slots needs one send and one recv slot per rank");
  // Empty slots issue no op (the transports skip bytes <= 0 as well).  An
  // empty send always faces an empty recv on the peer, so this is the same
  // wire traffic as a zero-count RCCL send/receive pair.
  std::vector<Transport::Op> sends, recvs;
  for (int p = 0; p < size; p++) {
    if (p == rank) continue;
    if (send[p].bytes > 0)
      sends.push_back(Transport::Op{send[p].ptr, send[p].bytes, p});
    if (recv[p].bytes > 0)
      recvs.push_back(Transport::Op{recv[p].ptr, recv[p].bytes, p});
  }
  tr->exchange(sends, recvs, stream);
  if (send[rank].bytes > 0 && recv[rank].bytes > 0) {
    TORCH_CHECK(send[rank].bytes == recv[rank].bytes,
                "cgx: self slot size mismatch (send ", send[rank].bytes,
                " vs recv ", recv[rank].bytes, " bytes)");
    CGX_HIP_CHECK(hipMemcpyAsync(recv[rank].ptr, send[rank].ptr,
                                 send[rank].bytes, hipMemcpyDeviceToDevice,
                                 stream));
  }
}

void allgather(Transport* tr, int rank, int size, const at::Tensor& in,
               const std::vector<at::Tensor>& outs, hipStream_t stream) {
  exchange_slots(tr, rank, std::vector<Buf>(size, buf_of(in)),
                 bufs_of(outs, size), stream);
}

void gather(Transport* tr, int rank, int size, int root, const at::Tensor& in,
            const std::vector<at::Tensor>& outs, hipStream_t stream) {
  exchange_slots(tr, rank, only(size, root, buf_of(in)),
                 rank == root ? bufs_of(outs, size) : std::vector<Buf>(size),
                 stream);
}

void scatter(Transport* tr, int rank, int size, int root,
             const std::vector<at::Tensor>& ins, const at::Tensor& out,
             hipStream_t stream) {
  exchange_slots(tr, rank,
                 rank == root ? bufs_of(ins, size) : std::vector<Buf>(size),
                 only(size, root, buf_of(out)), stream);
}

void alltoall(Transport* tr, int rank, int size,
              const std::vector<at::Tensor>& ins,
              const std::vector<at::Tensor>& outs, hipStream_t stream) {
  exchange_slots(tr, rank, bufs_of(ins, size), bufs_of(outs, size), stream);
}

void alltoall_base(Transport* tr, int rank, int size, const at::Tensor& in,
                   const at::Tensor& out, std::vector<int64_t> isplit,
                   std::vector<int64_t> osplit, hipStream_t stream) {
  if (osplit.empty()) {
    TORCH_CHECK(out.numel() % size == 0 && in.numel() % size == 0,
                "cgx: alltoall_base tensor not divisible by world size");
    osplit.assign(size, out.numel() / size);
    isplit.assign(size, in.numel() / size);
  } else {
    // splits are in units of dim-0 rows
    int64_t orow = out.dim() > 0 && out.size(0) > 0 ? out.numel() / out.size(0) : 1;
    int64_t irow = in.dim() > 0 && in.size(0) > 0 ? in.numel() / in.size(0) : 1;
    for (auto& v : osplit) v *= orow;
    for (auto& v : isplit) v *= irow;
  }
  TORCH_CHECK((int)isplit.size() == size && (int)osplit.size() == size,
              "cgx: alltoall_base needs one split per rank on both sides");
  (void)nccl_dtype(in);
  (void)nccl_dtype(out);
  const int es = in.element_size();
  // slot p = `split[p]` elements at the prefix sum of the splits before it
  auto cut = [&](const at::Tensor& t, const std::vector<int64_t>& split) {
    std::vector<Buf> bufs;
    int64_t off = 0;
    for (int64_t n : split) {
      TORCH_CHECK(n >= 0 && off + n <= t.numel(),
                  "cgx: alltoall_base splits exceed the tensor");
      bufs.push_back(Buf{static_cast<char*>(t.data_ptr()) + off * es, n * es});
      off += n;
    }
    return bufs;
  };
  exchange_slots(tr, rank, cut(in, isplit), cut(out, osplit), stream);
}

}  // namespace coll
}  // namespace cgx
