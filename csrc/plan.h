// Chunk planning for the compressed allreduce: which bytes of a bucket go
// through which chunk, and which slices of a chunk belong to which rank.
//
// Pure host arithmetic: no HIP calls, no ATen.  Every rank runs it
// identically over shared metadata, so compressed byte sizes agree on both
// sides of an exchange without a size handshake.  The engine (engine.h) owns
// the streams, events and staging that execute a plan.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "compress.h"
#include "config.h"

namespace cgx {

// A contiguous compressible piece of the flat bucket tensor.
struct LayerView {
  char* data;
  int64_t numel;
  int bits;
  int bucket_size;
};

struct Slice {  // one layer piece inside one rank chunk
  char* data;
  int64_t n;
  int bits;
  int bucket;
  int64_t comp_off;  // byte offset of this slice in the chunk's comp stream
  bool skip_incomplete = false;
  int64_t fb_off = 0;  // element offset in the chunk's error-feedback buf
};

struct ChunkPlan {
  std::vector<std::vector<Slice>> rs;  // per-rank slice lists
  std::vector<int64_t> comp;           // per-rank compressed bytes
  std::vector<int64_t> offs, szs;
  int64_t n = 0;

  // The compressed streams of several ranks laid out back to back.
  struct Packed {
    std::vector<Slice> slices;  // comp_off rebased by the owning rank's off
    std::vector<int64_t> off;   // per rank: exclusive prefix of comp
    int64_t total = 0;
  };
  // Every rank in rank order, `skip_rank` left out (-1: none; its off is 0).
  Packed pack(int skip_rank = -1) const;
};

// Mirror of the partition walk (reference Quantizer::GetSizesAndOffsets,
// compressor.cc:265-299); exposed for tests via bindings.
void partition(int64_t num_elements, int world_size,
               const std::vector<int64_t>& layer_numels, int esize,
               std::vector<int64_t>* offsets, std::vector<int64_t>* sizes);

// Rank partition of one chunk and each rank's slices of it.  Empty (n == 0,
// no per-rank vectors) when the views hold no elements.
ChunkPlan plan_chunk(const std::vector<LayerView>& views, DType dt, int ws,
                     bool skip_incomplete);

struct BucketPlan {
  // layers that travel uncompressed, adjacent ones merged: (ptr, count)
  std::vector<std::pair<char*, int64_t>> uncomp;
  // tensor-fusion chunks over the compressible layers, in bucket order
  std::vector<std::vector<LayerView>> chunks;
};
BucketPlan plan_bucket(const std::vector<LayerView>& views,
                       const EngineConfig& cfg, int esize);

// Where peer p's stream lands among the ws-1 receive slots of `rank`.
inline int recv_slot(int p, int rank) { return p < rank ? p : p - 1; }

}  // namespace cgx
