// Process-global layer registry (parity with the reference's static
// MPIAllReduce_Operation::RegisterLayer / Compressor config registry,
// mpi_allreduce_operations.h:37-49, compressor.h:93-107).  Pure std.
#pragma once

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace cgx {

struct LayerConfig {
  int bits = 32;
  int bucket_size = 512;
};

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

}  // namespace cgx
