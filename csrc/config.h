// Environment-derived engine configuration.  Pure std.
#pragma once

#include <cstdint>

namespace cgx {

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

// Integer environment variable, `dflt` when unset or empty.
int64_t env_int(const char* name, int64_t dflt);

}  // namespace cgx
