// Environment-derived configuration: the only place the library reads the
// environment.  Pure std.
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
  bool intra_broadcast = true;  // CGX_INTRA_BROADCAST=0: multi-node runs
                                // reduce flat instead of hierarchically
  bool error_feedback = false;  // CGX_ERROR_FEEDBACK (needs bucket%8==0)
  static EngineConfig from_env();  // re-read every bucket like the reference
};

// Two boolean conventions coexist and are kept per variable:
//   env_int(name, d) != 0   numeric: "yes" parses as 0, i.e. false
//   env_flag(name, d)       textual: anything but the literal "0" is true

// Integer environment variable, `dflt` when unset or empty.
int64_t env_int(const char* name, int64_t dflt);

// Boolean environment variable: `dflt` when unset or empty, false for the
// literal "0", true for anything else.
bool env_flag(const char* name, bool dflt = false);

// Variables read outside EngineConfig, each at the moment its reader needs:
bool env_hierarchical();    // CGX_HIERARCHICAL, default on; once, at init
bool env_verbose();         // CGX_VERBOSE; once, at init
bool env_blocking_wait();   // CGX_BLOCKING_WAIT; on every Work::wait
bool env_p2p_anysource();   // CGX_P2P_ANYSOURCE; first call, then cached
bool env_timings();         // CGX_TIMINGS (numeric); first call, then cached
int env_max_blocks();       // CGX_MAX_BLOCKS, 0 when unset or not positive;
                            // first call, then cached

}  // namespace cgx
