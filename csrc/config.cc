// Implementation of EngineConfig (see config.h).
#include "config.h"

#include <cstdlib>
#include <cstring>

namespace cgx {

int64_t env_int(const char* name, int64_t dflt) {
  const char* v = std::getenv(name);
  if (!v || !*v) return dflt;
  return std::atoll(v);
}

bool env_flag(const char* name, bool dflt) {
  const char* v = std::getenv(name);
  if (!v || !*v) return dflt;
  return std::strcmp(v, "0") != 0;
}

bool env_hierarchical() { return env_flag("CGX_HIERARCHICAL", true); }
bool env_verbose() { return env_flag("CGX_VERBOSE"); }
bool env_blocking_wait() { return env_flag("CGX_BLOCKING_WAIT"); }

bool env_p2p_anysource() {
  static const bool v = env_flag("CGX_P2P_ANYSOURCE");
  return v;
}

bool env_timings() {
  static const bool v = env_int("CGX_TIMINGS", 0) != 0;
  return v;
}

int env_max_blocks() {
  static const int v = [] {
    const int x = (int)env_int("CGX_MAX_BLOCKS", 0);
    return x > 0 ? x : 0;
  }();
  return v;
}

EngineConfig EngineConfig::from_env() {
  EngineConfig c;
  c.fusion_bytes = env_int("CGX_FUSION_BUFFER_SIZE_MB", 64) << 20;
  if (c.fusion_bytes < 2048) c.fusion_bytes = 2048;
  c.min_elems = env_int("CGX_COMPRESSION_MINIMAL_SIZE", 16);
  c.default_bits = (int)env_int("CGX_COMPRESSION_QUANTIZATION_BITS", 32);
  c.default_bucket = (int)env_int("CGX_COMPRESSION_BUCKET_SIZE", 512);
  c.stochastic = env_int("CGX_STOCHASTIC_ROUNDING", 1) != 0;
  c.skip_incomplete =
      env_int("CGX_COMPRESSION_SKIP_INCOMPLETE_BUCKETS", 0) != 0;
  c.dummy = env_int("CGX_DEBUG_DUMMY_COMPRESSION", 0) != 0;
  c.intra_compress = env_int("CGX_INTRA_COMPRESS", 1) != 0;
  c.intra_broadcast = env_flag("CGX_INTRA_BROADCAST", true);
  c.error_feedback = env_int("CGX_ERROR_FEEDBACK", 0) != 0;
  c.debug_a2a = env_int("CGX_DEBUG_ALL_TO_ALL_REDUCTION", 0) != 0;
  const char* fr = std::getenv("CGX_COMPRESSION_FAKE_RATIO");
  if (fr && *fr) c.fake_ratio = std::atof(fr);
  if (!(c.fake_ratio > 0.0 && c.fake_ratio <= 1.0)) c.fake_ratio = 1.0;
  // Reduction algorithm selection, independently for the intra-node and
  // cross-node engines (reference mpi_allreduce_operations.cc:90-115:
  // intra default SRA, cross default Ring).  The legacy CGX_REDUCTION_TYPE
  // alias drives whichever specific variable is unset.
  auto is_ring = [](const char* v, bool dflt) {
    if (!v || !*v) return dflt;
    return std::strcmp(v, "Ring") == 0 || std::strcmp(v, "ring") == 0 ||
           std::strcmp(v, "RING") == 0;
  };
  const char* legacy = std::getenv("CGX_REDUCTION_TYPE");
  const char* inner = std::getenv("CGX_INNER_REDUCTION_TYPE");
  const char* cross = std::getenv("CGX_CROSS_REDUCTION_TYPE");
  c.ring = is_ring(inner && *inner ? inner : legacy, false);
  c.cross_ring = is_ring(cross && *cross ? cross : legacy, true);
  return c;
}

}  // namespace cgx
