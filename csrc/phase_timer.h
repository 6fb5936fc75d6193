// CGX_TIMINGS=1: per-phase GPU timing of each SRA chunk (quantize /
// round-1 comm / decode+requantize / round-2 comm / final decode),
// aggregated and printed every 50 chunks (the reference had no
// timers at all).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cgx {

class PhaseTimer {
 public:
  explicit PhaseTimer(int rank) : rank_(rank) {}
  ~PhaseTimer();
  PhaseTimer(const PhaseTimer&) = delete;
  PhaseTimer& operator=(const PhaseTimer&) = delete;

  // Start timing a chunk on `qs` (event 0).  A disabled chunk, or one that
  // finds the ring full of in-flight chunks, turns mark/finish into no-ops.
  void begin(hipStream_t qs, bool enabled);
  void mark(int idx, hipStream_t stream);  // idx 1..5
  void finish();
  // Collect the in-flight slots and print the final averages (short runs
  // would otherwise never reach the 50-chunk periodic print).
  void drain();

 private:
  static constexpr int kRing = 4;
  static constexpr int kEv = 6;
  void collect(int slot);  // fold one finished slot into the sums
  void print(const char* suffix) const;  // the five-phase line

  int rank_;
  hipEvent_t ev_[kRing][kEv] = {};
  bool pending_[kRing] = {};
  int cur_ = 0;
  double sum_ms_[kEv - 1] = {};
  int64_t count_ = 0;
  bool inited_ = false;
  bool timing_ = false;  // the chunk between begin and finish is timed
  int slot_ = -1;        // its ring slot
};

}  // namespace cgx
