// Implementation of the SRA phase timer (see phase_timer.h).
#include "phase_timer.h"

#include <cstdio>

#include "check.h"

namespace cgx {

PhaseTimer::~PhaseTimer() {
  if (!inited_) return;
  for (int r = 0; r < kRing; r++)
    for (int e = 0; e < kEv; e++)
      if (ev_[r][e]) (void)hipEventDestroy(ev_[r][e]);
}

void PhaseTimer::collect(int slot) {
  // the slot's last event has completed: fold its phase times into the sums
  for (int p = 0; p + 1 < kEv; p++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev_[slot][p], ev_[slot][p + 1]) == hipSuccess)
      sum_ms_[p] += ms;
  }
  count_++;
  pending_[slot] = false;
}

void PhaseTimer::print(const char* suffix) const {
  fprintf(stderr,
          "[cgx timings rank %d, %lld chunks%s] quantize %.3f ms | "
          "comm1 %.3f | decode+requant %.3f | comm2 %.3f | decode2 %.3f\n",
          rank_, (long long)count_, suffix, sum_ms_[0] / count_,
          sum_ms_[1] / count_, sum_ms_[2] / count_, sum_ms_[3] / count_,
          sum_ms_[4] / count_);
}

void PhaseTimer::drain() {
  if (!inited_) return;
  for (int r = 0; r < kRing; r++) {
    if (pending_[r] && hipEventSynchronize(ev_[r][kEv - 1]) == hipSuccess)
      collect(r);
  }
  if (count_ > 0) print(" total");
}

void PhaseTimer::begin(hipStream_t qs, bool enabled) {
  timing_ = enabled;
  slot_ = -1;
  if (!enabled) return;
  if (!inited_) {
    for (int r = 0; r < kRing; r++)
      for (int e = 0; e < kEv; e++)
        CGX_HIP_CHECK(hipEventCreate(&ev_[r][e]));  // timing-capable
    inited_ = true;
  }
  const int slot = cur_;
  cur_ = (cur_ + 1) % kRing;
  if (pending_[slot]) {
    if (hipEventQuery(ev_[slot][kEv - 1]) == hipSuccess) {
      collect(slot);
      if (count_ % 50 == 0) print("");
    } else {
      timing_ = false;  // ring full of in-flight chunks: skip this one
      return;
    }
  }
  slot_ = slot;
  CGX_HIP_CHECK(hipEventRecord(ev_[slot][0], qs));
}

void PhaseTimer::mark(int idx, hipStream_t stream) {
  if (!timing_ || slot_ < 0) return;
  CGX_HIP_CHECK(hipEventRecord(ev_[slot_][idx], stream));
}

void PhaseTimer::finish() {
  if (timing_ && slot_ >= 0) pending_[slot_] = true;
}

}  // namespace cgx
