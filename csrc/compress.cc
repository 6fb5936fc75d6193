// The launch router (see compress.h): pure host code, no HIP calls.
#include "compress.h"

#include <algorithm>
#include <map>
#include <utility>

namespace cgx {
namespace {

template <typename Group>
using GroupMap = std::map<std::pair<int, int>, Group>;

template <typename Group>
Group& group_of(GroupMap<Group>& groups, int bits, int kind) {
  Group& g = groups[{bits, kind}];
  g.bits = bits;
  g.kind = kind;
  return g;
}

template <typename Group>
std::vector<Group> in_order(GroupMap<Group>& groups) {
  std::vector<Group> out;
  out.reserve(groups.size());
  for (auto& kv : groups) out.push_back(std::move(kv.second));
  return out;
}

// The one place desc flags are composed.
int32_t desc_flags(bool skip_incomplete, bool tail_only) {
  return (skip_incomplete ? kFlagSkipIncomplete : 0) |
         (tail_only ? kFlagTailOnly : 0);
}

// A skip_incomplete slice with a partial last bucket carries a raw residual
// tail; a tail-only desc never does (quantize tails exist only without
// skip_incomplete, and a skip_incomplete nq is a multiple of 8).
template <typename Slice>
bool has_residual(const Slice& s, bool tail_only) {
  return !tail_only && s.skip_incomplete && (s.n % s.bucket) != 0;
}

void add_quant(QuantGroup& g, const QuantSlice& s, bool tail_only,
               int64_t buckets) {
  if (g.cum.empty()) g.cum.push_back(0);
  g.descs.push_back(QuantDesc{s.in, s.out, s.fb, s.n, s.bucket,
                              desc_flags(s.skip_incomplete, tail_only)});
  g.cum.push_back(g.cum.back() + buckets);
  g.any_residual |= has_residual(s, tail_only);
}

}  // namespace

std::vector<QuantGroup> route_quantize(const std::vector<QuantSlice>& slices) {
  GroupMap<QuantGroup> groups;
  for (const QuantSlice& s : slices) {
    if (s.n <= 0) continue;
    const int64_t full = s.n / s.bucket;
    const int64_t quantized =
        s.skip_incomplete ? full : (s.n + s.bucket - 1) / s.bucket;
    if ((s.bucket % 8) != 0) {
      add_quant(group_of(groups, s.bits, kTwoPass), s, false, quantized);
      continue;
    }
    const bool aligned = (reinterpret_cast<uintptr_t>(s.in) & 15) == 0;
    if (s.fb || !aligned || s.n < s.bucket || s.bucket > 2048) {
      add_quant(group_of(groups, s.bits, kGeneric), s, false, quantized);
      continue;
    }
    const int ng = s.bucket >> 3;  // 8-element groups per bucket
    const bool small_pow2 = ng < 64 && (ng & (ng - 1)) == 0;
    QuantGroup& g = group_of(groups, s.bits, small_pow2 ? kSub : kFast);
    add_quant(g, s, false, full);
    g.max_gpl = std::max(g.max_gpl, (ng + 63) >> 6);
    if (!s.skip_incomplete && (s.n % s.bucket) != 0)
      add_quant(group_of(groups, s.bits, kGeneric), s, true, 1);
  }
  return in_order(groups);
}

std::vector<DequantGroup> route_dequantize(
    const std::vector<DequantSlice>& slices, DType dt, int64_t src_stride,
    int nsrc, bool add) {
  GroupMap<DequantGroup> groups;
  auto push = [&](int kind, const DequantSlice& s, bool tail_only,
                  int64_t work) {
    DequantGroup& g = group_of(groups, s.bits, kind);
    g.descs.push_back(DequantDesc{s.in, s.out, s.n, src_stride, s.bucket,
                                  nsrc, add ? 1 : 0,
                                  desc_flags(s.skip_incomplete, tail_only)});
    g.total_groups += work;
    g.any_residual |= has_residual(s, tail_only);
  };
  for (const DequantSlice& s : slices) {
    if (s.n <= 0) continue;
    const int64_t nq =
        slice_geom(s.n, s.bucket, s.bits, elem_size(dt), s.skip_incomplete)
            .nq;
    const int64_t work = (nq + 7) / 8;
    if ((s.bucket % 8) != 0 || nq >= (int64_t(1) << 31)) {
      push(kGeneric, s, false, work);
      continue;
    }
    push(kFast, s, false, work);
    // the fast kernel decodes whole 4-element (fp32) / 8-element (16-bit)
    // units only
    const bool ragged = elem_size(dt) == 4 ? (nq & 3) != 0 : (nq & 7) != 0;
    if (ragged) push(kGeneric, s, true, 1);
  }
  return in_order(groups);
}

}  // namespace cgx
