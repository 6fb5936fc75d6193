// Implementation of chunk planning (see plan.h).
#include "plan.h"

#include <algorithm>

namespace cgx {

void partition(int64_t num_elements, int ws,
               const std::vector<int64_t>& lnumels, int esize,
               std::vector<int64_t>* offsets, std::vector<int64_t>* sizes) {
  // Mirror of torch_cgx_amd.parallel.partition.partition (tested against it).
  int64_t offset = 0;
  size_t li = 0;
  int64_t n_elem = lnumels.empty() ? 0 : std::min(lnumels[0], num_elements);
  const int64_t unit = (esize == 2) ? 8 : 4;
  int64_t remaining = num_elements;
  for (int r = 0; r < ws; r++) {
    const int64_t per = remaining / (ws - r);
    int64_t cur = 0;
    while (cur < per) {
      if (n_elem <= per - cur) {
        cur += n_elem;
        li++;
        if (li == lnumels.size()) break;
        n_elem = std::min(lnumels[li], num_elements);
      } else {
        const int64_t want = per - cur;
        const int64_t aligned =
            std::min(((want + unit - 1) / unit) * unit, n_elem);
        cur += aligned;
        n_elem -= aligned;
      }
    }
    remaining -= cur;
    sizes->push_back(cur);
    offsets->push_back(offset);
    offset += cur;
  }
}

ChunkPlan plan_chunk(const std::vector<LayerView>& views, DType dt, int ws,
                     bool skip_incomplete) {
  ChunkPlan pl;
  const int es = elem_size(dt);
  std::vector<int64_t> lnumels;
  lnumels.reserve(views.size());
  for (const auto& v : views) {
    lnumels.push_back(v.numel);
    pl.n += v.numel;
  }
  if (pl.n == 0) return pl;
  partition(pl.n, ws, lnumels, es, &pl.offs, &pl.szs);
  pl.rs.resize(ws);
  pl.comp.assign(ws, 0);
  for (int r = 0; r < ws; r++) {
    const int64_t start = pl.offs[r], end = pl.offs[r] + pl.szs[r];
    int64_t pos = 0, coff = 0;
    for (const auto& v : views) {
      const int64_t lo = std::max(pos, start);
      const int64_t hi = std::min(pos + v.numel, end);
      if (hi > lo) {
        pl.rs[r].push_back(Slice{v.data + (lo - pos) * es, hi - lo, v.bits,
                                 v.bucket_size, coff, skip_incomplete, lo});
        coff += buffer_size(hi - lo, dt, v.bits, v.bucket_size,
                            skip_incomplete);
      }
      pos += v.numel;
      if (pos >= end) break;
    }
    pl.comp[r] = coff;
  }
  return pl;
}

ChunkPlan::Packed ChunkPlan::pack(int skip_rank) const {
  Packed out;
  out.off.assign(rs.size(), 0);
  for (int r = 0; r < (int)rs.size(); r++) {
    if (r == skip_rank) continue;
    out.off[r] = out.total;
    out.total += comp[r];
    for (const auto& sl : rs[r]) {
      Slice t = sl;
      t.comp_off += out.off[r];
      out.slices.push_back(t);
    }
  }
  return out;
}

// CGX_COMPRESSION_FAKE_RATIO < 1: reduce only a fraction of each chunk
// (bandwidth experiments; intentionally lossy -- reference
// mpi_allreduce_operations.cc:143-144).  keep >= 16, so the first view
// always survives.
static void trim_chunk(std::vector<LayerView>& chunk, double ratio) {
  int64_t total = 0;
  for (const auto& v : chunk) total += v.numel;
  int64_t keep = std::max<int64_t>(16, (int64_t)(total * ratio));
  size_t kept = 0;
  for (auto& v : chunk) {
    if (keep <= 0) break;
    v.numel = std::min(v.numel, keep);
    keep -= v.numel;
    kept++;
  }
  chunk.resize(kept);
}

BucketPlan plan_bucket(const std::vector<LayerView>& views,
                       const EngineConfig& cfg, int es) {
  BucketPlan bp;
  const int64_t fusion_elems = std::max<int64_t>(256, cfg.fusion_bytes / es);
  std::vector<LayerView> cur;
  int64_t cur_n = 0;
  auto emit = [&](std::vector<LayerView>&& chunk) {
    if (cfg.fake_ratio < 1.0) trim_chunk(chunk, cfg.fake_ratio);
    bp.chunks.push_back(std::move(chunk));
  };
  auto flush = [&]() {
    if (cur.empty()) return;
    emit(std::move(cur));
    cur.clear();
    cur_n = 0;
  };
  for (const auto& v : views) {
    const bool c = !cfg.dummy && v.bits <= 8 && v.numel > cfg.min_elems;
    if (!c) {
      // uncompressed: merge with the previous range when adjacent in memory
      if (!bp.uncomp.empty() &&
          bp.uncomp.back().first + bp.uncomp.back().second * es == v.data) {
        bp.uncomp.back().second += v.numel;
      } else {
        bp.uncomp.emplace_back(v.data, v.numel);
      }
    } else if (v.numel >= fusion_elems) {
      // a layer of a whole fusion buffer or more travels alone, in pieces
      flush();
      for (int64_t o = 0; o < v.numel; o += fusion_elems)
        emit({LayerView{v.data + o * es, std::min(fusion_elems, v.numel - o),
                        v.bits, v.bucket_size}});
    } else {
      if (cur_n + v.numel > fusion_elems) flush();
      cur.push_back(v);
      cur_n += v.numel;
    }
  }
  flush();
  return bp;
}

}  // namespace cgx
