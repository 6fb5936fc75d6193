// Implementation of the layer registry (see registry.h).
#include "registry.h"

namespace cgx {

Registry& Registry::get() {
  static Registry r;
  return r;
}

void Registry::register_layer(int bucket_idx, int layer_idx, int64_t numel,
                              int bits, int bucket_size) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = by_idx_.find(bucket_idx);
  if (it == by_idx_.end()) {
    by_idx_[bucket_idx] = order_.size();
    order_.emplace_back();
    order_.back().idx = bucket_idx;
    it = by_idx_.find(bucket_idx);
  }
  BucketInfo& b = order_[it->second];
  if (layer_idx == 0) {  // re-registration resets the bucket
    b.numels.clear();
    b.cfgs.clear();
    b.total = 0;
  }
  b.numels.push_back(numel);
  LayerConfig c;
  c.bits = bits;
  c.bucket_size = bucket_size > 0 ? bucket_size : 512;
  b.cfgs.push_back(c);
  b.total += numel;
  cursor_ = 0;
}

void Registry::set_bits(int bucket_idx, int layer_idx, int bits) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = by_idx_.find(bucket_idx);
  if (it == by_idx_.end()) return;
  auto& b = order_[it->second];
  if (layer_idx >= 0 && (size_t)layer_idx < b.cfgs.size())
    b.cfgs[layer_idx].bits = bits;
}

void Registry::set_bucket_size(int bucket_idx, int layer_idx, int bucket_size) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = by_idx_.find(bucket_idx);
  if (it == by_idx_.end()) return;
  auto& b = order_[it->second];
  if (layer_idx >= 0 && (size_t)layer_idx < b.cfgs.size())
    b.cfgs[layer_idx].bucket_size = bucket_size;
}

void Registry::clear() {
  std::lock_guard<std::mutex> g(mu_);
  order_.clear();
  by_idx_.clear();
  bound_.clear();
  cursor_ = 0;
}

bool Registry::empty() {
  std::lock_guard<std::mutex> g(mu_);
  return order_.empty();
}

std::vector<Registry::BucketInfo> Registry::snapshot() {
  std::lock_guard<std::mutex> g(mu_);
  return order_;
}

bool Registry::next(int64_t numel, const void* key, BucketInfo* out) {
  std::lock_guard<std::mutex> g(mu_);
  if (order_.empty()) return false;
  // pointer identity first: a previously seen flat-bucket storage resolves
  // to the bucket it matched before, regardless of cursor position
  if (key) {
    auto it = bound_.find(key);
    if (it != bound_.end()) {
      const size_t i = it->second;
      if (i < order_.size() && order_[i].total == numel) {
        *out = order_[i];
        cursor_ = i + 1;
        return true;
      }
      bound_.erase(it);  // bucket rebuilt or storage reused: unlearn
    }
  }
  const size_t n = order_.size();
  const size_t start = cursor_ % n;
  // prefer the cursor position; otherwise any bucket whose total matches
  for (size_t k = 0; k < n; k++) {
    const size_t i = (start + k) % n;
    if (order_[i].total == numel) {
      *out = order_[i];
      cursor_ = i + 1;
      if (key) bound_[key] = i;
      return true;
    }
  }
  return false;
}

}  // namespace cgx
