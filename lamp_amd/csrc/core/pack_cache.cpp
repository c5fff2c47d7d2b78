// The packed-filter cache of the convolution backends: see pack_cache.h for the contract.
#include "pack_cache.h"

#include <algorithm>
#include <vector>
#include "switches.h"

namespace lamp {

static std::mutex g_instances_mu;
static std::vector<PackCache*>& instances() { static std::vector<PackCache*> v; return v; }   // (the caches are other files' globals)

PackCache::PackCache() { std::lock_guard<std::mutex> lk(g_instances_mu); instances().push_back(this); }

bool PackCache::cacheable(const Tensor* w, const Tensor* w2) {
  return sw().pack_cache && w->st->owned && !w->st->scratch && (!w2 || (w2->st->owned && !w2->st->scratch));
}

Tensor* PackCache::find(const PackKey& key, uint64_t version, uint64_t version2) {
  std::lock_guard<std::mutex> lk(mu_);
  auto it = map_.find(key);
  if (it == map_.end() || it->second.version != version || it->second.version2 != version2) return nullptr;
  it->second.tick = ++tick_;
  if (allocator_capturing()) it->second.pinned = true;   // the graph being captured records this address: never evict the entry
  hits_++;
  return retain(it->second.packed);
}

void PackCache::insert(const PackKey& key, uint64_t version, uint64_t version2, Tensor* packed) {
  std::lock_guard<std::mutex> lk(mu_);
  packs_++;
  auto it = map_.find(key);
  if (it != map_.end()) { release(it->second.packed); map_.erase(it); }
  if (map_.size() >= kCapacity) {               // evict the least recently used entry that no captured graph reads
    auto victim = map_.end();
    for (auto i = map_.begin(); i != map_.end(); ++i)
      if (!i->second.pinned && (victim == map_.end() || i->second.tick < victim->second.tick)) victim = i;
    if (victim != map_.end()) { release(victim->second.packed); map_.erase(victim); }
  }
  map_[key] = PackEntry{version, version2, retain(packed), ++tick_, allocator_capturing()};
}

void PackCache::touch(PackEntry& e, uint64_t version, uint64_t version2) {
  e.version = version; e.version2 = version2; e.tick = ++tick_; repacked_++;
}

void PackCache::walk(hipStream_t st, const std::function<bool(const PackKey&, PackEntry&)>& visit, const std::function<void()>& queued) {
  std::lock_guard<std::mutex> lk(mu_);
  for (auto it = map_.begin(); it != map_.end();) {
    if (it->first.st != st || visit(it->first, it->second) || it->second.pinned) { ++it; continue; }
    release(it->second.packed);
    it = map_.erase(it);
  }
  queued();
}

void PackCache::repack(lamp_tensor* const* params, int n, hipStream_t st, int dtype, int max,
                       const std::function<bool(int, const Tensor*, const PackKey&, Tensor*)>& add, const std::function<void(int, bool)>& flush) {
  std::lock_guard<std::mutex> lk(mu_);
  if (map_.empty()) return;
  std::vector<std::pair<PackEntry*, uint64_t>> done;    // (entry, storage version its image now corresponds to)
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    if (cnt == max) { flush(cnt, false); cnt = 0; }     // one launch per `max` images, and the loop goes on
    const Tensor* w = params[i];
    if (!w || !w->is_device() || w->dtype != dtype || w->ndim != 4 || !w->st->owned || !w->is_contiguous()) continue;
    auto it = map_.find(PackKey::filter(w, (int)w->sizes[2], (int)w->sizes[0], (int)w->sizes[1], st));
    if (it == map_.end() || !add(cnt, w, it->first, it->second.packed)) continue;
    done.push_back({&it->second, version_of(w)});
    cnt++;
  }
  if (cnt > 0) flush(cnt, true);
  for (auto& d : done) touch(*d.first, d.second);
}

}  // namespace lamp

// For the tests (not in the public header; a cache hit and a fresh pack give the same values, only this tells them apart):
// {entries, pinned entries, hits, packs (misses that launched a pack), images re-packed by the optimiser's hook}, summed over the instances
extern "C" int lamp_debug_pack_cache_counts(uint64_t out[5]) {
  using namespace lamp;
  std::fill(out, out + 5, 0);
  std::lock_guard<std::mutex> lk(g_instances_mu);
  for (PackCache* c : instances()) {
    std::lock_guard<std::mutex> lc(c->mu_);
    out[0] += c->map_.size();
    for (auto& kv : c->map_) out[1] += kv.second.pinned ? 1 : 0;
    out[2] += c->hits_; out[3] += c->packs_; out[4] += c->repacked_;
  }
  return 0;
}
