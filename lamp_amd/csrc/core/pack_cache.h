// The packed-filter cache of the convolution backends that pack their filters: conv_igemm.hip (bf16 implicit GEMM), conv_igemm_f32.hip
// (f32 / f64 implicit GEMM), conv_narrow.hip (bf16 narrow) and conv_small.hip (cs2_*, f32 / f64 narrow).  Each owns ONE instance; the
// backends keep their image sizes, their pack kernels and those kernels' argument blocks.  Host code only.
//
// A packed image is cached per (filter storage, view, geometry tag, stream) while the storage's version is unchanged: every kernel that
// writes a tensor obtains a mutable pointer through Tensor::data() / ptr<T>(), which bumps the version (core/tensor.h), so "same version"
// proves "same contents".  A training step packs each filter once, with frozen weights nothing is packed again at all.
//
// The contract (a captured HIP graph keeps READING a cached image's address, so a stale or evicted image trains on old weights):
//  - A hit needs equal storage versions, of both filters where the image holds a pair.  Versions are read with memory_order_relaxed.
//  - Storages that wrap caller memory (lamp_tensor_from_blob) and `scratch` storages (a strided filter's contiguous copy, which dies
//    with the call) are never cached: cacheable().
//  - The optimiser's hook re-packs IN PLACE: the packed tensor's address does not change across optimiser steps, so a graph captured
//    earlier keeps reading current weights.  The entry belongs to the hook's stream, so every convolution that read the old image is
//    ordered before the pack launch.
//  - Pinned entries (found or inserted while a graph was being captured) are never evicted and never dropped.
//  - The re-pack loop continues past every full batch (it once stopped at 16 images, and a replayed graph that had captured a cache
//    hit kept reading the stale seventeenth).
//  - A narrow image is re-packed only from tensors the hook was handed (no data pointers are kept in an entry).  A pair entry with one
//    filter absent is dropped unless pinned; a pinned one stays, stale by its versions, as when a parameter is written outside the
//    optimiser.
//  - The cache's lock is held from the walk until the pack launches are queued (the narrow hook's last batch: until it is handed over).
//  - The narrow images of the hook's last batch ride in the implicit-GEMM pack launch (ig_ncv_pack_many_kernel, conv_igemm.hip).
// LAMP_PACK_CACHE=0 disables the caches, LAMP_PACK_AFTER_STEP=0 the optimiser's hook (conv_repack_cached, conv.hip): lazy packs at first use.
#pragma once
#include <array>
#include <functional>
#include <map>
#include <mutex>
#include <tuple>
#include "tensor.h"

extern "C" int lamp_debug_pack_cache_counts(uint64_t out[5]);

namespace lamp {

struct PackKey {
  uint64_t uid; int64_t offset;       // the filter's storage and view
  std::array<int, 8> tag;             // the backend's geometry tag (unused slots 0)
  hipStream_t st;
  uint64_t uid2; int64_t offset2;     // the sibling filter packed into the same image (0 / 0: none)
  bool operator<(const PackKey& o) const { return std::tie(uid, offset, tag, st, uid2, offset2) < std::tie(o.uid, o.offset, o.tag, o.st, o.uid2, o.offset2); }
  // the key of a single filter [Cout][Cin][KS][KS] of one element type: tag = KS, Cout, Cin, dtype
  static PackKey filter(const Tensor* w, int KS, int Cout, int Cin, hipStream_t st) {
    return PackKey{w->st->uid, w->offset, {KS, Cout, Cin, w->dtype}, st, 0, 0};
  }
};
struct PackEntry { uint64_t version, version2; Tensor* packed; uint64_t tick; bool pinned; };   // version2: the sibling's; pinned: a captured graph reads this address

class PackCache {
 public:
  static constexpr size_t kCapacity = 256;
  PackCache();
  static bool cacheable(const Tensor* w, const Tensor* w2 = nullptr);
  static uint64_t version_of(const Tensor* w) { return w ? w->st->version.load(std::memory_order_relaxed) : 0; }

  Tensor* find(const PackKey& key, uint64_t version, uint64_t version2 = 0);    // +1 handle on the cached image, or nullptr
  // after a miss's pack launch: replaces the key's entry, evicts the least recently used unpinned entry at capacity, retains `packed`
  void insert(const PackKey& key, uint64_t version, uint64_t version2, Tensor* packed);

  // The entries of one stream, under the cache's lock.  visit() may bring an entry up to date with touch() (the image is being packed
  // again from current weights) or return false to drop it - a pinned entry stays whatever it returns.  queued() runs after the last
  // entry, still under the lock: the place for the pack launches that are left.
  void walk(hipStream_t st, const std::function<bool(const PackKey&, PackEntry&)>& visit, const std::function<void()>& queued);
  void touch(PackEntry& e, uint64_t version, uint64_t version2 = 0);

  // The optimiser hook of the single-filter caches: for every parameter of `dtype` whose image (key PackKey::filter of its own sizes)
  // is cached on `st`, add(slot, weight, key, packed) puts the image into the backend's argument block (false: not this one);
  // flush(cnt, last) launches the pack of slots 0 .. cnt - 1, after every `max` images and once more (last) for what is left at the
  // end.  Then the entries move to the weights' current versions.
  void repack(lamp_tensor* const* params, int n, hipStream_t st, int dtype, int max,
              const std::function<bool(int, const Tensor*, const PackKey&, Tensor*)>& add, const std::function<void(int, bool)>& flush);

 private:
  friend int ::lamp_debug_pack_cache_counts(uint64_t out[5]);
  std::mutex mu_;
  std::map<PackKey, PackEntry> map_;
  uint64_t tick_ = 0;
  uint64_t hits_ = 0, packs_ = 0, repacked_ = 0;     // lamp_debug_pack_cache_counts
};

}  // namespace lamp
