// The integer tickets of the split-K decode kernels (decode.hip, recurrent_decode.hip): the workgroups of a tile draw one each, the one that
// draws the last adds the slices' sums in slice order and puts the ticket back to zero.
#pragma once
#include <map>
#include <mutex>
#include "device_utils.h"

namespace lamp {

constexpr int kDecMaxTiles = 4096;    // tickets per stream

// the tickets of a stream's split-K launches: zeroed once, every launch leaves them zero.  One buffer per (device, stream): launches on one
// stream are ordered, launches on two streams never share a ticket.
inline unsigned* dec_tickets(int device, hipStream_t st) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, unsigned*> bufs;
  std::lock_guard<std::mutex> lk(mu);
  auto it = bufs.find({device, st});
  if (it != bufs.end()) return it->second;
  void* q = nullptr;
  HIP_CHECK(hipMalloc(&q, kDecMaxTiles * sizeof(unsigned)));
  HIP_CHECK(hipMemsetAsync(q, 0, kDecMaxTiles * sizeof(unsigned), st));
  bufs[{device, st}] = (unsigned*)q;
  return (unsigned*)q;
}

}  // namespace lamp
