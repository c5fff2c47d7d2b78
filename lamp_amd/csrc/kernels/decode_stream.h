// The split-K weight-streaming kernels of decoding (decode.hip: out = epilogue(LN(x) . W); recurrent_decode.hip: the recurrent cell on
// [table[token], state] . W) share everything but three things, which an operation type supplies to the one body, decode_stream_body.h, that each kernel includes:
//   prepare(tid, lane, wave)   what a workgroup works out per row before the image, with its barrier
//   image(r, k)                the value of row r at position k of K, in acc_t
//   finish(a, r, n0)           what becomes of the finished sums of the lane's CL columns n0 .. of row r
// The body: grid (tiles of 64 * CL columns, S slices of K), four waves that each take a quarter of the slice.  The slice of the row
// operand sits in LDS (acc_t) as [k][row] and is read as a broadcast; a lane owns CL neighbouring columns in CL / V packets, keeps
// RT x CL sums and has the weight packets of dec_unroll steps of k in flight.  The waves' sums are added in wave order through LDS.  With
// more than one slice every workgroup stores its sums into its slab, publishes them (agent-scope release, then an integer ticket per tile),
// and the workgroup that draws the last ticket acquires, adds the slabs in slice order (a wave per row, kDecSlabBatch slabs' loads in
// flight), finishes and puts the ticket back to zero.  No floating atomic, every sum in a fixed order.
// The host side is one plan (dec_plan: a value worked out from the sizes and a CU count, no device touched), the choice of a lane's
// columns (dec_form) and the ladder over the row counts (dec_rt_ladder); tests/test_decode_plan.py pins all three.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <type_traits>
#include "device_utils.h"

namespace lamp {

constexpr int kDecMaxRows = LAMP_DECODE_MAX_ROWS;
constexpr int kDecKcMax = 256;        // the longest slice of K a workgroup takes: the LDS image is [kDecKcMax][RT]
constexpr int kDecUnroll = 8;         // steps of k whose weight packets are in flight per lane (dec_unroll: 4 when a lane's columns are more than 16 bytes)
constexpr int kDecWaves = 4;          // waves of a workgroup: each takes a quarter of the workgroup's slice of K
constexpr int kDecStep = kDecWaves * kDecUnroll;   // slices of K are multiples of this
constexpr int kDecMaxSlices = 16;     // slices of K across workgroups (8 beyond four rows)
constexpr int kDecSlabBatch = 8;      // slabs whose loads the reducing workgroup keeps in flight
constexpr int kDecMaxTiles = 4096;    // tickets per stream
// what a launch computes: 0 .. 2 are LAMP_RECURRENT_RNN / _GRU / _LSTM (GRU: its first phase)
constexpr int kDecFormGru2 = 3;       // GRU's second phase
constexpr int kDecFormLinear = 4;     // decode_linear_kn_kernel

__device__ __forceinline__ float dec_erf(float v) { return erff(v); }
__device__ __forceinline__ double dec_erf(double v) { return erf(v); }
__device__ __forceinline__ float dec_exp(float v) { return expf(v); }
__device__ __forceinline__ double dec_exp(double v) { return exp(v); }
__device__ __forceinline__ float dec_log(float v) { return logf(v); }
__device__ __forceinline__ double dec_log(double v) { return log(v); }
__device__ __forceinline__ float dec_tanh(float v) { return tanhf(v); }
__device__ __forceinline__ double dec_tanh(double v) { return tanh(v); }
template <class T> __device__ __forceinline__ T dec_sigmoid(T x) { return T(1) / (T(1) + dec_exp(-x)); }   // rc_sigmoid of recurrent.hip

constexpr int dec_unroll(int CL, size_t tsize) { return CL * tsize > 16 ? kDecUnroll / 2 : kDecUnroll; }

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
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

inline bool dec_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs) if (q && (uintptr_t)q % 16) return false;
  return true;
}
// the one stride of a tensor that is a vector or one row / column of a matrix; `must`: what to say of one that is not
inline int64_t dec_vector_stride(const lamp_tensor* v, const char* must) {
  int64_t stride = 1;
  int big = 0;
  for (int i = 0; i < v->ndim; i++) if (v->sizes[i] != 1) { big++; stride = v->strides[i]; }
  LAMP_CHECK(big <= 1, must << ", got " << v->describe());
  return stride;
}

// a lane's columns: CL of them in packets of V, `unroll` steps of k in flight.  The cells own whole hidden units (LSTM four gates, GRU's
// first phase three), everything else one packet; V > 1 only when N % V == 0 and w is 16-byte aligned, and never for GRU's three columns.
struct DecForm { int CL, V, unroll; };
inline DecForm dec_form(int form, int64_t N, size_t tsize, bool aligned) {
  const int VW = 16 / (int)tsize;
  const int V = form != LAMP_RECURRENT_GRU && N % VW == 0 && aligned ? VW : 1;
  const int CL = form == LAMP_RECURRENT_LSTM ? 4 : form == LAMP_RECURRENT_GRU ? 3 : V;
  return {CL, V, dec_unroll(CL, tsize)};
}

// slices of K: about two waves per compute unit in all, at most kDecMaxSlices slices, none shorter than two unrolled steps per wave or
// longer than the LDS image, and no more slab bytes than weight bytes
struct DecPlan { int64_t tiles; int Kc, S; dim3 grid, block; };
inline DecPlan dec_plan(int64_t K, int64_t N, int64_t R, int CL, size_t tsize, size_t asize, int64_t cus) {
  const int64_t tiles = (N + 64 * CL - 1) / (64 * CL);
  LAMP_CHECK(tiles <= kDecMaxTiles, N << " columns are more than " << kDecMaxTiles << " tiles");
  int64_t want = (cus / 2 + tiles - 1) / tiles;
  want = std::min<int64_t>(std::min<int64_t>(want, R > 4 ? kDecMaxSlices / 2 : kDecMaxSlices), std::max<int64_t>(1, (int64_t)(K * tsize) / (int64_t)(R * asize)));
  int64_t Kc = (K + want - 1) / want;
  Kc = std::min<int64_t>(kDecKcMax, (std::max<int64_t>(Kc, 2 * kDecStep) + kDecStep - 1) / kDecStep * kDecStep);
  const int64_t S = (K + Kc - 1) / Kc;
  return {tiles, (int)Kc, (int)S, dim3((unsigned)tiles, (unsigned)S), dim3(64 * kDecWaves)};
}
// the plan into the launch's arguments; S > 1: the slabs (kept alive by `slab`) and the stream's tickets
template <class A, class P>
void dec_plan_apply(P& p, const DecPlan& pl, int dev, hipStream_t st, Hold& slab) {
  p.Kc = pl.Kc; p.S = pl.S;
  if (pl.S == 1) return;
  int64_t ss[3] = {pl.S, p.R, p.N};
  slab = Hold(new_tensor(ss, 3, sizeof(A) == 8 ? kF64 : kF32, dev));
  p.slab = slab->ptr<A>();
  p.ticket = dec_tickets(dev, st);
}

// the kernels are built for 1, 4 and 16 rows: launch(std::integral_constant<int, RT>)
inline int dec_rt(int R) { return R == 1 ? 1 : R <= 4 ? 4 : 16; }
template <class F> void dec_rt_ladder(int R, F&& launch) {
  switch (dec_rt(R)) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default: launch(std::integral_constant<int, 16>{}); break;
  }
}

}  // namespace lamp
