// BERT's input embedding (lamp-core/src/main/scala/lamp/nn/bert/bert.scala:395-404):
//   embedded = tokenEmbedding(tokens) + segmentEmbedding(segments) + positionalEmbedding[:, :T]
// as one launch forward and a grouped, gather-only gradient; f32, f64 and bf16.
//
// Forward (bert_embedding_fwd_kernel): a thread per packet of an output row reads the three source packets and adds them in the chain's
// order.  f32 / f64 round after each addition, so the result has the bits of Embedding + Embedding + slice; bf16 adds in f32 and rounds once.
//
// Backward.  A table's gradient is a segment sum keyed by id: dW[v, :] = sum of dout[n, :] over the positions n with ids[n] == v.  The
// positions of BOTH tables are grouped at once: an entry e < N is position e of the token table, an entry e >= N position e - N of the
// segment table; table t owns the groups base_t .. base_t + R_t, the last of which ("nowhere") takes every id outside [0, R_t) and the
// padding id.
//   bert_group_keys_kernel    key of every entry, and the histogram of the keys (integer atomics, one per distinct key of a wave)
//   bert_group_rowptr_kernel  one workgroup: the exclusive prefix sum of the histogram (rowptr) and of the groups' chunk counts (chunkptr)
//   lamp_argsort              the entries stably sorted by key: inside a group the positions ascend
//   bert_chunk_sum_kernel     a group of more than kBertLongRow entries is cut into chunks of kBertLongRow; a wave per chunk writes the
//                             chunk's sum (acc_t) into a workspace
//   bert_row_sum_kernel       a wave per group: a short group is summed in order in acc_t and rounded once, a long one is the sum of its
//                             chunks' partial sums in chunk order; a group without entries writes zeros.  Every element of every output row
//                             is written exactly once, there is no fill and no floating atomic: the result is a function of the input.
// The lanes of a wave run across the columns in packets of 16 bytes where D * sizeof(T) and the addresses allow it, one element otherwise;
// columns beyond one wave's reach are tiled in grid.y.  dPositional is a launch of its own: a thread per packet of a position sums over
// the batch in ascending order.
#include <algorithm>
#include <cstdint>
#include "device_utils.h"

namespace lamp {
namespace {

constexpr int kBertLongRow = 128;   // a group with more entries is summed in chunks of this many
constexpr int kBertWaves = 4;       // waves (= groups or chunks) per workgroup
constexpr int kBertUnroll = 4;      // gradient rows in flight per wave

struct BertTables {                 // the tables one backward call groups (1 or 2)
  const int64_t* ids[2];
  void* out[2];
  int64_t rows[2];                  // R_t
  int64_t base[3];                  // first group of table t; base[nt] = number of groups
  int nt;
};

template <class T, int V> __device__ __forceinline__ Vec<T, V> bert_load(const T* p) { return *reinterpret_cast<const Vec<T, V>*>(p); }
template <class T, int V> __device__ __forceinline__ void bert_store(T* p, const Vec<T, V>& v) { *reinterpret_cast<Vec<T, V>*>(p) = v; }

// ---- forward --------------------------------------------------------------------------------------------------------------------------------
template <class T, int V>
__global__ __launch_bounds__(256) void bert_embedding_fwd_kernel(const T* __restrict__ tokW, const T* __restrict__ segW, const T* __restrict__ pos,
                                                                 const int64_t* __restrict__ tokens, const int64_t* __restrict__ segments,
                                                                 T* __restrict__ out, int64_t N, int64_t Tn, int64_t D, int64_t Vt, int64_t Vs) {
  using A = acc_t<T>;
  const int64_t ppr = D / V, total = N * ppr;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = p / ppr, c = (p - n * ppr) * V, t = n % Tn;
    int64_t a = tokens[n], s = segments[n];
    if (a < 0) a += Vt;
    if (s < 0) s += Vs;
    Vec<T, V> va, vs, r;
    // the bound is tested before an address is formed
    if (a >= 0 && a < Vt) va = bert_load<T, V>(tokW + a * D + c);
    else {
#pragma unroll
      for (int j = 0; j < V; j++) va.v[j] = store_as<T>(A(0));
    }
    if (s >= 0 && s < Vs) vs = bert_load<T, V>(segW + s * D + c);
    else {
#pragma unroll
      for (int j = 0; j < V; j++) vs.v[j] = store_as<T>(A(0));
    }
    const Vec<T, V> vp = bert_load<T, V>(pos + t * D + c);
#pragma unroll
    for (int j = 0; j < V; j++) {
      // T = A (f32 / f64): two roundings, as the chain's two adds; bf16: both adds in f32, one rounding
      const A ab = load_as<A>(va.v[j]) + load_as<A>(vs.v[j]);
      r.v[j] = store_as<T>(ab + load_as<A>(vp.v[j]));
    }
    bert_store<T, V>(out + n * D + c, r);
  }
}

// ---- grouping -------------------------------------------------------------------------------------------------------------------------------
// keys[e] = the group of entry e; counts[g] += 1.  The lanes of a wave that share a key add once: a table of two rows, or a batch that is
// half padding, would otherwise queue thousands of atomics on one address.
__global__ __launch_bounds__(256) void bert_group_keys_kernel(BertTables tb, int64_t N, int64_t paddingIdx, int64_t* __restrict__ keys,
                                                              int* __restrict__ counts) {
  const int64_t total = (int64_t)tb.nt * N;
  const int lane = threadIdx.x & 63;
  // whole waves enter the loop body together (the bound is rounded up to the wave): the ballots below see every lane
  const int64_t rounded = (total + 63) / 64 * 64;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < rounded; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t key = -1;
    if (e < total) {
      const int t = e >= N ? 1 : 0;
      const int64_t id = tb.ids[t][e - (int64_t)t * N], R = tb.rows[t];
      key = tb.base[t] + ((id >= 0 && id < R && id != paddingIdx) ? id : R);
      keys[e] = key;
    }
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
      const int first = __ffsll((long long)todo) - 1;
      const int64_t k = lane_bcast(key, first);
      const unsigned long long same = __ballot(key == k);
      if (lane == first) atomicAdd(&counts[k], (int)__popcll(same));
      todo &= ~same;
    }
  }
}

// rowptr = exclusive prefix sum of counts ([G + 1]); chunkptr = exclusive prefix sum of the groups' chunk counts ([G + 1]): a group of more
// than kBertLongRow entries that is no table's "nowhere" group has ceil(count / kBertLongRow) chunks, every other group none.
// One workgroup: thread t owns a contiguous share of the groups, the shares' sums are scanned through LDS; G beyond 1024 only makes the
// shares longer.
__global__ __launch_bounds__(1024) void bert_group_rowptr_kernel(const int* __restrict__ counts, int* __restrict__ rowptr, int* __restrict__ chunkptr,
                                                                 int64_t G, BertTables tb) {
  __shared__ int part[1024], cpart[1024];
  const int t = threadIdx.x;
  const int64_t per = (G + 1023) / 1024;
  const int64_t b = t * per < G ? t * per : G, e = b + per < G ? b + per : G;
  auto chunks = [&](int64_t g, int c) {
    bool nowhere = false;
    for (int u = 0; u < tb.nt; u++) nowhere |= g == tb.base[u] + tb.rows[u];
    return (c > kBertLongRow && !nowhere) ? (c + kBertLongRow - 1) / kBertLongRow : 0;
  };
  int s = 0, cs = 0;
  for (int64_t i = b; i < e; i++) { const int c = counts[i]; s += c; cs += chunks(i, c); }
  part[t] = s; cpart[t] = cs;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0, cv = t >= o ? cpart[t - o] : 0;
    __syncthreads();
    part[t] += v; cpart[t] += cv;
    __syncthreads();
  }
  int run = part[t] - s, crun = cpart[t] - cs;
  for (int64_t i = b; i < e; i++) {
    const int c = counts[i];
    rowptr[i] = run; chunkptr[i] = crun;
    run += c; crun += chunks(i, c);
  }
  if (t == 1023) { rowptr[G] = part[1023]; chunkptr[G] = cpart[1023]; }
}

// ---- sums -----------------------------------------------------------------------------------------------------------------------------------
// acc += sum over p in [b, e), in that order, of dout[position(perm[p]), c .. c + V); b, e wave-uniform
template <class T, int V>
__device__ __forceinline__ void bert_gather(acc_t<T> (&acc)[V], const T* __restrict__ doutc, int64_t D, const int64_t* __restrict__ perm, int64_t N,
                                            int64_t b, int64_t e) {
  using A = acc_t<T>;
  int64_t p = b;
  for (; p + kBertUnroll <= e; p += kBertUnroll) {
    Vec<T, V> v[kBertUnroll];
#pragma unroll
    for (int u = 0; u < kBertUnroll; u++) {
      int64_t n = perm[p + u];
      if (n >= N) n -= N;
      v[u] = bert_load<T, V>(doutc + n * D);
    }
#pragma unroll
    for (int u = 0; u < kBertUnroll; u++)
#pragma unroll
      for (int j = 0; j < V; j++) acc[j] += load_as<A>(v[u].v[j]);
  }
  for (; p < e; p++) {
    int64_t n = perm[p];
    if (n >= N) n -= N;
    const Vec<T, V> v = bert_load<T, V>(doutc + n * D);
#pragma unroll
    for (int j = 0; j < V; j++) acc[j] += load_as<A>(v.v[j]);
  }
}

// chunk j of the long groups -> partial[j, :] (acc_t).  The group of a chunk is found by bisection in chunkptr.
template <class T, int V>
__global__ __launch_bounds__(64 * kBertWaves) void bert_chunk_sum_kernel(const T* __restrict__ dout, const int64_t* __restrict__ perm,
                                                                         const int* __restrict__ rowptr, const int* __restrict__ chunkptr,
                                                                         acc_t<T>* __restrict__ partial, int64_t N, int64_t D, int64_t G,
                                                                         int64_t maxChunks) {
  using A = acc_t<T>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * kBertWaves + wave;
  if (j >= maxChunks || j >= chunkptr[G]) return;
  int64_t lo = 0, hi = G - 1;                       // the last g with chunkptr[g] <= j: its chunkptr[g + 1] > j
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (chunkptr[mid] <= j) lo = mid; else hi = mid - 1;
  }
  const int64_t g = lo;
  const int64_t b = rowptr[g] + (j - chunkptr[g]) * kBertLongRow;
  const int64_t e = min(b + (int64_t)kBertLongRow, (int64_t)rowptr[g + 1]);
  const int64_t c = ((int64_t)blockIdx.y * 64 + lane) * V;
  if (c >= D) return;
  A acc[V];
#pragma unroll
  for (int k = 0; k < V; k++) acc[k] = A(0);
  bert_gather<T, V>(acc, dout + c, D, perm, N, b, e);
#pragma unroll
  for (int k = 0; k < V; k++) partial[j * D + c + k] = acc[k];
}

// a wave per group -> its row of its table
template <class T, int V>
__global__ __launch_bounds__(64 * kBertWaves) void bert_row_sum_kernel(BertTables tb, const T* __restrict__ dout, const int64_t* __restrict__ perm,
                                                                       const int* __restrict__ rowptr, const int* __restrict__ chunkptr,
                                                                       const acc_t<T>* __restrict__ partial, int64_t N, int64_t D) {
  using A = acc_t<T>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * kBertWaves + wave;
  if (g >= tb.base[tb.nt]) return;
  const int t = (tb.nt > 1 && g >= tb.base[1]) ? 1 : 0;
  const int64_t r = g - tb.base[t];
  if (r >= tb.rows[t]) return;                      // the "nowhere" group
  const int64_t c = ((int64_t)blockIdx.y * 64 + lane) * V;
  if (c >= D) return;
  const int64_t b = rowptr[g], e = rowptr[g + 1];
  A acc[V];
#pragma unroll
  for (int k = 0; k < V; k++) acc[k] = A(0);
  if (e - b <= kBertLongRow) {
    bert_gather<T, V>(acc, dout + c, D, perm, N, b, e);
  } else {
    for (int64_t j = chunkptr[g]; j < chunkptr[g + 1]; j++)
#pragma unroll
      for (int k = 0; k < V; k++) acc[k] += partial[j * D + c + k];
  }
  Vec<T, V> o;
#pragma unroll
  for (int k = 0; k < V; k++) o.v[k] = store_as<T>(acc[k]);
  bert_store<T, V>(static_cast<T*>(tb.out[t]) + r * D + c, o);
}

// dpos[t, :] = sum over b ascending of dout[b, t, :] (acc_t, rounded once) for t < T, zero for T <= t < L
template <class T, int V>
__global__ __launch_bounds__(256) void bert_positional_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dpos, int64_t B, int64_t Tn, int64_t L, int64_t D) {
  using A = acc_t<T>;
  const int64_t ppr = D / V, total = L * ppr;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = p / ppr, c = (p - t * ppr) * V;
    A acc[V];
#pragma unroll
    for (int k = 0; k < V; k++) acc[k] = A(0);
    if (t < Tn) {
      for (int64_t b = 0; b < B; b++) {
        const Vec<T, V> v = bert_load<T, V>(dout + (b * Tn + t) * D + c);
#pragma unroll
        for (int k = 0; k < V; k++) acc[k] += load_as<A>(v.v[k]);
      }
    }
    Vec<T, V> o;
#pragma unroll
    for (int k = 0; k < V; k++) o.v[k] = store_as<T>(acc[k]);
    bert_store<T, V>(dpos + t * D + c, o);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
// elements per packet: 16 bytes where the row length and every address allow it, one element otherwise
int bert_packet(int dtype, int64_t D, std::initializer_list<const void*> ptrs) {
  const int w = (int)(16 / dtype_size(dtype));
  if (D % w) return 1;
  for (const void* p : ptrs) if ((uintptr_t)p % 16) return 1;
  return w;
}
void check_ids(const lamp_tensor* ids, const char* what, int64_t B, int64_t Tn) {
  check_device_tensor(ids, what);
  LAMP_CHECK(ids->dtype == kI64, what << " must be int64, got " << ids->describe());
  LAMP_CHECK(ids->ndim == 2 && ids->sizes[0] == B && ids->sizes[1] == Tn, what << " " << ids->describe() << " is not [" << B << ", " << Tn << "]");
}
bool bert_dtype(int dt) { return dt == kF32 || dt == kF64 || dt == kBF16; }

// packet width as a template argument: f32 {4, 1}, f64 {2, 1}, bf16 {8, 1}
#define BERT_DISPATCH(DT, VW, T, V, ...)                                                                                   \
  switch (DT) {                                                                                                            \
    case kF32: { using T = float; if ((VW) == 4) { constexpr int V = 4; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } } break;     \
    case kF64: { using T = double; if ((VW) == 2) { constexpr int V = 2; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } } break;    \
    default: { using T = bf16_t; if ((VW) == 8) { constexpr int V = 8; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } } break;      \
  }

}  // namespace
}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_bert_long_row(int64_t* out) {
  LAMP_API_BEGIN
  *out = kBertLongRow;
  LAMP_API_END
}

int lamp_bert_embedding_forward(lamp_tensor** out, const lamp_tensor* tokenWeight, const lamp_tensor* segmentWeight, const lamp_tensor* positional,
                                const lamp_tensor* tokens, const lamp_tensor* segments) {
  LAMP_API_BEGIN
  check_device_tensor(tokenWeight, "tokenWeight"); check_device_tensor(segmentWeight, "segmentWeight"); check_device_tensor(positional, "positional");
  check_device_tensor(tokens, "tokens");
  const int dt = tokenWeight->dtype;
  LAMP_CHECK(bert_dtype(dt), "bert_embedding: f32, f64 or bf16 tables, got " << tokenWeight->describe());
  LAMP_CHECK(segmentWeight->dtype == dt && positional->dtype == dt, "bert_embedding: the tables differ in type: " << tokenWeight->describe() << ", "
                                                                        << segmentWeight->describe() << ", " << positional->describe());
  LAMP_CHECK(tokenWeight->ndim == 2 && segmentWeight->ndim == 2, "bert_embedding: tokenWeight and segmentWeight must be [V, D] and [Vs, D], got "
                                                                     << tokenWeight->describe() << " and " << segmentWeight->describe());
  const int64_t Vt = tokenWeight->sizes[0], D = tokenWeight->sizes[1], Vs = segmentWeight->sizes[0];
  LAMP_CHECK(segmentWeight->sizes[1] == D, "bert_embedding: segmentWeight " << segmentWeight->describe() << " has not tokenWeight's " << D << " columns");
  LAMP_CHECK((positional->ndim == 2 || (positional->ndim == 3 && positional->sizes[0] == 1)) && positional->sizes[positional->ndim - 1] == D,
             "bert_embedding: positional must be [1, L, " << D << "] or [L, " << D << "], got " << positional->describe());
  const int64_t L = positional->sizes[positional->ndim - 2];
  LAMP_CHECK(tokens->dtype == kI64 && tokens->ndim == 2, "bert_embedding: tokens must be int64 [B, T], got " << tokens->describe());
  const int64_t B = tokens->sizes[0], Tn = tokens->sizes[1], N = B * Tn;
  check_ids(segments, "segments", B, Tn);
  LAMP_CHECK(Tn <= L, "bert_embedding: " << Tn << " tokens per sequence, the positional table has " << L << " rows");
  const int dev = tokenWeight->device();
  LAMP_CHECK(segmentWeight->device() == dev && positional->device() == dev && tokens->device() == dev && segments->device() == dev,
             "bert_embedding: the arguments live on different devices");
  Hold tw(contiguous(tokenWeight)), sw(contiguous(segmentWeight)), pc(contiguous(positional)), tc(contiguous(tokens)), sc(contiguous(segments));
  int64_t os[3] = {B, Tn, D};
  Hold o(new_tensor(os, 3, dt, dev));
  if (N * D) {
    hipStream_t st = current_stream(dev);
    const int vw = bert_packet(dt, D, {tw->raw(), sw->raw(), pc->raw(), o->raw()});
    const double sz = (double)dtype_size(dt);
    KernelTimer kt("bert_embedding_fwd", 2.0 * N * D, (3.0 * N * D + (double)Tn * D) * sz + 16.0 * N, st);
    const int grid = grid_for(N * (D / vw), 256);
    BERT_DISPATCH(dt, vw, T, V, hipLaunchKernelGGL((bert_embedding_fwd_kernel<T, V>), dim3(grid), dim3(256), 0, st, tw->ptr<T>(), sw->ptr<T>(), pc->ptr<T>(),
                                                   tc->ptr<int64_t>(), sc->ptr<int64_t>(), o->ptr<T>(), N, Tn, D, Vt, Vs));
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take();
  LAMP_API_END
}

int lamp_bert_embedding_backward(lamp_tensor** dToken_or_null, lamp_tensor** dSegment_or_null, lamp_tensor** dPositional_or_null, const lamp_tensor* dout,
                                 const lamp_tensor* tokens, const lamp_tensor* segments, int64_t V, int64_t Vs, int64_t L, int64_t paddingIdx) {
  LAMP_API_BEGIN
  check_device_tensor(dout, "dout");
  const int dt = dout->dtype, dev = dout->device();
  LAMP_CHECK(bert_dtype(dt), "bert_embedding_backward: f32, f64 or bf16, got " << dout->describe());
  LAMP_CHECK(dout->ndim == 3, "bert_embedding_backward: dout must be [B, T, D], got " << dout->describe());
  const int64_t B = dout->sizes[0], Tn = dout->sizes[1], D = dout->sizes[2], N = B * Tn;
  LAMP_CHECK(V > 0 && Vs > 0 && L >= Tn, "bert_embedding_backward: V = " << V << ", Vs = " << Vs << ", L = " << L << " for sequences of " << Tn);
  LAMP_CHECK(2 * N < ((int64_t)1 << 31) && V + Vs + 2 < ((int64_t)1 << 31), "bert_embedding_backward: too many positions or rows");
  hipStream_t st = current_stream(dev);
  const double sz = (double)dtype_size(dt);
  Hold dc(contiguous(dout));
  Hold dtok, dseg, dpos;

  BertTables tb{};
  Hold idc[2];
  auto add_table = [&](const lamp_tensor* ids, const char* what, int64_t R, Hold& o) {
    check_ids(ids, what, B, Tn);
    LAMP_CHECK(ids->device() == dev, what << " and dout live on different devices");
    int64_t ws[2] = {R, D};
    o = Hold(new_tensor(ws, 2, dt, dev));
    idc[tb.nt] = Hold(contiguous(ids));
    tb.ids[tb.nt] = idc[tb.nt]->ptr<int64_t>();
    tb.out[tb.nt] = o->data();
    tb.rows[tb.nt] = R;
    tb.base[tb.nt + 1] = tb.base[tb.nt] + R + 1;
    tb.nt++;
  };
  if (dToken_or_null) add_table(tokens, "tokens", V, dtok);
  if (dSegment_or_null) add_table(segments, "segments", Vs, dseg);

  if (tb.nt && D) {
    if (N == 0) {
      if (dtok.get()) fill_zero(dtok.get());
      if (dseg.get()) fill_zero(dseg.get());
    } else {
      const int64_t G = tb.base[tb.nt], E = (int64_t)tb.nt * N;
      int64_t es[1] = {E}, gs[1] = {G}, g1[1] = {G + 1};
      Hold keys(new_tensor(es, 1, kI64, dev)), counts(new_tensor(gs, 1, kI32, dev)), rowptr(new_tensor(g1, 1, kI32, dev)), chunkptr(new_tensor(g1, 1, kI32, dev));
      fill_zero(counts.get());
      {
        KernelTimer kt("bert_group_keys", 0, 16.0 * E, st);
        hipLaunchKernelGGL(bert_group_keys_kernel, dim3(grid_for(E, 256)), dim3(256), 0, st, tb, N, paddingIdx, keys->ptr<int64_t>(), counts->ptr<int>());
        LAMP_LAUNCH_CHECK();
      }
      {
        KernelTimer kt("bert_group_rowptr", 0, 12.0 * G, st);
        hipLaunchKernelGGL(bert_group_rowptr_kernel, dim3(1), dim3(1024), 0, st, counts->ptr<int>(), rowptr->ptr<int>(), chunkptr->ptr<int>(), G, tb);
        LAMP_LAUNCH_CHECK();
      }
      lamp_tensor* pt = nullptr;
      LAMP_CHECK(lamp_argsort(&pt, keys.get(), 1, 0, 0) == 0, lamp_last_error());
      Hold perm(pt);
      LAMP_CHECK(perm->dtype == kI64 && perm->numel() == E && perm->is_contiguous(), "internal: perm " << perm->describe());
      // a long group has more than kBertLongRow entries, so at most E / (kBertLongRow + 1) groups are long, and a group of c entries has
      // at most c / kBertLongRow + 1 chunks
      const int64_t maxChunks = E > kBertLongRow ? E / kBertLongRow + E / (kBertLongRow + 1) : 0;
      Hold partial;
      const int adt = dt == kF64 ? kF64 : kF32;
      int64_t ps[2] = {std::max<int64_t>(maxChunks, 1), D};
      partial = Hold(new_tensor(ps, 2, adt, dev));
      // packets are read from dout and written to the tables' rows; the workspace is accessed element by element
      const int vw = bert_packet(dt, D, {dc->raw(), tb.out[0], tb.out[tb.nt - 1]});
      const unsigned tiles = (unsigned)((D / vw + 63) / 64);
      if (maxChunks) {
        KernelTimer kt("bert_chunk_sum", (double)E * D, (double)E * D * sz + 8.0 * E, st);
        BERT_DISPATCH(dt, vw, T, VW, hipLaunchKernelGGL((bert_chunk_sum_kernel<T, VW>), dim3((unsigned)((maxChunks + kBertWaves - 1) / kBertWaves), tiles),
                                                        dim3(64 * kBertWaves), 0, st, dc->ptr<T>(), perm->ptr<int64_t>(), rowptr->ptr<int>(),
                                                        chunkptr->ptr<int>(), partial->ptr<acc_t<T>>(), N, D, G, maxChunks));
        LAMP_LAUNCH_CHECK();
      }
      {
        KernelTimer kt("bert_row_sum", (double)E * D, ((double)E + (double)G) * D * sz + 8.0 * E + 8.0 * G, st);
        BERT_DISPATCH(dt, vw, T, VW, hipLaunchKernelGGL((bert_row_sum_kernel<T, VW>), dim3((unsigned)((G + kBertWaves - 1) / kBertWaves), tiles),
                                                        dim3(64 * kBertWaves), 0, st, tb, dc->ptr<T>(), perm->ptr<int64_t>(), rowptr->ptr<int>(),
                                                        chunkptr->ptr<int>(), partial->ptr<acc_t<T>>(), N, D));
        LAMP_LAUNCH_CHECK();
      }
    }
  }
  if (dPositional_or_null) {
    int64_t ps[3] = {1, L, D};
    dpos = Hold(new_tensor(ps, 3, dt, dev));
    if (L * D) {
      const int vw = bert_packet(dt, D, {dc->raw(), dpos->raw()});
      KernelTimer kt("bert_positional_bwd", (double)N * D, ((double)N + L) * D * sz, st);
      BERT_DISPATCH(dt, vw, T, VW, hipLaunchKernelGGL((bert_positional_bwd_kernel<T, VW>), dim3(grid_for(L * (D / vw), 256)), dim3(256), 0, st, dc->ptr<T>(),
                                                      dpos->ptr<T>(), B, Tn, L, D));
      LAMP_LAUNCH_CHECK();
    }
  }
  if (dToken_or_null) *dToken_or_null = dtok.take();
  if (dSegment_or_null) *dSegment_or_null = dseg.take();
  if (dPositional_or_null) *dPositional_or_null = dpos.take();
  LAMP_API_END
}

}  // extern "C"
