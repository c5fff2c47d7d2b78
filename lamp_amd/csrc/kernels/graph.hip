// Graph layers, f32 and f64: graph convolution (GCN), graph attention, message passing (MPNN) and the minibatches of small graphs
// (the collate kernels and the pooling over a sorted batch), each below under a heading of its own.  The reference builds sparse tensors or chains of indexSelect / indexAdd; here the edges are grouped per node once per graph
// (lamp_gcn_adjacency, lamp_graph_edge_csr: a rowptr and the stably sorted edges) and every sum per node is a gather-only kernel of one
// shape, the row kernel:
//
// A workgroup of kWaves waves owns kWaves neighbouring rows (nodes), a wave one row; the 64 lanes run across the columns in packets of V
// elements (16 bytes where the widths, pitches and addresses allow it), columns beyond one wave's reach are tiled in grid.y: every row
// read is one coalesced read and the output row one coalesced write.  Per 64 edges a wave reads what it needs of them once, one entry
// per lane, and hands the entries round with v_readlane, so a row's address is wave-uniform; U rows are in flight per wave
// (for_each_edge).  No atomics: a row's sum runs over its edges in the grouping's order, which the stable sort fixes, so a result is a
// function of the input alone.  A row of more than kLongRow edges (a hub) would serialise its wave: all waves of the workgroup take a
// contiguous share of its edges (wave_share) and wave 0 adds their partial sums through LDS in wave order (merge_shares).  GCN takes
// its long rows one after the other inside the workgroup; the other kernels give them a grid slice each (row_turn).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>
#include "device_utils.h"

namespace lamp {
namespace {

constexpr int kWaves = 16;          // waves (= rows) per workgroup of a row kernel
constexpr int kLongRow = 256;       // a row with more edges is split across the workgroup's waves
constexpr int kGcnUnroll = 8;       // neighbour rows in flight per wave
constexpr int kMpnnUnroll = 4;      // edge rows in flight per wave
constexpr int kMpnnEdgeBlock = 256; // threads per workgroup of the per-edge kernels

// what a lane reads of one edge before any row is read: NI indices and NF factors
template <class T, int NI, int NF> struct EdgeEntry {
  int64_t i[NI] = {};
  T f[NF ? NF : 1] = {};
  // lane k's entry, in every lane (k wave-uniform)
  __device__ __forceinline__ EdgeEntry bcast(int k) const {
    EdgeEntry r;
#pragma unroll
    for (int j = 0; j < NI; j++) r.i[j] = lane_bcast(i[j], k);
#pragma unroll
    for (int j = 0; j < NF; j++) r.f[j] = lane_bcast(f[j], k);
    return r;
  }
};
// what a lane has fetched for one edge: NS scalars and its packet of the edge's row
template <class T, int V, int NS> struct EdgeItem {
  T s[NS ? NS : 1];
  Vec<T, V> v;
};

// use(fetch(entry of edge p)) for p in [b, e), in that order (b and e wave-uniform): lane l reads load(p + l) for 64 edges at a time, the
// entries go round by bcast, U fetches are in flight before the first is used.  Every lane takes part in the index reads, also one that
// holds no column and fetches nothing.
template <int U, class Load, class Fetch, class Use>
__device__ __forceinline__ void for_each_edge(int64_t b, int64_t e, int lane, Load load, Fetch fetch, Use use) {
  for (int64_t p = b; p < e; p += 64) {
    const int n = (int)(e - p < 64 ? e - p : 64);
    decltype(load(p)) mine;
    if (lane < n) mine = load(p + lane);
    int k = 0;
    for (; k + U <= n; k += U) {
      decltype(fetch(mine)) item[U];
#pragma unroll
      for (int u = 0; u < U; u++) item[u] = fetch(mine.bcast(k + u));
#pragma unroll
      for (int u = 0; u < U; u++) use(item[u]);
    }
    for (; k < n; k++) use(fetch(mine.bcast(k)));
  }
}

// wave's share [lo, hi) of n items split over the workgroup's waves: contiguous, in wave order
struct Share { int64_t lo, hi; };
__device__ __forceinline__ Share wave_share(int64_t n, int wave) {
  const int64_t chunk = (n + kWaves - 1) / kWaves;
  const int64_t lo = wave * chunk < n ? wave * chunk : n;
  return {lo, lo + chunk < n ? lo + chunk : n};
}

// The row schedule of a grid of (ceil(N / kWaves), tiles, kWaves + 1) workgroups.  Slice z = 0 is the own turn: every wave its own row,
// unless it is a long one.  Slice z = k + 1 is the turn of the workgroup's k-th row if it is long, by all waves of the workgroup: `own`,
// r and takes() are then the same in every thread of the workgroup, so the barriers of that turn are.  A grid slice per k, so that long
// rows that are neighbours (hubs numbered 0, 1, 2, ...) run side by side and not one after the other in their workgroup; the workgroups
// of the slices k >= 0 whose row is short, nearly all of them, read two row pointers and leave.
// A kernel writes `for (int k = first_turn(); is_turn(k); k++) { const RowTurn t = row_turn(k, N, wave); ... }`: a loop of one turn, left
// with `continue`.  It stays a loop because the compiler's choice of which products of GatAcc::merge it contracts into an fma differs
// between the loop and the straight line, and the results of these kernels are held bitwise from release to release.
struct RowTurn {
  bool own;
  int64_t r;      // -1: no row
  // whether a row of n edges is this turn's business; and the wave's share of its edges
  __device__ __forceinline__ bool takes(int64_t n) const { return own != (n > kLongRow); }
  __device__ __forceinline__ Share share(int64_t n, int wave) const { return own ? Share{0, n} : wave_share(n, wave); }
};
__device__ __forceinline__ int first_turn() { return (int)blockIdx.z - 1; }
__device__ __forceinline__ bool is_turn(int k) { return k < (int)blockIdx.z && k < kWaves; }
__device__ __forceinline__ RowTurn row_turn(int k, int64_t N, int wave) {
  const int64_t row0 = (int64_t)blockIdx.x * kWaves;
  const int nrows = (int)(N - row0 < kWaves ? N - row0 : kWaves), i = k < 0 ? wave : k;
  return {k < 0, i < nrows ? row0 + i : -1};
}

// acc[a] of wave 0 += acc[a] of the waves 1, 2, ... in that order.  Every thread of the workgroup calls it.
template <class T, int V, int NA>
__device__ __forceinline__ void merge_shares(Vec<T, V> (&acc)[NA], Vec<T, V> (&part)[NA][kWaves][64], int wave, int lane, bool active) {
#pragma unroll
  for (int a = 0; a < NA; a++) part[a][wave][lane] = acc[a];
  __syncthreads();
  if (wave == 0 && active) {
#pragma unroll 1
    for (int w = 1; w < kWaves; w++) {
#pragma unroll
      for (int a = 0; a < NA; a++) {
        const Vec<T, V> q = part[a][w][lane];
#pragma unroll
        for (int j = 0; j < V; j++) acc[a].v[j] += q.v[j];
      }
    }
  }
  __syncthreads();
}

// ---- graph convolution (lamp-core/src/main/scala/lamp/nn/graph/GCN.scala:30-145) ------------------------------------------------------------
// D^-1/2 (A + A' + I) D^-1/2 X over a CSR of A + A'.  The reference builds a sparse COO tensor and multiplies it with `mm`; this library
// has no sparse tensor.  lamp_gcn_adjacency turns the edge list into (rowptr, col, dinv) once per graph, lamp_gcn_aggregate is the
// product, a row kernel (see the head of the file) whose entry per neighbour is col[p] and dinv[col[p]].  The matrix is symmetric, so
// the gradient with respect to X is the same kernel applied to the incoming gradient.

// acc += sum over p in [b, e), in that order, of dinv[col[p]] * x[col[p], c0 .. c0 + V).  xc = x + c0; lanes with `active` false hold
// no column (c0 >= D) and load no row.
template <class T, int V>
__device__ __forceinline__ void gcn_gather(Vec<T, V>& acc, const T* __restrict__ xc, int64_t ldx, const int64_t* __restrict__ col,
                                           const T* __restrict__ dinv, int64_t b, int64_t e, int lane, bool active) {
  using Entry = EdgeEntry<T, 1, 1>;
  using Item = EdgeItem<T, V, 1>;
  for_each_edge<kGcnUnroll>(
      b, e, lane,
      [&](int64_t p) {
        Entry en;
        en.i[0] = col[p];
        en.f[0] = dinv[en.i[0]];
        return en;
      },
      [&](const Entry& en) { return Item{{en.f[0]}, active ? load_packet<T, V>(xc + en.i[0] * ldx) : zero_packet<T, V>()}; },
      [&](const Item& it) {
#pragma unroll
        for (int j = 0; j < V; j++) acc.v[j] += it.s[0] * it.v.v[j];
      });
}

// out[r, :] = dinv[r] * (dinv[r] * x[r, :] + sum over the row's neighbours c, in CSR order, of dinv[c] * x[c, :]).  D % V == 0.
// grid: (ceil(N / kWaves), ceil(D / (64 * V))), block: kWaves * 64.
template <class T, int V>
__global__ __launch_bounds__(kWaves * 64) void gcn_aggregate_kernel(T* __restrict__ out, int64_t ldo, const T* __restrict__ x, int64_t ldx,
                                                                        const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                                        const T* __restrict__ dinv, int64_t N, int64_t D) {
  __shared__ Vec<T, V> part[kWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t c0 = ((int64_t)blockIdx.y * 64 + lane) * V;
  const bool active = c0 < D;
  const int64_t row0 = (int64_t)blockIdx.x * kWaves;
  const T* xc = x + c0;

  // every wave its own row, unless it is a long one
  const int64_t r = row0 + wave;
  if (r < N) {
    const int64_t b = rowptr[r], e = rowptr[r + 1];
    if (e - b <= kLongRow) {
      const T dr = dinv[r];
      Vec<T, V> acc = active ? load_packet<T, V>(xc + r * ldx) : zero_packet<T, V>();
#pragma unroll
      for (int j = 0; j < V; j++) acc.v[j] *= dr;
      gcn_gather<T, V>(acc, xc, ldx, col, dinv, b, e, lane, active);
      if (active) {
#pragma unroll
        for (int j = 0; j < V; j++) acc.v[j] *= dr;
        *reinterpret_cast<Vec<T, V>*>(out + r * ldo + c0) = acc;
      }
    }
  }

  // the long rows of this workgroup, one after the other, by all its waves (the conditions are the same in every thread of the workgroup).
  // Not merge_shares: this sum starts from the row's own term and adds the shares 0 to kWaves - 1 to it.
  const int nrows = (int)(N - row0 < kWaves ? N - row0 : kWaves);
  for (int k = 0; k < nrows; k++) {
    const int64_t lr = row0 + k;
    const int64_t b = rowptr[lr], e = rowptr[lr + 1];
    if (e - b <= kLongRow) continue;
    const Share sh = wave_share(e - b, wave);
    Vec<T, V> acc = zero_packet<T, V>();
    gcn_gather<T, V>(acc, xc, ldx, col, dinv, b + sh.lo, b + sh.hi, lane, active);
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && active) {
      const T dr = dinv[lr];
      Vec<T, V> s = load_packet<T, V>(xc + lr * ldx);
#pragma unroll
      for (int j = 0; j < V; j++) s.v[j] *= dr;
      for (int w = 0; w < kWaves; w++) {
        const Vec<T, V> q = part[w][lane];
#pragma unroll
        for (int j = 0; j < V; j++) s.v[j] += q.v[j];
      }
#pragma unroll
      for (int j = 0; j < V; j++) s.v[j] *= dr;
      *reinterpret_cast<Vec<T, V>*>(out + lr * ldo + c0) = s;
    }
    __syncthreads();
  }
}

// per workgroup the smallest and the largest value of a[0, n) and b[0, n) (b == nullptr: of a alone): out[2 * blockIdx.x] = min,
// out[2 * blockIdx.x + 1] = max
__global__ __launch_bounds__(256) void gcn_index_range_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t n,
                                                              int64_t* __restrict__ out) {
  __shared__ int64_t smn[4], smx[4];
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = a[i], w = b ? b[i] : v;
    mn = min(mn, min(v, w));
    mx = max(mx, max(v, w));
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) { mn = min(mn, smn[w]); mx = max(mx, smx[w]); }
    out[2 * blockIdx.x] = mn;
    out[2 * blockIdx.x + 1] = mx;
  }
}

// rowptr = exclusive prefix sum of counts ([N + 1], rowptr[N] = total), dinv = (counts + 1)^-1/2 (dinv == nullptr: the prefix sum
// alone).  counts == nullptr: all zero.
// One workgroup: thread t owns a contiguous share of the nodes, the shares' sums are scanned through LDS.
template <class T>
__global__ __launch_bounds__(1024) void gcn_rowptr_dinv_kernel(const int64_t* __restrict__ counts, int64_t* __restrict__ rowptr, T* __restrict__ dinv,
                                                               int64_t N) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (N + 1023) / 1024;
  const int64_t b = t * per < N ? t * per : N, e = b + per < N ? b + per : N;
  int64_t s = 0;
  if (counts) for (int64_t i = b; i < e; i++) s += counts[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int64_t v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t i = b; i < e; i++) {
    const int64_t c = counts ? counts[i] : 0;
    rowptr[i] = run;
    run += c;
    if (dinv) dinv[i] = (T)(1.0 / sqrt((double)(c + 1)));
  }
  if (t == 1023) rowptr[N] = part[1023];
}

// ---- graph attention (lamp-core/src/main/scala/lamp/nn/graph/GraphAttention.scala:172-197) ---------------------------------------------------
// Everything from `activations` to `h`: a softmax of score [E, H] over the edges that share a destination, and the sum of the source
// nodes' value rows [N, H, V] under those weights.  The reference writes it as exp / indexAdd / log / indexSelect / exp / indexSelect /
// Mult / indexAdd against one global maximum; here the edges are grouped by destination once per graph (lamp_graph_edge_csr: rowptr
// [N + 1] and the edge ids stably sorted by endpoint).
//
// gat_forward_kernel and gat_backward_value_kernel are row kernels (see the head of the file) over the C = H * V columns in packets of VW
// elements; an edge's entry is its id and its source row.  A packet of two may straddle a head boundary (V odd): ONE = false keeps a
// softmax state per element then, ONE = true one per lane; packets of four are used only where V % 4 == 0.  The softmax is the online
// form with one exp per edge and head: against the row's running maximum m, either the new score is larger (the sums so far are scaled
// by exp(m - x)) or it is not (it enters as exp(x - m)).
// edges in flight per wave (f64's exp leaves room for fewer)
template <class T> constexpr int gat_unroll() { return sizeof(T) == 8 ? 2 : 4; }

__device__ __forceinline__ float gat_exp(float x) { return expf(x); }
__device__ __forceinline__ double gat_exp(double x) { return exp(x); }
__device__ __forceinline__ float gat_log(float x) { return logf(x); }
__device__ __forceinline__ double gat_log(double x) { return log(x); }
template <class T> __device__ __forceinline__ T gat_neg_inf() { return -(T)INFINITY; }

// per lane: the running maximum m and the sum s = sum exp(x - m) of each head its packet touches, and a = sum exp(x - m) * value
template <class T, int VW, bool ONE> struct GatAcc {
  static constexpr int NH = ONE ? 1 : VW;
  T m[NH], s[NH];
  Vec<T, VW> a;
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int h = 0; h < NH; h++) { m[h] = gat_neg_inf<T>(); s[h] = T(0); }
    a = zero_packet<T, VW>();
  }
  // one edge: its scores x (finite) for the packet's heads and its value packet v
  __device__ __forceinline__ void step(const T (&x)[NH], const Vec<T, VW>& v) {
    T scale[NH], p[NH];
#pragma unroll
    for (int h = 0; h < NH; h++) {
      const bool up = x[h] > m[h];
      const T t = gat_exp(up ? m[h] - x[h] : x[h] - m[h]);      // m = -inf: exp(-inf) = 0
      scale[h] = up ? t : T(1);
      p[h] = up ? T(1) : t;
      m[h] = up ? x[h] : m[h];
      s[h] = s[h] * scale[h] + p[h];
    }
#pragma unroll
    for (int j = 0; j < VW; j++) a.v[j] = a.v[j] * scale[ONE ? 0 : j] + p[ONE ? 0 : j] * v.v[j];
  }
  // the state (mw, sw, q) of the edges that follow this one's
  __device__ __forceinline__ void merge(const T (&mw)[NH], const T (&sw)[NH], const Vec<T, VW>& q) {
    T cr[NH], cw[NH];
#pragma unroll
    for (int h = 0; h < NH; h++) {
      cr[h] = T(1); cw[h] = T(0);
      if (sw[h] > T(0)) {                                       // an empty share has m = -inf and takes no part
        const T mn = m[h] > mw[h] ? m[h] : mw[h];
        cr[h] = gat_exp(m[h] - mn);
        cw[h] = gat_exp(mw[h] - mn);
        m[h] = mn;
        s[h] = s[h] * cr[h] + sw[h] * cw[h];
      }
    }
#pragma unroll
    for (int j = 0; j < VW; j++) a.v[j] = a.v[j] * cr[ONE ? 0 : j] + q.v[j] * cw[ONE ? 0 : j];
  }
};

// use(item) for the edges perm[b .. e) in that order: item.s[.] = tab[edge, hh[.]] (tab [E, H]: the scores or the weights) and item.v =
// row src[edge], columns c0 .. c0 + VW (rc = rows + c0, pitch ld).  Lanes with `active` false hold no column: they get zeros.
template <class T, int VW, bool ONE, class Use>
__device__ __forceinline__ void gat_for_each_edge(const T* __restrict__ tab, int64_t H, const int (&hh)[ONE ? 1 : VW], const T* __restrict__ rc, int64_t ld,
                                                  const int64_t* __restrict__ perm, const int64_t* __restrict__ src, int64_t b, int64_t e, int lane,
                                                  bool active, Use use) {
  constexpr int NH = ONE ? 1 : VW;
  using Entry = EdgeEntry<T, 2, 0>;
  using Item = EdgeItem<T, VW, NH>;
  for_each_edge<gat_unroll<T>()>(
      b, e, lane,
      [&](int64_t p) {
        Entry en;
        en.i[0] = perm[p];
        en.i[1] = src[en.i[0]];
        return en;
      },
      [&](const Entry& en) {
        Item it;
#pragma unroll
        for (int h = 0; h < NH; h++) it.s[h] = active ? tab[en.i[0] * H + hh[h]] : T(0);
        it.v = active ? load_packet<T, VW>(rc + en.i[1] * ld) : zero_packet<T, VW>();
        return it;
      },
      use);
}

// out[r, c0 ..] = a / s, and lse[r, h] = m + log s from the lane that holds head h's first column; a row without an edge: zeros and -inf
template <class T, int VW, bool ONE>
__device__ __forceinline__ void gat_finish(const GatAcc<T, VW, ONE>& st, T* __restrict__ out, T* __restrict__ lse, int64_t r, int64_t C, int64_t H, int V,
                                           int c0, const int (&hh)[ONE ? 1 : VW]) {
  Vec<T, VW> o;
#pragma unroll
  for (int j = 0; j < VW; j++) {
    const T sj = st.s[ONE ? 0 : j];
    o.v[j] = sj > T(0) ? st.a.v[j] / sj : T(0);
    if ((!ONE || j == 0) && (c0 + j) % V == 0) lse[r * H + hh[ONE ? 0 : j]] = sj > T(0) ? st.m[ONE ? 0 : j] + gat_log(sj) : gat_neg_inf<T>();
  }
  *reinterpret_cast<Vec<T, VW>*>(out + r * C + c0) = o;
}

// out [N, C], lse [N, H] from score [E, H], value [N, H, V] (C = H * V, C % VW == 0; ONE: V % VW == 0) over the incoming grouping
// (rowptr, perm).  grid: (ceil(N / kWaves), ceil(C / (64 * VW)), kWaves + 1), block: kWaves * 64.
template <class T, int VW, bool ONE>
__global__ __launch_bounds__(kWaves * 64) void gat_forward_kernel(T* __restrict__ out, T* __restrict__ lse, const T* __restrict__ score,
                                                                      const T* __restrict__ value, const int64_t* __restrict__ edgeI,
                                                                      const int64_t* __restrict__ rowptr, const int64_t* __restrict__ perm, int64_t N,
                                                                      int64_t H, int V) {
  constexpr int NH = ONE ? 1 : VW;
  __shared__ Vec<T, VW> part[kWaves][64];
  __shared__ T pm[kWaves][NH][64], ps[kWaves][NH][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t C = H * V;
  const int c0 = ((int)blockIdx.y * 64 + lane) * VW;
  const bool active = c0 < C;
  int hh[NH];
#pragma unroll
  for (int h = 0; h < NH; h++) hh[h] = active ? (c0 + h) / V : 0;

  for (int k = first_turn(); is_turn(k); k++) {
    const RowTurn t = row_turn(k, N, wave);
    int64_t b = 0, n = 0;
    if (t.r >= 0) { b = rowptr[t.r]; n = rowptr[t.r + 1] - b; }
    if (!t.takes(n)) continue;
    const Share sh = t.share(n, wave);
    GatAcc<T, VW, ONE> st;
    st.init();
    gat_for_each_edge<T, VW, ONE>(score, H, hh, value + c0, C, perm, edgeI, b + sh.lo, b + sh.hi, lane, active,
                                  [&](const EdgeItem<T, VW, NH>& it) { st.step(it.s, it.v); });
    if (t.own) {
      if (active && t.r >= 0) gat_finish<T, VW, ONE>(st, out, lse, t.r, C, H, V, c0, hh);
      continue;
    }
    // not merge_shares: a share's state is rescaled to the common maximum as it is added (GatAcc::merge)
    part[wave][lane] = st.a;
#pragma unroll
    for (int h = 0; h < NH; h++) { pm[wave][h][lane] = st.m[h]; ps[wave][h][lane] = st.s[h]; }
    __syncthreads();
    if (wave == 0 && active) {
#pragma unroll 1
      for (int w = 1; w < kWaves; w++) {
        T mw[NH], sw[NH];
#pragma unroll
        for (int h = 0; h < NH; h++) { mw[h] = pm[w][h][lane]; sw[h] = ps[w][h][lane]; }
        st.merge(mw, sw, part[w][lane]);
      }
      gat_finish<T, VW, ONE>(st, out, lse, t.r, C, H, V, c0, hh);
    }
    __syncthreads();
  }
}

// dvalue[i, h, :] = sum over the edges e leaving i (the outgoing grouping, in its order) of a[e, h] * dout[edgeJ[e], h, :].  Same grid,
// same split of a long row; the partial sums are added in wave order.
template <class T, int VW, bool ONE>
__global__ __launch_bounds__(kWaves * 64) void gat_backward_value_kernel(T* __restrict__ dvalue, const T* __restrict__ a, const T* __restrict__ dout,
                                                                             const int64_t* __restrict__ edgeJ, const int64_t* __restrict__ rowptr,
                                                                             const int64_t* __restrict__ perm, int64_t N, int64_t H, int V) {
  constexpr int NH = ONE ? 1 : VW;
  __shared__ Vec<T, VW> part[1][kWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t C = H * V;
  const int c0 = ((int)blockIdx.y * 64 + lane) * VW;
  const bool active = c0 < C;
  int hh[NH];
#pragma unroll
  for (int h = 0; h < NH; h++) hh[h] = active ? (c0 + h) / V : 0;

  for (int k = first_turn(); is_turn(k); k++) {
    const RowTurn t = row_turn(k, N, wave);
    int64_t b = 0, n = 0;
    if (t.r >= 0) { b = rowptr[t.r]; n = rowptr[t.r + 1] - b; }
    if (!t.takes(n)) continue;
    const Share sh = t.share(n, wave);
    Vec<T, VW> acc[1] = {zero_packet<T, VW>()};
    gat_for_each_edge<T, VW, ONE>(a, H, hh, dout + c0, C, perm, edgeJ, b + sh.lo, b + sh.hi, lane, active, [&](const EdgeItem<T, VW, NH>& it) {
#pragma unroll
      for (int j = 0; j < VW; j++) acc[0].v[j] += it.s[ONE ? 0 : j] * it.v.v[j];
    });
    if (!t.own) merge_shares(acc, part, wave, lane, active);
    if (active && t.r >= 0 && (t.own || wave == 0)) *reinterpret_cast<Vec<T, VW>*>(dvalue + t.r * C + c0) = acc[0];
  }
}

// m = max and s = sum exp(. - m) of score[perm[rb .. re), h]: lanes across the edges, two butterflies, every lane gets both.  The score
// gradient takes the weights from these and not from lse: m + log s rounded to the type has lost log2 |m| bits of the weight
// exp(score - m) / s, which the forward pass, working against m, never loses.
template <class T>
__device__ __forceinline__ void gat_row_softmax(T& m, T& s, const T* __restrict__ score, const int64_t* __restrict__ perm, int64_t rb, int64_t re, int64_t H,
                                                int h, int lane) {
  m = gat_neg_inf<T>();
  for (int64_t p = rb + lane; p < re; p += 64) {
    const T x = score[perm[p] * H + h];
    m = x > m ? x : m;
  }
  m = wave_max(m);
  s = T(0);
  for (int64_t p = rb + lane; p < re; p += 64) s += gat_exp(score[perm[p] * H + h] - m);
  s = wave_sum(s);
}

// The edges perm[b .. e) of destination j, whose edges are perm[rb .. re): a[e, h] = exp(score[e, h] - m) / s with the row's m and s,
// dscore[e, h] = a * (<dout[j, h, :], value[i, h, :]> - delta), delta[j, h] = <dout[j, h, :], out[j, h, :]>, each written once by one lane.
// Two forms, chosen per launch:
//   lph > 0  (V = lph * VW, lph a power of two up to 64): lanes across the C columns in packets, tile after tile; a head's columns sit in
//            lph neighbouring lanes, its dot product is a butterfly over them, its first lane writes.  gat_unroll value rows in flight.
//   lph == 0 (any V; VW = 1): head after head, lanes across the head's V columns, the dot product a butterfly over the wave, lane 0 writes.
// Either order of additions is fixed.
template <class T, int VW>
__device__ __forceinline__ void gat_score_edges(T* __restrict__ dscore, T* __restrict__ aout, const T* __restrict__ dout, const T* __restrict__ out,
                                                const T* __restrict__ score, const T* __restrict__ value, const int64_t* __restrict__ edgeI,
                                                const int64_t* __restrict__ perm, int64_t j, int64_t rb, int64_t re, int64_t b, int64_t e, int64_t H, int V,
                                                int lph, int lane) {
  constexpr int kGatUnroll = sizeof(T) * VW == 16 ? 2 : gat_unroll<T>();     // 16-byte packets: two rows in flight keep the kernel inside 64 VGPRs
  const int64_t C = H * V;
  if (b >= e) return;
  if (lph > 0) {
    for (int t0 = 0; t0 < C; t0 += 64 * VW) {
      const int c0 = t0 + lane * VW;
      const bool active = c0 < C;
      const int h = active ? c0 / V : 0;
      const bool writer = active && (lane & (lph - 1)) == 0;
      const Vec<T, VW> g = active ? load_packet<T, VW>(dout + j * C + c0) : zero_packet<T, VW>();
      const Vec<T, VW> o = active ? load_packet<T, VW>(out + j * C + c0) : zero_packet<T, VW>();
      T delta = T(0);
#pragma unroll
      for (int q = 0; q < VW; q++) delta += g.v[q] * o.v[q];
      for (int off = 1; off < lph; off <<= 1) delta += __shfl_xor(delta, off, 64);
      T mj = T(0), sj = T(1);                                   // of this lane's head, from the heads of this tile
      const int hEnd = (int)((t0 + 64 * VW < C ? t0 + 64 * VW : C) / V);
      for (int ht = t0 / V; ht < hEnd; ht++) {
        T mt, st;
        gat_row_softmax<T>(mt, st, score, perm, rb, re, H, ht, lane);
        if (ht == h) { mj = mt; sj = st; }
      }
      const T* vc = value + c0;
      for (int64_t p = b; p < e; p += 64) {
        const int n = (int)(e - p < 64 ? e - p : 64);
        int64_t ed = 0, sr = 0;
        if (lane < n) { ed = perm[p + lane]; sr = edgeI[ed]; }
        for (int k = 0; k < n; k += kGatUnroll) {
          Vec<T, VW> v[kGatUnroll];
          T x[kGatUnroll];
#pragma unroll
          for (int u = 0; u < kGatUnroll; u++) {
            const int ku = k + u < n ? k + u : n - 1;            // past the end: the last edge again, not written
            const int64_t eu = lane_bcast(ed, ku), su = lane_bcast(sr, ku);
            v[u] = active ? load_packet<T, VW>(vc + su * C) : zero_packet<T, VW>();
            x[u] = writer ? score[eu * H + h] : T(0);
          }
#pragma unroll
          for (int u = 0; u < kGatUnroll; u++) {
            T d = T(0);
#pragma unroll
            for (int q = 0; q < VW; q++) d += g.v[q] * v[u].v[q];
            for (int off = 1; off < lph; off <<= 1) d += __shfl_xor(d, off, 64);
            if (k + u < n) {
              const int64_t eu = lane_bcast(ed, k + u);
              if (writer) {
                const T a = gat_exp(x[u] - mj) / sj;
                aout[eu * H + h] = a;
                dscore[eu * H + h] = a * (d - delta);
              }
            }
          }
        }
      }
    }
  } else {
    for (int h = 0; h < H; h++) {
      const T* gj = dout + j * C + (int64_t)h * V;
      const T* oj = out + j * C + (int64_t)h * V;
      T delta = T(0);
      for (int v = lane; v < V; v += 64) delta += gj[v] * oj[v];
      delta = wave_sum(delta);
      T mj, sj;
      gat_row_softmax<T>(mj, sj, score, perm, rb, re, H, h, lane);
      for (int64_t p = b; p < e; p += 64) {
        const int n = (int)(e - p < 64 ? e - p : 64);
        int64_t ed = 0, sr = 0;
        if (lane < n) { ed = perm[p + lane]; sr = edgeI[ed]; }
        for (int k = 0; k < n; k++) {
          const int64_t eu = lane_bcast(ed, k), su = lane_bcast(sr, k);
          const T* vi = value + su * C + (int64_t)h * V;
          T d = T(0);
          for (int v = lane; v < V; v += 64) d += gj[v] * vi[v];
          d = wave_sum(d);
          if (lane == 0) {
            const T a = gat_exp(score[eu * H + h] - mj) / sj;
            aout[eu * H + h] = a;
            dscore[eu * H + h] = a * (d - delta);
          }
        }
      }
    }
  }
}

// grid: (ceil(N / kWaves), 1, kWaves + 1), block: kWaves * 64.  A wave per destination; the edges of a long row are shared out among the
// workgroup's waves (nothing is summed across edges, so nothing is merged).
template <class T, int VW>
__global__ __launch_bounds__(kWaves * 64) __attribute__((amdgpu_num_sgpr(96))) void gat_backward_score_kernel(
    T* __restrict__ dscore, T* __restrict__ aout, const T* __restrict__ dout, const T* __restrict__ out, const T* __restrict__ score,
    const T* __restrict__ value, const int64_t* __restrict__ edgeI, const int64_t* __restrict__ rowptr, const int64_t* __restrict__ perm, int64_t N,
    int64_t H, int V, int lph) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int k = first_turn(); is_turn(k); k++) {
    const RowTurn t = row_turn(k, N, wave);
    if (t.r < 0) continue;
    const int64_t rb = rowptr[t.r], re = rowptr[t.r + 1];
    if (!t.takes(re - rb)) continue;
    const Share sh = t.share(re - rb, wave);
    gat_score_edges<T, VW>(dscore, aout, dout, out, score, value, edgeI, perm, t.r, rb, re, rb + sh.lo, rb + sh.hi, H, V, lph, lane);
  }
}

// ---- message passing (lamp-core/src/main/scala/lamp/nn/graph/MPNN.scala) ---------------------------------------------------------------------
// The two data movements of an MPNN layer.  The message cat(edgeFeatures, x[edgeI], x[edgeJ]) and MPNN.aggregate's backward are per
// edge: a row has no sum, so these kernels run a thread per packet over a flat index of rows x packets (no idle lane at any width,
// neighbouring lanes on neighbouring packets).  The message's gradient with respect to x and MPNN.aggregate are sums per node over the
// groupings of lamp_graph_edge_csr: mpnn_node_sum_kernel, a row kernel (see the head of the file) whose entry per edge is the edge id
// and the factors of its end points.  No atomics, every element written once, nothing synchronises with the host.

// out[n] = (T) f32(count^p), count = rowptr[n + 1] - rowptr[n]: the reference's pow of a long tensor is an f32 tensor, cast afterwards.
// p = -0.5 (HALF) is 1 / sqrt(count) in two f32 roundings, as ATen's pow computes it; p = -1 is 1 / count.  count = 0 gives +inf.
template <class T, bool HALF>
__global__ __launch_bounds__(256) void mpnn_degree_factor_kernel(T* __restrict__ out, const int64_t* __restrict__ rowptr, int64_t N) {
  const int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float c = (float)(rowptr[n + 1] - rowptr[n]);
  // each f32 operation as an f64 one rounded to f32: the same value (a square root or a quotient of f32 operands rounds to f32 alike from 53
  // bits as from the exact result), whatever the build makes of f32 sqrt and division
  const float s = HALF ? (float)sqrt((double)c) : c;
  out[n] = (T)(float)(1.0 / (double)s);
}

// which row and which packet slot of it a thread of a per-edge kernel holds: a flat index over rows x slots, so no lane idles whatever the
// number of slots, and neighbouring lanes hold neighbouring packets.  The index is 32 bits wide (one unsigned division per thread; the
// host refuses more than 2^31 packets); a thread past the last packet gets a row past the last.
struct MpnnSlot { int64_t row; int slot; };
__device__ __forceinline__ MpnnSlot mpnn_slot(uint32_t slots) {
  const uint32_t idx = blockIdx.x * (uint32_t)kMpnnEdgeBlock + threadIdx.x;
  const uint32_t r = idx / slots;
  return {(int64_t)r, (int)(idx - r * slots)};
}

// msg[e, :] = [ edge[e, 0:Fe] | x[edgeI[e], 0:D] | x[edgeJ[e], 0:D] ]: slot s < se is packet s (VE elements) of the edge segment, then sx
// packets (VX elements) of x[edgeI[e]], then sx of x[edgeJ[e]].  The host chooses VE and VX per segment (mpnn_message_packets).
template <class T, int VE, int VX>
__global__ __launch_bounds__(kMpnnEdgeBlock) void mpnn_message_kernel(T* __restrict__ msg, const T* __restrict__ edge, int64_t lde, const T* __restrict__ x,
                                                                     int64_t ldx, const int64_t* __restrict__ edgeI, const int64_t* __restrict__ edgeJ, int64_t E,
                                                                     int Fe, int D, uint32_t slots) {
  const MpnnSlot t = mpnn_slot(slots);
  const int se = Fe / VE, sx = D / VX;
  if (t.row >= E || t.slot >= se + 2 * sx) return;
  T* o = msg + t.row * ((int64_t)Fe + 2 * (int64_t)D);
  if (t.slot < se) {
    const int c = t.slot * VE;
    *reinterpret_cast<Vec<T, VE>*>(o + c) = load_packet<T, VE>(edge + t.row * lde + c);
  } else {
    const bool second = t.slot - se >= sx;
    const int c = (t.slot - se - (second ? sx : 0)) * VX;
    const int64_t node = second ? edgeJ[t.row] : edgeI[t.row];
    *reinterpret_cast<Vec<T, VX>*>(o + Fe + (second ? D : 0) + c) = load_packet<T, VX>(x + node * ldx + c);
  }
}

// dst[e, 0:C] = src[e, 0:C] of rows with the pitches ldd and lds (dedge = dmsg[:, 0:Fe])
template <class T, int V>
__global__ __launch_bounds__(kMpnnEdgeBlock) void mpnn_columns_kernel(T* __restrict__ dst, int64_t ldd, const T* __restrict__ src, int64_t lds, int64_t E, int C,
                                                                     uint32_t slots) {
  const MpnnSlot t = mpnn_slot(slots);
  const int c = t.slot * V;
  if (t.row >= E || c >= C) return;
  *reinterpret_cast<Vec<T, V>*>(dst + t.row * ldd + c) = load_packet<T, V>(src + t.row * lds + c);
}

// dmsg[e, :] = ((dout[edgeJ[e], :] [+ dout[edgeI[e], :] if aggregateJ]) [* fJ[edgeJ[e]]]) [* fI[edgeI[e]]]; a null factor is absent
template <class T, int V>
__global__ __launch_bounds__(kMpnnEdgeBlock) void mpnn_aggregate_backward_kernel(T* __restrict__ dmsg, const T* __restrict__ dout, const int64_t* __restrict__ edgeI,
                                                                                const int64_t* __restrict__ edgeJ, const T* __restrict__ fI,
                                                                                const T* __restrict__ fJ, int aggregateJ, int64_t E, int M, uint32_t slots) {
  const MpnnSlot t = mpnn_slot(slots);
  const int c = t.slot * V;
  if (t.row >= E || c >= M) return;
  const int64_t i = edgeI[t.row], j = edgeJ[t.row];
  Vec<T, V> g = load_packet<T, V>(dout + j * M + c);
  if (aggregateJ) {
    const Vec<T, V> h = load_packet<T, V>(dout + i * M + c);
#pragma unroll
    for (int q = 0; q < V; q++) g.v[q] += h.v[q];
  }
  if (fJ) {
    const T f = fJ[j];
#pragma unroll
    for (int q = 0; q < V; q++) g.v[q] *= f;
  }
  if (fI) {
    const T f = fI[i];
#pragma unroll
    for (int q = 0; q < V; q++) g.v[q] *= f;
  }
  *reinterpret_cast<Vec<T, V>*>(dmsg + t.row * M + c) = g;
}

// acc += sum over the edges ed = perm[b .. e), in that order, of t(ed) = (row[ed * ld + c0 ..] [* fI[edgeI[ed]]]) [* fJ[edgeJ[ed]]] (rc = row
// + c0).  The products are rounded before they are added (no contraction into an fma): a term has the bits the chain of Mult nodes gives
// it.  Lanes with `active` false hold no column and load no row.
template <class T, int V, bool FI, bool FJ>
__device__ __forceinline__ void mpnn_gather(Vec<T, V>& acc, const T* __restrict__ rc, int64_t ld, const int64_t* __restrict__ perm,
                                            const int64_t* __restrict__ edgeI, const int64_t* __restrict__ edgeJ, const T* __restrict__ fI,
                                            const T* __restrict__ fJ, int64_t b, int64_t e, int lane, bool active) {
  constexpr int NF = (FI ? 1 : 0) + (FJ ? 1 : 0), J = FI ? 1 : 0;      // fI's factor first, then fJ's
  using Entry = EdgeEntry<T, 1, NF>;
  using Item = EdgeItem<T, V, NF>;
  for_each_edge<kMpnnUnroll>(
      b, e, lane,
      [&](int64_t p) {
        Entry en;
        en.i[0] = perm[p];
        if constexpr (FI) en.f[0] = fI[edgeI[en.i[0]]];
        if constexpr (FJ) en.f[J] = fJ[edgeJ[en.i[0]]];
        return en;
      },
      [&](const Entry& en) {
        Item it;
#pragma unroll
        for (int q = 0; q < NF; q++) it.s[q] = en.f[q];
        it.v = active ? load_packet<T, V>(rc + en.i[0] * ld) : zero_packet<T, V>();
        return it;
      },
      [&](const Item& it) {
#pragma clang fp contract(off)
#pragma unroll
        for (int j = 0; j < V; j++) {
          T t = it.v.v[j];
          if constexpr (FI) t = t * it.s[0];
          if constexpr (FJ) t = t * it.s[J];
          acc.v[j] = acc.v[j] + t;
        }
      });
}

// out[r, 0:C] from the rows src[ed, off .. off + C) of the edges of node r: the sum over those of grouping 1 (columns off1) and, where
// rowptr2 is not null, the sum over those of grouping 2 (columns off2), each in its grouping's order, the two added last - as the chains
// add them (MPNN.aggregate: aggregateI + aggregateJ over incoming and outgoing; the message's gradient with respect to x: the two
// gathers' gradients, outgoing at Fe and incoming at Fe + D).  A node whose two groups together hold more than kLongRow edges is
// split: the waves take contiguous shares of the concatenated sequence, and either sum's partial sums are added in wave order.
// grid: (ceil(N / kWaves), ceil(C / (64 * V)), kWaves + 1), block: kWaves * 64.
template <class T, int V, bool FI, bool FJ>
__global__ __launch_bounds__(kWaves * 64) void mpnn_node_sum_kernel(T* __restrict__ out, const T* __restrict__ src, int64_t ld, int64_t off1, int64_t off2,
                                                                        const int64_t* __restrict__ rowptr1, const int64_t* __restrict__ perm1,
                                                                        const int64_t* __restrict__ rowptr2, const int64_t* __restrict__ perm2,
                                                                        const int64_t* __restrict__ edgeI, const int64_t* __restrict__ edgeJ,
                                                                        const T* __restrict__ fI, const T* __restrict__ fJ, int64_t N, int64_t C) {
  __shared__ Vec<T, V> part[2][kWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t c0 = ((int64_t)blockIdx.y * 64 + lane) * V;
  const bool active = c0 < C;

  for (int k = first_turn(); is_turn(k); k++) {
    const RowTurn t = row_turn(k, N, wave);
    int64_t b1 = 0, n1 = 0, b2 = 0, n2 = 0;
    if (t.r >= 0) {
      b1 = rowptr1[t.r]; n1 = rowptr1[t.r + 1] - b1;
      if (rowptr2) { b2 = rowptr2[t.r]; n2 = rowptr2[t.r + 1] - b2; }
    }
    if (!t.takes(n1 + n2)) continue;
    const Share sh = t.share(n1 + n2, wave);       // of the n1 + n2 edges
    Vec<T, V> acc[2] = {zero_packet<T, V>(), zero_packet<T, V>()};
    if (sh.lo < n1) mpnn_gather<T, V, FI, FJ>(acc[0], src + off1 + c0, ld, perm1, edgeI, edgeJ, fI, fJ, b1 + sh.lo, b1 + (sh.hi < n1 ? sh.hi : n1), lane, active);
    if (sh.hi > n1) mpnn_gather<T, V, FI, FJ>(acc[1], src + off2 + c0, ld, perm2, edgeI, edgeJ, fI, fJ, b2 + (sh.lo > n1 ? sh.lo - n1 : 0), b2 + sh.hi - n1, lane, active);
    if (!t.own) merge_shares(acc, part, wave, lane, active);
    if (active && t.r >= 0 && (t.own || wave == 0)) {
      if (rowptr2) {
#pragma unroll
        for (int j = 0; j < V; j++) acc[0].v[j] += acc[1].v[j];
      }
      *reinterpret_cast<Vec<T, V>*>(out + t.r * C + c0) = acc[0];
    }
  }
}

// the widest packet (in elements, at most 16 bytes) that divides every length (widths, column offsets, row pitches) and at which every
// address is aligned
template <class T> int packet_width(std::initializer_list<int64_t> lengths, std::initializer_list<const Tensor*> ts) {
  for (int v = 16 / (int)sizeof(T); v > 1; v >>= 1) {
    bool ok = true;
    for (int64_t l : lengths) ok = ok && l % v == 0;
    for (const Tensor* t : ts) ok = ok && ((uintptr_t)t->raw() % (v * sizeof(T))) == 0;
    if (ok) return v;
  }
  return 1;
}
// f(std::integral_constant<int, v>()) for a packet width of T: four (four-byte types only), two or one
template <class T, class F> void with_packet(int v, F f) {
  if constexpr (sizeof(T) == 4) {
    if (v == 4) { f(std::integral_constant<int, 4>()); return; }
  }
  if (v == 2) f(std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 1>());
}
// f(T()) for the floating type T of dtype, which is kF32 or kF64
template <class F> void with_float(int dtype, F f) {
  if (dtype == kF32) f(float());
  else f(double());
}
// the grid of a row kernel: a workgroup per kWaves rows, the C columns in packets of v tiled in y (C = v = 1: a kernel that does not
// tile its columns), `slices` in z
dim3 row_grid(int64_t N, int64_t C, int v, int slices) {
  const int64_t tiles = (C + 64 * v - 1) / (64 * v), groups = (N + kWaves - 1) / kWaves;
  LAMP_CHECK(tiles <= 65535 && groups <= INT32_MAX, "a graph of " << N << " nodes in " << tiles << " column tiles is too large");
  return dim3((unsigned)groups, (unsigned)tiles, (unsigned)slices);
}

void check_i64_vector(const Tensor* t, const Tensor* first, const char* what) {
  check_device_tensor(t, what);
  check_same_device(t, first);
  LAMP_CHECK(t->dtype == kI64 && t->ndim == 1, what << " must be an int64 vector, got " << t->describe());
}

// every entry of a (and of b, where given; both int64 [n], contiguous, n > 0) lies in [0, N), or an error: one reduction kernel and one host
// read, before anything uses an entry as an index
void check_index_range(const char* tag, const Tensor* a, const Tensor* b, int64_t N, hipStream_t st) {
  const int64_t n = a->numel();
  const int nb = grid_for(n, 256, 2);
  int64_t ms[1] = {2 * (int64_t)nb};
  Hold mm(new_tensor(ms, 1, kI64, a->device()));
  {
    KernelTimer kt(tag, 0, (double)n * (b ? 16 : 8), st);
    hipLaunchKernelGGL(gcn_index_range_kernel, dim3(nb), dim3(256), 0, st, a->ptr<int64_t>(), b ? b->ptr<int64_t>() : nullptr, n, mm->ptr<int64_t>());
    LAMP_LAUNCH_CHECK();
  }
  std::vector<int64_t> h(2 * (size_t)nb);
  HIP_CHECK(hipMemcpyAsync(h.data(), mm->ptr<int64_t>(), h.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (int i = 0; i < nb; i++) { mn = std::min(mn, h[2 * i]); mx = std::max(mx, h[2 * i + 1]); }
  LAMP_CHECK(mn >= 0 && mx < N, "edge endpoints must lie in [0, " << N << "), got " << mn << " .. " << mx);
}

// the packet width of gat_forward_kernel / gat_backward_value_kernel: the widest that C and the addresses allow, but four only where it
// stays inside a head (a softmax state per element costs an exp each)
template <class T> int gat_gather_packet(int64_t C, int V, std::initializer_list<const Tensor*> ts) {
  int vw = packet_width<T>({C}, ts);
  while (vw > 2 && V % vw) vw >>= 1;
  return vw;
}
// f(width, ONE) for those two kernels: ONE where no packet straddles a head boundary
template <class T, class F> void gat_with_packet(int vw, int V, F f) {
  with_packet<T>(vw, [&](auto W) {
    if constexpr (decltype(W)::value == 2) {
      if (V % 2) { f(W, std::false_type()); return; }
    }
    f(W, std::true_type());
  });
}
// the packet form of gat_backward_score_kernel: V = lph * vw with lph a power of two up to 64; 0 where V has no such split
int gat_lanes_per_head(int V, int vw) {
  if (V % vw) return 0;
  const int lph = V / vw;
  return lph <= 64 && (lph & (lph - 1)) == 0 ? lph : 0;
}

// every tensor of vs is an int64 vector of n entries on first's device, or the error "<its name> <the tensor> <why>"
using NamedTensors = std::initializer_list<std::pair<const Tensor*, const char*>>;
void check_i64_vectors(NamedTensors vs, const Tensor* first, int64_t n, const std::string& why) {
  for (auto& v : vs) {
    check_i64_vector(v.first, first, v.second);
    LAMP_CHECK(v.first->numel() == n, v.second << " " << v.first->describe() << " " << why);
  }
}
void check_rowptrs(NamedTensors vs, const Tensor* first, int64_t N) {
  check_i64_vectors(vs, first, N + 1, "does not belong to a graph of " + std::to_string(N) + " nodes");
}

// score [E, H], value [N, H, V] of one floating type, the index vectors int64 [E], the grouping's rowptr [N + 1]
struct GatShape { int64_t E, H, N, V; };
GatShape gat_check(const Tensor* score, const Tensor* value, NamedTensors edgeVectors, NamedTensors rowptrs) {
  check_device_tensor(score, "score");
  check_device_tensor(value, "value");
  check_same_device(value, score);
  LAMP_CHECK(score->dtype == kF32 || score->dtype == kF64, "f32 and f64 only, got " << score->describe());
  LAMP_CHECK(value->dtype == score->dtype, "value " << value->describe() << " is not of score's type " << score->describe());
  LAMP_CHECK(score->ndim == 2, "score " << score->describe() << " must be [E, H]");
  LAMP_CHECK(value->ndim == 3 && value->sizes[1] == score->sizes[1],
             "value " << value->describe() << " must be [N, H, V] with the H = " << score->sizes[1] << " heads of score " << score->describe());
  const GatShape g{score->sizes[0], score->sizes[1], value->sizes[0], value->sizes[2]};
  LAMP_CHECK(g.H * g.V <= INT32_MAX / 2, "value " << value->describe() << " has too many columns");
  check_i64_vectors(edgeVectors, score, g.E, "does not have score's " + std::to_string(g.E) + " edges: edgeI and edgeJ differ in length?");
  check_rowptrs(rowptrs, score, g.N);
  return g;
}

// the grid of a per-edge kernel: rows of `slots` packets (slots >= 1), a thread per packet; see mpnn_slot
struct MpnnEdgeGrid { dim3 grid; uint32_t slots; };
MpnnEdgeGrid mpnn_edge_grid(int64_t rows, int64_t slots) {
  LAMP_CHECK(slots >= 1 && rows * slots <= ((int64_t)1 << 31), rows << " rows of " << slots << " packets are too many");
  return {dim3((unsigned)((rows * slots + kMpnnEdgeBlock - 1) / kMpnnEdgeBlock)), (uint32_t)slots};
}
// a [rows, cols] tensor whose rows are read in place (unit column stride and rows that do not overlap, whatever the row pitch) or a
// dense copy (of a broadcast gradient, say); -> its row pitch
Tensor* rows_in_place(const Tensor* t, int64_t* ld) {
  const int64_t rows = t->sizes[0], cols = t->sizes[1];
  const bool in_place = (cols == 1 || t->strides[1] == 1) && (rows == 1 || t->strides[0] >= cols);
  Tensor* r = in_place ? retain(t) : contiguous(t);
  *ld = rows == 1 ? cols : r->strides[0];
  return r;
}
// The groups 0 .. N - 1 of keys (int64 [n], contiguous, every entry in [0, N): check_index_range comes first).  -> rowptr [N + 1];
// *perm = the stable permutation that sorts the keys ([n]); dinv, where given ([N], f32 or f64) = (group size + 1)^-1/2.
Tensor* group_keys(const Tensor* keys, int64_t N, Hold* perm, Tensor* dinv, const char* tag, hipStream_t st) {
  const int dev = keys->device();
  const int64_t n = keys->numel();
  int64_t n1[1] = {N + 1}, ns[1] = {n};
  Hold rp(new_tensor(n1, 1, kI64, dev)), counts;
  if (n) {
    lamp_tensor* t = nullptr;
    LAMP_CHECK(lamp_argsort(&t, keys, 1, 0, 0) == 0, lamp_last_error());
    *perm = Hold(t);
    LAMP_CHECK(lamp_bincount(&t, keys, nullptr, N) == 0, lamp_last_error());
    counts = Hold(t);
    LAMP_CHECK(counts->numel() == N && (*perm)->numel() == n && (*perm)->dtype == kI64, "internal: counts " << counts->describe() << ", perm " << (*perm)->describe());
  } else {
    *perm = Hold(new_tensor(ns, 1, kI64, dev));
  }
  KernelTimer kt(tag, 0, (double)N * (16 + (dinv ? dtype_size(dinv->dtype) : 0)), st);
  with_float(dinv ? dinv->dtype : kF32, [&](auto z) {
    using T = decltype(z);
    hipLaunchKernelGGL((gcn_rowptr_dinv_kernel<T>), dim3(1), dim3(1024), 0, st, counts.get() ? counts->ptr<int64_t>() : nullptr, rp->ptr<int64_t>(),
                       dinv ? dinv->ptr<T>() : nullptr, N);
  });
  LAMP_LAUNCH_CHECK();
  return rp.take();
}
void mpnn_check_float(const Tensor* t, const char* what, const Tensor* first) {
  check_device_tensor(t, what);
  check_same_device(t, first);
  LAMP_CHECK(first->dtype == kF32 || first->dtype == kF64, "f32 and f64 only, got " << first->describe());
  LAMP_CHECK(t->dtype == first->dtype, what << " " << t->describe() << " is not of the type of " << first->describe());
}
// a factor vector: null, or [N] of message's type
void mpnn_check_factor(const Tensor* f, const char* what, const Tensor* first, int64_t N) {
  if (!f) return;
  mpnn_check_float(f, what, first);
  LAMP_CHECK(f->ndim == 1 && f->numel() == N, what << " " << f->describe() << " must be [" << N << "]");
}

struct MpnnSum {
  Tensor* out; const Tensor* src; int64_t ld, off1, off2;
  const Tensor *rowptr1, *perm1, *rowptr2, *perm2, *edgeI, *edgeJ, *fI, *fJ;
  int64_t N, C;
};
// v: the packet width, as packet_width gives it for the widths, offsets and tensors of a
template <class T, bool FI, bool FJ> void mpnn_sum_launch(int v, const MpnnSum& a, hipStream_t st) {
  auto ip = [](const Tensor* t) { return t ? t->ptr<int64_t>() : nullptr; };
  with_packet<T>(v, [&](auto W) {
    constexpr int V = decltype(W)::value;
    hipLaunchKernelGGL((mpnn_node_sum_kernel<T, V, FI, FJ>), row_grid(a.N, a.C, V, kWaves + 1), dim3(kWaves * 64), 0, st, a.out->ptr<T>(), a.src->ptr<T>(), a.ld,
                       a.off1, a.off2, ip(a.rowptr1), ip(a.perm1), ip(a.rowptr2), ip(a.perm2), ip(a.edgeI), ip(a.edgeJ), a.fI ? a.fI->ptr<T>() : nullptr,
                       a.fJ ? a.fJ->ptr<T>() : nullptr, a.N, a.C);
  });
}
// MPNN.aggregate: a factor that is null is a kernel without that multiplication
template <class T> void mpnn_aggregate_launch(int v, const MpnnSum& a, hipStream_t st) {
  if (a.fI && a.fJ) mpnn_sum_launch<T, true, true>(v, a, st);
  else if (a.fI) mpnn_sum_launch<T, true, false>(v, a, st);
  else if (a.fJ) mpnn_sum_launch<T, false, true>(v, a, st);
  else mpnn_sum_launch<T, false, false>(v, a, st);
}

// ---- graph minibatches (lamp-data/src/main/scala/lamp/data/GraphBatchStream.scala) ---------------------------------------------------------
// A batch of whole graphs is block-diagonal: its node and edge rows are ragged copies out of the packed data set, and its groupings are
// the data set's own with two offsets added, because graph g's entries sit at [edgePtr[g], edgePtr[g + 1]) of inPerm / outPerm, at twice
// that of the adjacency's col, and its rows at [nodePtr[g], nodePtr[g + 1]) of every rowptr and of dinv, each in the order a grouping of
// the batch alone would have (the sorts are stable).  So nothing is sorted, counted or scanned per batch, nothing is read back, and the
// kernels are copies: a thread per output element (or packet), which finds its graph by a binary search of the batch's slice of the
// epoch's plan - rows of (srcNodeBase, dstNodeBase, srcEdgeBase, dstEdgeBase) - and writes every element once.
// VertexPooling over such a batch sums consecutive rows: segment_pool_kernel, a row kernel (see the head of the file) without an index.
constexpr int kPlanCols = 4;      // columns of a plan row: source and destination base of the nodes, then of the edges
constexpr int kPoolUnroll = 8;    // node rows in flight per wave of segment_pool_kernel

// the graph b in [0, B) of a batch whose rows of column `c` of the plan are the bases of an output: base[b] <= k < base[b + 1], with
// base[B] = total > k.  Graphs without a row (equal bases) are passed over.
__device__ __forceinline__ int plan_find(const int64_t* __restrict__ plan, int c, int B, int64_t k) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (plan[(int64_t)mid * kPlanCols + c] <= k) lo = mid; else hi = mid;
  }
  return lo;
}

// out[dstBase[b] + k, 0:slots) = src[srcBase[b] + k, 0:slots) in packets P, (srcBase, dstBase) = the plan's columns (c, c + 1); rows of
// `slots` packets, dense
template <class P>
__global__ __launch_bounds__(kMpnnEdgeBlock) void graph_batch_rows_kernel(P* __restrict__ out, const P* __restrict__ src, const int64_t* __restrict__ plan, int c,
                                                                         int B, int64_t rows, uint32_t slots) {
  const MpnnSlot t = mpnn_slot(slots);
  if (t.row >= rows) return;
  const int64_t* pb = plan + (int64_t)plan_find(plan, c + 1, B, t.row) * kPlanCols;
  out[t.row * slots + t.slot] = src[(pb[c] + t.row - pb[c + 1]) * slots + t.slot];
}

struct BatchNodes {
  int64_t *pool, *graphPtr, *adjRowptr, *inRowptr, *outRowptr;
  const int64_t *setAdjRowptr, *setInRowptr, *setOutRowptr;
};
// thread n of [0, N]: node n's entries of the node-sized arrays (a null output is absent), thread N the totals; threads [0, B] graphPtr
template <class T>
__global__ __launch_bounds__(256) void graph_batch_nodes_kernel(BatchNodes a, T* __restrict__ dinv, const T* __restrict__ setDinv, const int64_t* __restrict__ plan,
                                                                int B, int64_t N, int64_t E) {
  const int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (n > N) return;
  if (n <= B) a.graphPtr[n] = n < B ? plan[n * kPlanCols + 1] : N;
  if (n == N) {
    if (a.adjRowptr) a.adjRowptr[N] = 2 * E;
    if (a.inRowptr) a.inRowptr[N] = E;
    if (a.outRowptr) a.outRowptr[N] = E;
    return;
  }
  const int b = plan_find(plan, 1, B, n);
  const int64_t* pb = plan + (int64_t)b * kPlanCols;
  const int64_t s = pb[0] + n - pb[1], shift = pb[3] - pb[2];
  a.pool[n] = b;
  if (a.adjRowptr) a.adjRowptr[n] = a.setAdjRowptr[s] + 2 * shift;
  if (a.inRowptr) a.inRowptr[n] = a.setInRowptr[s] + shift;
  if (a.outRowptr) a.outRowptr[n] = a.setOutRowptr[s] + shift;
  if (dinv) dinv[n] = setDinv[s];
}

struct BatchEdges {
  int64_t *edgeI, *edgeJ, *col, *inPerm, *outPerm;
  const int64_t *setEdgeI, *setEdgeJ, *setCol, *setInPerm, *setOutPerm;
};
// thread k of [0, E): edge k's endpoints and its entries of the two permutations, and the two entries of col at the same place in either
// half of its graph's 2 * Eg entries (so both halves are read and written coalesced)
__global__ __launch_bounds__(256) void graph_batch_edges_kernel(BatchEdges a, const int64_t* __restrict__ plan, int B, int64_t E) {
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= E) return;
  const int b = plan_find(plan, 3, B, k);
  const int64_t* pb = plan + (int64_t)b * kPlanCols;
  const int64_t j = k - pb[3], s = pb[2] + j, nodeShift = pb[1] - pb[0], edgeShift = pb[3] - pb[2];
  a.edgeI[k] = a.setEdgeI[s] + nodeShift;
  a.edgeJ[k] = a.setEdgeJ[s] + nodeShift;
  if (a.inPerm) a.inPerm[k] = a.setInPerm[s] + edgeShift;
  if (a.outPerm) a.outPerm[k] = a.setOutPerm[s] + edgeShift;
  if (a.col) {
    const int64_t eg = (b + 1 < B ? pb[kPlanCols + 3] : E) - pb[3];
    a.col[2 * pb[3] + j] = a.setCol[2 * pb[2] + j] + nodeShift;
    a.col[2 * pb[3] + eg + j] = a.setCol[2 * pb[2] + eg + j] + nodeShift;
  }
}

// *bad (zero before the launch) = 1 where an edge e of [0, E) has an endpoint outside the rows [nodePtr[g], nodePtr[g + 1]) of its own
// graph g, the one with edgePtr[g] <= e < edgePtr[g + 1]; every thread that finds one stores the same word
__global__ __launch_bounds__(256) void graph_set_check_kernel(int64_t* __restrict__ bad, const int64_t* __restrict__ edgeI, const int64_t* __restrict__ edgeJ,
                                                              const int64_t* __restrict__ nodePtr, const int64_t* __restrict__ edgePtr, int64_t G, int64_t E) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= E) return;
  int64_t lo = 0, hi = G;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (edgePtr[mid] <= e) lo = mid; else hi = mid;
  }
  const int64_t b = nodePtr[lo], t = nodePtr[lo + 1], i = edgeI[e], j = edgeJ[e];
  if (i < b || i >= t || j < b || j >= t) *bad = 1;
}

// acc += x[b, c0 ..] + x[b + 1, c0 ..] + ... + x[e - 1, c0 ..], in that order (xc = x + c0), kPoolUnroll rows in flight
template <class T, int V>
__device__ __forceinline__ void pool_rows(Vec<T, V>& acc, const T* __restrict__ xc, int64_t ldx, int64_t b, int64_t e) {
  int64_t r = b;
  for (; r + kPoolUnroll <= e; r += kPoolUnroll) {
    Vec<T, V> row[kPoolUnroll];
#pragma unroll
    for (int u = 0; u < kPoolUnroll; u++) row[u] = load_packet<T, V>(xc + (r + u) * ldx);
#pragma unroll
    for (int u = 0; u < kPoolUnroll; u++) {
#pragma unroll
      for (int j = 0; j < V; j++) acc.v[j] += row[u].v[j];
    }
  }
  for (; r < e; r++) {
    const Vec<T, V> row = load_packet<T, V>(xc + r * ldx);
#pragma unroll
    for (int j = 0; j < V; j++) acc.v[j] += row.v[j];
  }
}

// out[g, :] = sum of the rows x[graphPtr[g] .. graphPtr[g + 1]) (entries clamped to [0, N]) in row order, over their number if `mean`.
// D % V == 0.  grid: (ceil(B / kWaves), ceil(D / (64 * V)), kWaves + 1), block: kWaves * 64.
template <class T, int V>
__global__ __launch_bounds__(kWaves * 64) void segment_pool_kernel(T* __restrict__ out, const T* __restrict__ x, int64_t ldx, const int64_t* __restrict__ graphPtr,
                                                                       int64_t B, int64_t N, int64_t D, int mean) {
  __shared__ Vec<T, V> part[1][kWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t c0 = ((int64_t)blockIdx.y * 64 + lane) * V;
  const bool active = c0 < D;

  for (int k = first_turn(); is_turn(k); k++) {
    const RowTurn t = row_turn(k, B, wave);
    int64_t b = 0, n = 0;
    if (t.r >= 0) {
      const int64_t lo = graphPtr[t.r], hi = graphPtr[t.r + 1];
      b = lo < 0 ? 0 : (lo > N ? N : lo);
      n = (hi < b ? b : (hi > N ? N : hi)) - b;
    }
    if (!t.takes(n)) continue;
    const Share sh = t.share(n, wave);
    Vec<T, V> acc[1] = {zero_packet<T, V>()};
    if (active) pool_rows<T, V>(acc[0], x + c0, ldx, b + sh.lo, b + sh.hi);
    if (!t.own) merge_shares(acc, part, wave, lane, active);
    if (active && t.r >= 0 && (t.own || wave == 0)) {
      if (mean) {
        const T cnt = (T)n;
#pragma unroll
        for (int j = 0; j < V; j++) acc[0].v[j] /= cnt;
      }
      *reinterpret_cast<Vec<T, V>*>(out + t.r * D + c0) = acc[0];
    }
  }
}

// dx[n, :] = dout[pool[n], :] (pool[n] clamped to [0, B)), over the node count of that graph if `mean`.  A thread per packet.
template <class T, int V>
__global__ __launch_bounds__(kMpnnEdgeBlock) void segment_pool_backward_kernel(T* __restrict__ dx, const T* __restrict__ dout, const int64_t* __restrict__ graphPtr,
                                                                              const int64_t* __restrict__ pool, int64_t N, int64_t B, int D, int mean,
                                                                              uint32_t slots) {
  const MpnnSlot t = mpnn_slot(slots);
  const int c = t.slot * V;
  if (t.row >= N || c >= D) return;
  int64_t g = pool[t.row];
  g = g < 0 ? 0 : (g >= B ? B - 1 : g);
  Vec<T, V> v = load_packet<T, V>(dout + g * D + c);
  if (mean) {
    const T cnt = (T)(graphPtr[g + 1] - graphPtr[g]);
#pragma unroll
    for (int q = 0; q < V; q++) v.v[q] /= cnt;
  }
  *reinterpret_cast<Vec<T, V>*>(dx + t.row * D + c) = v;
}

// a batch's slice [off, off + B) of the plan (int64 [G, 4], contiguous on the device) -> its first row
const int64_t* plan_slice(const Tensor* plan, int64_t off, int64_t B) {
  check_device_tensor(plan, "plan");
  LAMP_CHECK(plan->dtype == kI64 && plan->ndim == 2 && plan->sizes[1] == kPlanCols && plan->is_contiguous(),
             "plan " << plan->describe() << " must be a contiguous int64 [G, " << kPlanCols << "]");
  LAMP_CHECK(B >= 1 && B <= INT32_MAX / 2 && off >= 0 && off + B <= plan->sizes[0], "the batch's graphs [" << off << ", " << off + B << ") do not lie in plan " << plan->describe());
  return plan->ptr<int64_t>() + off * kPlanCols;
}
// a set-wide array given beside a batch: null, or an int64 vector on the plan's device of at least `least` entries (a batch may repeat a
// graph, so its totals say nothing about the set's)
void check_set_vector(const Tensor* t, const char* what, const Tensor* plan, int64_t least) {
  if (!t) return;
  check_i64_vector(t, plan, what);
  LAMP_CHECK(t->is_contiguous() && t->numel() >= least, what << " " << t->describe() << " must be contiguous and hold at least " << least << " entries");
}
// the copy unit of lamp_graph_batch_rows: the widest of 16, 8, 4, 2, 1 bytes that divides a row of `bytes` bytes and at which both
// addresses are aligned
int copy_unit(int64_t bytes, const void* a, const void* b) {
  for (int u = 16; u > 1; u >>= 1)
    if (bytes % u == 0 && (uintptr_t)a % u == 0 && (uintptr_t)b % u == 0) return u;
  return 1;
}

}  // namespace
}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_gcn_long_row(int64_t* out) {
  LAMP_API_BEGIN
  *out = kLongRow;
  LAMP_API_END
}

int lamp_gcn_adjacency(lamp_tensor** rowptr, lamp_tensor** col, lamp_tensor** dinv, const lamp_tensor* edgeI, const lamp_tensor* edgeJ, int64_t numNodes,
                       int dtype) {
  LAMP_API_BEGIN
  check_device_tensor(edgeI, "edgeI");
  check_i64_vector(edgeI, edgeI, "edgeI");
  check_i64_vector(edgeJ, edgeI, "edgeJ");
  LAMP_CHECK(edgeI->numel() == edgeJ->numel(), "edgeI " << edgeI->describe() << " and edgeJ " << edgeJ->describe() << " differ in length");
  LAMP_CHECK(dtype == kF32 || dtype == kF64, "f32 and f64 only, got " << dtype_name(dtype));
  LAMP_CHECK(numNodes >= 0, "numNodes = " << numNodes);
  const int dev = edgeI->device();
  const int64_t N = numNodes, E = edgeI->numel();
  LAMP_CHECK(2 * E < ((int64_t)1 << 31), "too many edges: " << E);
  hipStream_t st = current_stream(dev);
  Hold ei(contiguous(edgeI)), ej(contiguous(edgeJ));
  int64_t ns[1] = {N};
  Hold dv(new_tensor(ns, 1, dtype, dev)), keys(retain(ei.get())), vals, cl;
  if (E) {
    // the range of both index vectors, before anything uses one of them as an index
    check_index_range("gcn_index_range", ei.get(), ej.get(), N, st);
    // the 2E directed entries (row, col) = (i, j) then (j, i), to be stably sorted by row
    lamp_tensor *ks[2] = {ei.get(), ej.get()}, *vs[2] = {ej.get(), ei.get()}, *t = nullptr;
    LAMP_CHECK(lamp_cat(&t, ks, 2, 0) == 0, lamp_last_error());
    keys = Hold(t);
    LAMP_CHECK(lamp_cat(&t, vs, 2, 0) == 0, lamp_last_error());
    vals = Hold(t);
  }
  Hold rp(group_keys(keys.get(), N, &cl, dv.get(), "gcn_rowptr_dinv", st));
  if (E) {
    lamp_tensor* t = nullptr;
    LAMP_CHECK(lamp_index_select(&t, vals.get(), 0, cl.get()) == 0, lamp_last_error());
    cl = Hold(t);
    LAMP_CHECK(cl->numel() == 2 * E, "internal: col " << cl->describe());
  }
  *rowptr = rp.take(); *col = cl.take(); *dinv = dv.take();
  LAMP_API_END
}

int lamp_gcn_aggregate(lamp_tensor** out, const lamp_tensor* x, const lamp_tensor* rowptr, const lamp_tensor* col, const lamp_tensor* dinv) {
  LAMP_API_BEGIN
  check_device_tensor(x, "x");
  LAMP_CHECK(x->dtype == kF32 || x->dtype == kF64, "f32 and f64 only, got " << x->describe());
  LAMP_CHECK(x->ndim == 2, "x " << x->describe() << " must be [N, D]");
  const int64_t N = x->sizes[0], D = x->sizes[1];
  check_rowptrs({{rowptr, "rowptr"}}, x, N);
  check_i64_vector(col, x, "col");
  check_device_tensor(dinv, "dinv");
  check_same_device(dinv, x);
  LAMP_CHECK(dinv->ndim == 1 && dinv->numel() == N && dinv->dtype == x->dtype, "dinv " << dinv->describe() << " must be [" << N << "] of x's type " << x->describe());
  int64_t ldx = 0;
  Hold xc(rows_in_place(x, &ldx)), rc(contiguous(rowptr)), cc(contiguous(col)), dc(contiguous(dinv));
  int64_t os[2] = {N, D};
  Hold o(new_tensor(os, 2, x->dtype, x->device()));
  if (N * D) {
    hipStream_t st = current_stream(x->device());
    const double nnz = (double)cc->numel();
    KernelTimer kt("gcn_aggregate", 2.0 * (nnz + 2.0 * N) * D, ((nnz + N) * D + (double)N * D) * dtype_size(x->dtype) + nnz * (8 + dtype_size(x->dtype)) + N * 8.0, st);
    with_float(x->dtype, [&](auto z) {
      using T = decltype(z);
      with_packet<T>(packet_width<T>({D, ldx}, {o.get(), xc.get()}), [&](auto W) {
        constexpr int V = decltype(W)::value;
        hipLaunchKernelGGL((gcn_aggregate_kernel<T, V>), row_grid(N, D, V, 1), dim3(kWaves * 64), 0, st, o->ptr<T>(), D, xc->ptr<T>(), ldx, rc->ptr<int64_t>(),
                           cc->ptr<int64_t>(), dc->ptr<T>(), N, D);
      });
    });
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take();
  LAMP_API_END
}

int lamp_gat_long_row(int64_t* out) {
  LAMP_API_BEGIN
  *out = kLongRow;
  LAMP_API_END
}

int lamp_graph_edge_csr(lamp_tensor** rowptr, lamp_tensor** perm, const lamp_tensor* index, int64_t numNodes) {
  LAMP_API_BEGIN
  check_device_tensor(index, "index");
  check_i64_vector(index, index, "index");
  LAMP_CHECK(numNodes >= 0, "numNodes = " << numNodes);
  const int64_t N = numNodes, E = index->numel();
  LAMP_CHECK(E < ((int64_t)1 << 31), "too many edges: " << E);
  hipStream_t st = current_stream(index->device());
  Hold ix(contiguous(index)), pm;
  if (E) check_index_range("graph_index_range", ix.get(), nullptr, N, st);
  Hold rp(group_keys(ix.get(), N, &pm, nullptr, "graph_edge_rowptr", st));
  *rowptr = rp.take(); *perm = pm.take();
  LAMP_API_END
}

int lamp_gat_forward(lamp_tensor** out, lamp_tensor** lse, const lamp_tensor* score, const lamp_tensor* value, const lamp_tensor* edgeI,
                     const lamp_tensor* inRowptr, const lamp_tensor* inPerm) {
  LAMP_API_BEGIN
  const GatShape g = gat_check(score, value, {{edgeI, "edgeI"}, {inPerm, "inPerm"}}, {{inRowptr, "inRowptr"}});
  const int64_t C = g.H * g.V;
  Hold sc(contiguous(score)), vc(contiguous(value)), ei(contiguous(edgeI)), rp(contiguous(inRowptr)), pm(contiguous(inPerm));
  int64_t os[2] = {g.N, C}, ls[2] = {g.N, g.H};
  Hold o(new_tensor(os, 2, score->dtype, score->device())), l(new_tensor(ls, 2, score->dtype, score->device()));
  if (g.N * g.H) {
    LAMP_CHECK(g.V > 0, "value " << value->describe() << " has no columns");
    hipStream_t st = current_stream(score->device());
    const double sz = (double)dtype_size(score->dtype), E = (double)g.E, N = (double)g.N;
    const int V = (int)g.V;
    KernelTimer kt("gat_forward", 2.0 * E * C + 4.0 * E * g.H + N * C, (E * C + N * C + E * g.H + N * g.H) * sz + E * 16 + N * 8, st);
    with_float(score->dtype, [&](auto z) {
      using T = decltype(z);
      gat_with_packet<T>(gat_gather_packet<T>(C, V, {o.get(), vc.get()}), V, [&](auto W, auto one) {
        constexpr int VW = decltype(W)::value;
        hipLaunchKernelGGL((gat_forward_kernel<T, VW, decltype(one)::value>), row_grid(g.N, C, VW, kWaves + 1), dim3(kWaves * 64), 0, st, o->ptr<T>(), l->ptr<T>(),
                           sc->ptr<T>(), vc->ptr<T>(), ei->ptr<int64_t>(), rp->ptr<int64_t>(), pm->ptr<int64_t>(), g.N, g.H, V);
      });
    });
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take(); *lse = l.take();
  LAMP_API_END
}

int lamp_gat_backward(lamp_tensor** dscore, lamp_tensor** dvalue, const lamp_tensor* dout, const lamp_tensor* out, const lamp_tensor* lse,
                      const lamp_tensor* score, const lamp_tensor* value, const lamp_tensor* edgeI, const lamp_tensor* edgeJ, const lamp_tensor* inRowptr,
                      const lamp_tensor* inPerm, const lamp_tensor* outRowptr, const lamp_tensor* outPerm) {
  LAMP_API_BEGIN
  const GatShape g = gat_check(score, value, {{edgeI, "edgeI"}, {edgeJ, "edgeJ"}, {inPerm, "inPerm"}, {outPerm, "outPerm"}},
                               {{inRowptr, "inRowptr"}, {outRowptr, "outRowptr"}});
  const int64_t C = g.H * g.V;
  for (auto& t : {std::make_pair(dout, "dout"), std::make_pair(out, "out"), std::make_pair(lse, "lse")}) {
    check_device_tensor(t.first, t.second);
    check_same_device(t.first, score);
    const int64_t cols = t.first == lse ? g.H : C;
    LAMP_CHECK(t.first->dtype == score->dtype && t.first->ndim == 2 && t.first->sizes[0] == g.N && t.first->sizes[1] == cols,
               t.second << " " << t.first->describe() << " must be [" << g.N << ", " << cols << "] of score's type " << score->describe());
  }
  Hold go(contiguous(dout)), oc(contiguous(out)), sc(contiguous(score)), vc(contiguous(value)), ei(contiguous(edgeI)),
      ej(contiguous(edgeJ)), irp(contiguous(inRowptr)), ipm(contiguous(inPerm)), orp(contiguous(outRowptr)), opm(contiguous(outPerm));
  int64_t ss[2] = {g.E, g.H}, vs[3] = {g.N, g.H, g.V};
  const int dt = score->dtype, dev = score->device();
  Hold ds(new_tensor(ss, 2, dt, dev)), a(new_tensor(ss, 2, dt, dev)), dv(new_tensor(vs, 3, dt, dev));
  if (g.N * g.H) {
    LAMP_CHECK(g.V > 0, "value " << value->describe() << " has no columns");
    hipStream_t st = current_stream(dev);
    const double sz = (double)dtype_size(dt), E = (double)g.E, N = (double)g.N;
    const int V = (int)g.V;
    if (g.E) {
      KernelTimer kt("gat_backward_score", 2.0 * E * C + 2.0 * N * C + 4.0 * E * g.H, (E * C + 2.0 * N * C + 3.0 * E * g.H + N * g.H) * sz + E * 16 + N * 8, st);
      with_float(dt, [&](auto z) {
        using T = decltype(z);
        // the packet form at the widest packet that has one (vw > 1 leaves the loop only with lph > 0); at vw = 1, lph = 0 where V is no
        // power of two up to 64: the form with lanes across a head
        int vw = packet_width<T>({C}, {go.get(), oc.get(), vc.get()});
        while (vw > 1 && !gat_lanes_per_head(V, vw)) vw >>= 1;
        const int lph = gat_lanes_per_head(V, vw);
        with_packet<T>(vw, [&](auto W) {
          hipLaunchKernelGGL((gat_backward_score_kernel<T, decltype(W)::value>), row_grid(g.N, 1, 1, kWaves + 1), dim3(kWaves * 64), 0, st, ds->ptr<T>(), a->ptr<T>(),
                             go->ptr<T>(), oc->ptr<T>(), sc->ptr<T>(), vc->ptr<T>(), ei->ptr<int64_t>(), irp->ptr<int64_t>(), ipm->ptr<int64_t>(), g.N, g.H, V, lph);
        });
      });
      LAMP_LAUNCH_CHECK();
    }
    {
      KernelTimer kt("gat_backward_value", 2.0 * E * C, (E * C + N * C + E * g.H) * sz + E * 16 + N * 8, st);
      with_float(dt, [&](auto z) {
        using T = decltype(z);
        gat_with_packet<T>(gat_gather_packet<T>(C, V, {dv.get(), go.get()}), V, [&](auto W, auto one) {
          constexpr int VW = decltype(W)::value;
          hipLaunchKernelGGL((gat_backward_value_kernel<T, VW, decltype(one)::value>), row_grid(g.N, C, VW, kWaves + 1), dim3(kWaves * 64), 0, st, dv->ptr<T>(),
                             a->ptr<T>(), go->ptr<T>(), ej->ptr<int64_t>(), orp->ptr<int64_t>(), opm->ptr<int64_t>(), g.N, g.H, V);
        });
      });
      LAMP_LAUNCH_CHECK();
    }
  }
  *dscore = ds.take(); *dvalue = dv.take();
  LAMP_API_END
}

int lamp_mpnn_long_row(int64_t* out) {
  LAMP_API_BEGIN
  *out = kLongRow;
  LAMP_API_END
}

int lamp_mpnn_degree_factor(lamp_tensor** out, const lamp_tensor* rowptr, double p, int dtype) {
  LAMP_API_BEGIN
  check_device_tensor(rowptr, "rowptr");
  check_i64_vector(rowptr, rowptr, "rowptr");
  LAMP_CHECK(rowptr->numel() >= 1, "rowptr " << rowptr->describe() << " must be [N + 1]");
  LAMP_CHECK(dtype == kF32 || dtype == kF64, "f32 and f64 only, got " << dtype_name(dtype));
  LAMP_CHECK(p == -0.5 || p == -1.0, "the exponent must be -0.5 or -1, got " << p);
  const int64_t N = rowptr->numel() - 1;
  Hold rp(contiguous(rowptr));
  int64_t ns[1] = {N};
  Hold o(new_tensor(ns, 1, dtype, rowptr->device()));
  if (N) {
    hipStream_t st = current_stream(rowptr->device());
    KernelTimer kt("mpnn_degree_factor", 2.0 * N, (double)N * (8 + dtype_size(dtype)), st);
    const dim3 grid((unsigned)((N + 255) / 256));
    if (dtype == kF32 && p == -0.5) hipLaunchKernelGGL((mpnn_degree_factor_kernel<float, true>), grid, dim3(256), 0, st, o->ptr<float>(), rp->ptr<int64_t>(), N);
    else if (dtype == kF32) hipLaunchKernelGGL((mpnn_degree_factor_kernel<float, false>), grid, dim3(256), 0, st, o->ptr<float>(), rp->ptr<int64_t>(), N);
    else if (p == -0.5) hipLaunchKernelGGL((mpnn_degree_factor_kernel<double, true>), grid, dim3(256), 0, st, o->ptr<double>(), rp->ptr<int64_t>(), N);
    else hipLaunchKernelGGL((mpnn_degree_factor_kernel<double, false>), grid, dim3(256), 0, st, o->ptr<double>(), rp->ptr<int64_t>(), N);
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take();
  LAMP_API_END
}

int lamp_mpnn_message_forward(lamp_tensor** out, const lamp_tensor* x, const lamp_tensor* edgeFeatures, const lamp_tensor* edgeI, const lamp_tensor* edgeJ) {
  LAMP_API_BEGIN
  check_device_tensor(x, "x");
  mpnn_check_float(edgeFeatures, "edgeFeatures", x);
  LAMP_CHECK(x->ndim == 2, "x " << x->describe() << " must be [N, D]");
  LAMP_CHECK(edgeFeatures->ndim == 2, "edgeFeatures " << edgeFeatures->describe() << " must be [E, Fe]");
  check_i64_vector(edgeI, x, "edgeI");
  check_i64_vector(edgeJ, x, "edgeJ");
  const int64_t E = edgeI->numel(), Fe = edgeFeatures->sizes[1], D = x->sizes[1], W = Fe + 2 * D;
  LAMP_CHECK(edgeJ->numel() == E, "edgeI " << edgeI->describe() << " and edgeJ " << edgeJ->describe() << " differ in length");
  LAMP_CHECK(edgeFeatures->sizes[0] == E, "edgeFeatures " << edgeFeatures->describe() << " does not have one row per edge (" << E << " edges)");
  LAMP_CHECK(E == 0 || x->sizes[0] > 0, "x " << x->describe() << " has no rows");
  LAMP_CHECK(W <= INT32_MAX / 2, "a message of " << W << " columns is too wide");
  int64_t lde = 0, ldx = 0;
  Hold ec(rows_in_place(edgeFeatures, &lde)), xc(rows_in_place(x, &ldx)), ei(contiguous(edgeI)), ej(contiguous(edgeJ));
  int64_t os[2] = {E, W};
  Hold o(new_tensor(os, 2, x->dtype, x->device()));
  if (E * W) {
    hipStream_t st = current_stream(x->device());
    KernelTimer kt("mpnn_message", 0, 2.0 * E * W * dtype_size(x->dtype) + E * 16.0, st);
    with_float(x->dtype, [&](auto z) {
      using T = decltype(z);
      // per segment: the edge segment starts every row (pitch W), the node segments start at Fe and Fe + D
      const int ve = packet_width<T>({Fe, W, lde}, {o.get(), ec.get()}), vx = packet_width<T>({D, Fe, W, ldx}, {o.get(), xc.get()});
      const MpnnEdgeGrid g = mpnn_edge_grid(E, Fe / ve + 2 * (D / vx));
      with_packet<T>(ve, [&](auto VE) {
        with_packet<T>(vx, [&](auto VX) {
          hipLaunchKernelGGL((mpnn_message_kernel<T, decltype(VE)::value, decltype(VX)::value>), g.grid, dim3(kMpnnEdgeBlock), 0, st, o->ptr<T>(), ec->ptr<T>(), lde,
                             xc->ptr<T>(), ldx, ei->ptr<int64_t>(), ej->ptr<int64_t>(), E, (int)Fe, (int)D, g.slots);
        });
      });
    });
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take();
  LAMP_API_END
}

int lamp_mpnn_message_backward(lamp_tensor** dx_or_null, lamp_tensor** dedge_or_null, const lamp_tensor* dmsg, int64_t numNodes, int64_t edgeDim,
                               const lamp_tensor* inRowptr, const lamp_tensor* inPerm, const lamp_tensor* outRowptr, const lamp_tensor* outPerm) {
  LAMP_API_BEGIN
  check_device_tensor(dmsg, "dmsg");
  LAMP_CHECK(dmsg->dtype == kF32 || dmsg->dtype == kF64, "f32 and f64 only, got " << dmsg->describe());
  LAMP_CHECK(dmsg->ndim == 2, "dmsg " << dmsg->describe() << " must be [E, edgeDim + 2 D]");
  const int64_t E = dmsg->sizes[0], W = dmsg->sizes[1], N = numNodes, Fe = edgeDim;
  LAMP_CHECK(N >= 0 && Fe >= 0 && W >= Fe && (W - Fe) % 2 == 0, "dmsg " << dmsg->describe() << " is not [E, " << Fe << " + 2 D]");
  LAMP_CHECK(W <= INT32_MAX / 2, "a message of " << W << " columns is too wide");
  const int64_t D = (W - Fe) / 2;
  const int dt = dmsg->dtype, dev = dmsg->device();
  hipStream_t st = current_stream(dev);
  const double sz = (double)dtype_size(dt);
  Hold g(contiguous(dmsg)), dx, de;
  if (dx_or_null) {
    check_rowptrs({{inRowptr, "inRowptr"}, {outRowptr, "outRowptr"}}, dmsg, N);
    check_i64_vectors({{inPerm, "inPerm"}, {outPerm, "outPerm"}}, dmsg, E, "does not have dmsg's " + std::to_string(E) + " edges");
    Hold irp(contiguous(inRowptr)), ipm(contiguous(inPerm)), orp(contiguous(outRowptr)), opm(contiguous(outPerm));
    int64_t xs[2] = {N, D};
    dx = Hold(new_tensor(xs, 2, dt, dev));
    if (N * D) {
      KernelTimer kt("mpnn_message_backward_x", 2.0 * E * D, (2.0 * E * D + (double)N * D) * sz + E * 16.0 + N * 16.0, st);
      const MpnnSum a{dx.get(), g.get(), W, Fe, Fe + D, orp.get(), opm.get(), irp.get(), ipm.get(), nullptr, nullptr, nullptr, nullptr, N, D};
      with_float(dt, [&](auto z) {
        using T = decltype(z);
        mpnn_sum_launch<T, false, false>(packet_width<T>({D, Fe, W}, {dx.get(), g.get()}), a, st);
      });
      LAMP_LAUNCH_CHECK();
    }
  }
  if (dedge_or_null) {
    int64_t es[2] = {E, Fe};
    de = Hold(new_tensor(es, 2, dt, dev));
    if (E * Fe) {
      // dedge = dmsg[:, 0:Fe]
      KernelTimer kt("mpnn_message_backward_edge", 0, 2.0 * E * Fe * sz, st);
      with_float(dt, [&](auto z) {
        using T = decltype(z);
        const int v = packet_width<T>({Fe, W}, {de.get(), g.get()});
        const MpnnEdgeGrid eg = mpnn_edge_grid(E, Fe / v);
        with_packet<T>(v, [&](auto V) {
          hipLaunchKernelGGL((mpnn_columns_kernel<T, decltype(V)::value>), eg.grid, dim3(kMpnnEdgeBlock), 0, st, de->ptr<T>(), Fe, g->ptr<T>(), W, E, (int)Fe, eg.slots);
        });
      });
      LAMP_LAUNCH_CHECK();
    }
  }
  if (dx_or_null) *dx_or_null = dx.take();
  if (dedge_or_null) *dedge_or_null = de.take();
  LAMP_API_END
}

int lamp_mpnn_aggregate_forward(lamp_tensor** out, const lamp_tensor* message, const lamp_tensor* edgeI, const lamp_tensor* edgeJ,
                                const lamp_tensor* inRowptr, const lamp_tensor* inPerm, const lamp_tensor* outRowptr_or_null,
                                const lamp_tensor* outPerm_or_null, const lamp_tensor* fI_or_null, const lamp_tensor* fJ_or_null, int aggregateJ) {
  LAMP_API_BEGIN
  check_device_tensor(message, "message");
  LAMP_CHECK(message->dtype == kF32 || message->dtype == kF64, "f32 and f64 only, got " << message->describe());
  LAMP_CHECK(message->ndim == 2, "message " << message->describe() << " must be [E, M]");
  const int64_t E = message->sizes[0], M = message->sizes[1];
  LAMP_CHECK(M <= INT32_MAX / 2, "message " << message->describe() << " has too many columns");
  check_i64_vector(inRowptr, message, "inRowptr");
  LAMP_CHECK(inRowptr->numel() >= 1, "inRowptr " << inRowptr->describe() << " must be [N + 1]");
  const int64_t N = inRowptr->numel() - 1;
  LAMP_CHECK(!aggregateJ || (outRowptr_or_null && outPerm_or_null), "aggregateJ needs the outgoing grouping");
  const Tensor *orp0 = aggregateJ ? outRowptr_or_null : nullptr, *opm0 = aggregateJ ? outPerm_or_null : nullptr;
  check_i64_vectors({{edgeI, "edgeI"}, {edgeJ, "edgeJ"}, {inPerm, "inPerm"}, {opm0 ? opm0 : inPerm, "outPerm"}}, message, E,
                    "does not have one entry per row of message " + message->describe());
  if (orp0) check_rowptrs({{orp0, "outRowptr"}}, message, N);
  mpnn_check_factor(fI_or_null, "fI", message, N);
  mpnn_check_factor(fJ_or_null, "fJ", message, N);
  Hold mc(contiguous(message)), ei(contiguous(edgeI)), ej(contiguous(edgeJ)), irp(contiguous(inRowptr)), ipm(contiguous(inPerm)), orp(orp0 ? contiguous(orp0) : nullptr),
      opm(opm0 ? contiguous(opm0) : nullptr), fi(fI_or_null ? contiguous(fI_or_null) : nullptr), fj(fJ_or_null ? contiguous(fJ_or_null) : nullptr);
  int64_t os[2] = {N, M};
  Hold o(new_tensor(os, 2, message->dtype, message->device()));
  if (N * M) {
    hipStream_t st = current_stream(message->device());
    const double sz = (double)dtype_size(message->dtype), terms = (aggregateJ ? 2.0 : 1.0) * E;
    KernelTimer kt("mpnn_aggregate", 3.0 * terms * M, (terms * M + (double)N * M) * sz + terms * (24 + 2 * sz) + N * 16.0, st);
    const MpnnSum a{o.get(), mc.get(), M, 0, 0, irp.get(), ipm.get(), orp.get(), opm.get(), ei.get(), ej.get(), fi.get(), fj.get(), N, M};
    with_float(message->dtype, [&](auto z) {
      using T = decltype(z);
      mpnn_aggregate_launch<T>(packet_width<T>({M}, {o.get(), mc.get()}), a, st);
    });
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take();
  LAMP_API_END
}

int lamp_mpnn_aggregate_backward(lamp_tensor** dmsg, const lamp_tensor* dout, const lamp_tensor* edgeI, const lamp_tensor* edgeJ,
                                 const lamp_tensor* fI_or_null, const lamp_tensor* fJ_or_null, int aggregateJ) {
  LAMP_API_BEGIN
  check_device_tensor(dout, "dout");
  LAMP_CHECK(dout->dtype == kF32 || dout->dtype == kF64, "f32 and f64 only, got " << dout->describe());
  LAMP_CHECK(dout->ndim == 2, "dout " << dout->describe() << " must be [N, M]");
  const int64_t N = dout->sizes[0], M = dout->sizes[1];
  LAMP_CHECK(M <= INT32_MAX / 2, "dout " << dout->describe() << " has too many columns");
  check_i64_vector(edgeI, dout, "edgeI");
  check_i64_vector(edgeJ, dout, "edgeJ");
  const int64_t E = edgeI->numel();
  LAMP_CHECK(edgeJ->numel() == E, "edgeI " << edgeI->describe() << " and edgeJ " << edgeJ->describe() << " differ in length");
  LAMP_CHECK(E == 0 || N > 0, "dout " << dout->describe() << " has no rows");
  mpnn_check_factor(fI_or_null, "fI", dout, N);
  mpnn_check_factor(fJ_or_null, "fJ", dout, N);
  Hold gc(contiguous(dout)), ei(contiguous(edgeI)), ej(contiguous(edgeJ)), fi(fI_or_null ? contiguous(fI_or_null) : nullptr), fj(fJ_or_null ? contiguous(fJ_or_null) : nullptr);
  int64_t ms[2] = {E, M};
  Hold o(new_tensor(ms, 2, dout->dtype, dout->device()));
  if (E * M) {
    hipStream_t st = current_stream(dout->device());
    const double sz = (double)dtype_size(dout->dtype);
    KernelTimer kt("mpnn_aggregate_backward", 3.0 * E * M, ((aggregateJ ? 3.0 : 2.0) * E * M + 2.0 * E) * sz + E * 16.0, st);
    with_float(dout->dtype, [&](auto z) {
      using T = decltype(z);
      const int v = packet_width<T>({M}, {o.get(), gc.get()});
      const MpnnEdgeGrid g = mpnn_edge_grid(E, M / v);
      with_packet<T>(v, [&](auto V) {
        hipLaunchKernelGGL((mpnn_aggregate_backward_kernel<T, decltype(V)::value>), g.grid, dim3(kMpnnEdgeBlock), 0, st, o->ptr<T>(), gc->ptr<T>(), ei->ptr<int64_t>(),
                           ej->ptr<int64_t>(), fi.get() ? fi->ptr<T>() : nullptr, fj.get() ? fj->ptr<T>() : nullptr, aggregateJ, E, (int)M, g.slots);
      });
    });
    LAMP_LAUNCH_CHECK();
  }
  *dmsg = o.take();
  LAMP_API_END
}

int lamp_graph_gather_backward(lamp_tensor** dx, const lamp_tensor* dout, const lamp_tensor* rowptr, const lamp_tensor* perm) {
  LAMP_API_BEGIN
  check_device_tensor(dout, "dout");
  LAMP_CHECK(dout->dtype == kF32 || dout->dtype == kF64, "f32 and f64 only, got " << dout->describe());
  LAMP_CHECK(dout->ndim == 2, "dout " << dout->describe() << " must be [E, C]");
  const int64_t E = dout->sizes[0], C = dout->sizes[1];
  LAMP_CHECK(C <= INT32_MAX / 2, "dout " << dout->describe() << " has too many columns");
  check_i64_vector(rowptr, dout, "rowptr");
  LAMP_CHECK(rowptr->numel() >= 1, "rowptr " << rowptr->describe() << " must be [N + 1]");
  check_i64_vectors({{perm, "perm"}}, dout, E, "does not have dout's " + std::to_string(E) + " rows");
  const int64_t N = rowptr->numel() - 1;
  Hold g(contiguous(dout)), rp(contiguous(rowptr)), pm(contiguous(perm));
  int64_t xs[2] = {N, C};
  Hold o(new_tensor(xs, 2, dout->dtype, dout->device()));
  if (N * C) {
    hipStream_t st = current_stream(dout->device());
    KernelTimer kt("graph_gather_backward", (double)E * C, ((double)E * C + (double)N * C) * dtype_size(dout->dtype) + E * 8.0 + N * 8.0, st);
    const MpnnSum a{o.get(), g.get(), C, 0, 0, rp.get(), pm.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, C};
    with_float(dout->dtype, [&](auto z) {
      using T = decltype(z);
      mpnn_sum_launch<T, false, false>(packet_width<T>({C}, {o.get(), g.get()}), a, st);
    });
    LAMP_LAUNCH_CHECK();
  }
  *dx = o.take();
  LAMP_API_END
}

int lamp_graph_batch_rows(lamp_tensor** out, const lamp_tensor* src, const lamp_tensor* plan, int64_t planOffset, int64_t numGraphs, int64_t outRows,
                          int edgeRows) {
  LAMP_API_BEGIN
  check_device_tensor(src, "src");
  const int64_t* pl = plan_slice(plan, planOffset, numGraphs);
  check_same_device(plan, src);
  LAMP_CHECK(src->ndim >= 1 && outRows >= 0, "src " << src->describe() << " must have a row per node or edge, and outRows = " << outRows << " must not be negative");
  Hold sc(contiguous(src));
  std::vector<int64_t> os = src->shape();
  os[0] = outRows;
  int64_t width = 1;
  for (int d = 1; d < src->ndim; d++) width *= src->sizes[d];
  Hold o(new_tensor(os, src->dtype, src->device()));
  const int64_t bytes = width * (int64_t)dtype_size(src->dtype);
  if (outRows * bytes) {
    hipStream_t st = current_stream(src->device());
    KernelTimer kt("graph_batch_rows", 0, 2.0 * outRows * bytes + outRows * 16.0, st);
    const int unit = copy_unit(bytes, o->raw(), sc->raw());
    const MpnnEdgeGrid g = mpnn_edge_grid(outRows, bytes / unit);
    auto launch = [&](auto p) {
      using P = decltype(p);
      hipLaunchKernelGGL((graph_batch_rows_kernel<P>), g.grid, dim3(kMpnnEdgeBlock), 0, st, (P*)o->data(), (const P*)sc->raw(), pl, edgeRows ? 2 : 0, (int)numGraphs,
                         outRows, g.slots);
    };
    if (unit == 16) launch(Vec<uint32_t, 4>());
    else if (unit == 8) launch(Vec<uint32_t, 2>());
    else if (unit == 4) launch(uint32_t());
    else if (unit == 2) launch(uint16_t());
    else launch(uint8_t());
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take();
  LAMP_API_END
}

int lamp_graph_batch_nodes(lamp_tensor** pool, lamp_tensor** graphPtr, lamp_tensor** adjRowptr_or_null, lamp_tensor** dinv_or_null,
                           lamp_tensor** inRowptr_or_null, lamp_tensor** outRowptr_or_null, const lamp_tensor* plan, int64_t planOffset, int64_t numGraphs,
                           int64_t numNodes, int64_t numEdges, const lamp_tensor* setAdjRowptr_or_null, const lamp_tensor* setDinv_or_null,
                           const lamp_tensor* setInRowptr_or_null, const lamp_tensor* setOutRowptr_or_null) {
  LAMP_API_BEGIN
  const int64_t* pl = plan_slice(plan, planOffset, numGraphs);
  const int64_t B = numGraphs, N = numNodes, E = numEdges;
  LAMP_CHECK(N >= B && E >= 0, "a batch of " << B << " graphs has " << N << " nodes and " << E << " edges: every graph must have a node");
  const Tensor *sa = setAdjRowptr_or_null, *sd = setDinv_or_null, *si = setInRowptr_or_null, *so = setOutRowptr_or_null;
  LAMP_CHECK((!sa || adjRowptr_or_null) && (!sd || dinv_or_null) && (!si || inRowptr_or_null) && (!so || outRowptr_or_null), "a set-wide array without its output");
  LAMP_CHECK(!sa == !sd, "the adjacency's rowptr and dinv come together");
  check_set_vector(sa, "setAdjRowptr", plan, 2);
  check_set_vector(si, "setInRowptr", plan, 2);
  check_set_vector(so, "setOutRowptr", plan, 2);
  if (sd) {
    check_device_tensor(sd, "setDinv");
    check_same_device(sd, plan);
    LAMP_CHECK((sd->dtype == kF32 || sd->dtype == kF64) && sd->ndim == 1 && sd->is_contiguous() && sd->numel() + 1 == sa->numel(),
               "setDinv " << sd->describe() << " must be a contiguous f32 / f64 vector of one entry per row of setAdjRowptr " << sa->describe());
  }
  const int dev = plan->device();
  int64_t ns[1] = {N}, n1[1] = {N + 1}, b1[1] = {B + 1};
  Hold pv(new_tensor(ns, 1, kI64, dev)), gp(new_tensor(b1, 1, kI64, dev)), ar(sa ? new_tensor(n1, 1, kI64, dev) : nullptr),
      dv(sd ? new_tensor(ns, 1, sd->dtype, dev) : nullptr), ir(si ? new_tensor(n1, 1, kI64, dev) : nullptr), orp(so ? new_tensor(n1, 1, kI64, dev) : nullptr);
  {
    hipStream_t st = current_stream(dev);
    auto wp = [](Hold& h) { return h.get() ? h->ptr<int64_t>() : nullptr; };
    auto rp = [](const Tensor* t) { return t ? t->ptr<int64_t>() : nullptr; };
    const BatchNodes a{wp(pv), wp(gp), wp(ar), wp(ir), wp(orp), rp(sa), rp(si), rp(so)};
    const double arrays = 1.0 + (sa ? 1 : 0) + (si ? 1 : 0) + (so ? 1 : 0);
    KernelTimer kt("graph_batch_index", 0, (double)N * (arrays * 16.0 + (sd ? 2.0 * dtype_size(sd->dtype) : 0.0)), st);
    with_float(sd ? sd->dtype : kF32, [&](auto z) {
      using T = decltype(z);
      hipLaunchKernelGGL((graph_batch_nodes_kernel<T>), dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, st, a, dv.get() ? dv->ptr<T>() : nullptr,
                         sd ? sd->ptr<T>() : nullptr, pl, (int)B, N, E);
    });
    LAMP_LAUNCH_CHECK();
  }
  *pool = pv.take(); *graphPtr = gp.take();
  if (adjRowptr_or_null) *adjRowptr_or_null = ar.take();
  if (dinv_or_null) *dinv_or_null = dv.take();
  if (inRowptr_or_null) *inRowptr_or_null = ir.take();
  if (outRowptr_or_null) *outRowptr_or_null = orp.take();
  LAMP_API_END
}

int lamp_graph_batch_edges(lamp_tensor** edgeI, lamp_tensor** edgeJ, lamp_tensor** col_or_null, lamp_tensor** inPerm_or_null, lamp_tensor** outPerm_or_null,
                           const lamp_tensor* plan, int64_t planOffset, int64_t numGraphs, int64_t numNodes, int64_t numEdges, const lamp_tensor* setEdgeI,
                           const lamp_tensor* setEdgeJ, const lamp_tensor* setCol_or_null, const lamp_tensor* setInPerm_or_null,
                           const lamp_tensor* setOutPerm_or_null) {
  LAMP_API_BEGIN
  const int64_t* pl = plan_slice(plan, planOffset, numGraphs);
  const int64_t B = numGraphs, N = numNodes, E = numEdges;
  LAMP_CHECK(N >= B && E >= 0 && 2 * E < ((int64_t)1 << 31), "a batch of " << B << " graphs has " << N << " nodes and " << E << " edges");
  const Tensor *sc = setCol_or_null, *si = setInPerm_or_null, *so = setOutPerm_or_null;
  LAMP_CHECK((!sc || col_or_null) && (!si || inPerm_or_null) && (!so || outPerm_or_null), "a set-wide array without its output");
  LAMP_CHECK(setEdgeI && setEdgeJ, "the set's edge list is null");
  check_set_vector(setEdgeI, "setEdgeI", plan, E ? 1 : 0);
  check_set_vector(setEdgeJ, "setEdgeJ", plan, setEdgeI->numel());
  check_set_vector(sc, "setCol", plan, 2 * setEdgeI->numel());
  check_set_vector(si, "setInPerm", plan, setEdgeI->numel());
  check_set_vector(so, "setOutPerm", plan, setEdgeI->numel());
  const int dev = plan->device();
  int64_t es[1] = {E}, e2[1] = {2 * E};
  Hold ei(new_tensor(es, 1, kI64, dev)), ej(new_tensor(es, 1, kI64, dev)), cl(sc ? new_tensor(e2, 1, kI64, dev) : nullptr),
      ip(si ? new_tensor(es, 1, kI64, dev) : nullptr), op(so ? new_tensor(es, 1, kI64, dev) : nullptr);
  if (E) {
    hipStream_t st = current_stream(dev);
    auto wp = [](Hold& h) { return h.get() ? h->ptr<int64_t>() : nullptr; };
    auto rp = [](const Tensor* t) { return t ? t->ptr<int64_t>() : nullptr; };
    const BatchEdges a{wp(ei), wp(ej), wp(cl), wp(ip), wp(op), rp(setEdgeI), rp(setEdgeJ), rp(sc), rp(si), rp(so)};
    KernelTimer kt("graph_batch_index", 0, (double)E * 16.0 * (2.0 + (sc ? 2 : 0) + (si ? 1 : 0) + (so ? 1 : 0)), st);
    hipLaunchKernelGGL(graph_batch_edges_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, a, pl, (int)B, E);
    LAMP_LAUNCH_CHECK();
  }
  *edgeI = ei.take(); *edgeJ = ej.take();
  if (col_or_null) *col_or_null = cl.take();
  if (inPerm_or_null) *inPerm_or_null = ip.take();
  if (outPerm_or_null) *outPerm_or_null = op.take();
  LAMP_API_END
}

int lamp_graph_set_check(lamp_tensor** bad, const lamp_tensor* edgeI, const lamp_tensor* edgeJ, const lamp_tensor* nodePtr, const lamp_tensor* edgePtr) {
  LAMP_API_BEGIN
  check_device_tensor(edgeI, "edgeI");
  check_i64_vector(edgeI, edgeI, "edgeI");
  check_i64_vector(edgeJ, edgeI, "edgeJ");
  check_i64_vector(nodePtr, edgeI, "nodePtr");
  check_i64_vector(edgePtr, edgeI, "edgePtr");
  const int64_t E = edgeI->numel(), G = nodePtr->numel() - 1;
  LAMP_CHECK(edgeJ->numel() == E, "edgeI " << edgeI->describe() << " and edgeJ " << edgeJ->describe() << " differ in length");
  LAMP_CHECK(G >= 1 && edgePtr->numel() == G + 1, "nodePtr " << nodePtr->describe() << " and edgePtr " << edgePtr->describe() << " must both be [G + 1], G >= 1");
  Hold ei(contiguous(edgeI)), ej(contiguous(edgeJ)), np(contiguous(nodePtr)), ep(contiguous(edgePtr));
  int64_t one[1] = {1};
  Hold b(new_tensor(one, 1, kI64, edgeI->device()));
  fill_zero(b.get());
  if (E) {
    hipStream_t st = current_stream(edgeI->device());
    KernelTimer kt("graph_set_check", 0, (double)E * 16.0, st);
    hipLaunchKernelGGL(graph_set_check_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, b->ptr<int64_t>(), ei->ptr<int64_t>(), ej->ptr<int64_t>(),
                       np->ptr<int64_t>(), ep->ptr<int64_t>(), G, E);
    LAMP_LAUNCH_CHECK();
  }
  *bad = b.take();
  LAMP_API_END
}

int lamp_segment_pool_forward(lamp_tensor** out, const lamp_tensor* x, const lamp_tensor* graphPtr, int mean) {
  LAMP_API_BEGIN
  check_device_tensor(x, "x");
  LAMP_CHECK(x->dtype == kF32 || x->dtype == kF64, "f32 and f64 only, got " << x->describe());
  LAMP_CHECK(x->ndim == 2, "x " << x->describe() << " must be [N, D]");
  check_i64_vector(graphPtr, x, "graphPtr");
  LAMP_CHECK(graphPtr->numel() >= 1, "graphPtr " << graphPtr->describe() << " must be [B + 1]");
  const int64_t N = x->sizes[0], D = x->sizes[1], B = graphPtr->numel() - 1;
  int64_t ldx = 0;
  Hold xc(rows_in_place(x, &ldx)), gp(contiguous(graphPtr));
  int64_t os[2] = {B, D};
  Hold o(new_tensor(os, 2, x->dtype, x->device()));
  if (B * D) {
    hipStream_t st = current_stream(x->device());
    const double sz = (double)dtype_size(x->dtype);
    KernelTimer kt("segment_pool", (double)N * D, ((double)N * D + (double)B * D) * sz + B * 8.0, st);
    with_float(x->dtype, [&](auto z) {
      using T = decltype(z);
      with_packet<T>(packet_width<T>({D, ldx}, {o.get(), xc.get()}), [&](auto W) {
        constexpr int V = decltype(W)::value;
        hipLaunchKernelGGL((segment_pool_kernel<T, V>), row_grid(B, D, V, kWaves + 1), dim3(kWaves * 64), 0, st, o->ptr<T>(), xc->ptr<T>(), ldx, gp->ptr<int64_t>(), B, N,
                           D, mean);
      });
    });
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take();
  LAMP_API_END
}

int lamp_segment_pool_backward(lamp_tensor** dx, const lamp_tensor* dout, const lamp_tensor* graphPtr, const lamp_tensor* pool, int mean) {
  LAMP_API_BEGIN
  check_device_tensor(dout, "dout");
  LAMP_CHECK(dout->dtype == kF32 || dout->dtype == kF64, "f32 and f64 only, got " << dout->describe());
  LAMP_CHECK(dout->ndim == 2, "dout " << dout->describe() << " must be [B, D]");
  const int64_t B = dout->sizes[0], D = dout->sizes[1];
  LAMP_CHECK(D <= INT32_MAX / 2, "dout " << dout->describe() << " has too many columns");
  check_i64_vector(pool, dout, "pool");
  check_i64_vectors({{graphPtr, "graphPtr"}}, dout, B + 1, "does not mark the " + std::to_string(B) + " graphs of dout");
  const int64_t N = pool->numel();
  LAMP_CHECK(N == 0 || B > 0, "dout " << dout->describe() << " has no rows");
  Hold gc(contiguous(dout)), gp(contiguous(graphPtr)), pc(contiguous(pool));
  int64_t xs[2] = {N, D};
  Hold o(new_tensor(xs, 2, dout->dtype, dout->device()));
  if (N * D) {
    hipStream_t st = current_stream(dout->device());
    KernelTimer kt("segment_pool_backward", mean ? (double)N * D : 0.0, 2.0 * N * D * dtype_size(dout->dtype) + N * 8.0, st);
    with_float(dout->dtype, [&](auto z) {
      using T = decltype(z);
      const int v = packet_width<T>({D}, {o.get(), gc.get()});
      const MpnnEdgeGrid g = mpnn_edge_grid(N, D / v);
      with_packet<T>(v, [&](auto V) {
        hipLaunchKernelGGL((segment_pool_backward_kernel<T, decltype(V)::value>), g.grid, dim3(kMpnnEdgeBlock), 0, st, o->ptr<T>(), gc->ptr<T>(), gp->ptr<int64_t>(),
                           pc->ptr<int64_t>(), N, B, (int)D, mean, g.slots);
      });
    });
    LAMP_LAUNCH_CHECK();
  }
  *dx = o.take();
  LAMP_API_END
}

}  // extern "C"
