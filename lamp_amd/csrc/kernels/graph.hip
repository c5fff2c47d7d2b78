// Graph convolution (lamp-core/src/main/scala/lamp/nn/graph/GCN.scala:30-145): D^-1/2 (A + A' + I) D^-1/2 X as one gather-only kernel
// over a CSR of A + A', f32 and f64.
//
// The reference builds a sparse COO tensor and multiplies it with `mm`; this library has no sparse tensor.  lamp_gcn_adjacency turns
// the edge list into (rowptr, col, dinv) once per graph, lamp_gcn_aggregate is the product.  The matrix is symmetric, so the gradient
// with respect to X is the same kernel applied to the incoming gradient.
//
// gcn_aggregate_kernel: a workgroup of kGcnWaves waves owns kGcnWaves neighbouring rows, a wave one row; the 64 lanes run across the
// feature dimension (V columns each, 16-byte packets where D and the row pitches allow it), so every neighbour row is one coalesced
// read and the output row one coalesced write.  Per 64 neighbours a wave reads col[p] and dinv[col[p]] once (one entry per lane) and
// hands them round with v_readlane: the row address is wave-uniform.  kGcnUnroll neighbour rows are in flight per wave.  No atomics: a
// row's sum runs over its neighbours in CSR order, which lamp_gcn_adjacency fixes (stable sort), so the result is a function of the
// input alone.  A row longer than kGcnLongRow (a hub) would serialise its wave: all waves of the workgroup take a contiguous share of
// its neighbours, park their partial sums in LDS, and wave 0 adds them in wave order.  D beyond one wave's reach is tiled in grid.y.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "device_utils.h"

namespace lamp {
namespace {

constexpr int kGcnWaves = 16;       // waves (= rows) per workgroup
constexpr int kGcnLongRow = 256;    // a row with more neighbours is split across the workgroup's waves
constexpr int kGcnUnroll = 8;       // neighbour rows in flight per wave

// the value lane k holds, in every lane (k wave-uniform)
__device__ __forceinline__ int64_t lane_bcast(int64_t v, int k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), k);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float lane_bcast(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ double lane_bcast(double v, int k) { return __longlong_as_double((long long)lane_bcast((int64_t)__double_as_longlong(v), k)); }

template <class T, int V> __device__ __forceinline__ Vec<T, V> gcn_zero() {
  Vec<T, V> z;
#pragma unroll
  for (int j = 0; j < V; j++) z.v[j] = T(0);
  return z;
}
template <class T, int V> __device__ __forceinline__ Vec<T, V> gcn_load(const T* p) { return *reinterpret_cast<const Vec<T, V>*>(p); }

// acc += sum over p in [b, e), in that order, of dinv[col[p]] * x[col[p], c0 .. c0 + V).  xc = x + c0; lanes with `active` false hold
// no column (c0 >= D): they take part in the index reads and load no row.  b and e are wave-uniform.
template <class T, int V>
__device__ __forceinline__ void gcn_gather(Vec<T, V>& acc, const T* __restrict__ xc, int64_t ldx, const int64_t* __restrict__ col,
                                           const T* __restrict__ dinv, int64_t b, int64_t e, int lane, bool active) {
  for (int64_t p = b; p < e; p += 64) {
    const int n = (int)(e - p < 64 ? e - p : 64);
    int64_t c = 0;
    T dv = T(0);
    if (lane < n) { c = col[p + lane]; dv = dinv[c]; }
    int k = 0;
    for (; k + kGcnUnroll <= n; k += kGcnUnroll) {
      Vec<T, V> v[kGcnUnroll];
      T d[kGcnUnroll];
#pragma unroll
      for (int u = 0; u < kGcnUnroll; u++) {
        const int64_t cu = lane_bcast(c, k + u);
        d[u] = lane_bcast(dv, k + u);
        v[u] = active ? gcn_load<T, V>(xc + cu * ldx) : gcn_zero<T, V>();
      }
#pragma unroll
      for (int u = 0; u < kGcnUnroll; u++)
#pragma unroll
        for (int j = 0; j < V; j++) acc.v[j] += d[u] * v[u].v[j];
    }
    for (; k < n; k++) {
      const int64_t cu = lane_bcast(c, k);
      const T d = lane_bcast(dv, k);
      const Vec<T, V> v = active ? gcn_load<T, V>(xc + cu * ldx) : gcn_zero<T, V>();
#pragma unroll
      for (int j = 0; j < V; j++) acc.v[j] += d * v.v[j];
    }
  }
}

// out[r, :] = dinv[r] * (dinv[r] * x[r, :] + sum over the row's neighbours c, in CSR order, of dinv[c] * x[c, :]).  D % V == 0.
// grid: (ceil(N / kGcnWaves), ceil(D / (64 * V))), block: kGcnWaves * 64.
template <class T, int V>
__global__ __launch_bounds__(kGcnWaves * 64) void gcn_aggregate_kernel(T* __restrict__ out, int64_t ldo, const T* __restrict__ x, int64_t ldx,
                                                                        const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                                        const T* __restrict__ dinv, int64_t N, int64_t D) {
  __shared__ Vec<T, V> part[kGcnWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t c0 = ((int64_t)blockIdx.y * 64 + lane) * V;
  const bool active = c0 < D;
  const int64_t row0 = (int64_t)blockIdx.x * kGcnWaves;
  const T* xc = x + c0;

  // every wave its own row, unless it is a long one
  const int64_t r = row0 + wave;
  if (r < N) {
    const int64_t b = rowptr[r], e = rowptr[r + 1];
    if (e - b <= kGcnLongRow) {
      const T dr = dinv[r];
      Vec<T, V> acc = active ? gcn_load<T, V>(xc + r * ldx) : gcn_zero<T, V>();
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

  // the long rows of this workgroup, one after the other, by all its waves (the conditions are the same in every thread of the workgroup)
  const int nrows = (int)(N - row0 < kGcnWaves ? N - row0 : kGcnWaves);
  for (int k = 0; k < nrows; k++) {
    const int64_t lr = row0 + k;
    const int64_t b = rowptr[lr], e = rowptr[lr + 1];
    if (e - b <= kGcnLongRow) continue;
    const int64_t chunk = (e - b + kGcnWaves - 1) / kGcnWaves;
    const int64_t pb = b + wave * chunk < e ? b + wave * chunk : e;
    const int64_t pe = pb + chunk < e ? pb + chunk : e;
    Vec<T, V> acc = gcn_zero<T, V>();
    gcn_gather<T, V>(acc, xc, ldx, col, dinv, pb, pe, lane, active);
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && active) {
      const T dr = dinv[lr];
      Vec<T, V> s = gcn_load<T, V>(xc + lr * ldx);
#pragma unroll
      for (int j = 0; j < V; j++) s.v[j] *= dr;
      for (int w = 0; w < kGcnWaves; w++) {
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
// [N + 1] and the edge ids stably sorted by endpoint) and every kernel is gather-only, without atomics, with a fixed order.
//
// gat_forward_kernel and gat_backward_value_kernel have gcn_aggregate_kernel's shape: a wave per row, lanes across the C = H * V columns
// in packets of VW elements, C tiled in grid.y, edge id and source row read once per 64 edges (one per lane) and passed round with
// v_readlane, kGatUnroll edges in flight, a row of more than kGatLongRow edges split over the workgroup's waves and merged through LDS
// by wave 0 in wave order.  A packet of two may straddle a head boundary (V odd): ONE = false keeps a softmax state per element then,
// ONE = true one per lane; packets of four are used only where V % 4 == 0.  The softmax is the online form with one exp per edge and
// head: against the row's running maximum m, either the new score is larger (the sums so far are scaled by exp(m - x)) or it is not (it
// enters as exp(x - m)).
constexpr int kGatWaves = 16;       // waves (= rows) per workgroup
constexpr int kGatLongRow = 256;    // a row with more edges is split across the workgroup's waves
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
    a = gcn_zero<T, VW>();
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

// st takes in the edges perm[b .. e) in that order: score[edge, hh[.]] and value row src[edge], columns c0 .. c0 + VW (vc = value + c0).
// Lanes with `active` false hold no column: they take part in the index reads and load nothing else.  b and e are wave-uniform.
template <class T, int VW, bool ONE>
__device__ __forceinline__ void gat_gather(GatAcc<T, VW, ONE>& st, const T* __restrict__ score, int64_t H, const int (&hh)[ONE ? 1 : VW],
                                           const T* __restrict__ vc, int64_t ldv, const int64_t* __restrict__ perm, const int64_t* __restrict__ src,
                                           int64_t b, int64_t e, int lane, bool active) {
  constexpr int NH = ONE ? 1 : VW, kGatUnroll = gat_unroll<T>();
  for (int64_t p = b; p < e; p += 64) {
    const int n = (int)(e - p < 64 ? e - p : 64);
    int64_t ed = 0, sr = 0;
    if (lane < n) { ed = perm[p + lane]; sr = src[ed]; }
    int k = 0;
    for (; k + kGatUnroll <= n; k += kGatUnroll) {
      Vec<T, VW> v[kGatUnroll];
      T x[kGatUnroll][NH];
#pragma unroll
      for (int u = 0; u < kGatUnroll; u++) {
        const int64_t eu = lane_bcast(ed, k + u), su = lane_bcast(sr, k + u);
#pragma unroll
        for (int h = 0; h < NH; h++) x[u][h] = active ? score[eu * H + hh[h]] : T(0);
        v[u] = active ? gcn_load<T, VW>(vc + su * ldv) : gcn_zero<T, VW>();
      }
#pragma unroll
      for (int u = 0; u < kGatUnroll; u++) st.step(x[u], v[u]);
    }
    for (; k < n; k++) {
      const int64_t eu = lane_bcast(ed, k), su = lane_bcast(sr, k);
      T x[NH];
#pragma unroll
      for (int h = 0; h < NH; h++) x[h] = active ? score[eu * H + hh[h]] : T(0);
      st.step(x, active ? gcn_load<T, VW>(vc + su * ldv) : gcn_zero<T, VW>());
    }
  }
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
// (rowptr, perm).  grid: (ceil(N / kGatWaves), ceil(C / (64 * VW))), block: kGatWaves * 64.
template <class T, int VW, bool ONE>
__global__ __launch_bounds__(kGatWaves * 64) void gat_forward_kernel(T* __restrict__ out, T* __restrict__ lse, const T* __restrict__ score,
                                                                      const T* __restrict__ value, const int64_t* __restrict__ edgeI,
                                                                      const int64_t* __restrict__ rowptr, const int64_t* __restrict__ perm, int64_t N,
                                                                      int64_t H, int V) {
  constexpr int NH = ONE ? 1 : VW;
  __shared__ Vec<T, VW> part[kGatWaves][64];
  __shared__ T pm[kGatWaves][NH][64], ps[kGatWaves][NH][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t C = H * V;
  const int c0 = ((int)blockIdx.y * 64 + lane) * VW;
  const bool active = c0 < C;
  int hh[NH];
#pragma unroll
  for (int h = 0; h < NH; h++) hh[h] = active ? (c0 + h) / V : 0;
  const int64_t row0 = (int64_t)blockIdx.x * kGatWaves;
  const T* vc = value + c0;
  const int nrows = (int)(N - row0 < kGatWaves ? N - row0 : kGatWaves);

  // k = blockIdx.z - 1.  k = -1: every wave its own row, unless it is a long one; k >= 0: row row0 + k if it is long, by all waves of the
  // workgroup (that condition is the same in every thread of the workgroup, so the barriers are).  A grid slice per k, so that long rows
  // that are neighbours (hubs numbered 0, 1, 2, ...) run side by side and not one after the other in their workgroup; the workgroups of the
  // slices k >= 0 whose row is short, nearly all of them, read two row pointers and leave.
  for (int k = (int)blockIdx.z - 1; k < (int)blockIdx.z && k < nrows; k++) {   // one turn: a grid slice per k
    const bool own = k < 0;
    const int64_t r = own ? (wave < nrows ? row0 + wave : -1) : row0 + k;
    int64_t b = 0, e = 0;
    if (r >= 0) { b = rowptr[r]; e = rowptr[r + 1]; }
    const bool longRow = e - b > kGatLongRow;
    if (own == longRow) continue;
    if (!own) {
      const int64_t chunk = (e - b + kGatWaves - 1) / kGatWaves;
      b = b + wave * chunk < e ? b + wave * chunk : e;
      e = b + chunk < e ? b + chunk : e;
    }
    GatAcc<T, VW, ONE> st;
    st.init();
    gat_gather<T, VW, ONE>(st, score, H, hh, vc, C, perm, edgeI, b, e, lane, active);
    if (own) {
      if (active && r >= 0) gat_finish<T, VW, ONE>(st, out, lse, r, C, H, V, c0, hh);
      continue;
    }
    part[wave][lane] = st.a;
#pragma unroll
    for (int h = 0; h < NH; h++) { pm[wave][h][lane] = st.m[h]; ps[wave][h][lane] = st.s[h]; }
    __syncthreads();
    if (wave == 0 && active) {
#pragma unroll 1
      for (int w = 1; w < kGatWaves; w++) {
        T mw[NH], sw[NH];
#pragma unroll
        for (int h = 0; h < NH; h++) { mw[h] = pm[w][h][lane]; sw[h] = ps[w][h][lane]; }
        st.merge(mw, sw, part[w][lane]);
      }
      gat_finish<T, VW, ONE>(st, out, lse, r, C, H, V, c0, hh);
    }
    __syncthreads();
  }
}

// acc += sum over the edges perm[b .. e), in that order, of a[edge, hh[.]] * x[src[edge], c0 .. c0 + VW) (xc = x + c0)
template <class T, int VW, bool ONE>
__device__ __forceinline__ void gat_weighted_gather(Vec<T, VW>& acc, const T* __restrict__ a, int64_t H, const int (&hh)[ONE ? 1 : VW],
                                                    const T* __restrict__ xc, int64_t ldx, const int64_t* __restrict__ perm,
                                                    const int64_t* __restrict__ src, int64_t b, int64_t e, int lane, bool active) {
  constexpr int NH = ONE ? 1 : VW, kGatUnroll = gat_unroll<T>();
  for (int64_t p = b; p < e; p += 64) {
    const int n = (int)(e - p < 64 ? e - p : 64);
    int64_t ed = 0, sr = 0;
    if (lane < n) { ed = perm[p + lane]; sr = src[ed]; }
    int k = 0;
    for (; k + kGatUnroll <= n; k += kGatUnroll) {
      Vec<T, VW> v[kGatUnroll];
      T w[kGatUnroll][NH];
#pragma unroll
      for (int u = 0; u < kGatUnroll; u++) {
        const int64_t eu = lane_bcast(ed, k + u), su = lane_bcast(sr, k + u);
#pragma unroll
        for (int h = 0; h < NH; h++) w[u][h] = active ? a[eu * H + hh[h]] : T(0);
        v[u] = active ? gcn_load<T, VW>(xc + su * ldx) : gcn_zero<T, VW>();
      }
#pragma unroll
      for (int u = 0; u < kGatUnroll; u++)
#pragma unroll
        for (int j = 0; j < VW; j++) acc.v[j] += w[u][ONE ? 0 : j] * v[u].v[j];
    }
    for (; k < n; k++) {
      const int64_t eu = lane_bcast(ed, k), su = lane_bcast(sr, k);
      T w[NH];
#pragma unroll
      for (int h = 0; h < NH; h++) w[h] = active ? a[eu * H + hh[h]] : T(0);
      const Vec<T, VW> v = active ? gcn_load<T, VW>(xc + su * ldx) : gcn_zero<T, VW>();
#pragma unroll
      for (int j = 0; j < VW; j++) acc.v[j] += w[ONE ? 0 : j] * v.v[j];
    }
  }
}

// dvalue[i, h, :] = sum over the edges e leaving i (the outgoing grouping, in its order) of a[e, h] * dout[edgeJ[e], h, :].  Same grid,
// same split of a long row; the partial sums are added in wave order.
template <class T, int VW, bool ONE>
__global__ __launch_bounds__(kGatWaves * 64) void gat_backward_value_kernel(T* __restrict__ dvalue, const T* __restrict__ a, const T* __restrict__ dout,
                                                                             const int64_t* __restrict__ edgeJ, const int64_t* __restrict__ rowptr,
                                                                             const int64_t* __restrict__ perm, int64_t N, int64_t H, int V) {
  constexpr int NH = ONE ? 1 : VW;
  __shared__ Vec<T, VW> part[kGatWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t C = H * V;
  const int c0 = ((int)blockIdx.y * 64 + lane) * VW;
  const bool active = c0 < C;
  int hh[NH];
#pragma unroll
  for (int h = 0; h < NH; h++) hh[h] = active ? (c0 + h) / V : 0;
  const int64_t row0 = (int64_t)blockIdx.x * kGatWaves;
  const T* xc = dout + c0;
  const int nrows = (int)(N - row0 < kGatWaves ? N - row0 : kGatWaves);

  for (int k = (int)blockIdx.z - 1; k < (int)blockIdx.z && k < nrows; k++) {   // one turn: a grid slice per k          // as in gat_forward_kernel
    const bool own = k < 0;
    const int64_t r = own ? (wave < nrows ? row0 + wave : -1) : row0 + k;
    int64_t b = 0, e = 0;
    if (r >= 0) { b = rowptr[r]; e = rowptr[r + 1]; }
    const bool longRow = e - b > kGatLongRow;
    if (own == longRow) continue;
    if (!own) {
      const int64_t chunk = (e - b + kGatWaves - 1) / kGatWaves;
      b = b + wave * chunk < e ? b + wave * chunk : e;
      e = b + chunk < e ? b + chunk : e;
    }
    Vec<T, VW> acc = gcn_zero<T, VW>();
    gat_weighted_gather<T, VW, ONE>(acc, a, H, hh, xc, C, perm, edgeJ, b, e, lane, active);
    if (own) {
      if (active && r >= 0) *reinterpret_cast<Vec<T, VW>*>(dvalue + r * C + c0) = acc;
      continue;
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && active) {
#pragma unroll 1
      for (int w = 1; w < kGatWaves; w++) {
        const Vec<T, VW> q = part[w][lane];
#pragma unroll
        for (int j = 0; j < VW; j++) acc.v[j] += q.v[j];
      }
      *reinterpret_cast<Vec<T, VW>*>(dvalue + r * C + c0) = acc;
    }
    __syncthreads();
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
      const Vec<T, VW> g = active ? gcn_load<T, VW>(dout + j * C + c0) : gcn_zero<T, VW>();
      const Vec<T, VW> o = active ? gcn_load<T, VW>(out + j * C + c0) : gcn_zero<T, VW>();
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
            v[u] = active ? gcn_load<T, VW>(vc + su * C) : gcn_zero<T, VW>();
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

// grid: (ceil(N / kGatWaves), 1, kGatWaves + 1), block: kGatWaves * 64.  A wave per destination; the edges of a long row are shared out among the workgroup's
// waves (nothing is summed across edges, so nothing is merged).
template <class T, int VW>
__global__ __launch_bounds__(kGatWaves * 64) __attribute__((amdgpu_num_sgpr(96))) void gat_backward_score_kernel(T* __restrict__ dscore, T* __restrict__ aout, const T* __restrict__ dout,
                                                                             const T* __restrict__ out, const T* __restrict__ score,
                                                                             const T* __restrict__ value,
                                                                             const int64_t* __restrict__ edgeI, const int64_t* __restrict__ rowptr,
                                                                             const int64_t* __restrict__ perm, int64_t N, int64_t H, int V, int lph) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t row0 = (int64_t)blockIdx.x * kGatWaves;
  const int nrows = (int)(N - row0 < kGatWaves ? N - row0 : kGatWaves);
  for (int k = (int)blockIdx.z - 1; k < (int)blockIdx.z && k < nrows; k++) {   // one turn: a grid slice per k          // k = -1: every wave its own short row; k >= 0: row row0 + k if it is long, by all waves
    const bool own = k < 0;
    const int64_t r = own ? (wave < nrows ? row0 + wave : -1) : row0 + k;
    if (r < 0) continue;
    const int64_t rb = rowptr[r], re = rowptr[r + 1];
    if (own == (re - rb > kGatLongRow)) continue;
    int64_t b = rb, e = re;
    if (!own) {
      const int64_t chunk = (re - rb + kGatWaves - 1) / kGatWaves;
      b = rb + wave * chunk < re ? rb + wave * chunk : re;
      e = b + chunk < re ? b + chunk : re;
    }
    gat_score_edges<T, VW>(dscore, aout, dout, out, score, value, edgeI, perm, r, rb, re, b, e, H, V, lph, lane);
  }
}

// ---- message passing (lamp-core/src/main/scala/lamp/nn/graph/MPNN.scala) ---------------------------------------------------------------------
// The two data movements of an MPNN layer.  The message cat(edgeFeatures, x[edgeI], x[edgeJ]) and MPNN.aggregate's backward are per
// edge: a row has no sum, so these kernels run a thread per packet over a flat index of rows x packets (no idle lane at any width,
// neighbouring lanes on neighbouring packets).  The message's gradient with respect to x and MPNN.aggregate are
// sums per node over the groupings of lamp_graph_edge_csr: gat_backward_value_kernel's shape (a wave per node, lanes across the columns
// in packets, columns tiled in grid.y, edge ids read once per 64 edges and passed round with v_readlane, kMpnnUnroll rows in flight, a
// node of more than kMpnnLongRow edges split over the workgroup's waves in a grid slice of its own and merged through LDS by wave 0 in
// wave order).  No atomics, every element written once, nothing synchronises with the host.
constexpr int kMpnnWaves = 16;      // waves (= nodes) per workgroup of the summing kernels
constexpr int kMpnnLongRow = 256;   // a node with more edges (both groupings together) is split across the workgroup's waves
constexpr int kMpnnUnroll = 4;      // edge rows in flight per wave
constexpr int kMpnnEdgeBlock = 256; // threads per workgroup of the per-edge kernels

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
    *reinterpret_cast<Vec<T, VE>*>(o + c) = gcn_load<T, VE>(edge + t.row * lde + c);
  } else {
    const bool second = t.slot - se >= sx;
    const int c = (t.slot - se - (second ? sx : 0)) * VX;
    const int64_t node = second ? edgeJ[t.row] : edgeI[t.row];
    *reinterpret_cast<Vec<T, VX>*>(o + Fe + (second ? D : 0) + c) = gcn_load<T, VX>(x + node * ldx + c);
  }
}

// dst[e, 0:C] = src[e, 0:C] of rows with the pitches ldd and lds (dedge = dmsg[:, 0:Fe])
template <class T, int V>
__global__ __launch_bounds__(kMpnnEdgeBlock) void mpnn_columns_kernel(T* __restrict__ dst, int64_t ldd, const T* __restrict__ src, int64_t lds, int64_t E, int C,
                                                                     uint32_t slots) {
  const MpnnSlot t = mpnn_slot(slots);
  const int c = t.slot * V;
  if (t.row >= E || c >= C) return;
  *reinterpret_cast<Vec<T, V>*>(dst + t.row * ldd + c) = gcn_load<T, V>(src + t.row * lds + c);
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
  Vec<T, V> g = gcn_load<T, V>(dout + j * M + c);
  if (aggregateJ) {
    const Vec<T, V> h = gcn_load<T, V>(dout + i * M + c);
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
// it.  Lanes with `active` false hold no column: they take part in the index reads and load no row.  b and e are wave-uniform.
template <class T, int V, bool FI, bool FJ>
__device__ __forceinline__ void mpnn_gather(Vec<T, V>& acc, const T* __restrict__ rc, int64_t ld, const int64_t* __restrict__ perm,
                                            const int64_t* __restrict__ edgeI, const int64_t* __restrict__ edgeJ, const T* __restrict__ fI,
                                            const T* __restrict__ fJ, int64_t b, int64_t e, int lane, bool active) {
#pragma clang fp contract(off)
  for (int64_t p = b; p < e; p += 64) {
    const int n = (int)(e - p < 64 ? e - p : 64);
    int64_t ed = 0;
    T fi = T(0), fj = T(0);
    if (lane < n) {
      ed = perm[p + lane];
      if (FI) fi = fI[edgeI[ed]];
      if (FJ) fj = fJ[edgeJ[ed]];
    }
    int k = 0;
    for (; k + kMpnnUnroll <= n; k += kMpnnUnroll) {
      Vec<T, V> v[kMpnnUnroll];
      T a[kMpnnUnroll], c[kMpnnUnroll];
#pragma unroll
      for (int u = 0; u < kMpnnUnroll; u++) {
        const int64_t eu = lane_bcast(ed, k + u);
        if (FI) a[u] = lane_bcast(fi, k + u);
        if (FJ) c[u] = lane_bcast(fj, k + u);
        v[u] = active ? gcn_load<T, V>(rc + eu * ld) : gcn_zero<T, V>();
      }
#pragma unroll
      for (int u = 0; u < kMpnnUnroll; u++)
#pragma unroll
        for (int j = 0; j < V; j++) {
          T t = v[u].v[j];
          if (FI) t = t * a[u];
          if (FJ) t = t * c[u];
          acc.v[j] = acc.v[j] + t;
        }
    }
    for (; k < n; k++) {
      const int64_t eu = lane_bcast(ed, k);
      const T a = FI ? lane_bcast(fi, k) : T(0), c = FJ ? lane_bcast(fj, k) : T(0);
      const Vec<T, V> v = active ? gcn_load<T, V>(rc + eu * ld) : gcn_zero<T, V>();
#pragma unroll
      for (int j = 0; j < V; j++) {
        T t = v.v[j];
        if (FI) t = t * a;
        if (FJ) t = t * c;
        acc.v[j] = acc.v[j] + t;
      }
    }
  }
}

// out[r, 0:C] from the rows src[ed, off .. off + C) of the edges of node r: the sum over those of grouping 1 (columns off1) and, where
// rowptr2 is not null, the sum over those of grouping 2 (columns off2), each in its grouping's order, the two added last - as the chains
// add them (MPNN.aggregate: aggregateI + aggregateJ over incoming and outgoing; the message's gradient with respect to x: the two
// gathers' gradients, outgoing at Fe and incoming at Fe + D).  A node whose two groups together hold more than kMpnnLongRow edges is
// split: the waves take contiguous shares of the concatenated sequence, and either sum's partial sums are added in wave order.
// grid: (ceil(N / kMpnnWaves), ceil(C / (64 * V)), kMpnnWaves + 1), block: kMpnnWaves * 64.
template <class T, int V, bool FI, bool FJ>
__global__ __launch_bounds__(kMpnnWaves * 64) void mpnn_node_sum_kernel(T* __restrict__ out, const T* __restrict__ src, int64_t ld, int64_t off1, int64_t off2,
                                                                        const int64_t* __restrict__ rowptr1, const int64_t* __restrict__ perm1,
                                                                        const int64_t* __restrict__ rowptr2, const int64_t* __restrict__ perm2,
                                                                        const int64_t* __restrict__ edgeI, const int64_t* __restrict__ edgeJ,
                                                                        const T* __restrict__ fI, const T* __restrict__ fJ, int64_t N, int64_t C) {
  __shared__ Vec<T, V> part[2][kMpnnWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t c0 = ((int64_t)blockIdx.y * 64 + lane) * V;
  const bool active = c0 < C;
  const int64_t row0 = (int64_t)blockIdx.x * kMpnnWaves;
  const int nrows = (int)(N - row0 < kMpnnWaves ? N - row0 : kMpnnWaves);

  for (int k = (int)blockIdx.z - 1; k < (int)blockIdx.z && k < nrows; k++) {   // one turn: a grid slice per k, as in gat_forward_kernel
    const bool own = k < 0;
    const int64_t r = own ? (wave < nrows ? row0 + wave : -1) : row0 + k;
    int64_t b1 = 0, n1 = 0, b2 = 0, n2 = 0;
    if (r >= 0) {
      b1 = rowptr1[r]; n1 = rowptr1[r + 1] - b1;
      if (rowptr2) { b2 = rowptr2[r]; n2 = rowptr2[r + 1] - b2; }
    }
    const int64_t total = n1 + n2;
    if (own == (total > kMpnnLongRow)) continue;
    int64_t lo = 0, hi = total;                 // this wave's share of the n1 + n2 edges
    if (!own) {
      const int64_t chunk = (total + kMpnnWaves - 1) / kMpnnWaves;
      lo = wave * chunk < total ? wave * chunk : total;
      hi = lo + chunk < total ? lo + chunk : total;
    }
    Vec<T, V> acc = gcn_zero<T, V>(), acc2 = gcn_zero<T, V>();
    if (lo < n1) mpnn_gather<T, V, FI, FJ>(acc, src + off1 + c0, ld, perm1, edgeI, edgeJ, fI, fJ, b1 + lo, b1 + (hi < n1 ? hi : n1), lane, active);
    if (hi > n1) mpnn_gather<T, V, FI, FJ>(acc2, src + off2 + c0, ld, perm2, edgeI, edgeJ, fI, fJ, b2 + (lo > n1 ? lo - n1 : 0), b2 + hi - n1, lane, active);
    if (own) {
      if (active && r >= 0) {
        if (rowptr2) {
#pragma unroll
          for (int j = 0; j < V; j++) acc.v[j] += acc2.v[j];
        }
        *reinterpret_cast<Vec<T, V>*>(out + r * C + c0) = acc;
      }
      continue;
    }
    part[0][wave][lane] = acc;
    part[1][wave][lane] = acc2;
    __syncthreads();
    if (wave == 0 && active) {
#pragma unroll 1
      for (int w = 1; w < kMpnnWaves; w++) {
        const Vec<T, V> q = part[0][w][lane];
#pragma unroll
        for (int j = 0; j < V; j++) acc.v[j] += q.v[j];
        const Vec<T, V> q2 = part[1][w][lane];
#pragma unroll
        for (int j = 0; j < V; j++) acc2.v[j] += q2.v[j];
      }
      if (rowptr2) {
#pragma unroll
        for (int j = 0; j < V; j++) acc.v[j] += acc2.v[j];
      }
      *reinterpret_cast<Vec<T, V>*>(out + r * C + c0) = acc;
    }
    __syncthreads();
  }
}

template <class T, int V>
void gcn_launch(Tensor* out, const Tensor* x, int64_t ldx, const Tensor* rowptr, const Tensor* col, const Tensor* dinv, int64_t N, int64_t D,
                hipStream_t st) {
  const int64_t tiles = (D + 64 * V - 1) / (64 * V), groups = (N + kGcnWaves - 1) / kGcnWaves;
  LAMP_CHECK(tiles <= 65535 && groups <= INT32_MAX, "x " << x->describe() << " is too large");
  hipLaunchKernelGGL((gcn_aggregate_kernel<T, V>), dim3((unsigned)groups, (unsigned)tiles), dim3(kGcnWaves * 64), 0, st, out->ptr<T>(), D, x->ptr<T>(), ldx,
                     rowptr->ptr<int64_t>(), col->ptr<int64_t>(), dinv->ptr<T>(), N, D);
  LAMP_LAUNCH_CHECK();
}
// the widest packet (in elements, at most 16 bytes) that D, x's row pitch and both base addresses allow
template <class T> int gcn_packet(const Tensor* out, const Tensor* x, int64_t ldx, int64_t D) {
  for (int v = 16 / (int)sizeof(T); v > 1; v >>= 1)
    if (D % v == 0 && ldx % v == 0 && ((uintptr_t)x->raw() % (v * sizeof(T))) == 0 && ((uintptr_t)out->raw() % (v * sizeof(T))) == 0) return v;
  return 1;
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

// the widest packet (in elements, at most 16 bytes) that C and the base addresses of contiguous [., C] tensors allow
template <class T> int gat_packet(int64_t C, std::initializer_list<const Tensor*> ts) {
  for (int v = 16 / (int)sizeof(T); v > 1; v >>= 1) {
    bool ok = C % v == 0;
    for (const Tensor* t : ts) ok = ok && ((uintptr_t)t->raw() % (v * sizeof(T))) == 0;
    if (ok) return v;
  }
  return 1;
}
struct GatGrid { dim3 grid, block; };
GatGrid gat_grid(int64_t N, int64_t C, int vw) {
  const int64_t tiles = (C + 64 * vw - 1) / (64 * vw), groups = (N + kGatWaves - 1) / kGatWaves;
  LAMP_CHECK(tiles <= 65535 && groups <= INT32_MAX, "a graph of " << N << " nodes with " << C << " columns is too large");
  return {dim3((unsigned)groups, (unsigned)tiles, kGatWaves + 1), dim3(kGatWaves * 64)};
}
// the packet width of gat_forward_kernel / gat_backward_value_kernel: the widest that C and the addresses allow, but four only where it
// stays inside a head (a softmax state per element costs an exp each)
template <class T> int gat_gather_packet(int64_t C, int V, std::initializer_list<const Tensor*> ts) {
  int vw = gat_packet<T>(C, ts);
  while (vw > 2 && V % vw) vw >>= 1;
  return vw;
}
// F<T, VW, ONE>::launch(args...) for that width: ONE where no packet straddles a head boundary
template <template <class, int, bool> class F, class T, class... A> void gat_dispatch(int vw, int V, A... a) {
  if constexpr (sizeof(T) == 4) {
    if (vw == 4) { F<T, 4, true>::launch(a...); return; }
  }
  if (vw == 2) { if (V % 2 == 0) F<T, 2, true>::launch(a...); else F<T, 2, false>::launch(a...); return; }
  F<T, 1, true>::launch(a...);
}
template <class T, int VW, bool ONE> struct GatForward {
  static void launch(GatGrid g, hipStream_t st, Tensor* out, Tensor* lse, const Tensor* score, const Tensor* value, const Tensor* edgeI, const Tensor* rowptr,
                     const Tensor* perm, int64_t N, int64_t H, int V) {
    hipLaunchKernelGGL((gat_forward_kernel<T, VW, ONE>), g.grid, g.block, 0, st, out->ptr<T>(), lse->ptr<T>(), score->ptr<T>(), value->ptr<T>(),
                       edgeI->ptr<int64_t>(), rowptr->ptr<int64_t>(), perm->ptr<int64_t>(), N, H, V);
  }
};
template <class T, int VW, bool ONE> struct GatBackwardValue {
  static void launch(GatGrid g, hipStream_t st, Tensor* dvalue, const Tensor* a, const Tensor* dout, const Tensor* edgeJ, const Tensor* rowptr, const Tensor* perm,
                     int64_t N, int64_t H, int V) {
    hipLaunchKernelGGL((gat_backward_value_kernel<T, VW, ONE>), g.grid, g.block, 0, st, dvalue->ptr<T>(), a->ptr<T>(), dout->ptr<T>(), edgeJ->ptr<int64_t>(),
                       rowptr->ptr<int64_t>(), perm->ptr<int64_t>(), N, H, V);
  }
};
template <class T, int VW>
void gat_backward_score_launch(hipStream_t st, Tensor* dscore, Tensor* a, const Tensor* dout, const Tensor* out, const Tensor* score, const Tensor* value,
                               const Tensor* edgeI, const Tensor* rowptr, const Tensor* perm, int64_t N, int64_t H, int V, int lph) {
  const int64_t groups = (N + kGatWaves - 1) / kGatWaves;
  LAMP_CHECK(groups <= INT32_MAX, "a graph of " << N << " nodes is too large");
  hipLaunchKernelGGL((gat_backward_score_kernel<T, VW>), dim3((unsigned)groups, 1, kGatWaves + 1), dim3(kGatWaves * 64), 0, st, dscore->ptr<T>(), a->ptr<T>(), dout->ptr<T>(),
                     out->ptr<T>(), score->ptr<T>(), value->ptr<T>(), edgeI->ptr<int64_t>(), rowptr->ptr<int64_t>(), perm->ptr<int64_t>(), N, H, V, lph);
}
// the packet form of gat_backward_score_kernel: V = lph * vw with lph a power of two up to 64; 0 where V has no such split
int gat_lanes_per_head(int V, int vw) {
  if (V % vw) return 0;
  const int lph = V / vw;
  return lph <= 64 && (lph & (lph - 1)) == 0 ? lph : 0;
}

// score [E, H], value [N, H, V] of one floating type, the index vectors int64 [E], the grouping's rowptr [N + 1]
struct GatShape { int64_t E, H, N, V; };
GatShape gat_check(const Tensor* score, const Tensor* value, std::initializer_list<std::pair<const Tensor*, const char*>> edgeVectors,
                   std::initializer_list<std::pair<const Tensor*, const char*>> rowptrs) {
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
  for (auto& v : edgeVectors) {
    check_i64_vector(v.first, score, v.second);
    LAMP_CHECK(v.first->numel() == g.E, v.second << " " << v.first->describe() << " does not have score's " << g.E << " edges: edgeI and edgeJ differ in length?");
  }
  for (auto& v : rowptrs) {
    check_i64_vector(v.first, score, v.second);
    LAMP_CHECK(v.first->numel() == g.N + 1, v.second << " " << v.first->describe() << " does not belong to a graph of " << g.N << " nodes");
  }
  return g;
}

// the widest packet (in elements, at most 16 bytes) that divides every length (widths, column offsets, row pitches) and at which every
// address is aligned
template <class T> int mpnn_packet(std::initializer_list<int64_t> lengths, std::initializer_list<const Tensor*> ts) {
  for (int v = 16 / (int)sizeof(T); v > 1; v >>= 1) {
    bool ok = true;
    for (int64_t l : lengths) ok = ok && l % v == 0;
    for (const Tensor* t : ts) ok = ok && ((uintptr_t)t->raw() % (v * sizeof(T))) == 0;
    if (ok) return v;
  }
  return 1;
}
// the grid of a per-edge kernel: rows of `slots` packets (slots >= 1), a thread per packet; see mpnn_slot
struct MpnnEdgeGrid { dim3 grid; uint32_t slots; };
MpnnEdgeGrid mpnn_edge_grid(int64_t rows, int64_t slots) {
  LAMP_CHECK(slots >= 1 && rows * slots <= ((int64_t)1 << 31), rows << " rows of " << slots << " packets are too many");
  return {dim3((unsigned)((rows * slots + kMpnnEdgeBlock - 1) / kMpnnEdgeBlock)), (uint32_t)slots};
}
// a [rows, cols] tensor whose rows are read in place (unit column stride, rows that do not overlap) or a dense copy; -> its row pitch
Tensor* mpnn_rows(const Tensor* t, int64_t* ld) {
  const int64_t rows = t->sizes[0], cols = t->sizes[1];
  const bool in_place = (cols == 1 || t->strides[1] == 1) && (rows == 1 || t->strides[0] >= cols);
  Tensor* r = in_place ? retain(t) : contiguous(t);
  *ld = rows == 1 ? cols : r->strides[0];
  return r;
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

template <class T, int VE, int VX>
void mpnn_message_launch(MpnnEdgeGrid g, hipStream_t st, Tensor* msg, const Tensor* edge, int64_t lde, const Tensor* x, int64_t ldx, const Tensor* edgeI,
                         const Tensor* edgeJ, int64_t E, int Fe, int D) {
  hipLaunchKernelGGL((mpnn_message_kernel<T, VE, VX>), g.grid, dim3(kMpnnEdgeBlock), 0, st, msg->ptr<T>(), edge->ptr<T>(), lde, x->ptr<T>(), ldx,
                     edgeI->ptr<int64_t>(), edgeJ->ptr<int64_t>(), E, Fe, D, g.slots);
}
template <class T, int VE>
void mpnn_message_launch_x(int vx, MpnnEdgeGrid g, hipStream_t st, Tensor* msg, const Tensor* edge, int64_t lde, const Tensor* x, int64_t ldx,
                           const Tensor* edgeI, const Tensor* edgeJ, int64_t E, int Fe, int D) {
  if constexpr (sizeof(T) == 4) {
    if (vx == 4) { mpnn_message_launch<T, VE, 4>(g, st, msg, edge, lde, x, ldx, edgeI, edgeJ, E, Fe, D); return; }
  }
  if (vx == 2) mpnn_message_launch<T, VE, 2>(g, st, msg, edge, lde, x, ldx, edgeI, edgeJ, E, Fe, D);
  else mpnn_message_launch<T, VE, 1>(g, st, msg, edge, lde, x, ldx, edgeI, edgeJ, E, Fe, D);
}
template <class T>
void mpnn_message_dispatch(hipStream_t st, Tensor* msg, const Tensor* edge, int64_t lde, const Tensor* x, int64_t ldx, const Tensor* edgeI, const Tensor* edgeJ,
                           int64_t E, int Fe, int D) {
  // per segment: the edge segment starts every row (pitch Fe + 2 D), the node segments start at Fe and Fe + D
  const int64_t W = (int64_t)Fe + 2 * (int64_t)D;
  const int ve = mpnn_packet<T>({Fe, W, lde}, {msg, edge}), vx = mpnn_packet<T>({D, Fe, W, ldx}, {msg, x});
  const MpnnEdgeGrid g = mpnn_edge_grid(E, Fe / ve + 2 * (int64_t)(D / vx));
  if constexpr (sizeof(T) == 4) {
    if (ve == 4) { mpnn_message_launch_x<T, 4>(vx, g, st, msg, edge, lde, x, ldx, edgeI, edgeJ, E, Fe, D); return; }
  }
  if (ve == 2) mpnn_message_launch_x<T, 2>(vx, g, st, msg, edge, lde, x, ldx, edgeI, edgeJ, E, Fe, D);
  else mpnn_message_launch_x<T, 1>(vx, g, st, msg, edge, lde, x, ldx, edgeI, edgeJ, E, Fe, D);
}

struct MpnnSum {
  Tensor* out; const Tensor* src; int64_t ld, off1, off2;
  const Tensor *rowptr1, *perm1, *rowptr2, *perm2, *edgeI, *edgeJ, *fI, *fJ;
  int64_t N, C;
};
template <class T, int V, bool FI, bool FJ> void mpnn_sum_launch(const MpnnSum& a, hipStream_t st) {
  const int64_t tiles = (a.C + 64 * V - 1) / (64 * V), groups = (a.N + kMpnnWaves - 1) / kMpnnWaves;
  LAMP_CHECK(tiles <= 65535 && groups <= INT32_MAX, "a graph of " << a.N << " nodes with " << a.C << " columns is too large");
  auto ip = [](const Tensor* t) { return t ? t->ptr<int64_t>() : nullptr; };
  hipLaunchKernelGGL((mpnn_node_sum_kernel<T, V, FI, FJ>), dim3((unsigned)groups, (unsigned)tiles, kMpnnWaves + 1), dim3(kMpnnWaves * 64), 0, st,
                     a.out->ptr<T>(), a.src->ptr<T>(), a.ld, a.off1, a.off2, ip(a.rowptr1), ip(a.perm1), ip(a.rowptr2), ip(a.perm2), ip(a.edgeI), ip(a.edgeJ),
                     a.fI ? a.fI->ptr<T>() : nullptr, a.fJ ? a.fJ->ptr<T>() : nullptr, a.N, a.C);
}
template <class T, bool FI, bool FJ> void mpnn_sum_packet(int v, const MpnnSum& a, hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (v == 4) { mpnn_sum_launch<T, 4, FI, FJ>(a, st); return; }
  }
  if (v == 2) mpnn_sum_launch<T, 2, FI, FJ>(a, st);
  else mpnn_sum_launch<T, 1, FI, FJ>(a, st);
}
// MPNN.aggregate: a factor that is null is a kernel without that multiplication
template <class T> void mpnn_aggregate_dispatch(int v, const MpnnSum& a, hipStream_t st) {
  if (a.fI && a.fJ) mpnn_sum_packet<T, true, true>(v, a, st);
  else if (a.fI) mpnn_sum_packet<T, true, false>(v, a, st);
  else if (a.fJ) mpnn_sum_packet<T, false, true>(v, a, st);
  else mpnn_sum_packet<T, false, false>(v, a, st);
}
template <class T>
void mpnn_columns_dispatch(hipStream_t st, Tensor* dst, int64_t ldd, const Tensor* src, int64_t lds, int64_t E, int C) {
  const int v = mpnn_packet<T>({C, ldd, lds}, {dst, src});
  const MpnnEdgeGrid g = mpnn_edge_grid(E, C / v);
  if constexpr (sizeof(T) == 4) {
    if (v == 4) { hipLaunchKernelGGL((mpnn_columns_kernel<T, 4>), g.grid, dim3(kMpnnEdgeBlock), 0, st, dst->ptr<T>(), ldd, src->ptr<T>(), lds, E, C, g.slots); return; }
  }
  if (v == 2) hipLaunchKernelGGL((mpnn_columns_kernel<T, 2>), g.grid, dim3(kMpnnEdgeBlock), 0, st, dst->ptr<T>(), ldd, src->ptr<T>(), lds, E, C, g.slots);
  else hipLaunchKernelGGL((mpnn_columns_kernel<T, 1>), g.grid, dim3(kMpnnEdgeBlock), 0, st, dst->ptr<T>(), ldd, src->ptr<T>(), lds, E, C, g.slots);
}
template <class T>
void mpnn_aggregate_backward_dispatch(hipStream_t st, Tensor* dmsg, const Tensor* dout, const Tensor* edgeI, const Tensor* edgeJ, const Tensor* fI, const Tensor* fJ,
                                      int aggregateJ, int64_t E, int M) {
  const int v = mpnn_packet<T>({M}, {dmsg, dout});
  const MpnnEdgeGrid g = mpnn_edge_grid(E, M / v);
  const T *pi = fI ? fI->ptr<T>() : nullptr, *pj = fJ ? fJ->ptr<T>() : nullptr;
  if constexpr (sizeof(T) == 4) {
    if (v == 4) { hipLaunchKernelGGL((mpnn_aggregate_backward_kernel<T, 4>), g.grid, dim3(kMpnnEdgeBlock), 0, st, dmsg->ptr<T>(), dout->ptr<T>(), edgeI->ptr<int64_t>(), edgeJ->ptr<int64_t>(), pi, pj, aggregateJ, E, M, g.slots); return; }
  }
  if (v == 2) hipLaunchKernelGGL((mpnn_aggregate_backward_kernel<T, 2>), g.grid, dim3(kMpnnEdgeBlock), 0, st, dmsg->ptr<T>(), dout->ptr<T>(), edgeI->ptr<int64_t>(), edgeJ->ptr<int64_t>(), pi, pj, aggregateJ, E, M, g.slots);
  else hipLaunchKernelGGL((mpnn_aggregate_backward_kernel<T, 1>), g.grid, dim3(kMpnnEdgeBlock), 0, st, dmsg->ptr<T>(), dout->ptr<T>(), edgeI->ptr<int64_t>(), edgeJ->ptr<int64_t>(), pi, pj, aggregateJ, E, M, g.slots);
}

}  // namespace
}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_gcn_long_row(int64_t* out) {
  LAMP_API_BEGIN
  *out = kGcnLongRow;
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
  int64_t ns[1] = {N}, n1[1] = {N + 1}, e2[1] = {2 * E};
  Hold rp(new_tensor(n1, 1, kI64, dev)), dv(new_tensor(ns, 1, dtype, dev)), cl, counts;
  if (E) {
    // the range of both index vectors, before anything uses one of them as an index
    check_index_range("gcn_index_range", ei.get(), ej.get(), N, st);
    // the 2E directed entries (row, col) = (i, j) then (j, i), stably sorted by row
    lamp_tensor *ks[2] = {ei.get(), ej.get()}, *vs[2] = {ej.get(), ei.get()}, *t = nullptr;
    LAMP_CHECK(lamp_cat(&t, ks, 2, 0) == 0, lamp_last_error());
    Hold keys(t);
    LAMP_CHECK(lamp_cat(&t, vs, 2, 0) == 0, lamp_last_error());
    Hold vals(t);
    LAMP_CHECK(lamp_argsort(&t, keys.get(), 1, 0, 0) == 0, lamp_last_error());
    Hold perm(t);
    LAMP_CHECK(lamp_index_select(&t, vals.get(), 0, perm.get()) == 0, lamp_last_error());
    cl = Hold(t);
    LAMP_CHECK(lamp_bincount(&t, keys.get(), nullptr, N) == 0, lamp_last_error());
    counts = Hold(t);
    LAMP_CHECK(counts->numel() == N && cl->numel() == 2 * E, "internal: counts " << counts->describe() << ", col " << cl->describe());
  } else {
    cl = Hold(new_tensor(e2, 1, kI64, dev));
  }
  {
    KernelTimer kt("gcn_rowptr_dinv", 0, (double)N * (16 + dtype_size(dtype)), st);
    const int64_t* cp = counts.get() ? counts->ptr<int64_t>() : nullptr;
    if (dtype == kF32) hipLaunchKernelGGL((gcn_rowptr_dinv_kernel<float>), dim3(1), dim3(1024), 0, st, cp, rp->ptr<int64_t>(), dv->ptr<float>(), N);
    else hipLaunchKernelGGL((gcn_rowptr_dinv_kernel<double>), dim3(1), dim3(1024), 0, st, cp, rp->ptr<int64_t>(), dv->ptr<double>(), N);
    LAMP_LAUNCH_CHECK();
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
  check_i64_vector(rowptr, x, "rowptr");
  check_i64_vector(col, x, "col");
  check_device_tensor(dinv, "dinv");
  check_same_device(dinv, x);
  LAMP_CHECK(rowptr->numel() == N + 1, "rowptr " << rowptr->describe() << " does not belong to a graph of " << N << " nodes");
  LAMP_CHECK(dinv->ndim == 1 && dinv->numel() == N && dinv->dtype == x->dtype, "dinv " << dinv->describe() << " must be [" << N << "] of x's type " << x->describe());
  // unit column stride and rows that do not overlap are read in place, whatever the row pitch; anything else (a broadcast gradient) is copied
  const bool in_place = (D == 1 || x->strides[1] == 1) && (N == 1 || x->strides[0] >= D);
  Hold xc(in_place ? retain(x) : contiguous(x)), rc(contiguous(rowptr)), cc(contiguous(col)), dc(contiguous(dinv));
  const int64_t ldx = N == 1 ? D : xc->strides[0];
  int64_t os[2] = {N, D};
  Hold o(new_tensor(os, 2, x->dtype, x->device()));
  if (N * D) {
    hipStream_t st = current_stream(x->device());
    const double nnz = (double)cc->numel();
    KernelTimer kt("gcn_aggregate", 2.0 * (nnz + 2.0 * N) * D, ((nnz + N) * D + (double)N * D) * dtype_size(x->dtype) + nnz * (8 + dtype_size(x->dtype)) + N * 8.0, st);
    if (x->dtype == kF32) {
      switch (gcn_packet<float>(o.get(), xc.get(), ldx, D)) {
        case 4: gcn_launch<float, 4>(o.get(), xc.get(), ldx, rc.get(), cc.get(), dc.get(), N, D, st); break;
        case 2: gcn_launch<float, 2>(o.get(), xc.get(), ldx, rc.get(), cc.get(), dc.get(), N, D, st); break;
        default: gcn_launch<float, 1>(o.get(), xc.get(), ldx, rc.get(), cc.get(), dc.get(), N, D, st);
      }
    } else {
      if (gcn_packet<double>(o.get(), xc.get(), ldx, D) == 2) gcn_launch<double, 2>(o.get(), xc.get(), ldx, rc.get(), cc.get(), dc.get(), N, D, st);
      else gcn_launch<double, 1>(o.get(), xc.get(), ldx, rc.get(), cc.get(), dc.get(), N, D, st);
    }
  }
  *out = o.take();
  LAMP_API_END
}

int lamp_gat_long_row(int64_t* out) {
  LAMP_API_BEGIN
  *out = kGatLongRow;
  LAMP_API_END
}

int lamp_graph_edge_csr(lamp_tensor** rowptr, lamp_tensor** perm, const lamp_tensor* index, int64_t numNodes) {
  LAMP_API_BEGIN
  check_device_tensor(index, "index");
  check_i64_vector(index, index, "index");
  LAMP_CHECK(numNodes >= 0, "numNodes = " << numNodes);
  const int dev = index->device();
  const int64_t N = numNodes, E = index->numel();
  LAMP_CHECK(E < ((int64_t)1 << 31), "too many edges: " << E);
  hipStream_t st = current_stream(dev);
  Hold ix(contiguous(index));
  int64_t n1[1] = {N + 1}, es[1] = {E};
  Hold rp(new_tensor(n1, 1, kI64, dev)), pm, counts;
  if (E) {
    check_index_range("graph_index_range", ix.get(), nullptr, N, st);
    lamp_tensor* t = nullptr;
    LAMP_CHECK(lamp_argsort(&t, ix.get(), 1, 0, 0) == 0, lamp_last_error());
    pm = Hold(t);
    LAMP_CHECK(lamp_bincount(&t, ix.get(), nullptr, N) == 0, lamp_last_error());
    counts = Hold(t);
    LAMP_CHECK(counts->numel() == N && pm->numel() == E && pm->dtype == kI64, "internal: counts " << counts->describe() << ", perm " << pm->describe());
  } else {
    pm = Hold(new_tensor(es, 1, kI64, dev));
  }
  {
    KernelTimer kt("graph_edge_rowptr", 0, (double)N * 16, st);
    hipLaunchKernelGGL((gcn_rowptr_dinv_kernel<float>), dim3(1), dim3(1024), 0, st, counts.get() ? counts->ptr<int64_t>() : nullptr, rp->ptr<int64_t>(),
                       (float*)nullptr, N);
    LAMP_LAUNCH_CHECK();
  }
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
    KernelTimer kt("gat_forward", 2.0 * E * C + 4.0 * E * g.H + N * C, (E * C + N * C + E * g.H + N * g.H) * sz + E * 16 + N * 8, st);
    if (score->dtype == kF32) {
      const int vw = gat_gather_packet<float>(C, (int)g.V, {o.get(), vc.get()});
      gat_dispatch<GatForward, float>(vw, (int)g.V, gat_grid(g.N, C, vw), st, o.get(), l.get(), sc.get(), vc.get(), ei.get(), rp.get(), pm.get(), g.N, g.H, (int)g.V);
    } else {
      const int vw = gat_gather_packet<double>(C, (int)g.V, {o.get(), vc.get()});
      gat_dispatch<GatForward, double>(vw, (int)g.V, gat_grid(g.N, C, vw), st, o.get(), l.get(), sc.get(), vc.get(), ei.get(), rp.get(), pm.get(), g.N, g.H, (int)g.V);
    }
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
      if (dt == kF32) {
        int vw = gat_packet<float>(C, {go.get(), oc.get(), vc.get()});
        while (vw > 1 && !gat_lanes_per_head(V, vw)) vw >>= 1;
        const int lph = gat_lanes_per_head(V, vw);
        if (lph && vw == 4) gat_backward_score_launch<float, 4>(st, ds.get(), a.get(), go.get(), oc.get(), sc.get(), vc.get(), ei.get(), irp.get(), ipm.get(), g.N, g.H, V, lph);
        else if (lph && vw == 2) gat_backward_score_launch<float, 2>(st, ds.get(), a.get(), go.get(), oc.get(), sc.get(), vc.get(), ei.get(), irp.get(), ipm.get(), g.N, g.H, V, lph);
        else gat_backward_score_launch<float, 1>(st, ds.get(), a.get(), go.get(), oc.get(), sc.get(), vc.get(), ei.get(), irp.get(), ipm.get(), g.N, g.H, V, lph);
      } else {
        int vw = gat_packet<double>(C, {go.get(), oc.get(), vc.get()});
        while (vw > 1 && !gat_lanes_per_head(V, vw)) vw >>= 1;
        const int lph = gat_lanes_per_head(V, vw);
        if (lph && vw == 2) gat_backward_score_launch<double, 2>(st, ds.get(), a.get(), go.get(), oc.get(), sc.get(), vc.get(), ei.get(), irp.get(), ipm.get(), g.N, g.H, V, lph);
        else gat_backward_score_launch<double, 1>(st, ds.get(), a.get(), go.get(), oc.get(), sc.get(), vc.get(), ei.get(), irp.get(), ipm.get(), g.N, g.H, V, lph);
      }
      LAMP_LAUNCH_CHECK();
    }
    {
      KernelTimer kt("gat_backward_value", 2.0 * E * C, (E * C + N * C + E * g.H) * sz + E * 16 + N * 8, st);
      if (dt == kF32) {
        const int vw = gat_gather_packet<float>(C, V, {dv.get(), go.get()});
        gat_dispatch<GatBackwardValue, float>(vw, V, gat_grid(g.N, C, vw), st, dv.get(), a.get(), go.get(), ej.get(), orp.get(), opm.get(), g.N, g.H, V);
      } else {
        const int vw = gat_gather_packet<double>(C, V, {dv.get(), go.get()});
        gat_dispatch<GatBackwardValue, double>(vw, V, gat_grid(g.N, C, vw), st, dv.get(), a.get(), go.get(), ej.get(), orp.get(), opm.get(), g.N, g.H, V);
      }
      LAMP_LAUNCH_CHECK();
    }
  }
  *dscore = ds.take(); *dvalue = dv.take();
  LAMP_API_END
}

int lamp_mpnn_long_row(int64_t* out) {
  LAMP_API_BEGIN
  *out = kMpnnLongRow;
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
  const int64_t E = edgeI->numel(), Fe = edgeFeatures->sizes[1], D = x->sizes[1];
  LAMP_CHECK(edgeJ->numel() == E, "edgeI " << edgeI->describe() << " and edgeJ " << edgeJ->describe() << " differ in length");
  LAMP_CHECK(edgeFeatures->sizes[0] == E, "edgeFeatures " << edgeFeatures->describe() << " does not have one row per edge (" << E << " edges)");
  LAMP_CHECK(E == 0 || x->sizes[0] > 0, "x " << x->describe() << " has no rows");
  LAMP_CHECK(Fe + 2 * D <= INT32_MAX / 2, "a message of " << Fe + 2 * D << " columns is too wide");
  int64_t lde = 0, ldx = 0;
  Hold ec(mpnn_rows(edgeFeatures, &lde)), xc(mpnn_rows(x, &ldx)), ei(contiguous(edgeI)), ej(contiguous(edgeJ));
  int64_t os[2] = {E, Fe + 2 * D};
  Hold o(new_tensor(os, 2, x->dtype, x->device()));
  if (E * (Fe + 2 * D)) {
    hipStream_t st = current_stream(x->device());
    KernelTimer kt("mpnn_message", 0, 2.0 * E * (Fe + 2 * D) * dtype_size(x->dtype) + E * 16.0, st);
    if (x->dtype == kF32) mpnn_message_dispatch<float>(st, o.get(), ec.get(), lde, xc.get(), ldx, ei.get(), ej.get(), E, (int)Fe, (int)D);
    else mpnn_message_dispatch<double>(st, o.get(), ec.get(), lde, xc.get(), ldx, ei.get(), ej.get(), E, (int)Fe, (int)D);
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
    for (auto& v : {std::make_pair(inRowptr, "inRowptr"), std::make_pair(outRowptr, "outRowptr")}) {
      check_i64_vector(v.first, dmsg, v.second);
      LAMP_CHECK(v.first->numel() == N + 1, v.second << " " << v.first->describe() << " does not belong to a graph of " << N << " nodes");
    }
    for (auto& v : {std::make_pair(inPerm, "inPerm"), std::make_pair(outPerm, "outPerm")}) {
      check_i64_vector(v.first, dmsg, v.second);
      LAMP_CHECK(v.first->numel() == E, v.second << " " << v.first->describe() << " does not have dmsg's " << E << " edges");
    }
    Hold irp(contiguous(inRowptr)), ipm(contiguous(inPerm)), orp(contiguous(outRowptr)), opm(contiguous(outPerm));
    int64_t xs[2] = {N, D};
    dx = Hold(new_tensor(xs, 2, dt, dev));
    if (N * D) {
      KernelTimer kt("mpnn_message_backward_x", 2.0 * E * D, (2.0 * E * D + (double)N * D) * sz + E * 16.0 + N * 16.0, st);
      const MpnnSum a{dx.get(), g.get(), W, Fe, Fe + D, orp.get(), opm.get(), irp.get(), ipm.get(), nullptr, nullptr, nullptr, nullptr, N, D};
      if (dt == kF32) mpnn_sum_packet<float, false, false>(mpnn_packet<float>({D, Fe, W}, {dx.get(), g.get()}), a, st);
      else mpnn_sum_packet<double, false, false>(mpnn_packet<double>({D, Fe, W}, {dx.get(), g.get()}), a, st);
      LAMP_LAUNCH_CHECK();
    }
  }
  if (dedge_or_null) {
    int64_t es[2] = {E, Fe};
    de = Hold(new_tensor(es, 2, dt, dev));
    if (E * Fe) {
      KernelTimer kt("mpnn_message_backward_edge", 0, 2.0 * E * Fe * sz, st);
      if (dt == kF32) mpnn_columns_dispatch<float>(st, de.get(), Fe, g.get(), W, E, (int)Fe);
      else mpnn_columns_dispatch<double>(st, de.get(), Fe, g.get(), W, E, (int)Fe);
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
  for (auto& v : {std::make_pair(edgeI, "edgeI"), std::make_pair(edgeJ, "edgeJ"), std::make_pair(inPerm, "inPerm"), std::make_pair(opm0 ? opm0 : inPerm, "outPerm")}) {
    check_i64_vector(v.first, message, v.second);
    LAMP_CHECK(v.first->numel() == E, v.second << " " << v.first->describe() << " does not have one entry per row of message " << message->describe());
  }
  if (orp0) {
    check_i64_vector(orp0, message, "outRowptr");
    LAMP_CHECK(orp0->numel() == N + 1, "outRowptr " << orp0->describe() << " does not belong to a graph of " << N << " nodes");
  }
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
    if (message->dtype == kF32) mpnn_aggregate_dispatch<float>(mpnn_packet<float>({M}, {o.get(), mc.get()}), a, st);
    else mpnn_aggregate_dispatch<double>(mpnn_packet<double>({M}, {o.get(), mc.get()}), a, st);
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
    if (dout->dtype == kF32) mpnn_aggregate_backward_dispatch<float>(st, o.get(), gc.get(), ei.get(), ej.get(), fi.get(), fj.get(), aggregateJ, E, (int)M);
    else mpnn_aggregate_backward_dispatch<double>(st, o.get(), gc.get(), ei.get(), ej.get(), fi.get(), fj.get(), aggregateJ, E, (int)M);
    LAMP_LAUNCH_CHECK();
  }
  *dmsg = o.take();
  LAMP_API_END
}

}  // extern "C"
