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

// per workgroup the smallest and the largest value of a[0, n) and b[0, n): out[2 * blockIdx.x] = min, out[2 * blockIdx.x + 1] = max
__global__ __launch_bounds__(256) void gcn_index_range_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t n,
                                                              int64_t* __restrict__ out) {
  __shared__ int64_t smn[4], smx[4];
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = a[i], w = b[i];
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

// rowptr = exclusive prefix sum of counts ([N + 1], rowptr[N] = total), dinv = (counts + 1)^-1/2.  counts == nullptr: all zero.
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
    dinv[i] = (T)(1.0 / sqrt((double)(c + 1)));
  }
  if (t == 1023) rowptr[N] = part[1023];
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
    const int nb = grid_for(E, 256, 2);
    int64_t ms[1] = {2 * (int64_t)nb};
    Hold mm(new_tensor(ms, 1, kI64, dev));
    {
      KernelTimer kt("gcn_index_range", 0, (double)E * 16, st);
      hipLaunchKernelGGL(gcn_index_range_kernel, dim3(nb), dim3(256), 0, st, ei->ptr<int64_t>(), ej->ptr<int64_t>(), E, mm->ptr<int64_t>());
      LAMP_LAUNCH_CHECK();
    }
    std::vector<int64_t> h(2 * (size_t)nb);
    HIP_CHECK(hipMemcpyAsync(h.data(), mm->ptr<int64_t>(), h.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    for (int i = 0; i < nb; i++) { mn = std::min(mn, h[2 * i]); mx = std::max(mx, h[2 * i + 1]); }
    LAMP_CHECK(mn >= 0 && mx < N, "edge endpoints must lie in [0, " << N << "), got " << mn << " .. " << mx);
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

}  // extern "C"
