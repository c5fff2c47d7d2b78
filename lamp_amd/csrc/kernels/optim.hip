// Fused multi-tensor optimiser kernels: AdamW, SGDW, RAdam, Yogi, global-norm gradient clipping and the
// flat gradient bucket used by data-parallel training.
//
// Replaces the per-tensor ATen call chains of lamp's optimisers with ONE launch over all
// parameter tensors (reference: lamp-core/src/main/scala/lamp/nn/AdamW.scala:101-176 - mul_,
// add_out, mul_, addcmul_out, sqrt, add_(eps), add_out(wd), addcdiv_out per tensor;
// nn/SGD.scala:46-98; nn/RAdam.scala:86-137; nn/Yogi.scala:93-129; nn/package.scala:72-100 gradientClippingInPlace;
// lamp-data/.../distributed/package.scala:690-719 averageGradients).
// The arithmetic and its order follow the reference line by line; the ResNet step has 37
// parameter tensors, i.e. ~300 tiny launches become one.
#include "device_utils.h"
#include "../core/strided.h"
#include "conv_backends.h"

namespace lamp {

constexpr int MT_MAX = 40;       // tensors per launch (the descriptor is a by-value kernel argument: 3.4 KB of the 4 KB limit; the ResNet has 37)
constexpr int MT_CHUNK = 1024;   // elements per workgroup (4096: the ResNet's 392 k parameters made ~130 workgroups for 256 CUs - 15 us per AdamW launch)

struct MultiArgs {
  int n;
  void* p[5][MT_MAX];            // up to 5 tensor lists
  int64_t numel[MT_MAX];
  int blk_start[MT_MAX + 1];     // prefix sums of per-tensor chunk counts
  double h[4][MT_MAX];           // per-tensor hyper parameters
  double s[4];                   // scalars
  int flags;
};

static_assert(sizeof(MultiArgs) <= 4096, "MultiArgs is passed by value: HIP kernel arguments are limited to 4 KB");

// the tensor whose chunks contain workgroup chunk `blk`: binary search (the descriptor lives in the kernel-argument segment: every probe
// is a dependent scalar load, and the linear walk over 40 tensors cost a 2-KB chunk more than its data did - 0.8 TB/s in the
// gradient-norm kernels of the language model)
__device__ __forceinline__ int mt_find(const MultiArgs& a, int blk) {
  int lo = 0, hi = a.n - 1;                   // invariant: blk_start[lo] <= blk < blk_start[hi + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (blk >= a.blk_start[mid]) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// AdamW.scala:124-166.  T = parameter/optimizer-state dtype (f32 or f64; bf16 state allowed),
// G = gradient dtype, M = model parameter dtype when a master (working) copy is used.
// p[0]=param (or master copy), p[1]=grad, p[2]=m, p[3]=v, p[4]=model param to down-cast into (or null)
// h[0]=stepParam (= sched*lr*sqrt(1-b2^t)/(1-b1^t) or sched*lr), h[1]=stepWd, h[2]=beta1, h[3]=beta2, s[0]=eps
template <class T, class G>
__global__ __launch_bounds__(256) void adamw_kernel(MultiArgs a) {
  using A = acc_t<T>;
  const int t = mt_find(a, blockIdx.x);
  const int64_t begin = (int64_t)(blockIdx.x - a.blk_start[t]) * MT_CHUNK;
  const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
  T* p = (T*)a.p[0][t];
  const G* g = (const G*)a.p[1][t];
  T* m = (T*)a.p[2][t];
  T* v = (T*)a.p[3][t];
  G* model = (G*)a.p[4][t];
  const A stepParam = (A)a.h[0][t], stepWd = (A)a.h[1][t], b1 = (A)a.h[2][t], b2 = (A)a.h[3][t];
  const A one_m_b1 = (A)(1.0 - a.h[2][t]), one_m_b2 = (A)(1.0 - a.h[3][t]);
  const A eps = (A)a.s[0];
  for (int64_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
    const A gr = load_as<A>(g[i]);
    A mt = load_as<A>(m[i]) * b1;          // mt *= b1
    mt = mt + one_m_b1 * gr;               // addOut(mt, mt, g, 1-b1)
    A vt = load_as<A>(v[i]) * b2;          // vt *= b2
    vt = vt + (one_m_b2 * gr) * gr;        // addcmulOut(vt, vt, g, g, 1-b2)
    A denom = (A)sqrt((double)vt);
    if (sizeof(A) == 4) denom = sqrtf((float)vt);
    denom = denom + eps;
    A pv = load_as<A>(p[i]);
    if (stepWd != A(0)) pv = pv + (-stepWd) * pv;      // addOut(param, param, param, -stepWd)
    pv = pv + ((-stepParam) * mt) / denom;             // addcdivOut(param, param, mt, denom, -stepParam)
    m[i] = store_as<T>(mt);
    v[i] = store_as<T>(vt);
    p[i] = store_as<T>(pv);
    if (model) model[i] = store_as<G>(load_as<acc_t<G>>(store_as<T>(pv)));
  }
}

// One chunk of an update over (param, grad, m, v) of ONE dtype: f(p, g, m, v) on acc_t values per element, every stored value rounded
// once.  These kernels are pure bandwidth (7 or 8 streams per element), so the chunk moves in 16-byte packets where all four bases are
// on one (a chunk starts a multiple of MT_CHUNK elements into its tensor: aligned iff the tensor is) and element-wise past the last
// whole packet.  WRITE_G: the gradient is written back (Yogi).
template <class T, bool WRITE_G, class F>
__device__ __forceinline__ void mt_update_chunk(const MultiArgs& a, int t, F f) {
  using A = acc_t<T>;
  constexpr int W = 16 / sizeof(T);
  const int64_t begin = (int64_t)(blockIdx.x - a.blk_start[t]) * MT_CHUNK;
  const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
  T* p = (T*)a.p[0][t];
  T* g = (T*)a.p[1][t];
  T* m = (T*)a.p[2][t];
  T* v = (T*)a.p[3][t];
  int64_t i0 = begin;
  if (((((uintptr_t)(p + begin)) | ((uintptr_t)(g + begin)) | ((uintptr_t)(m + begin)) | ((uintptr_t)(v + begin))) & 15) == 0) {
    const int nv = (int)((end - begin) / W);
    Vec<T, W>* pq = reinterpret_cast<Vec<T, W>*>(p + begin);
    Vec<T, W>* gq = reinterpret_cast<Vec<T, W>*>(g + begin);
    Vec<T, W>* mq = reinterpret_cast<Vec<T, W>*>(m + begin);
    Vec<T, W>* vq = reinterpret_cast<Vec<T, W>*>(v + begin);
    for (int q = threadIdx.x; q < nv; q += blockDim.x) {
      Vec<T, W> pk = pq[q], gk = gq[q], mk = mq[q], vk = vq[q];
#pragma unroll
      for (int k = 0; k < W; k++) {
        A pv = load_as<A>(pk.v[k]), gr = load_as<A>(gk.v[k]), mt = load_as<A>(mk.v[k]), vt = load_as<A>(vk.v[k]);
        f(pv, gr, mt, vt);
        pk.v[k] = store_as<T>(pv); mk.v[k] = store_as<T>(mt); vk.v[k] = store_as<T>(vt);
        if (WRITE_G) gk.v[k] = store_as<T>(gr);
      }
      pq[q] = pk; mq[q] = mk; vq[q] = vk;
      if (WRITE_G) gq[q] = gk;
    }
    i0 = begin + (int64_t)nv * W;
  }
  for (int64_t i = i0 + threadIdx.x; i < end; i += blockDim.x) {
    A pv = load_as<A>(p[i]), gr = load_as<A>(g[i]), mt = load_as<A>(m[i]), vt = load_as<A>(v[i]);
    f(pv, gr, mt, vt);
    p[i] = store_as<T>(pv); m[i] = store_as<T>(mt); v[i] = store_as<T>(vt);
    if (WRITE_G) g[i] = store_as<T>(gr);
  }
}
template <class A> __device__ __forceinline__ A mt_sqrt(A x) { return (A)sqrt((double)x); }
template <> __device__ __forceinline__ float mt_sqrt<float>(float x) { return sqrtf(x); }

// RAdam.scala:86-137, in adamw_kernel's expression order.  RECT = this step is rectified for every tensor of the launch (rho > 4, a host
// decision per tensor from stepCount and its beta2: the host groups the tensors of a call by branch).
// p[0]=param, p[1]=grad, p[2]=m, p[3]=v; h[0]=stepParam, h[1]=stepWd (= sched*wd, NOT times lr), h[2]=beta1, h[3]=beta2, s[0]=eps
template <class T, bool RECT>
__global__ __launch_bounds__(256) void radam_kernel(MultiArgs a) {
  using A = acc_t<T>;
  const int t = mt_find(a, blockIdx.x);
  const A stepParam = (A)a.h[0][t], stepWd = (A)a.h[1][t], b1 = (A)a.h[2][t], b2 = (A)a.h[3][t];
  const A one_m_b1 = (A)(1.0 - a.h[2][t]), one_m_b2 = (A)(1.0 - a.h[3][t]);
  const A eps = (A)a.s[0];
  mt_update_chunk<T, false>(a, t, [&](A& pv, A& gr, A& mt, A& vt) {
    mt = mt * b1;                          // mt *= b1
    mt = mt + one_m_b1 * gr;               // add_out(mt, mt, g, 1-b1)
    vt = vt * b2;                          // vt *= b2
    vt = vt + (one_m_b2 * gr) * gr;        // addcmul_out(vt, vt, g, g, 1-b2)
    if (stepWd != A(0)) pv = pv + (-stepWd) * pv;      // add_out(param, param, param, -stepWd)
    if (RECT) {
      const A denom = mt_sqrt<A>(vt) + eps;
      pv = pv + ((-stepParam) * mt) / denom;           // addcdiv_out(param, param, mt, denom, -stepParam)
    } else {
      pv = pv + (-stepParam) * mt;                     // add_out(param, param, mt, -stepParam)
    }
  });
}

// a product rounded to A that the compiler may not contract into the operation that consumes it
template <class A> __device__ __forceinline__ A rounded_mul(A x, A y) {
#pragma clang fp contract(off)
  A r = x * y;
  asm volatile("" : "+v"(r));
  return r;
}

// Yogi.scala:93-129.  The gradient is OVERWRITTEN with g*g*sign(v - g*g), as the reference's gradients.pow_(2); gradients *= sign do: its
// KAT steps twice with one gradient tensor, and the second step's values are those of a step on -g^2 (adamw.test.scala:128-155).
// g*g is a rounded value BEFORE the subtraction: contracted into v - g*g the sign would be that of the exact product, non-zero wherever
// v == round(g*g), and v would move by 2(1-b2)g^2 there.
// h[0]=stepParam (= sched*lr / (1-b1^t) or sched*lr), h[1]=stepWd (= sched*wd), h[2]=beta1, h[3]=beta2, s[0]=eps,
// s[1]=1/sqrt(1-b2^t) (flags & 1: debias; a launch holds tensors of one such factor)
template <class T>
__global__ __launch_bounds__(256) void yogi_kernel(MultiArgs a) {
  using A = acc_t<T>;
  const int t = mt_find(a, blockIdx.x);
  const A stepParam = (A)a.h[0][t], stepWd = (A)a.h[1][t], b1 = (A)a.h[2][t];
  const A one_m_b1 = (A)(1.0 - a.h[2][t]), one_m_b2 = (A)(1.0 - a.h[3][t]);
  const A eps = (A)a.s[0], debiasDenom = (A)a.s[1];
  const bool debias = a.flags & 1;
  mt_update_chunk<T, true>(a, t, [&](A& pv, A& gr, A& mt, A& vt) {
    mt = mt * b1;                          // mt *= b1
    mt = mt + one_m_b1 * gr;               // add_out(mt, mt, g, 1-b1)
    const A g2 = rounded_mul(gr, gr);      // gradients.pow_(2)
    const A diff = vt - g2;                // sub(vt, gradients)
    const A sgn = (A)((diff > A(0)) - (diff < A(0)));   // sign_(): -1, 0, +1
    const A gn = g2 * sgn;                 // gradients *= tmp (exact)
    vt = vt - one_m_b2 * gn;               // sub_out(vt, vt, gradients, 1-b2)
    A denom = mt_sqrt<A>(vt);
    if (debias) denom = denom * debiasDenom;
    denom = denom + eps;
    if (stepWd != A(0)) pv = pv + (-stepWd) * pv;      // addOut(param, param, param, -stepWd)
    pv = pv + ((-stepParam) * mt) / denom;             // addcdiv_out(param, param, mt, denom, -stepParam)
    gr = gn;
  });
}

// SGD.scala:46-98. p[0]=param, p[1]=grad, p[2]=velocity (or null); h[0]=lr*sched, h[1]=wd*sched, h[2]=momentum
template <class T>
__global__ __launch_bounds__(256) void sgdw_kernel(MultiArgs a) {
  using A = acc_t<T>;
  const int t = mt_find(a, blockIdx.x);
  const int64_t begin = (int64_t)(blockIdx.x - a.blk_start[t]) * MT_CHUNK;
  const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
  T* p = (T*)a.p[0][t];
  const T* g = (const T*)a.p[1][t];
  T* vel = (T*)a.p[2][t];
  const A lr = (A)a.h[0][t], wd = (A)a.h[1][t], mom = (A)a.h[2][t];
  for (int64_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
    A pv = load_as<A>(p[i]);
    const A gr = load_as<A>(g[i]);
    if (!vel) {
      if (wd != A(0)) pv = pv + (-wd) * pv;
      pv = pv + (-lr) * gr;
    } else {
      A vv = load_as<A>(vel[i]) * mom;
      vv = vv + lr * gr;
      if (wd != A(0)) pv = pv + (-wd) * pv;
      pv = pv + A(-1) * vv;
      vel[i] = store_as<T>(vv);
    }
    p[i] = store_as<T>(pv);
  }
}

// sum of squares per workgroup -> partial[blockIdx.x] (deterministic two stage reduction)
template <class T>
__global__ __launch_bounds__(256) void mt_sumsq_kernel(MultiArgs a, acc_t<T>* __restrict__ partial, int per_wg) {
  using A = acc_t<T>;
  __shared__ A sm[4];
  // a workgroup takes `per_wg` consecutive chunks (a 2-KB chunk per workgroup is bound by the dispatch rate: 21 k workgroups in 46 us)
  A acc = 0;
  const int nblk = a.blk_start[a.n];
  int t = blockIdx.x * per_wg < nblk ? mt_find(a, blockIdx.x * per_wg) : 0;
  for (int j = 0; j < per_wg; j++) {
    const int blk = blockIdx.x * per_wg + j;
    if (blk >= nblk) break;
    while (blk >= a.blk_start[t + 1]) t++;
    const int64_t begin = (int64_t)(blk - a.blk_start[t]) * MT_CHUNK;
    const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
    const T* g = (const T*)a.p[0][t];
    // 16-byte packets where the chunk starts on one
    constexpr int W = 16 / sizeof(T);
    int64_t i0 = begin;
    if ((((uintptr_t)(g + begin)) & 15) == 0) {
      const int64_t nv = (end - begin) / W;
      const Vec<T, W>* gv = reinterpret_cast<const Vec<T, W>*>(g + begin);
      for (int64_t v = threadIdx.x; v < nv; v += blockDim.x) {
        const Vec<T, W> pk = gv[v];
#pragma unroll
        for (int k = 0; k < W; k++) { const A x = load_as<A>(pk.v[k]); acc += x * x; }
      }
      i0 = begin + nv * W;
    }
    for (int64_t i = i0 + threadIdx.x; i < end; i += blockDim.x) { const A x = load_as<A>(g[i]); acc += x * x; }
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
// total[0] += sum(partial) ; single workgroup
template <class A>
__global__ __launch_bounds__(256) void mt_accumulate_kernel(const A* __restrict__ partial, int n, A* __restrict__ total, int overwrite) {
  __shared__ A sm[4];
  A acc = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partial[i];
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) total[0] = overwrite ? acc : total[0] + acc;
}
// g *= min(1, theta / sqrt(total))     nn/package.scala:88-97
template <class T>
__global__ __launch_bounds__(256) void mt_clip_scale_kernel(MultiArgs a, const acc_t<T>* __restrict__ total, int per_wg) {
  using A = acc_t<T>;
  // same rounding points as the reference: norm = sqrt(sum) in the gradient dtype, scalar = theta/norm, min(scalar, 1)
  const A norm = (A)load_as<A>(store_as<T>((A)sqrt((double)total[0])));
  A sc = (A)a.s[0] / norm;
  sc = (sc < A(1) || sc != sc) ? sc : A(1);  // NaN norm: ATen minimum propagates NaN (a bare `sc < 1 ? sc : 1` turns it into 1)
  const int nblk = a.blk_start[a.n];
  int t = blockIdx.x * per_wg < nblk ? mt_find(a, blockIdx.x * per_wg) : 0;
  for (int j = 0; j < per_wg; j++) {
    const int blk = blockIdx.x * per_wg + j;
    if (blk >= nblk) break;
    while (blk >= a.blk_start[t + 1]) t++;
    const int64_t begin = (int64_t)(blk - a.blk_start[t]) * MT_CHUNK;
    const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
    T* g = (T*)a.p[0][t];
    constexpr int W = 16 / sizeof(T);
    int64_t i0 = begin;
    if ((((uintptr_t)(g + begin)) & 15) == 0) {
      const int64_t nv = (end - begin) / W;
      Vec<T, W>* gv = reinterpret_cast<Vec<T, W>*>(g + begin);
      for (int64_t v = threadIdx.x; v < nv; v += blockDim.x) {
        Vec<T, W> pk = gv[v];
#pragma unroll
        for (int k = 0; k < W; k++) pk.v[k] = store_as<T>((A)(load_as<A>(pk.v[k]) * sc));
        gv[v] = pk;
      }
      i0 = begin + nv * W;
    }
    for (int64_t i = i0 + threadIdx.x; i < end; i += blockDim.x) g[i] = store_as<T>((A)(load_as<A>(g[i]) * sc));
  }
}

// bucket[off_t + i] = scale * t[i] (as f32) ; p[0] = tensors, h[0][t] = element offset inside the bucket
template <class T>
__global__ __launch_bounds__(256) void mt_flatten_kernel(MultiArgs a, float* __restrict__ bucket) {
  const int t = mt_find(a, blockIdx.x);
  const int64_t begin = (int64_t)(blockIdx.x - a.blk_start[t]) * MT_CHUNK;
  const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
  const T* src = (const T*)a.p[0][t];
  float* dst = bucket + (int64_t)a.h[0][t];
  const float scale = (float)a.s[0];
  for (int64_t i = begin + threadIdx.x; i < end; i += blockDim.x) dst[i] = scale * load_as<float>(src[i]);
}
template <class T>
__global__ __launch_bounds__(256) void mt_unflatten_kernel(MultiArgs a, const float* __restrict__ bucket, int64_t last_index) {
  const int t = mt_find(a, blockIdx.x);
  const int64_t begin = (int64_t)(blockIdx.x - a.blk_start[t]) * MT_CHUNK;
  const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
  T* dst = (T*)a.p[0][t];
  const float* src = bucket + (int64_t)a.h[0][t];
  const float div = last_index >= 0 ? bucket[last_index] : 1.0f;
  for (int64_t i = begin + threadIdx.x; i < end; i += blockDim.x) dst[i] = store_as<T>((acc_t<T>)(src[i] / div));
}

// ---- Shampoo (nn/Shampoo.scala:86-197) -----------------------------------------------------------------------
// The momentum blend of every tensor with momentum > 0, in place in the GRADIENT as the reference does (Shampoo.scala:107-113):
// g *= 1-mom; g = g + mom*last; last = g.   p[0]=grad, p[1]=lastGradient; h[0]=momentum
template <class T>
__global__ __launch_bounds__(256) void shampoo_blend_kernel(MultiArgs a) {
  const int t = mt_find(a, blockIdx.x);
  const int64_t begin = (int64_t)(blockIdx.x - a.blk_start[t]) * MT_CHUNK;
  const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
  T* g = (T*)a.p[0][t];
  T* last = (T*)a.p[1][t];
  const T mom = (T)a.h[0][t], one_m = (T)(1.0 - a.h[0][t]);
  for (int64_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
    T v = rounded_mul(g[i], one_m);        // gradients *= (1 - mom)
    v = v + mom * last[i];                 // addOut(gradients, gradients, lastGradient, mom)
    g[i] = v;
    last[i] = v;                           // lastGradient.copyFrom(gradients)
  }
}
// the statistics of a side kept as a vector: stat[i] += sum_j g[i][j]^2 (one wave per row) and stat[j] += sum_i g[i][j]^2 (one thread per column)
template <class T>
__global__ __launch_bounds__(256) void shampoo_row_sumsq_kernel(T* __restrict__ stat, const T* __restrict__ g, int64_t d1, int64_t d2) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= d1) return;
  T s = 0;
  for (int64_t j = threadIdx.x & 63; j < d2; j += 64) { const T v = g[row * d2 + j]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) stat[row] += s;
}
template <class T>
__global__ __launch_bounds__(256) void shampoo_col_sumsq_kernel(T* __restrict__ stat, const T* __restrict__ g, int64_t d1, int64_t d2) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= d2) return;
  T s = 0;
  for (int64_t i = 0; i < d1; i++) { const T v = g[i * d2 + j]; s += v * v; }
  stat[j] += s;
}
// out[i][j] = (accumulate ? out[i][j] : 0) + alpha * ((l ? l[i] : 1) * in[i][j]) * (r ? r[j] : 1): a vector side of the update
template <class T>
__global__ __launch_bounds__(256) void shampoo_scale_kernel(T* __restrict__ out, const T* __restrict__ in, const T* __restrict__ l,
                                                            const T* __restrict__ r, int64_t d1, int64_t d2, T alpha, int accumulate) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < d1 * d2; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / d2, j = e - i * d2;
    T v = in[e];
    if (l) v = l[i] * v;
    if (r) v = v * r[j];
    out[e] = accumulate ? out[e] + alpha * v : v;
  }
}
// the inverse fourth roots.  Reference mode: diag(s^-1/4) dense, s in descending order (what Shampoo.scala:143-146 evaluates to).
template <class T>
__global__ __launch_bounds__(256) void shampoo_diag_root_kernel(T* __restrict__ out, const double* __restrict__ s, int n) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n * n; e += gridDim.x * 256) {
    const int i = e / n, j = e - i * n;
    out[e] = i == j ? (T)pow(s[i], -0.25) : T(0);
  }
}
// paper mode: out = U diag(s^-1/4), the left factor of U diag(s^-1/4) U^T
__global__ __launch_bounds__(256) void shampoo_scale_cols_kernel(double* __restrict__ out, const double* __restrict__ U, const double* __restrict__ s, int n) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n * n; e += gridDim.x * 256) out[e] = U[e] * pow(s[e % n], -0.25);
}
template <class T> __device__ __forceinline__ T shampoo_root(T x) { return (T)pow((double)x, -0.25); }
template <> __device__ __forceinline__ float shampoo_root<float>(float x) { return powf(x, -0.25f); }
template <class T>
__global__ __launch_bounds__(256) void shampoo_vec_root_kernel(T* __restrict__ out, const T* __restrict__ stat, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = shampoo_root<T>(stat[i]);
}

// ---- model-state operations of the training drivers (IOLoops.epochs / SWA.epochs) -------------------------------
// One chunk of a two-list operation dst <- f(dst, src) over elements of type T: 16-byte packets where both bases are on one (a chunk
// starts a multiple of MT_CHUNK elements into its tensor: aligned iff the tensor is), element-wise past the last whole packet and for
// the whole chunk otherwise.
template <class T, class F>
__device__ __forceinline__ void mt_pair_chunk(const MultiArgs& a, int t, F f) {
  constexpr int W = 16 / sizeof(T);
  const int64_t begin = (int64_t)(blockIdx.x - a.blk_start[t]) * MT_CHUNK;
  const int64_t end = min(begin + MT_CHUNK, a.numel[t]);
  T* d = (T*)a.p[0][t];
  const T* s = (const T*)a.p[1][t];
  int64_t i0 = begin;
  if (((((uintptr_t)(d + begin)) | ((uintptr_t)(s + begin))) & 15) == 0) {
    const int nv = (int)((end - begin) / W);
    Vec<T, W>* dq = reinterpret_cast<Vec<T, W>*>(d + begin);
    const Vec<T, W>* sq = reinterpret_cast<const Vec<T, W>*>(s + begin);
    for (int q = threadIdx.x; q < nv; q += blockDim.x) {
      Vec<T, W> dk = dq[q];
      const Vec<T, W> sk = sq[q];
#pragma unroll
      for (int k = 0; k < W; k++) dk.v[k] = f(dk.v[k], sk.v[k]);
      dq[q] = dk;
    }
    i0 = begin + (int64_t)nv * W;
  }
  for (int64_t i = i0 + threadIdx.x; i < end; i += blockDim.x) d[i] = f(d[i], s[i]);
}

// SWA.scala:136-145 updateAccumulator, in place on the accumulator: tmp1 = avg * n; tmp2 = tmp1 + current; avg = tmp2 / (n + 1).  The
// reference stores three tensors, so each of the three results is rounded to T; the product is a rounded value before the addition
// (contracted, avg*n + cur would be rounded once), and the division is the true quotient lamp_div_scalar computes, not a product with
// the reciprocal.  p[0]=avg, p[1]=current; s[0]=n, s[1]=n+1
template <class T>
__global__ __launch_bounds__(256) void swa_average_kernel(MultiArgs a) {
  using A = acc_t<T>;
  const int t = mt_find(a, blockIdx.x);
  const A n = (A)a.s[0], n1 = (A)a.s[1];
  mt_pair_chunk<T>(a, t, [&](T avg, T cur) {
    const T scaled = store_as<T>(rounded_mul(load_as<A>(avg), n));                // ATen.mul_1(avg, n)
    const T sum = store_as<T>((A)(load_as<A>(scaled) + load_as<A>(cur)));         // ATen.add_0(tmp1, current, 1d)
    return store_as<T>((A)(load_as<A>(sum) / n1));                                // ATen.div_2(tmp2, n + 1)
  });
}

// dst[i] = src[i] over tensors of one element size (U: an unsigned integer of that size - the bytes move, whatever the dtype).
// p[0]=dst, p[1]=src
template <class U>
__global__ __launch_bounds__(256) void state_copy_kernel(MultiArgs a) {
  const int t = mt_find(a, blockIdx.x);
  mt_pair_chunk<U>(a, t, [](U, U src) { return src; });
}

// host: iterate over the tensor lists in groups of MT_MAX
template <class Fill, class Launch>
static void for_each_group(int n, const int64_t* numels, Fill fill, Launch launch) {
  for (int base = 0; base < n; base += MT_MAX) {
    MultiArgs a{};
    a.n = std::min(MT_MAX, n - base);
    int blk = 0;
    for (int t = 0; t < a.n; t++) {
      a.numel[t] = numels[base + t];
      a.blk_start[t] = blk;
      blk += (int)((a.numel[t] + MT_CHUNK - 1) / MT_CHUNK);
      fill(a, t, base + t);
    }
    a.blk_start[a.n] = blk;
    if (blk > 0) launch(a, blk);
  }
}

static void check_list(lamp_tensor* const* ts, int n, const char* what, int dtype, int device) {
  for (int i = 0; i < n; i++) {
    check_device_tensor(ts[i], what);
    LAMP_CHECK(ts[i]->is_contiguous(), what << "[" << i << "] must be contiguous");
    if (dtype >= 0) LAMP_CHECK(ts[i]->dtype == dtype, what << "[" << i << "] has dtype " << dtype_name(ts[i]->dtype) << ", expected " << dtype_name(dtype));
    LAMP_CHECK(ts[i]->device() == device, what << "[" << i << "] is on another device");
  }
}

// RAdam / Yogi: parameter, gradient and both moments of a tensor have one dtype (RAdam.scala:44-49: the moments are zeros_like(param)).
// Everything is checked before the first launch, so a rejected call has written nothing.
static void check_moment_step(const char* who, lamp_tensor* const* params, lamp_tensor* const* grads, lamp_tensor* const* m,
                              lamp_tensor* const* v, int n) {
  check_device_tensor(params[0], "parameter");                 // host parameters: the staging layer runs the step on GPU copies
  const int dev = params[0]->device();
  for (int i = 0; i < n; i++) {
    const struct { lamp_tensor* t; const char* what; } lists[4] = {{params[i], "parameter"}, {grads[i], "gradient"}, {m[i], "first moment"}, {v[i], "second moment"}};
    for (const auto& l : lists) {
      check_device_tensor(l.t, l.what);
      LAMP_CHECK(l.t->device() == dev, who << ": " << l.what << " " << i << " is on another device");
      LAMP_CHECK(l.t->is_contiguous(), who << ": " << l.what << " " << i << " must be contiguous");
      LAMP_CHECK(l.t->dtype == params[i]->dtype, who << ": " << l.what << " " << i << " has dtype " << dtype_name(l.t->dtype) << ", the parameter " << dtype_name(params[i]->dtype));
      LAMP_CHECK(l.t->numel() == params[i]->numel(), who << ": " << l.what << " " << i << " has " << l.t->numel() << " elements, the parameter " << params[i]->numel());
    }
    const int dt = params[i]->dtype;
    LAMP_CHECK(dt == kF32 || dt == kF64 || dt == kBF16 || dt == kF16, who << ": unsupported dtype " << dtype_name(dt));
  }
}
// one homogeneous launch sequence per (dtype, key) class of the tensors: launch(dtype, indices of the class)
template <class Launch>
static void for_each_class(lamp_tensor* const* params, const std::vector<int>& key, int nkeys, Launch launch) {
  for (int dt : {kF32, kF64, kBF16, kF16})
    for (int k = 0; k < nkeys; k++) {
      std::vector<int> sel;
      for (size_t i = 0; i < key.size(); i++) if (params[i]->dtype == dt && key[i] == k) sel.push_back((int)i);
      if (!sel.empty()) launch(dt, sel);
    }
}


// swa_average / state_copy: pair i of the two lists has one dtype, one element count, one device (the first pair's) and is contiguous;
// `floating`: every dtype is f32, f64, bf16 or f16.  Everything is checked before the first launch, so a rejected call has written nothing.
static void check_state_pair(const char* who, const char* dname, lamp_tensor* const* dst, const char* sname, lamp_tensor* const* src, int n,
                             bool floating) {
  LAMP_CHECK(n > 0 && dst && src, who << ": null tensor list");
  check_device_tensor(dst[0], dname);                          // host state: the staging layer runs the kernel on GPU copies
  const int dev = dst[0]->device();
  for (int i = 0; i < n; i++) {
    const struct { lamp_tensor* t; const char* what; } lists[2] = {{dst[i], dname}, {src[i], sname}};
    for (const auto& l : lists) {
      LAMP_CHECK(l.t != nullptr, who << ": " << l.what << " " << i << " is null");
      check_device_tensor(l.t, l.what);
      LAMP_CHECK(l.t->device() == dev, who << ": " << l.what << " " << i << " is on another device");
      LAMP_CHECK(l.t->is_contiguous(), who << ": " << l.what << " " << i << " must be contiguous");
    }
    LAMP_CHECK(src[i]->dtype == dst[i]->dtype, who << ": " << sname << " " << i << " has dtype " << dtype_name(src[i]->dtype) << ", the " << dname << " "
                                                   << dtype_name(dst[i]->dtype));
    LAMP_CHECK(src[i]->numel() == dst[i]->numel(), who << ": " << sname << " " << i << " has " << src[i]->numel() << " elements, the " << dname << " "
                                                       << dst[i]->numel());
    if (floating) LAMP_CHECK(is_float(dst[i]->dtype), who << ": tensor " << i << " has dtype " << dtype_name(dst[i]->dtype) << ", not a floating point type");
    else { const size_t w = dst[i]->itemsize(); LAMP_CHECK(w == 1 || w == 2 || w == 4 || w == 8, who << ": tensor " << i << " has elements of " << w << " bytes"); }
  }
}
static int64_t mt_elements(const MultiArgs& a) {
  int64_t e = 0;
  for (int t = 0; t < a.n; t++) e += a.numel[t];
  return e;
}

}  // namespace lamp

using namespace lamp;

// The bucket layout on HOST tensors (same offsets, same f32 arithmetic: bucket = scale * g rounded to f32, g = bucket / last as f32):
// a control-plane process can pack / unpack gradients that live in host memory - the exchange protocol of the data-parallel step
// is testable between CPU-only ranks, and host-resident replicas (lamp's CPU device) can take part in an exchange.
template <class T>
static void host_flatten(float* bucket, lamp_tensor* const* ts, int n, const std::vector<int64_t>& offs, double scale) {
  const float sc = (float)scale;
  for (int i = 0; i < n; i++) {
    const T* src = ts[i]->ptr<T>();
    float* dst = bucket + offs[i];
    for (int64_t k = 0, e = ts[i]->numel(); k < e; k++) dst[k] = sc * load_as<float>(src[k]);
  }
}
template <class T>
static void host_unflatten(lamp_tensor* const* ts, int n, const float* bucket, const std::vector<int64_t>& offs, int64_t last) {
  const float div = last >= 0 ? bucket[last] : 1.0f;
  for (int i = 0; i < n; i++) {
    T* dst = ts[i]->ptr<T>();
    const float* src = bucket + offs[i];
    for (int64_t k = 0, e = ts[i]->numel(); k < e; k++) dst[k] = store_as<T>((acc_t<T>)(src[k] / div));
  }
}
static bool all_host(const lamp_tensor* bucket, lamp_tensor* const* ts, int n) {
  if (bucket->is_device()) return false;
  for (int i = 0; i < n; i++) {
    LAMP_CHECK(ts[i] && !ts[i]->is_device(), "host bucket with a device tensor in the list");
    LAMP_CHECK(ts[i]->is_contiguous() && ts[i]->dtype == ts[0]->dtype, "host bucket: tensors must be contiguous and of one dtype");
  }
  return true;
}

extern "C" {

int lamp_gradient_clipping_(lamp_tensor* const* grads, int n, double theta) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  const int dtype = grads[0]->dtype, dev = grads[0]->device();
  check_list(grads, n, "gradients", dtype, dev);
  hipStream_t st = current_stream(dev);
  std::vector<int64_t> numels(n);
  for (int i = 0; i < n; i++) numels[i] = grads[i]->numel();
  LAMP_DISPATCH_FLOAT(dtype, T, {
    using A = acc_t<T>;
    const int adt = std::is_same<A, double>::value ? kF64 : kF32;
    int64_t one[1] = {1};
    Hold total(new_tensor(one, 1, adt, dev));
    bool first = true;
    for_each_group(n, numels.data(), [&](MultiArgs& a, int t, int gi) { a.p[0][t] = grads[gi]->data(); },
                   [&](MultiArgs& a, int blk) {
                     // up to 16 chunks per workgroup once there are more than 8 chunks per CU (small models keep one: the ResNet has 383 chunks)
                     const int per_wg = std::min(16, std::max(1, blk / (8 * num_cus()))), wgs = (blk + per_wg - 1) / per_wg;
                     int64_t ps[1] = {wgs};
                     Hold partial(new_tensor(ps, 1, adt, dev));
                     hipLaunchKernelGGL((mt_sumsq_kernel<T>), dim3(wgs), dim3(256), 0, st, a, partial->ptr<A>(), per_wg);
                     hipLaunchKernelGGL((mt_accumulate_kernel<A>), dim3(1), dim3(256), 0, st, partial->ptr<A>(), wgs, total->ptr<A>(), first ? 1 : 0);
                     first = false;
                   });
    LAMP_LAUNCH_CHECK();
    for_each_group(n, numels.data(), [&](MultiArgs& a, int t, int gi) { a.p[0][t] = grads[gi]->data(); a.s[0] = theta; },
                   [&](MultiArgs& a, int blk) {
                     const int per_wg = std::min(16, std::max(1, blk / (8 * num_cus()))), wgs = (blk + per_wg - 1) / per_wg;
                     hipLaunchKernelGGL((mt_clip_scale_kernel<T>), dim3(wgs), dim3(256), 0, st, a, total->ptr<A>(), per_wg);
                   });
    LAMP_LAUNCH_CHECK();
  });
  LAMP_API_END
}

int lamp_adamw_step_(lamp_tensor* const* params, lamp_tensor* const* grads, lamp_tensor* const* m, lamp_tensor* const* v,
                     lamp_tensor* const* master, int n, const double* lr, const double* weight_decay, const double* beta1,
                     const double* beta2, double eps, double schedule_factor, int64_t step_count, int debias) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  check_device_tensor(params[0], "parameter");                 // host parameters: the staging layer runs the step on GPU copies
  const int dev = params[0]->device();
  hipStream_t st = current_stream(dev);
  // group tensors by (state dtype, grad dtype) so that each launch is homogeneous
  for (int pass_state : {kF32, kF64, kBF16, kF16}) {
    for (int pass_grad : {kF32, kF64, kBF16, kF16}) {
      std::vector<int> sel;
      for (int i = 0; i < n; i++) {
        check_device_tensor(params[i], "parameter"); check_device_tensor(grads[i], "gradient");
        const Tensor* state_holder = (master && master[i]) ? master[i] : params[i];
        if (state_holder->dtype == pass_state && grads[i]->dtype == pass_grad) sel.push_back(i);
      }
      if (sel.empty()) continue;
      std::vector<int64_t> numels(sel.size());
      for (size_t k = 0; k < sel.size(); k++) {
        const int i = sel[k];
        const Tensor* holder = (master && master[i]) ? master[i] : params[i];
        numels[k] = holder->numel();
        LAMP_CHECK(grads[i]->numel() == numels[k] && m[i]->numel() == numels[k] && v[i]->numel() == numels[k], "adamw: tensor " << i << " size mismatch");
        LAMP_CHECK(m[i]->dtype == pass_state && v[i]->dtype == pass_state, "adamw: moment buffers of tensor " << i << " must have the dtype of the (working) parameter");
        LAMP_CHECK(holder->is_contiguous() && grads[i]->is_contiguous() && m[i]->is_contiguous() && v[i]->is_contiguous() && params[i]->is_contiguous(), "adamw: tensors must be contiguous");
        if (master && master[i]) LAMP_CHECK(params[i]->dtype == grads[i]->dtype, "adamw mixed precision: model parameter and gradient dtypes differ");
        else LAMP_CHECK(params[i]->dtype == grads[i]->dtype, "adamw: parameter and gradient dtypes differ");
      }
      auto fill = [&](MultiArgs& a, int t, int gi) {
        const int i = sel[gi];
        const bool mixed = master && master[i];
        a.p[0][t] = mixed ? master[i]->data() : params[i]->data();
        a.p[1][t] = grads[i]->data();
        a.p[2][t] = m[i]->data();
        a.p[3][t] = v[i]->data();
        a.p[4][t] = mixed ? params[i]->data() : nullptr;
        const double b1 = beta1[i], b2 = beta2[i];
        const double stepParam = debias ? schedule_factor * lr[i] * std::sqrt(1 - std::pow(b2, (double)step_count)) / (1 - std::pow(b1, (double)step_count))
                                        : schedule_factor * lr[i];
        a.h[0][t] = stepParam;
        a.h[1][t] = stepParam * weight_decay[i];
        a.h[2][t] = b1;
        a.h[3][t] = b2;
        a.s[0] = eps;
      };
#define ADAMW_LAUNCH(T, G) for_each_group((int)sel.size(), numels.data(), fill, [&](MultiArgs& a, int blk) { hipLaunchKernelGGL((adamw_kernel<T, G>), dim3(blk), dim3(256), 0, st, a); })
      if (pass_state == kF32 && pass_grad == kF32) ADAMW_LAUNCH(float, float);
      else if (pass_state == kF64 && pass_grad == kF64) ADAMW_LAUNCH(double, double);
      else if (pass_state == kF32 && pass_grad == kBF16) ADAMW_LAUNCH(float, bf16_t);
      else if (pass_state == kBF16 && pass_grad == kBF16) ADAMW_LAUNCH(bf16_t, bf16_t);
      else if (pass_state == kF32 && pass_grad == kF16) ADAMW_LAUNCH(float, f16_t);      // mixed precision on half parameters (adamw.test.scala:96-127)
      else if (pass_state == kF16 && pass_grad == kF16) ADAMW_LAUNCH(f16_t, f16_t);
      else LAMP_CHECK(false, "adamw: unsupported (state, gradient) dtype pair " << dtype_name(pass_state) << "/" << dtype_name(pass_grad));
#undef ADAMW_LAUNCH
      LAMP_LAUNCH_CHECK();
    }
  }
  conv_repack_cached(params, n, st);      // the convolution weights' packed images follow the update (conv.hip)
  LAMP_API_END
}

int lamp_radam_step_(lamp_tensor* const* params, lamp_tensor* const* grads, lamp_tensor* const* m, lamp_tensor* const* v, int n,
                     const double* lr, const double* weight_decay, const double* beta1, const double* beta2, double eps,
                     double schedule_factor, int64_t step_count) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  check_moment_step("radam", params, grads, m, v, n);
  hipStream_t st = current_stream(params[0]->device());
  // RAdam.scala:98-115,135: the branch and the step size are host scalars per tensor
  std::vector<int> rect(n);
  std::vector<double> stepParam(n);
  for (int i = 0; i < n; i++) {
    const double b1 = beta1[i], b2 = beta2[i], t = (double)step_count;
    const double beta2PowT = std::pow(b2, t);
    const double rhoInf = (2.0 / (1.0 - b2)) - 1;
    const double rho = rhoInf - (2.0 * t * beta2PowT / (1.0 - beta2PowT));
    rect[i] = rho > 4;          // rhoInf <= 4 (beta2 <= 0.6) is never rectified: (rhoInf - 4) is evaluated under rho > 4 only
    stepParam[i] = rect[i] ? schedule_factor * lr[i] * std::sqrt((1 - beta2PowT) * ((rho - 4) / (rhoInf - 4)) * ((rho - 2) / rho) * (rhoInf / (rhoInf - 2))) / (1 - std::pow(b1, t))
                           : schedule_factor * lr[i] / (1 - std::pow(b1, t));
  }
  for_each_class(params, rect, 2, [&](int dt, const std::vector<int>& sel) {
    std::vector<int64_t> numels(sel.size());
    for (size_t k = 0; k < sel.size(); k++) numels[k] = params[sel[k]]->numel();
    auto fill = [&](MultiArgs& a, int t, int gi) {
      const int i = sel[gi];
      a.p[0][t] = params[i]->data(); a.p[1][t] = grads[i]->data(); a.p[2][t] = m[i]->data(); a.p[3][t] = v[i]->data();
      a.h[0][t] = stepParam[i];
      a.h[1][t] = schedule_factor * weight_decay[i];
      a.h[2][t] = beta1[i];
      a.h[3][t] = beta2[i];
      a.s[0] = eps;
    };
    const bool r = rect[sel[0]];
    LAMP_DISPATCH_FLOAT(dt, T, for_each_group((int)sel.size(), numels.data(), fill, [&](MultiArgs& a, int blk) {
      if (r) hipLaunchKernelGGL((radam_kernel<T, true>), dim3(blk), dim3(256), 0, st, a);
      else hipLaunchKernelGGL((radam_kernel<T, false>), dim3(blk), dim3(256), 0, st, a);
    }));
    LAMP_LAUNCH_CHECK();
  });
  conv_repack_cached(params, n, st);      // the convolution weights' packed images follow the update (conv.hip)
  LAMP_API_END
}

int lamp_yogi_step_(lamp_tensor* const* params, lamp_tensor* const* grads, lamp_tensor* const* m, lamp_tensor* const* v, int n,
                    const double* lr, const double* weight_decay, const double* beta1, const double* beta2, double eps,
                    double schedule_factor, int64_t step_count, int debias) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  check_moment_step("yogi", params, grads, m, v, n);
  hipStream_t st = current_stream(params[0]->device());
  // Yogi.scala:113-116: denom *= 1/sqrt(1-b2^t), a scalar of the launch - tensors are grouped by its value (one class unless beta2 differs)
  std::vector<int> cls(n, 0);
  std::vector<double> denomFactor;
  for (int i = 0; i < n; i++) {
    const double f = debias ? 1.0 / std::sqrt(1 - std::pow(beta2[i], (double)step_count)) : 1.0;
    size_t k = 0;
    while (k < denomFactor.size() && denomFactor[k] != f) k++;
    if (k == denomFactor.size()) denomFactor.push_back(f);
    cls[i] = (int)k;
  }
  for_each_class(params, cls, (int)denomFactor.size(), [&](int dt, const std::vector<int>& sel) {
    std::vector<int64_t> numels(sel.size());
    for (size_t k = 0; k < sel.size(); k++) numels[k] = params[sel[k]]->numel();
    auto fill = [&](MultiArgs& a, int t, int gi) {
      const int i = sel[gi];
      a.p[0][t] = params[i]->data(); a.p[1][t] = grads[i]->data(); a.p[2][t] = m[i]->data(); a.p[3][t] = v[i]->data();
      const double debiasTerm = debias ? 1.0 / (1 - std::pow(beta1[i], (double)step_count)) : 1.0;
      a.h[0][t] = schedule_factor * lr[i] * debiasTerm;
      a.h[1][t] = schedule_factor * weight_decay[i];
      a.h[2][t] = beta1[i];
      a.h[3][t] = beta2[i];
      a.s[0] = eps;
      a.s[1] = denomFactor[cls[i]];
      a.flags = debias ? 1 : 0;
    };
    LAMP_DISPATCH_FLOAT(dt, T, for_each_group((int)sel.size(), numels.data(), fill,
                                              [&](MultiArgs& a, int blk) { hipLaunchKernelGGL((yogi_kernel<T>), dim3(blk), dim3(256), 0, st, a); }));
    LAMP_LAUNCH_CHECK();
  });
  conv_repack_cached(params, n, st);
  LAMP_API_END
}

// One Shampoo step over the tensors whose gradient is defined (Shampoo.scala:96-196, as written).  A side of the
// statistics is a matrix ([d, d], d <= 512) or a vector ([d]); the shapes of lt / rt say which.  Everything is checked before the first
// launch, so a rejected call has written nothing.
int lamp_shampoo_step_(lamp_tensor* const* params, lamp_tensor* const* grads, lamp_tensor* const* lt, lamp_tensor* const* ltinv,
                       lamp_tensor* const* rt, lamp_tensor* const* rtinv, lamp_tensor* const* last, int n, const double* lr,
                       const double* momentum, int64_t step_count, int64_t update_every, int paper_preconditioner) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  LAMP_CHECK(update_every >= 1, "shampoo: updatePreconditionerEveryNIterations must be positive, got " << update_every);
  check_device_tensor(params[0], "parameter");                 // host parameters: the staging layer runs the step on GPU copies
  const int dev = params[0]->device();
  std::vector<int64_t> d1(n), d2(n);
  for (int i = 0; i < n; i++) {
    const struct { lamp_tensor* t; const char* what; } lists[7] = {{params[i], "parameter"}, {grads[i], "gradient"}, {lt[i], "lt"}, {ltinv[i], "ltinv"},
                                                                   {rt[i], "rt"}, {rtinv[i], "rtinv"}, {last[i], "lastGradient"}};
    for (const auto& l : lists) {
      check_device_tensor(l.t, l.what);
      LAMP_CHECK(l.t->device() == dev, "shampoo: " << l.what << " " << i << " is on another device");
      LAMP_CHECK(l.t->is_contiguous(), "shampoo: " << l.what << " " << i << " must be contiguous");
      LAMP_CHECK(l.t->dtype == params[i]->dtype, "shampoo: " << l.what << " " << i << " has dtype " << dtype_name(l.t->dtype) << ", the parameter " << dtype_name(params[i]->dtype));
    }
    const lamp_tensor* p = params[i];
    // no half precisions: the reference has no mixed mode, and eps = 1e-4 statistics do not survive bf16 accumulation
    LAMP_CHECK(p->dtype == kF32 || p->dtype == kF64, "shampoo: parameter " << i << " is " << dtype_name(p->dtype) << ", only f32 and f64 are supported");
    LAMP_CHECK(p->ndim >= 1 && p->numel() > 0, "shampoo: parameter " << i << " is " << p->describe() << ": a 0-d or empty parameter has no shape(0)");
    LAMP_CHECK(grads[i]->shape() == p->shape(), "shampoo: gradient " << i << " is " << grads[i]->describe() << ", the parameter " << p->describe());
    LAMP_CHECK(last[i]->numel() == p->numel(), "shampoo: lastGradient " << i << " is " << last[i]->describe() << ", the parameter " << p->describe());
    d1[i] = p->sizes[0];
    d2[i] = p->numel() / d1[i];
    const struct { const lamp_tensor* t; const lamp_tensor* inv; int64_t d; const char* what; } sides[2] = {{lt[i], ltinv[i], d1[i], "lt"}, {rt[i], rtinv[i], d2[i], "rt"}};
    for (const auto& sd : sides) {
      const bool matrix = sd.t->ndim == 2 && sd.t->sizes[0] == sd.d && sd.t->sizes[1] == sd.d && sd.d <= 512;
      const bool vector = sd.t->ndim == 1 && sd.t->sizes[0] == sd.d;
      LAMP_CHECK(matrix || vector, "shampoo: " << sd.what << " " << i << " is " << sd.t->describe() << ", expected [" << sd.d << "," << sd.d << "] (side <= 512) or [" << sd.d << "]");
      LAMP_CHECK(sd.inv->shape() == sd.t->shape(), "shampoo: " << sd.what << "inv " << i << " is " << sd.inv->describe() << ", " << sd.what << " " << sd.t->describe());
    }
  }
  hipStream_t st = current_stream(dev);
#define SH_CALL(expr) do { if ((expr) != 0) throw Error(lamp_last_error()); } while (0)
#define SH_DISPATCH(DT, T, ...) do { if ((DT) == kF32) { using T = float; __VA_ARGS__; } else { using T = double; __VA_ARGS__; } } while (0)
  // 1. momentum, one launch per dtype over the tensors that have one
  for (int dt : {kF32, kF64}) {
    std::vector<int> sel;
    for (int i = 0; i < n; i++) if (params[i]->dtype == dt && momentum[i] > 0) sel.push_back(i);
    if (sel.empty()) continue;
    std::vector<int64_t> numels(sel.size());
    for (size_t k = 0; k < sel.size(); k++) numels[k] = params[sel[k]]->numel();
    auto fill = [&](MultiArgs& a, int t, int gi) { const int i = sel[gi]; a.p[0][t] = grads[i]->data(); a.p[1][t] = last[i]->data(); a.h[0][t] = momentum[i]; };
    SH_DISPATCH(dt, T, for_each_group((int)sel.size(), numels.data(), fill,
                                      [&](MultiArgs& a, int blk) { hipLaunchKernelGGL((shampoo_blend_kernel<T>), dim3(blk), dim3(256), 0, st, a); }));
    LAMP_LAUNCH_CHECK();
  }
  // 2. statistics: lt += G G^T, rt += G^T G through the GEMMs' beta = 1 epilogue; a vector side takes the sums of squares
  std::vector<Hold> g2(n), p2(n);
  for (int i = 0; i < n; i++) {
    const int64_t sz[2] = {d1[i], d2[i]}, sr[2] = {d2[i], 1};
    g2[i] = Hold(new_view(grads[i], sz, sr, 2, grads[i]->offset));
    p2[i] = Hold(new_view(params[i], sz, sr, 2, params[i]->offset));
    if (lt[i]->ndim == 2) SH_CALL(lamp_addmm_out_transposed2(lt[i], lt[i], g2[i].get(), g2[i].get(), 1.0, 1.0));
    if (rt[i]->ndim == 2) SH_CALL(lamp_addmm_out_transposed1(rt[i], rt[i], g2[i].get(), g2[i].get(), 1.0, 1.0));
    if (params[i]->dtype == kF32) {
      if (lt[i]->ndim == 1) hipLaunchKernelGGL((shampoo_row_sumsq_kernel<float>), dim3((unsigned)((d1[i] + 3) / 4)), dim3(256), 0, st, lt[i]->ptr<float>(), grads[i]->ptr<const float>(), d1[i], d2[i]);
      if (rt[i]->ndim == 1) hipLaunchKernelGGL((shampoo_col_sumsq_kernel<float>), dim3((unsigned)((d2[i] + 255) / 256)), dim3(256), 0, st, rt[i]->ptr<float>(), grads[i]->ptr<const float>(), d1[i], d2[i]);
    } else {
      if (lt[i]->ndim == 1) hipLaunchKernelGGL((shampoo_row_sumsq_kernel<double>), dim3((unsigned)((d1[i] + 3) / 4)), dim3(256), 0, st, lt[i]->ptr<double>(), grads[i]->ptr<const double>(), d1[i], d2[i]);
      if (rt[i]->ndim == 1) hipLaunchKernelGGL((shampoo_col_sumsq_kernel<double>), dim3((unsigned)((d2[i] + 255) / 256)), dim3(256), 0, st, rt[i]->ptr<double>(), grads[i]->ptr<const double>(), d1[i], d2[i]);
    }
  }
  LAMP_LAUNCH_CHECK();
  // 3. the inverse fourth roots: on every step up to 100, then on every update_every-th (Shampoo.scala:137-139)
  if (!(step_count > 100 && step_count % update_every != 0)) {
    std::vector<lamp_tensor*> mats, invs;
    std::vector<Hold> vals, vecs;
    for (int i = 0; i < n; i++)
      for (int side = 0; side < 2; side++) {
        lamp_tensor* s = side ? rt[i] : lt[i];
        lamp_tensor* inv = side ? rtinv[i] : ltinv[i];
        if (s->ndim == 2) {
          mats.push_back(s); invs.push_back(inv);
          const int64_t vs[1] = {s->sizes[0]};
          vals.emplace_back(new_tensor(vs, 1, kF64, dev));
          if (paper_preconditioner) vecs.emplace_back(new_tensor(s->sizes, 2, kF64, dev));
        } else {
          const int64_t len = s->sizes[0];
          if (s->dtype == kF32) hipLaunchKernelGGL((shampoo_vec_root_kernel<float>), dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, inv->ptr<float>(), s->ptr<const float>(), len);
          else hipLaunchKernelGGL((shampoo_vec_root_kernel<double>), dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, inv->ptr<double>(), s->ptr<const double>(), len);
        }
      }
    LAMP_LAUNCH_CHECK();
    if (!mats.empty()) {
      std::vector<lamp_tensor*> vh, uh;
      for (auto& h : vals) vh.push_back(h.get());
      for (auto& h : vecs) uh.push_back(h.get());
      SH_CALL(lamp_symmetric_eig(mats.data(), (int)mats.size(), vh.data(), paper_preconditioner ? uh.data() : nullptr, nullptr));
      for (size_t k = 0; k < mats.size(); k++) {
        const int side = (int)mats[k]->sizes[0], blocks = std::min(1024, (side * side + 255) / 256);
        if (!paper_preconditioner) {
          if (invs[k]->dtype == kF32) hipLaunchKernelGGL((shampoo_diag_root_kernel<float>), dim3(blocks), dim3(256), 0, st, invs[k]->ptr<float>(), vh[k]->ptr<const double>(), side);
          else hipLaunchKernelGGL((shampoo_diag_root_kernel<double>), dim3(blocks), dim3(256), 0, st, invs[k]->ptr<double>(), vh[k]->ptr<const double>(), side);
        } else {
          Hold us(new_like(uh[k])), root(invs[k]->dtype == kF64 ? retain(invs[k]) : new_like(uh[k]));
          hipLaunchKernelGGL(shampoo_scale_cols_kernel, dim3(blocks), dim3(256), 0, st, us->ptr<double>(), uh[k]->ptr<const double>(), vh[k]->ptr<const double>(), side);
          SH_CALL(lamp_addmm_out_transposed2(root.get(), nullptr, us.get(), uh[k], 0.0, 1.0));       // (U diag(s^-1/4)) U^T in f64
          if (invs[k]->dtype != kF64) copy_into(invs[k], root.get());                               // ... cast to the gradient's dtype
        }
      }
      LAMP_LAUNCH_CHECK();
    }
  }
  // 4. p += -lr * ltinv G rtinv; the second product carries -lr and the accumulation in its epilogue
  for (int i = 0; i < n; i++) {
    const bool lm = lt[i]->ndim == 2, rm = rt[i]->ndim == 2;
    const int blocks = (int)std::min<int64_t>(4096, (d1[i] * d2[i] + 255) / 256);
    Hold t1;
    if (lm) { lamp_tensor* o = nullptr; SH_CALL(lamp_mm(&o, ltinv[i], g2[i].get())); t1 = Hold(o); }
    SH_DISPATCH(params[i]->dtype, T, {
      {
        if (!lm && rm) {
          t1 = Hold(new_like(g2[i].get()));
          hipLaunchKernelGGL((shampoo_scale_kernel<T>), dim3(blocks), dim3(256), 0, st, t1->ptr<T>(), grads[i]->ptr<const T>(), ltinv[i]->ptr<const T>(), (const T*)nullptr, d1[i], d2[i], T(1), 0);
        } else if (lm && !rm) {
          hipLaunchKernelGGL((shampoo_scale_kernel<T>), dim3(blocks), dim3(256), 0, st, params[i]->ptr<T>(), t1->ptr<const T>(), (const T*)nullptr, rtinv[i]->ptr<const T>(), d1[i], d2[i], (T)(-lr[i]), 1);
        } else if (!lm && !rm) {
          hipLaunchKernelGGL((shampoo_scale_kernel<T>), dim3(blocks), dim3(256), 0, st, params[i]->ptr<T>(), grads[i]->ptr<const T>(), ltinv[i]->ptr<const T>(), rtinv[i]->ptr<const T>(), d1[i], d2[i], (T)(-lr[i]), 1);
        }
      }
    });
    if (rm) SH_CALL(lamp_addmm_out(p2[i].get(), p2[i].get(), t1.get(), rtinv[i], 1.0, -lr[i]));
  }
  LAMP_LAUNCH_CHECK();
#undef SH_CALL
#undef SH_DISPATCH
  conv_repack_cached(params, n, st);      // the convolution weights' packed images follow the update (conv.hip)
  LAMP_API_END
}

int lamp_sgdw_step_(lamp_tensor* const* params, lamp_tensor* const* grads, lamp_tensor* const* velocity, int n, const double* lr,
                    const double* weight_decay, const double* momentum, double schedule_factor) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  const int dtype = params[0]->dtype, dev = params[0]->device();
  check_list(params, n, "parameters", dtype, dev);
  check_list(grads, n, "gradients", dtype, dev);
  std::vector<int64_t> numels(n);
  for (int i = 0; i < n; i++) {
    numels[i] = params[i]->numel();
    LAMP_CHECK(grads[i]->numel() == numels[i], "sgdw: size mismatch");
    if (velocity && velocity[i]) LAMP_CHECK(velocity[i]->numel() == numels[i] && velocity[i]->dtype == dtype && velocity[i]->is_contiguous(), "sgdw: bad velocity buffer");
  }
  hipStream_t st = current_stream(dev);
  LAMP_DISPATCH_FLOAT(dtype, T, for_each_group(n, numels.data(),
      [&](MultiArgs& a, int t, int gi) {
        a.p[0][t] = params[gi]->data(); a.p[1][t] = grads[gi]->data();
        a.p[2][t] = (velocity && velocity[gi]) ? velocity[gi]->data() : nullptr;
        a.h[0][t] = lr[gi] * schedule_factor; a.h[1][t] = weight_decay[gi] * schedule_factor; a.h[2][t] = momentum ? momentum[gi] : 0.0;
      },
      [&](MultiArgs& a, int blk) { hipLaunchKernelGGL((sgdw_kernel<T>), dim3(blk), dim3(256), 0, st, a); }));
  LAMP_LAUNCH_CHECK();
  conv_repack_cached(params, n, st);
  LAMP_API_END
}

int lamp_flatten_into_(lamp_tensor* bucket, lamp_tensor* const* ts, int n, double scale) {
  LAMP_API_BEGIN
  LAMP_CHECK(bucket, "bucket is null");
  LAMP_CHECK(bucket->dtype == kF32 && bucket->is_contiguous(), "the gradient bucket must be a contiguous f32 tensor");
  if (n == 0) return 0;
  std::vector<int64_t> numels(n), offs(n);
  int64_t off = 0;
  for (int i = 0; i < n; i++) { LAMP_CHECK(ts[i], "null tensor in the list"); numels[i] = ts[i]->numel(); offs[i] = off; off += numels[i]; }
  LAMP_CHECK(off <= bucket->numel(), "bucket too small: " << bucket->numel() << " < " << off);
  if (all_host(bucket, ts, n)) {
    LAMP_DISPATCH_FLOAT(ts[0]->dtype, T, host_flatten<T>(bucket->ptr<float>(), ts, n, offs, scale));
    return 0;
  }
  check_device_tensor(bucket, "bucket");
  const int dtype = ts[0]->dtype, dev = bucket->device();
  check_list(ts, n, "tensors", dtype, dev);
  hipStream_t st = current_stream(dev);
  LAMP_DISPATCH_FLOAT(dtype, T, for_each_group(n, numels.data(),
      [&](MultiArgs& a, int t, int gi) { a.p[0][t] = ts[gi]->data(); a.h[0][t] = (double)offs[gi]; a.s[0] = scale; },
      [&](MultiArgs& a, int blk) { hipLaunchKernelGGL((mt_flatten_kernel<T>), dim3(blk), dim3(256), 0, st, a, bucket->ptr<float>()); }));
  LAMP_LAUNCH_CHECK();
  LAMP_API_END
}

int lamp_unflatten_from_(lamp_tensor* const* ts, int n, const lamp_tensor* bucket, int divide_by_last_element) {
  LAMP_API_BEGIN
  LAMP_CHECK(bucket, "bucket is null");
  LAMP_CHECK(bucket->dtype == kF32 && bucket->is_contiguous(), "the gradient bucket must be a contiguous f32 tensor");
  if (n == 0) return 0;
  std::vector<int64_t> numels(n), offs(n);
  int64_t off = 0;
  for (int i = 0; i < n; i++) { LAMP_CHECK(ts[i], "null tensor in the list"); numels[i] = ts[i]->numel(); offs[i] = off; off += numels[i]; }
  LAMP_CHECK(off <= bucket->numel(), "bucket too small");
  const int64_t last = divide_by_last_element ? bucket->numel() - 1 : -1;
  if (all_host(bucket, ts, n)) {
    LAMP_DISPATCH_FLOAT(ts[0]->dtype, T, host_unflatten<T>(ts, n, bucket->ptr<float>(), offs, last));
    return 0;
  }
  check_device_tensor(bucket, "bucket");
  const int dtype = ts[0]->dtype, dev = bucket->device();
  check_list(ts, n, "tensors", dtype, dev);
  hipStream_t st = current_stream(dev);
  LAMP_DISPATCH_FLOAT(dtype, T, for_each_group(n, numels.data(),
      [&](MultiArgs& a, int t, int gi) { a.p[0][t] = ts[gi]->data(); a.h[0][t] = (double)offs[gi]; },
      [&](MultiArgs& a, int blk) { hipLaunchKernelGGL((mt_unflatten_kernel<T>), dim3(blk), dim3(256), 0, st, a, bucket->ptr<float>(), last); }));
  LAMP_LAUNCH_CHECK();
  LAMP_API_END
}

// The running mean of the weight average, in place on the accumulator (swa_average_kernel): one launch per MT_MAX tensors per dtype.
int lamp_swa_average_(lamp_tensor* const* avg, lamp_tensor* const* cur, int n, int64_t number_of_averaged_models) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  LAMP_CHECK(number_of_averaged_models >= 0, "swa_average: numberOfAveragedModels must not be negative, got " << number_of_averaged_models);
  check_state_pair("swa_average", "accumulator", avg, "current", cur, n, true);
  hipStream_t st = current_stream(avg[0]->device());
  for_each_class(avg, std::vector<int>(n, 0), 1, [&](int dt, const std::vector<int>& sel) {
    std::vector<int64_t> numels(sel.size());
    for (size_t k = 0; k < sel.size(); k++) numels[k] = avg[sel[k]]->numel();
    auto fill = [&](MultiArgs& a, int t, int gi) {
      a.p[0][t] = avg[sel[gi]]->data(); a.p[1][t] = cur[sel[gi]]->data();
      a.s[0] = (double)number_of_averaged_models;
      a.s[1] = (double)(number_of_averaged_models + 1);
    };
    LAMP_DISPATCH_FLOAT(dt, T, for_each_group((int)sel.size(), numels.data(), fill, [&](MultiArgs& a, int blk) {
      const double elems = (double)mt_elements(a);
      KernelTimer kt("swa_average", 3.0 * elems, 3.0 * elems * sizeof(T), st);
      hipLaunchKernelGGL((swa_average_kernel<T>), dim3(blk), dim3(256), 0, st, a);
    }));
    LAMP_LAUNCH_CHECK();
  });
  LAMP_API_END
}

// dst[i] <- src[i] for n tensor pairs of any dtype (state_copy_kernel): one launch per MT_MAX tensors per element size.  The snapshot
// of a module's state, its restore, and Module.load from tensors that already live on the module's device in its dtypes.
int lamp_state_copy_(lamp_tensor* const* dst, lamp_tensor* const* src, int n) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  check_state_pair("state_copy", "destination", dst, "source", src, n, false);
  hipStream_t st = current_stream(dst[0]->device());
  for (size_t width : {(size_t)1, (size_t)2, (size_t)4, (size_t)8}) {
    std::vector<int> sel;
    for (int i = 0; i < n; i++) if (dst[i]->itemsize() == width) sel.push_back(i);
    if (sel.empty()) continue;
    std::vector<int64_t> numels(sel.size());
    for (size_t k = 0; k < sel.size(); k++) numels[k] = dst[sel[k]]->numel();
    auto fill = [&](MultiArgs& a, int t, int gi) { a.p[0][t] = dst[sel[gi]]->data(); a.p[1][t] = src[sel[gi]]->data(); };
    auto launch = [&](MultiArgs& a, int blk) {
      KernelTimer kt("state_copy", 0, 2.0 * (double)mt_elements(a) * (double)width, st);
      if (width == 1) hipLaunchKernelGGL((state_copy_kernel<uint8_t>), dim3(blk), dim3(256), 0, st, a);
      else if (width == 2) hipLaunchKernelGGL((state_copy_kernel<uint16_t>), dim3(blk), dim3(256), 0, st, a);
      else if (width == 4) hipLaunchKernelGGL((state_copy_kernel<uint32_t>), dim3(blk), dim3(256), 0, st, a);
      else hipLaunchKernelGGL((state_copy_kernel<uint64_t>), dim3(blk), dim3(256), 0, st, a);
    };
    for_each_group((int)sel.size(), numels.data(), fill, launch);
    LAMP_LAUNCH_CHECK();
  }
  LAMP_API_END
}

}  // extern "C"
