// Language-model decode: one new token per row against a key / value cache (host/generate.cpp; the reference generates a token by running the
// whole model over the whole prefix, lamp-data/src/main/scala/lamp/data/languagemodel/package.scala:35-114).  f32, f64 and bf16; bf16
// accumulates in f32, f64 in f64.  R <= 16 rows make every product a weight-streaming problem: the weights go from memory to registers in
// 16-byte packets, there is no matrix-pipe tile and no LDS round trip for them.
//
//   decode_linear_kn_kernel   out = residual + scale * act(LN(x) . W + bias), W [K, N]: an operation of the body decode_stream_body.h (which
//                             holds the stream loop, the wave and slab reductions and the ticket protocol).  The operation works out the
//                             rows' statistics, gives LN(x) as the image and applies the epilogue to a lane's one packet of columns.
//   decode_linear_nk_kernel   the same for W [N, K] (logits against the embedding table): a wave per column, the lanes split K in packets, the
//                             64 sums are added by the fixed butterfly of wave_sum.
//   decode_attention_kernel   a workgroup per (row, head): copies the new key and value into position t, scores q . K^T over 0 .. t (a group of
//                             lanes per position, the new key taken from qkv), exp(log_softmax) through LDS, then P . V with the columns across
//                             the lanes and the positions dealt to 256 / d groups whose sums are added in group order.
//   sample_logits_kernel      a workgroup per row: maximum, exp((l - max) / temperature) in f64, the threads' contiguous shares scanned as
//                             multinomial_cdf_kernel scans them, first index whose running sum exceeds u * total.
//   decode_embedding_kernel   tokenWeight[token] + positionWeight[t]
// No kernel uses a floating atomic and every sum has a fixed order: the results are functions of the inputs, bit for bit.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), decode_linear_kn_kernel at 1 / 2 .. 4 / 5 .. 16 rows:
//   packet form (bf16 x 8, f32 x 4, f64 x 2 columns)  bf16 104 / 128 / 242 VGPRs    f32  66 /  76 / 136     f64  68 /  88 / 136
//   element form                                      bf16  46 /  66 /  76          f32  44 /  66 /  72     f64  60 /  64 /  82
// (bf16 at 5 .. 16 rows: 128 sums and 8 packets in flight, two waves per SIMD).  No kernel of this file uses scratch memory.
#include <cstdio>
#include <cstring>
#include "decode_stream.h"
#include "philox.h"

namespace lamp {
namespace {

constexpr int kDecNkWaves = 4;        // columns per workgroup of the [N, K] kernel
constexpr int kDecAttUnroll = 4;      // positions per lane group of the attention kernel whose key loads are in flight together

template <class T> struct DecLinear {
  const T* x; const T* w; T* out;
  const T* lnScale; const T* lnBias; const T* bias; const T* scale; const T* residual;
  acc_t<T>* slab; unsigned* ticket;
  int64_t K, N;
  int R, Kc, S, ln, act;
  double eps;
};

// bias, activation, scale and residual in acc_t on the sum itself, one rounding at the store: nothing between the product and the output
// of a launch is a stored activation
template <class T>
__device__ __forceinline__ T dec_epilogue(acc_t<T> a, int64_t r, int64_t n, const DecLinear<T>& p) {
  using A = acc_t<T>;
  if (p.bias) a += load_as<A>(p.bias[n]);
  if (p.act == LAMP_DECODE_ACT_GELU) a = a * A(0.5) * (A(1) + dec_erf(a * A(0.70710678118654752440)));
  if (p.scale) a = a * load_as<A>(p.scale[n]) + load_as<A>(p.residual[r * p.N + n]);
  return store_as<T>(a);
}

template <class T>
__device__ __forceinline__ acc_t<T> dec_normalise(acc_t<T> v, acc_t<T> mu, acc_t<T> rstd, const T* lnScale, const T* lnBias, int64_t k) {
  using A = acc_t<T>;
  v = (v - mu) * rstd;
  if (lnScale) v *= load_as<A>(lnScale[k]);
  if (lnBias) v += load_as<A>(lnBias[k]);
  return v;
}

// the statistics of the rows wave, wave + W, ... (W waves in the workgroup) into stat[2 r], stat[2 r + 1]: the loads of all of a wave's rows
// are in flight together, two passes
template <class T, int RT, int W>
__device__ __forceinline__ void dec_stats(const T* __restrict__ x, int64_t K, int R, double eps, int lane, int wave, acc_t<T>* stat) {
  using A = acc_t<T>;
  constexpr int RW = (RT + W - 1) / W;
  A s[RW], mu[RW];
#pragma unroll
  for (int q = 0; q < RW; q++) s[q] = A(0);
  for (int64_t k = lane; k < K; k += 64)
#pragma unroll
    for (int q = 0; q < RW; q++) { const int r = wave + W * q; if (r < R) s[q] += load_as<A>(x[(int64_t)r * K + k]); }
#pragma unroll
  for (int q = 0; q < RW; q++) { mu[q] = wave_sum(s[q]) / (A)K; s[q] = A(0); }
  for (int64_t k = lane; k < K; k += 64)
#pragma unroll
    for (int q = 0; q < RW; q++) {
      const int r = wave + W * q;
      if (r < R) { const A dlt = load_as<A>(x[(int64_t)r * K + k]) - mu[q]; s[q] += dlt * dlt; }
    }
#pragma unroll
  for (int q = 0; q < RW; q++) {
    const int r = wave + W * q;
    const A m2 = wave_sum(s[q]);
    if (r < R && lane == 0) { stat[2 * r] = mu[q]; stat[2 * r + 1] = A(1) / (A)sqrt((double)(m2 / (A)K + (A)eps)); }
  }
}

// ---- W [K, N] -------------------------------------------------------------------------------------------------------------------------------
// the operation of decode_stream_body.h: the image is LN(x), a finished sum goes through dec_epilogue.  V > 1 only when N % V == 0 and
// W is 16-byte aligned.
template <class T, int V, int RT> struct DecLinearOp {
  using A = acc_t<T>;
  const DecLinear<T>& p;
  A* stat;                            // LDS [2 RT]: mean and 1 / std of the rows
  __device__ __forceinline__ void prepare(int tid, int lane, int wave) {
    if (p.ln) {
      dec_stats<T, RT, kDecWaves>(p.x, p.K, p.R, p.eps, lane, wave, stat);
      __syncthreads();
    }
  }
  __device__ __forceinline__ A image(int r, int64_t k) const {
    A v = load_as<A>(p.x[(int64_t)r * p.K + k]);
    if (p.ln) v = dec_normalise<T>(v, stat[2 * r], stat[2 * r + 1], p.lnScale, p.lnBias, k);
    return v;
  }
  __device__ __forceinline__ void finish(const A (&a)[V], int r, int64_t n0) const {
#pragma unroll
    for (int j = 0; j < V; j++) p.out[(int64_t)r * p.N + n0 + j] = dec_epilogue<T>(a[j], r, n0 + j, p);
  }
};
template <class T, int V, int RT>
__global__ __launch_bounds__(64 * kDecWaves) void decode_linear_kn_kernel(DecLinear<T> p) {
  __shared__ acc_t<T> stat[2 * RT];
  DecLinearOp<T, V, RT> op{p, stat};
  constexpr int CL = V;
  const int64_t K = p.K;
#include "decode_stream_body.h"
}

// ---- W [N, K] -------------------------------------------------------------------------------------------------------------------------------
// grid ceil(N / kDecNkWaves), 64 * kDecNkWaves threads: a wave per column.  V > 1 only when K % V == 0 and x, W (and the norm's vectors) are
// 16-byte aligned.
template <class T, int V, int RT>
__global__ __launch_bounds__(64 * kDecNkWaves) void decode_linear_nk_kernel(DecLinear<T> p) {
  using A = acc_t<T>;
  __shared__ A stat[2 * RT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t K = p.K, N = p.N;
  const int R = p.R;
  if (p.ln) {
    dec_stats<T, RT, kDecNkWaves>(p.x, K, R, p.eps, lane, wave, stat);
    __syncthreads();
  }
  const int64_t n = (int64_t)blockIdx.x * kDecNkWaves + wave;
  if (n >= N) return;
  A acc[RT];
#pragma unroll
  for (int r = 0; r < RT; r++) acc[r] = A(0);
  const T* wr = p.w + n * K;
  for (int64_t k = (int64_t)lane * V; k < K; k += 64 * V) {
    const Vec<T, V> wv = load_packet<T, V>(wr + k);
#pragma unroll
    for (int r = 0; r < RT; r++) {
      if (r < R) {
        const Vec<T, V> xv = load_packet<T, V>(p.x + (int64_t)r * K + k);
#pragma unroll
        for (int j = 0; j < V; j++) {
          A v = load_as<A>(xv.v[j]);
          if (p.ln) v = dec_normalise<T>(v, stat[2 * r], stat[2 * r + 1], p.lnScale, p.lnBias, k + j);
          acc[r] += v * load_as<A>(wv.v[j]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RT; r++) {
    if (r < R) {
      const A s = wave_sum(acc[r]);
      if (lane == 0) p.out[(int64_t)r * N + n] = dec_epilogue<T>(s, r, n, p);
    }
  }
}

// ---- attention over the cache ---------------------------------------------------------------------------------------------------------------
// grid (H, R), 256 threads; dynamic LDS: q [d], scores [t + 1], partial sums [256], reduction scratch [4], all acc_t.
// lpr: lanes per position, a power of two <= 64 with lpr * V >= min(d, 64 * V).  V > 1 only when d % V == 0 and qkv and the caches are aligned.
template <class T, int V>
__global__ __launch_bounds__(256) void decode_attention_kernel(const T* __restrict__ qkv, T* __restrict__ kcache, T* __restrict__ vcache, T* __restrict__ out,
                                                               int64_t H, int64_t d, int64_t Tmax, int64_t t, int lpr, acc_t<T> invSqrtD) {
  using A = acc_t<T>;
  extern __shared__ __align__(16) unsigned char dec_smem[];
  A* q = reinterpret_cast<A*>(dec_smem);
  A* sc = q + d;
  A* part = sc + (t + 1);
  A* red = part + 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = blockIdx.y, h = blockIdx.x, HD = H * d;
  const T* qrow = qkv + r * 3 * HD + h * d;
  const T* krow = qrow + HD;
  const T* vrow = qrow + 2 * HD;
  T* kbase = kcache + (r * H + h) * Tmax * d;
  T* vbase = vcache + (r * H + h) * Tmax * d;
  for (int64_t c = tid; c < d; c += 256) {
    q[c] = load_as<A>(qrow[c]);
    kbase[t * d + c] = krow[c];
    vbase[t * d + c] = vrow[c];
  }
  __syncthreads();
  // scores: the new position is read from qkv, so no thread depends on another's store to the cache
  const int rpw = 64 / lpr, sub = lane / lpr, sl = lane - sub * lpr;
  for (int64_t j0 = (int64_t)wave * rpw; j0 <= t; j0 += 4 * rpw * kDecAttUnroll) {
    A a[kDecAttUnroll];               // kDecAttUnroll positions per group of lanes: their loads are in flight together
#pragma unroll
    for (int u = 0; u < kDecAttUnroll; u++) {
      const int64_t j = j0 + (int64_t)u * 4 * rpw + sub;
      a[u] = A(0);
      if (j <= t) {
        const T* kr = j == t ? krow : kbase + j * d;
        for (int64_t c = (int64_t)sl * V; c < d; c += (int64_t)lpr * V) {
          const Vec<T, V> kv = load_packet<T, V>(kr + c);
#pragma unroll
          for (int i = 0; i < V; i++) a[u] += q[c + i] * load_as<A>(kv.v[i]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kDecAttUnroll; u++) {
      const int64_t j = j0 + (int64_t)u * 4 * rpw + sub;
      for (int off = lpr >> 1; off > 0; off >>= 1) a[u] += __shfl_xor(a[u], off, 64);
      if (j <= t && sl == 0) sc[j] = a[u] * invSqrtD;
    }
  }
  __syncthreads();
  // maskedSoftmax: exp(logSoftMax(scores)), in acc_t
  A m = -INFINITY;
  for (int64_t j = tid; j <= t; j += 256) m = sc[j] > m ? sc[j] : m;
  m = block_max(m, red);
  A ssum = A(0);
  for (int64_t j = tid; j <= t; j += 256) ssum += dec_exp(sc[j] - m);
  ssum = block_sum(ssum, red);
  const A lse = dec_log(ssum);
  for (int64_t j = tid; j <= t; j += 256) sc[j] = dec_exp((sc[j] - m) - lse);
  __syncthreads();
  // P . V: thread (g, c) sums the positions j = g, g + ng, ...; the groups' sums are added in group order
  const int ng = (int)(256 / d), g = (int)(tid / d), c = (int)(tid - g * d);
  A a = A(0);
  if (g < ng)
#pragma unroll 8
    for (int64_t j = g; j <= t; j += ng) {
      const T* vr = j == t ? vrow : vbase + j * d;
      a += sc[j] * load_as<A>(vr[c]);
    }
  part[tid] = a;
  __syncthreads();
  if (tid < d) {
    A s = A(0);
    for (int g2 = 0; g2 < ng; g2++) s += part[g2 * d + tid];
    out[r * HD + h * d + tid] = store_as<T>(s);
  }
}

// ---- sampler --------------------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void sample_logits_kernel(const T* __restrict__ logits, int64_t V, double temperature, const double* __restrict__ uniforms,
                                                            int64_t* __restrict__ out, int64_t ostride, uint64_t seed, uint64_t offset,
                                                            int* __restrict__ assert_word) {
  __shared__ double part[256];
  __shared__ double red[4];
  __shared__ long long found[256];
  __shared__ double total;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const T* lr = logits + row * V;
  const int64_t per = (V + 255) / 256, b = min((int64_t)tid * per, V), e = min(b + per, V);
  double m = -INFINITY;
  int bad = 0;
  for (int64_t i = b; i < e; i++) {
    const double v = (double)load_as<acc_t<T>>(lr[i]);
    if (!(fabs(v) <= 1.7e308)) bad = 1;
    m = fmax(m, v);
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid == 0) { *(volatile int*)assert_word = kAssertSampleLogits; out[row * ostride] = 0; }
    return;
  }
  m = block_max(m, red);
  double s = 0.0;
  for (int64_t i = b; i < e; i++) s += exp(((double)load_as<acc_t<T>>(lr[i]) - m) / temperature);
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int k = 0; k < 256; k++) { const double v = part[k]; part[k] = run; run += v; }
    total = run;
  }
  __syncthreads();
  double u;
  if (uniforms) u = uniforms[row];
  else { Philox ph(seed, (uint64_t)row, offset); const uint4 qd = ph.next(); u = u01(qd.x, qd.y); }
  const double target = u * total;
  double run = part[tid];
  long long f = V;
  for (int64_t i = b; i < e; i++) {
    run += exp(((double)load_as<acc_t<T>>(lr[i]) - m) / temperature);
    if (run > target) { f = i; break; }
  }
  found[tid] = f;
  __syncthreads();
  if (tid == 0) {
    long long first = V - 1;          // the shares ascend with the thread: the first thread that found one holds the first index
    for (int k = 0; k < 256; k++) if (found[k] < V) { first = found[k]; break; }
    out[row * ostride] = first;
  }
}

// ---- embedding of the new token -------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void decode_embedding_kernel(const T* __restrict__ tokW, const T* __restrict__ posW, const int64_t* __restrict__ tokens,
                                                               int64_t tstride, T* __restrict__ out, int64_t R, int64_t D, int64_t Vt, int64_t t,
                                                               int* __restrict__ assert_word) {
  using A = acc_t<T>;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < R * D; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D, c = i - r * D;
    const int64_t tok = tokens[r * tstride];
    A v = A(0);
    if (tok >= 0 && tok < Vt) v = load_as<A>(tokW[tok * D + c]);   // the bound is tested before an address is formed
    else *(volatile int*)assert_word = kAssertIndexRange;
    out[i] = store_as<T>(v + load_as<A>(posW[t * D + c]));
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
bool dec_dtype(int dt) { return dt == kF32 || dt == kF64 || dt == kBF16; }
// p holds the operands and R, K, N; the tiling is decided here
template <class T>
void dec_linear_run(DecLinear<T> p, bool transposed, int dev, hipStream_t st) {
  constexpr int VW = 16 / (int)sizeof(T);
  if (transposed) {
    const bool vec = p.K % VW == 0 && dec_aligned({p.x, p.w, p.lnScale, p.lnBias});
    const dim3 grid((unsigned)((p.N + kDecNkWaves - 1) / kDecNkWaves));
    dec_rt_ladder(p.R, [&](auto rt) {
      constexpr int RT = decltype(rt)::value;
      if (vec) hipLaunchKernelGGL((decode_linear_nk_kernel<T, VW, RT>), grid, dim3(64 * kDecNkWaves), 0, st, p);
      else hipLaunchKernelGGL((decode_linear_nk_kernel<T, 1, RT>), grid, dim3(64 * kDecNkWaves), 0, st, p);
    });
    return;
  }
  const DecForm f = dec_form(kDecFormLinear, p.N, sizeof(T), dec_aligned({p.w}));
  const DecPlan pl = dec_plan(p.K, p.N, p.R, f.CL, sizeof(T), sizeof(acc_t<T>), num_cus());
  Hold slab;
  dec_plan_apply<acc_t<T>>(p, pl, dev, st, slab);
  dec_rt_ladder(p.R, [&](auto rt) {
    constexpr int RT = decltype(rt)::value;
    if (f.V > 1) hipLaunchKernelGGL((decode_linear_kn_kernel<T, VW, RT>), pl.grid, pl.block, 0, st, p);
    else hipLaunchKernelGGL((decode_linear_kn_kernel<T, 1, RT>), pl.grid, pl.block, 0, st, p);
  });
}

}  // namespace
}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_decode_linear(lamp_tensor** out, const lamp_tensor* x, const lamp_tensor* w, int transposed, int layer_norm, double ln_eps,
                       const lamp_tensor* ln_scale_or_null, const lamp_tensor* ln_bias_or_null, const lamp_tensor* bias_or_null, int act,
                       const lamp_tensor* scale_or_null, const lamp_tensor* residual_or_null) {
  LAMP_API_BEGIN
  check_device_tensor(x, "x"); check_device_tensor(w, "w");
  const int dt = x->dtype, dev = x->device();
  LAMP_CHECK(dec_dtype(dt), "f32, f64 or bf16, got " << x->describe());
  LAMP_CHECK(x->ndim == 2 && w->ndim == 2 && w->dtype == dt && w->device() == dev, "x must be [R, K] and w a matrix of its type and device, got "
                                                                                        << x->describe() << " and " << w->describe());
  const int64_t R = x->sizes[0], K = x->sizes[1], N = transposed ? w->sizes[0] : w->sizes[1];
  LAMP_CHECK(R >= 1 && R <= kDecMaxRows, R << " rows: this is the kernel of 1 .. " << kDecMaxRows << " rows, larger products are lamp_mm's");
  LAMP_CHECK((transposed ? w->sizes[1] : w->sizes[0]) == K && K >= 1 && N >= 1, "x " << x->describe() << " does not multiply w " << w->describe()
                                                                                     << (transposed ? " transposed" : ""));
  LAMP_CHECK(act == LAMP_DECODE_ACT_NONE || act == LAMP_DECODE_ACT_GELU, "act must be LAMP_DECODE_ACT_NONE or LAMP_DECODE_ACT_GELU");
  LAMP_CHECK((scale_or_null == nullptr) == (residual_or_null == nullptr), "scale and residual come together");
  LAMP_CHECK(layer_norm || (!ln_scale_or_null && !ln_bias_or_null), "ln_scale / ln_bias without layer_norm");
  auto vector_arg = [&](const lamp_tensor* v, const char* what, int64_t n, bool row_ok) {
    if (!v) return;
    check_device_tensor(v, what);
    LAMP_CHECK(v->dtype == dt && v->device() == dev && v->numel() == n && (v->ndim == 1 || (row_ok && v->ndim == 2 && v->sizes[0] == 1)),
               what << " must hold " << n << " elements of x's type, got " << v->describe());
  };
  vector_arg(ln_scale_or_null, "ln_scale", K, false); vector_arg(ln_bias_or_null, "ln_bias", K, false);
  vector_arg(bias_or_null, "bias", N, true); vector_arg(scale_or_null, "scale", N, false);
  if (residual_or_null) {
    check_device_tensor(residual_or_null, "residual");
    LAMP_CHECK(residual_or_null->dtype == dt && residual_or_null->device() == dev && residual_or_null->ndim == 2 && residual_or_null->sizes[0] == R &&
                   residual_or_null->sizes[1] == N, "residual must be [" << R << ", " << N << "] of x's type, got " << residual_or_null->describe());
  }
  Hold xc(contiguous(x)), wc(contiguous(w));
  Hold lsc(ln_scale_or_null ? contiguous(ln_scale_or_null) : nullptr), lbc(ln_bias_or_null ? contiguous(ln_bias_or_null) : nullptr);
  Hold bc(bias_or_null ? contiguous(bias_or_null) : nullptr), sc(scale_or_null ? contiguous(scale_or_null) : nullptr);
  Hold rc(residual_or_null ? contiguous(residual_or_null) : nullptr);
  int64_t os[2] = {R, N};
  Hold o(new_tensor(os, 2, dt, dev));
  hipStream_t st = current_stream(dev);
  const double sz = (double)dtype_size(dt);
  KernelTimer kt(transposed ? "decode_linear_nk" : "decode_linear_kn", 2.0 * R * K * N, ((double)K * N + (double)R * (K + N)) * sz, st);
#define DEC_LINEAR(T)                                                                                                                   \
  {                                                                                                                                     \
    DecLinear<T> p{};                                                                                                                   \
    p.x = xc->ptr<T>(); p.w = wc->ptr<T>(); p.out = o->ptr<T>();                                                                        \
    p.lnScale = lsc.get() ? lsc->ptr<T>() : nullptr; p.lnBias = lbc.get() ? lbc->ptr<T>() : nullptr;                                    \
    p.bias = bc.get() ? bc->ptr<T>() : nullptr; p.scale = sc.get() ? sc->ptr<T>() : nullptr;                                            \
    p.residual = rc.get() ? rc->ptr<T>() : nullptr;                                                                                     \
    p.K = K; p.N = N; p.R = (int)R; p.ln = layer_norm ? 1 : 0; p.act = act; p.eps = ln_eps;                                             \
    dec_linear_run<T>(p, transposed != 0, dev, st);                                                                                     \
  }
  switch (dt) {
    case kF32: DEC_LINEAR(float) break;
    case kF64: DEC_LINEAR(double) break;
    default: DEC_LINEAR(bf16_t) break;
  }
#undef DEC_LINEAR
  LAMP_LAUNCH_CHECK();
  *out = o.take();
  LAMP_API_END
}

int lamp_decode_attention(lamp_tensor** out, const lamp_tensor* qkv, lamp_tensor* kcache, lamp_tensor* vcache, int64_t t, int64_t num_heads) {
  LAMP_API_BEGIN
  check_device_tensor(qkv, "qkv"); check_device_tensor(kcache, "kcache"); check_device_tensor(vcache, "vcache");
  const int dt = qkv->dtype, dev = qkv->device();
  LAMP_CHECK(dec_dtype(dt), "f32, f64 or bf16, got " << qkv->describe());
  LAMP_CHECK(qkv->ndim == 2 && num_heads >= 1 && qkv->sizes[1] % (3 * num_heads) == 0 && qkv->sizes[1] > 0,
             "qkv must be [R, 3 * " << num_heads << " * d], got " << qkv->describe());
  const int64_t R = qkv->sizes[0], H = num_heads, d = qkv->sizes[1] / (3 * H);
  LAMP_CHECK(R >= 1 && R <= 65535 && d <= 256, "R = " << R << ", d = " << d << ": at most 65535 rows and 256 values per head");
  for (const lamp_tensor* c : {(const lamp_tensor*)kcache, (const lamp_tensor*)vcache})
    LAMP_CHECK(c->dtype == dt && c->device() == dev && c->ndim == 4 && c->sizes[0] == R && c->sizes[1] == H && c->sizes[3] == d && c->is_contiguous() &&
                   c->sizes[2] == kcache->sizes[2], "the caches must be contiguous [" << R << ", " << H << ", Tmax, " << d << "] of qkv's type, got " << c->describe());
  const int64_t Tmax = kcache->sizes[2];
  LAMP_CHECK(t >= 0 && t < Tmax, "position " << t << " is outside a cache of " << Tmax);
  Hold qc(contiguous(qkv));
  int64_t os[2] = {R, H * d};
  Hold o(new_tensor(os, 2, dt, dev));
  hipStream_t st = current_stream(dev);
  const int vw = (int)(16 / dtype_size(dt));
  const size_t asz = dt == kF64 ? 8 : 4;
  const size_t lds = (size_t)(d + (t + 1) + 256 + 4) * asz;
  LAMP_CHECK(lds <= 48 * 1024, "a cache of " << (t + 1) << " positions does not fit the kernel's LDS");
  const bool vec = d % vw == 0 && dec_aligned({qc->raw(), kcache->raw(), vcache->raw()});
  const int V = vec ? vw : 1;
  int lpr = 1;
  while (lpr < 64 && (int64_t)lpr * V < d) lpr <<= 1;
  const double sz = (double)dtype_size(dt);
  KernelTimer kt("decode_attention", 4.0 * R * H * (t + 1) * d, (2.0 * R * H * (t + 1) * d + 4.0 * R * H * d) * sz, st);
  const double inv = 1.0 / std::sqrt((double)d);
#define DEC_ATT(T, VV) hipLaunchKernelGGL((decode_attention_kernel<T, VV>), dim3((unsigned)H, (unsigned)R), dim3(256), lds, st, qc->ptr<T>(), kcache->ptr<T>(), \
                                          vcache->ptr<T>(), o->ptr<T>(), H, d, Tmax, t, lpr, (acc_t<T>)inv)
  switch (dt) {
    case kF32: if (vec) DEC_ATT(float, 4); else DEC_ATT(float, 1); break;
    case kF64: if (vec) DEC_ATT(double, 2); else DEC_ATT(double, 1); break;
    default: if (vec) DEC_ATT(bf16_t, 8); else DEC_ATT(bf16_t, 1); break;
  }
#undef DEC_ATT
  LAMP_LAUNCH_CHECK();
  *out = o.take();
  LAMP_API_END
}

int lamp_sample_logits_out(lamp_tensor* out, const lamp_tensor* logits, double temperature, const lamp_tensor* uniforms_or_null) {
  LAMP_API_BEGIN
  check_device_tensor(logits, "logits"); check_device_tensor(out, "out");
  const int dt = logits->dtype, dev = logits->device();
  LAMP_CHECK(dec_dtype(dt), "f32, f64 or bf16 logits, got " << logits->describe());
  LAMP_CHECK(logits->ndim == 2 && logits->sizes[1] >= 1, "logits must be [R, V], got " << logits->describe());
  LAMP_CHECK(temperature > 0.0, "temperature must be positive, got " << temperature);
  const int64_t R = logits->sizes[0], V = logits->sizes[1];
  LAMP_CHECK(out->dtype == kI64 && out->device() == dev && out->numel() == R, "out must hold " << R << " int64 elements on the logits' device, got " << out->describe());
  const int64_t ostride = dec_vector_stride(out, "out must be a vector or one column of a matrix");
  if (uniforms_or_null) {
    check_device_tensor(uniforms_or_null, "uniforms");
    LAMP_CHECK(uniforms_or_null->dtype == kF64 && uniforms_or_null->device() == dev && uniforms_or_null->numel() == R && uniforms_or_null->is_contiguous(),
               "uniforms must be contiguous f64 [" << R << "], got " << uniforms_or_null->describe());
  }
  if (R == 0) return 0;
  Hold lc(contiguous(logits));
  hipStream_t st = current_stream(dev);
  const uint64_t off = uniforms_or_null ? 0 : next_philox_offset(2);
  KernelTimer kt("sample_logits", 3.0 * R * V, 3.0 * R * V * (double)dtype_size(dt) + 16.0 * R, st);
#define DEC_SAMPLE(T) hipLaunchKernelGGL((sample_logits_kernel<T>), dim3((unsigned)R), dim3(256), 0, st, lc->ptr<T>(), V, temperature,                           \
                                         uniforms_or_null ? uniforms_or_null->ptr<double>() : (const double*)nullptr, out->ptr<int64_t>(), ostride, philox_seed(), \
                                         off, device_assert_word(dev))
  switch (dt) {
    case kF32: DEC_SAMPLE(float); break;
    case kF64: DEC_SAMPLE(double); break;
    default: DEC_SAMPLE(bf16_t); break;
  }
#undef DEC_SAMPLE
  LAMP_LAUNCH_CHECK();
  LAMP_API_END
}

int lamp_sample_logits(lamp_tensor** out, const lamp_tensor* logits, double temperature, const lamp_tensor* uniforms_or_null) {
  LAMP_API_BEGIN
  check_device_tensor(logits, "logits");
  LAMP_CHECK(logits->ndim == 2, "logits must be [R, V], got " << logits->describe());
  int64_t os[1] = {logits->sizes[0]};
  Hold o(new_tensor(os, 1, kI64, logits->device()));
  LAMP_CHECK(lamp_sample_logits_out(o.get(), logits, temperature, uniforms_or_null) == 0, lamp_last_error());
  *out = o.take();
  LAMP_API_END
}

int lamp_decode_embedding(lamp_tensor** out, const lamp_tensor* tokenWeight, const lamp_tensor* positionWeight, const lamp_tensor* tokens, int64_t t) {
  LAMP_API_BEGIN
  check_device_tensor(tokenWeight, "tokenWeight"); check_device_tensor(positionWeight, "positionWeight"); check_device_tensor(tokens, "tokens");
  const int dt = tokenWeight->dtype, dev = tokenWeight->device();
  LAMP_CHECK(dec_dtype(dt), "f32, f64 or bf16 tables, got " << tokenWeight->describe());
  LAMP_CHECK(tokenWeight->ndim == 2 && positionWeight->ndim == 2 && positionWeight->dtype == dt && positionWeight->sizes[1] == tokenWeight->sizes[1] &&
                 positionWeight->device() == dev, "the tables must be [V, D] and [L, D] of one type, got " << tokenWeight->describe() << " and "
                                                                                                             << positionWeight->describe());
  LAMP_CHECK(t >= 0 && t < positionWeight->sizes[0], "position " << t << " is outside a table of " << positionWeight->sizes[0] << " rows");
  LAMP_CHECK(tokens->dtype == kI64 && tokens->device() == dev, "tokens must be int64 on the tables' device, got " << tokens->describe());
  const int64_t R = tokens->numel(), D = tokenWeight->sizes[1];
  const int64_t tstride = dec_vector_stride(tokens, "tokens must be a vector or one column of a matrix");
  Hold tw(contiguous(tokenWeight)), pw(contiguous(positionWeight));
  int64_t os[2] = {R, D};
  Hold o(new_tensor(os, 2, dt, dev));
  if (R * D) {
    hipStream_t st = current_stream(dev);
    KernelTimer kt("decode_embedding", (double)R * D, 3.0 * R * D * (double)dtype_size(dt) + 8.0 * R, st);
#define DEC_EMB(T) hipLaunchKernelGGL((decode_embedding_kernel<T>), dim3(grid_for(R * D, 256)), dim3(256), 0, st, tw->ptr<T>(), pw->ptr<T>(), tokens->ptr<int64_t>(), \
                                      tstride, o->ptr<T>(), R, D, tokenWeight->sizes[0], t, device_assert_word(dev))
    switch (dt) {
      case kF32: DEC_EMB(float); break;
      case kF64: DEC_EMB(double); break;
      default: DEC_EMB(bf16_t); break;
    }
#undef DEC_EMB
    LAMP_LAUNCH_CHECK();
  }
  *out = o.take();
  LAMP_API_END
}

// Test tool, needs no GPU: the launch of a [R, K] . [K, N] product of these kernels through the functions dec_linear_run and rd_step_run use, on
// a device of `cus` compute units.  form: kDecFormLinear, or the cell (LAMP_RECURRENT_*, kDecFormGru2) whose packed matrix w is; dims =
// {K, N}; w_aligned: w sits on a 16-byte boundary.  One line into buf:
// "tiles=<column tiles> kc=<K per slice> s=<slices> grid=<x>x<y> block=<threads> cl=<columns per lane> v=<packet> rt=<rows built for> unroll=<n>"
int lamp_debug_decode_plan(int dtype, int form, int64_t R, const int64_t* dims, int w_aligned, int cus, char* buf, int buflen) {
  LAMP_API_BEGIN
  LAMP_CHECK(dims && buf && buflen > 0 && cus > 0 && R >= 1 && R <= kDecMaxRows && dims[0] >= 1 && dims[1] >= 1, "lamp_debug_decode_plan: bad arguments");
  LAMP_CHECK(form >= 0 && form <= kDecFormLinear && (form == kDecFormLinear ? dec_dtype(dtype) : dtype == kF32 || dtype == kF64),
             "lamp_debug_decode_plan: a linear product in f32, f64 or bf16, or a cell in f32 or f64");
  const size_t tsize = dtype_size(dtype), asize = dtype == kF64 ? 8 : 4;
  const DecForm f = dec_form(form, dims[1], tsize, w_aligned != 0);
  const DecPlan pl = dec_plan(dims[0], dims[1], R, f.CL, tsize, asize, cus);
  char line[256];
  const int n = snprintf(line, sizeof(line), "tiles=%lld kc=%d s=%d grid=%ux%u block=%u cl=%d v=%d rt=%d unroll=%d\n", (long long)pl.tiles, pl.Kc, pl.S,
                         pl.grid.x, pl.grid.y, pl.block.x, f.CL, f.V, dec_rt((int)R), f.unroll);
  LAMP_CHECK(n < buflen, "lamp_debug_decode_plan: buffer too small");
  memcpy(buf, line, n + 1);
  LAMP_API_END
}

}  // extern "C"
