// Convolution (1-D / 2-D, groups, stride, padding, dilation, transposed) forward and backward.
//
// Replaces ATen.convolution and ATen.convolution_backward(output_mask[3]) as lamp's single
// Convolution op calls them (reference: lamp-core/src/main/scala/lamp/autograd/ops.scala:1547-1651;
// Conv2D module lamp-core/.../nn/Conv2D.scala:8-83; Conv1D and Conv2DTransposed route through the
// same op with 1-element / transposed=true arguments).
//
// Layout NCHW (NCL for 1-D is treated as H = 1), weights [Cout, Cin/g, kh, kw]
// (transposed: [Cin, Cout/g, kh, kw]).
//
// This file holds the general direct kernels (every geometry, f32/f64/bf16, fp32 accumulation for
// bf16).  The implicit-GEMM MFMA kernels for the wide 3x3 / 1x1 layers of the CIFAR ResNet live
// in conv_igemm.hip and are selected by conv_dispatch when the geometry qualifies.  1-D and transposed convolutions in bf16 / f32
// that would run the direct kernels ask the general implicit-GEMM kernels of conv_gen.hip first (lamp_convolution_matrix_path).
#include "device_utils.h"
#include "../core/strided.h"
#include "../core/switches.h"
#include "conv_geom.h"
#include <atomic>
#include "conv_backends.h"

namespace lamp {

// lamp_convolution_matrix_path: process-wide, on by default
static std::atomic<int> g_conv_matrix_path{1};
bool conv_matrix_path() { return g_conv_matrix_path.load(std::memory_order_relaxed) != 0; }
// conv_gen.hip is asked for the 1-D and the transposed geometries only, and only where the direct kernels would run
static bool gen_asked(const ConvGeom& g, int nspatial) { return conv_matrix_path() && (g.transposed || nspatial == 1); }

// out[n, co, ho, wo] = bias[co] + sum_{ci, r, s} x[n, ci, ho*sh - ph + r*dh, wo*sw - pw + s*dw] * w[co, ci_l, r, s]
template <class T>
__global__ __launch_bounds__(256) void conv_fwd_direct_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ bias,
                                                              T* __restrict__ y, ConvGeom g) {
  using A = acc_t<T>;
  const int64_t total = g.N * g.Cout * g.Ho * g.Wo;
  const int cin_g = (int)(g.Cin / g.groups), cout_g = (int)(g.Cout / g.groups);
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int wo = (int)(e % g.Wo);
    const int ho = (int)((e / g.Wo) % g.Ho);
    const int co = (int)((e / (g.Wo * g.Ho)) % g.Cout);
    const int64_t n = e / (g.Wo * g.Ho * g.Cout);
    const int grp = co / cout_g;
    A acc = bias ? load_as<A>(bias[co]) : A(0);
    const T* wp = w + (int64_t)co * cin_g * g.kh * g.kw;
    for (int cl = 0; cl < cin_g; cl++) {
      const T* xp = x + ((n * g.Cin + grp * cin_g + cl) * g.H) * g.W;
      for (int r = 0; r < g.kh; r++) {
        const int h = ho * g.sh - g.ph + r * g.dh;
        if (h < 0 || h >= g.H) continue;
        for (int s = 0; s < g.kw; s++) {
          const int ww = wo * g.sw - g.pw + s * g.dw;
          if (ww < 0 || ww >= g.W) continue;
          acc += load_as<A>(xp[h * g.W + ww]) * load_as<A>(wp[(cl * g.kh + r) * g.kw + s]);
        }
      }
    }
    y[e] = store_as<T>(acc);
  }
}

// dx[n, ci, h, w] = sum_{co in group, r, s} dy[n, co, ho, wo] * w[co, ci_l, r, s],  h = ho*sh - ph + r*dh
template <class T>
__global__ __launch_bounds__(256) void conv_dgrad_direct_kernel(const T* __restrict__ dy, const T* __restrict__ w, const T* __restrict__ bias,
                                                                T* __restrict__ dx, ConvGeom g) {
  using A = acc_t<T>;
  const int64_t total = g.N * g.Cin * g.H * g.W;
  const int cin_g = (int)(g.Cin / g.groups), cout_g = (int)(g.Cout / g.groups);
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int wi = (int)(e % g.W);
    const int hi = (int)((e / g.W) % g.H);
    const int ci = (int)((e / (g.W * g.H)) % g.Cin);
    const int64_t n = e / (g.W * g.H * g.Cin);
    const int grp = ci / cin_g, cl = ci - grp * cin_g;
    A acc = bias ? load_as<A>(bias[ci]) : A(0);   // bias only used when this kernel runs a transposed forward
    for (int r = 0; r < g.kh; r++) {
      const int hn = hi + g.ph - r * g.dh;
      if (hn < 0 || hn % g.sh != 0) continue;
      const int ho = hn / g.sh;
      if (ho >= g.Ho) continue;
      for (int s = 0; s < g.kw; s++) {
        const int wn = wi + g.pw - s * g.dw;
        if (wn < 0 || wn % g.sw != 0) continue;
        const int wo = wn / g.sw;
        if (wo >= g.Wo) continue;
        for (int col = 0; col < cout_g; col++) {
          const int co = grp * cout_g + col;
          acc += load_as<A>(dy[((n * g.Cout + co) * g.Ho + ho) * g.Wo + wo]) *
                 load_as<A>(w[(((int64_t)co * cin_g + cl) * g.kh + r) * g.kw + s]);
        }
      }
    }
    dx[e] = store_as<T>(acc);
  }
}

// dw[co, ci_l, r, s] = sum_{n, ho, wo} dy[n, co, ho, wo] * x[n, ci, ho*sh - ph + r*dh, wo*sw - pw + s*dw]
// one workgroup per (co, ci_l); up to MAXRS kernel taps kept in registers
constexpr int MAXRS = 49;
template <class T, int RS>
__global__ __launch_bounds__(256) void conv_wgrad_direct_kernel(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ dw, ConvGeom g) {
  using A = acc_t<T>;
  __shared__ A sm[4];
  const int cin_g = (int)(g.Cin / g.groups), cout_g = (int)(g.Cout / g.groups);
  const int co = blockIdx.x / cin_g, cl = blockIdx.x % cin_g;
  const int grp = co / cout_g;
  const int ci = grp * cin_g + cl;
  const int khkw = g.kh * g.kw;
  A acc[RS];
#pragma unroll
  for (int i = 0; i < RS; i++) acc[i] = A(0);
  const int64_t per = g.Ho * g.Wo, total = g.N * per;
  for (int64_t e = threadIdx.x; e < total; e += blockDim.x) {
    const int64_t n = e / per;
    const int p = (int)(e - n * per);
    const int ho = p / (int)g.Wo, wo = p - ho * (int)g.Wo;
    const A gy = load_as<A>(dy[(n * g.Cout + co) * per + p]);
    const T* xp = x + (n * g.Cin + ci) * g.H * g.W;
#pragma unroll
    for (int rs = 0; rs < RS; rs++) {
      if (rs < khkw) {
        const int r = rs / g.kw, s = rs - r * g.kw;
        const int h = ho * g.sh - g.ph + r * g.dh, ww = wo * g.sw - g.pw + s * g.dw;
        if (h >= 0 && h < g.H && ww >= 0 && ww < g.W) acc[rs] += gy * load_as<A>(xp[h * g.W + ww]);
      }
    }
  }
#pragma unroll
  for (int rs = 0; rs < RS; rs++) {
    if (rs < khkw) {
      A v = block_sum(acc[rs], sm);
      if (threadIdx.x == 0) dw[((int64_t)co * cin_g + cl) * khkw + rs] = store_as<T>(v);
    }
  }
}

// wgrad for the narrow layers (3..16 channels, large images): the reduction runs over N*Ho*Wo
// pixels and the result is tiny, so parallelise over IMAGES: a workgroup stages one image of x and
// dy in LDS (as the accumulation type), every thread owns one filter tap (co, ci, r, s) [or a pixel
// slice of it when there are fewer taps than threads] and walks the image; per-workgroup partial
// filters go to a workspace and are summed by conv_wgrad_reduce_kernel (deterministic order).
template <class T>
__global__ __launch_bounds__(256) void conv_wgrad_lds_kernel(const T* __restrict__ dy, const T* __restrict__ x, acc_t<T>* __restrict__ partial,
                                                             ConvGeom g, int O, int PS, int images_per_block) {
  using A = acc_t<T>;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  A* xs = reinterpret_cast<A*>(smem_raw);                     // [Cin][H][W]
  A* ds = xs + g.Cin * g.H * g.W;                             // [Cout][Ho][Wo]
  A* accs = ds + g.Cout * g.Ho * g.Wo;                        // [O]
  const int tid = threadIdx.x;
  const int cin_g = (int)(g.Cin / g.groups), cout_g = (int)(g.Cout / g.groups);
  const int khkw = g.kh * g.kw;
  for (int o = tid; o < O; o += blockDim.x) accs[o] = A(0);
  const int64_t n0 = (int64_t)blockIdx.x * images_per_block;
  const int64_t n1 = min(n0 + images_per_block, g.N);
  const int xsz = (int)(g.Cin * g.H * g.W), dsz = (int)(g.Cout * g.Ho * g.Wo);
  const int KO = (O + 255) / 256;                              // taps per thread when O > 256
  for (int64_t n = n0; n < n1; n++) {
    __syncthreads();
    const T* xp = x + n * xsz;
    const T* dp = dy + n * dsz;
    for (int i = tid; i < xsz; i += blockDim.x) xs[i] = load_as<A>(xp[i]);
    for (int i = tid; i < dsz; i += blockDim.x) ds[i] = load_as<A>(dp[i]);
    __syncthreads();
    for (int k = 0; k < KO; k++) {
      int o, slice;
      if (O >= 256) { o = tid + k * 256; slice = 0; }
      else { o = tid % O; slice = tid / O; }
      if (o >= O || slice >= PS) continue;
      const int rs = o % khkw, cl = (o / khkw) % cin_g, co = o / (khkw * cin_g);
      const int r = rs / g.kw, s = rs - r * g.kw;
      const int ci = (co / cout_g) * cin_g + cl;
      const A* xc = xs + ci * g.H * g.W;
      const A* dc = ds + co * g.Ho * g.Wo;
      // valid output range for this tap (no per-pixel bounds checks in the inner loop)
      const int off_h = r * g.dh - g.ph, off_w = s * g.dw - g.pw;
      int ho_lo = off_h < 0 ? (-off_h + g.sh - 1) / g.sh : 0;
      int wo_lo = off_w < 0 ? (-off_w + g.sw - 1) / g.sw : 0;
      int ho_hi = (int)min<int64_t>(g.Ho, (g.H - 1 - off_h) / g.sh + 1);
      int wo_hi = (int)min<int64_t>(g.Wo, (g.W - 1 - off_w) / g.sw + 1);
      if (g.H - 1 - off_h < 0) ho_hi = 0;
      if (g.W - 1 - off_w < 0) wo_hi = 0;
      A acc = A(0);
      for (int ho = ho_lo + slice; ho < ho_hi; ho += PS) {
        const A* xr = xc + (ho * g.sh + off_h) * g.W + off_w;
        const A* dr = dc + ho * g.Wo;
        for (int wo = wo_lo; wo < wo_hi; wo++) acc += dr[wo] * xr[wo * g.sw];
      }
      if (PS > 1) atomicAdd(&accs[o], acc);
      else accs[o] += acc;
    }
  }
  __syncthreads();
  for (int o = tid; o < O; o += blockDim.x) partial[(int64_t)blockIdx.x * O + o] = accs[o];
}
// one wavefront per filter tap: lanes stride over the per-workgroup partials (coalescing across taps is not
// needed, the partial buffer is a few MB and L2 resident), fixed summation order => deterministic
template <class T>
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const acc_t<T>* __restrict__ partial, T* __restrict__ dw, int O, int nblocks) {
  using A = acc_t<T>;
  const int lane = threadIdx.x & 63;
  const int o = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
  if (o >= O) return;
  A a = 0;
  for (int b = lane; b < nblocks; b += 64) a += partial[(int64_t)b * O + o];
  a = wave_sum(a);
  if (lane == 0) dw[o] = store_as<T>(a);
}

ConvGeom make_geom(const Tensor* x, const Tensor* w, const int64_t* stride, const int64_t* padding, const int64_t* dilation,
                   int nspatial, int transposed, const int64_t* output_padding, int64_t groups) {
  LAMP_CHECK(nspatial == 1 || nspatial == 2, "only 1-D and 2-D convolutions are supported (got " << nspatial << " spatial dims)");
  LAMP_CHECK(x->ndim == nspatial + 2 && w->ndim == nspatial + 2, "convolution: input " << x->describe() << " / weight " << w->describe()
             << " do not have " << nspatial + 2 << " dims");
  LAMP_CHECK(groups >= 1, "groups must be >= 1");
  ConvGeom g{};
  g.transposed = transposed;
  g.groups = groups;
  const bool two = nspatial == 2;
  g.sh = two ? (int)stride[0] : 1; g.sw = (int)stride[two ? 1 : 0];
  g.ph = two ? (int)padding[0] : 0; g.pw = (int)padding[two ? 1 : 0];
  g.dh = two ? (int)dilation[0] : 1; g.dw = (int)dilation[two ? 1 : 0];
  g.kh = two ? (int)w->sizes[2] : 1; g.kw = (int)w->sizes[two ? 3 : 2];
  const int oph = (transposed && output_padding) ? (two ? (int)output_padding[0] : 0) : 0;
  const int opw = (transposed && output_padding) ? (int)output_padding[two ? 1 : 0] : 0;
  LAMP_CHECK(g.sh > 0 && g.sw > 0 && g.dh > 0 && g.dw > 0 && g.ph >= 0 && g.pw >= 0, "bad convolution geometry");
  g.N = x->sizes[0];
  // In "regular" terms (Cin, H, W) is the side with the larger image for transposed convs.
  if (!transposed) {
    g.Cin = x->sizes[1]; g.H = two ? x->sizes[2] : 1; g.W = x->sizes[two ? 3 : 2];
    g.Cout = w->sizes[0];
    LAMP_CHECK(w->sizes[1] * groups == g.Cin, "convolution: weight " << w->describe() << " expects " << w->sizes[1] * groups
               << " input channels, input has " << g.Cin);
    LAMP_CHECK(g.Cout % groups == 0, "out channels not divisible by groups");
    g.Ho = (g.H + 2 * g.ph - g.dh * (g.kh - 1) - 1) / g.sh + 1;
    g.Wo = (g.W + 2 * g.pw - g.dw * (g.kw - 1) - 1) / g.sw + 1;
    LAMP_CHECK(g.Ho > 0 && g.Wo > 0, "convolution output would be empty");
  } else {
    // transposed conv: x plays the role of dy of a regular conv whose input is the (bigger) output
    g.Cout = x->sizes[1]; g.Ho = two ? x->sizes[2] : 1; g.Wo = x->sizes[two ? 3 : 2];
    LAMP_CHECK(w->sizes[0] == g.Cout, "transposed convolution: weight " << w->describe() << " expects " << w->sizes[0] << " input channels");
    g.Cin = w->sizes[1] * groups;
    g.H = (g.Ho - 1) * g.sh - 2 * g.ph + g.dh * (g.kh - 1) + oph + 1;
    g.W = (g.Wo - 1) * g.sw - 2 * g.pw + g.dw * (g.kw - 1) + opw + 1;
    LAMP_CHECK(g.H > 0 && g.W > 0, "transposed convolution output would be empty");
  }
  return g;
}

template <class T> static void launch_fwd(const Tensor* x, const Tensor* w, const Tensor* b, Tensor* y, const ConvGeom& g, hipStream_t st) {
  const int64_t total = g.N * g.Cout * g.Ho * g.Wo;
  if (!total) return;
  KernelTimer kt("conv_fwd_direct", conv_flops(g), conv_bytes(g, sizeof(T)), st);
  hipLaunchKernelGGL((conv_fwd_direct_kernel<T>), dim3(grid_for(total, 256, 16)), dim3(256), 0, st, x->ptr<T>(), w->ptr<T>(),
                     b ? b->ptr<T>() : (const T*)nullptr, y->ptr<T>(), g);
  LAMP_LAUNCH_CHECK();
}
template <class T> static void launch_dgrad(const Tensor* dy, const Tensor* w, const Tensor* b, Tensor* dx, const ConvGeom& g, hipStream_t st) {
  const int64_t total = g.N * g.Cin * g.H * g.W;
  if (!total) return;
  KernelTimer kt("conv_dgrad_direct", conv_flops(g), conv_bytes(g, sizeof(T)), st);
  hipLaunchKernelGGL((conv_dgrad_direct_kernel<T>), dim3(grid_for(total, 256, 16)), dim3(256), 0, st, dy->ptr<T>(), w->ptr<T>(),
                     b ? b->ptr<T>() : (const T*)nullptr, dx->ptr<T>(), g);
  LAMP_LAUNCH_CHECK();
}
template <class T> static void launch_wgrad(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st) {
  const int64_t blocks = g.Cout * (g.Cin / g.groups);
  if (!blocks) return;
  const int khkw = g.kh * g.kw;
  {
    using A = acc_t<T>;
    const int64_t O = blocks * khkw;
    const size_t lds = (size_t)(g.Cin * g.H * g.W + g.Cout * g.Ho * g.Wo + O) * sizeof(A);
    if (lds <= 150 * 1024 && O <= 8192) {
      const int nb = (int)std::min<int64_t>(g.N, (int64_t)num_cus() * 2);
      const int ipb = (int)((g.N + nb - 1) / nb);
      const int nblocks = (int)((g.N + ipb - 1) / ipb);
      const int PS = O >= 256 ? 1 : (int)(256 / O);
      int64_t ps[1] = {(int64_t)nblocks * O};
      Hold partial(new_tensor(ps, 1, std::is_same<A, double>::value ? kF64 : kF32, dy->device()));
      allow_big_lds((const void*)conv_wgrad_lds_kernel<T>);
      {
        KernelTimer kt("conv_wgrad_lds", conv_flops(g), conv_bytes(g, sizeof(T)), st);
        hipLaunchKernelGGL((conv_wgrad_lds_kernel<T>), dim3(nblocks), dim3(256), lds, st, dy->ptr<T>(), x->ptr<T>(), partial->ptr<A>(), g, (int)O, PS, ipb);
        LAMP_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL((conv_wgrad_reduce_kernel<T>), dim3((unsigned)((O * 64 + 255) / 256)), dim3(256), 0, st, partial->ptr<A>(), dw->ptr<T>(), (int)O, nblocks);
      LAMP_LAUNCH_CHECK();
      return;
    }
  }
  LAMP_CHECK(khkw <= MAXRS, "kernel window larger than " << MAXRS << " taps is not supported");
  KernelTimer kt("conv_wgrad_direct", conv_flops(g), conv_bytes(g, sizeof(T)), st);
  if (khkw == 1) hipLaunchKernelGGL((conv_wgrad_direct_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, st, dy->ptr<T>(), x->ptr<T>(), dw->ptr<T>(), g);
  else if (khkw <= 9) hipLaunchKernelGGL((conv_wgrad_direct_kernel<T, 9>), dim3((unsigned)blocks), dim3(256), 0, st, dy->ptr<T>(), x->ptr<T>(), dw->ptr<T>(), g);
  else if (khkw <= 25) hipLaunchKernelGGL((conv_wgrad_direct_kernel<T, 25>), dim3((unsigned)blocks), dim3(256), 0, st, dy->ptr<T>(), x->ptr<T>(), dw->ptr<T>(), g);
  else hipLaunchKernelGGL((conv_wgrad_direct_kernel<T, MAXRS>), dim3((unsigned)blocks), dim3(256), 0, st, dy->ptr<T>(), x->ptr<T>(), dw->ptr<T>(), g);
  LAMP_LAUNCH_CHECK();
}

// The optimisers' hook: the packed filter images of the parameters just written on this stream follow the update in place, in one launch
// per backend (the narrow images ride in the implicit-GEMM one) - the next step's convolutions, and a HIP graph captured earlier, find
// them fresh.  Values are exactly those a lazy pack at first use would produce.  LAMP_PACK_AFTER_STEP=0 restores the lazy packs.
void conv_repack_cached(lamp_tensor* const* params, int n, hipStream_t st) {
  if (!sw().pack_after_step) return;
  igemm_repack_cached(params, n, st);
  igemm32_repack_cached(params, n, st);
  small_repack_cached(params, n, st);
}

Tensor* reduce_dims(const Tensor* a, const int64_t* dims, int ndims, bool keepdim, int op);

template <class T>
__global__ __launch_bounds__(256) void bn_relu_materialise_kernel(const T* __restrict__ x, T* __restrict__ y, const float4* __restrict__ affine, int64_t total,
                                                                  int64_t C, int64_t HW) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = affine[(i / HW) % C];
    T o = store_as<T>(__builtin_fmaf(load_as<float>(x[i]) - a.x, a.y, a.z));           // norm.hip bn_affine<float>, rounded as bn_apply rounds
    if (load_as<float>(o) < 0.f) o = store_as<T>(0.f);
    y[i] = o;
  }
}
Tensor* bn_relu_materialise(const Tensor* xc, const Tensor* affine, hipStream_t st) {
  Hold y(new_like(xc));
  const int64_t total = xc->numel(), C = xc->sizes[1];
  int64_t HW = 1;
  for (int i = 2; i < xc->ndim; i++) HW *= xc->sizes[i];
  if (total > 0) {
    const float4* aff = reinterpret_cast<const float4*>(affine->ptr<float>());
    const dim3 grid(grid_for(total, 256));
    if (xc->dtype == kBF16) hipLaunchKernelGGL((bn_relu_materialise_kernel<bf16_t>), grid, dim3(256), 0, st, xc->ptr<bf16_t>(), y->ptr<bf16_t>(), aff, total, C, HW);
    else if (xc->dtype == kF16) hipLaunchKernelGGL((bn_relu_materialise_kernel<f16_t>), grid, dim3(256), 0, st, xc->ptr<f16_t>(), y->ptr<f16_t>(), aff, total, C, HW);
    else hipLaunchKernelGGL((bn_relu_materialise_kernel<float>), grid, dim3(256), 0, st, xc->ptr<float>(), y->ptr<float>(), aff, total, C, HW);
    LAMP_LAUNCH_CHECK();
  }
  return y.take();
}
// a filter as the kernels want it: itself (+1) when contiguous, otherwise a copy that lives for this call only and is marked so that the
// packed-weight caches do not keep images of it
static Tensor* contiguous_filter(const Tensor* w) {
  Tensor* c = contiguous(w);
  if (c->st != w->st) c->st->scratch = true;
  return c;
}
}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_convolution(lamp_tensor** out, const lamp_tensor* x, const lamp_tensor* w, const lamp_tensor* bias, const int64_t* stride,
                     const int64_t* padding, const int64_t* dilation, int nspatial, int transposed, const int64_t* output_padding,
                     int64_t groups) {
  LAMP_API_BEGIN
  check_device_tensor(x, "input"); check_device_tensor(w, "weight");
  LAMP_CHECK(x->dtype == w->dtype, "convolution: input " << x->describe() << " and weight " << w->describe() << " have different dtypes");
  ConvGeom g = make_geom(x, w, stride, padding, dilation, nspatial, transposed, output_padding, groups);
  const int64_t out_c = transposed ? g.Cin : g.Cout;
  if (bias) { check_device_tensor(bias, "bias"); LAMP_CHECK(bias->numel() == out_c && bias->dtype == x->dtype, "convolution: bias must have " << out_c << " elements"); }
  Hold xc(contiguous(x)), wc(contiguous_filter(w));
  Hold bc(bias ? contiguous(bias) : nullptr);
  std::vector<int64_t> oshape = {g.N, out_c};
  if (nspatial == 2) oshape.push_back(transposed ? g.H : g.Ho);
  oshape.push_back(transposed ? g.W : g.Wo);
  Hold y(new_tensor(oshape, x->dtype, x->device()));
  hipStream_t st = current_stream(x->device());
  if (!transposed) {
    if (!igemm_conv_fwd(xc.get(), wc.get(), bc.get(), y.get(), g, st) && !igemm32_conv_fwd(xc.get(), wc.get(), bc.get(), y.get(), g, st) &&
        !narrow_conv_fwd(xc.get(), wc.get(), bc.get(), y.get(), g, st) && !small_conv_fwd(xc.get(), wc.get(), bc.get(), y.get(), g, st) &&
        !(gen_asked(g, nspatial) && gen_conv_fwd(xc.get(), wc.get(), bc.get(), y.get(), g, st))) {
      LAMP_DISPATCH_FLOAT(x->dtype, T, (launch_fwd<T>(xc.get(), wc.get(), bc.get(), y.get(), g, st)));
    }
  } else if (!(gen_asked(g, nspatial) && gen_conv_dgrad(xc.get(), wc.get(), bc.get(), y.get(), g, st))) {
    LAMP_DISPATCH_FLOAT(x->dtype, T, (launch_dgrad<T>(xc.get(), wc.get(), bc.get(), y.get(), g, st)));
  }
  *out = y.take();
  LAMP_API_END
}

// Process-wide: on (the default), 1-D and transposed convolutions that would run the direct kernels ask conv_gen.hip first; off, they
// run the direct kernels.  Returns the previous setting through previous_or_null.
int lamp_convolution_matrix_path(int on, int* previous_or_null) {
  LAMP_API_BEGIN
  const int prev = g_conv_matrix_path.exchange(on ? 1 : 0);
  if (previous_or_null) *previous_or_null = prev;
  LAMP_API_END
}

int lamp_convolution_pair(lamp_tensor* out2[2], const lamp_tensor* x, const lamp_tensor* w_a, const lamp_tensor* bias_a, const int64_t* stride_a,
                          const int64_t* padding_a, const int64_t* dilation_a, const lamp_tensor* w_b, const lamp_tensor* bias_b,
                          const int64_t* stride_b, const int64_t* padding_b, const int64_t* dilation_b, int nspatial, int64_t groups) {
  LAMP_API_BEGIN
  out2[0] = out2[1] = nullptr;
  check_device_tensor(x, "input"); check_device_tensor(w_a, "weight a"); check_device_tensor(w_b, "weight b");
  const int64_t zero2[2] = {0, 0};
  bool fused = false;
  if (nspatial == 2 && x->dtype == w_a->dtype && x->dtype == w_b->dtype && x->dtype == kBF16 && (!bias_a || bias_a->is_device()) && (!bias_b || bias_b->is_device())) {
    ConvGeom ga = make_geom(x, w_a, stride_a, padding_a, dilation_a, nspatial, 0, zero2, groups);
    ConvGeom gb = make_geom(x, w_b, stride_b, padding_b, dilation_b, nspatial, 0, zero2, groups);
    const bool biases_ok = (!bias_a || (bias_a->numel() == ga.Cout && bias_a->dtype == x->dtype)) && (!bias_b || (bias_b->numel() == gb.Cout && bias_b->dtype == x->dtype));
    if (biases_ok && ga.Ho == gb.Ho && ga.Wo == gb.Wo) {
      Hold xc(contiguous(x)), wa(contiguous_filter(w_a)), wb(contiguous_filter(w_b));
      Hold ba(bias_a ? contiguous(bias_a) : nullptr), bb(bias_b ? contiguous(bias_b) : nullptr);
      Hold ya(new_tensor({ga.N, ga.Cout, ga.Ho, ga.Wo}, x->dtype, x->device())), yb(new_tensor({gb.N, gb.Cout, gb.Ho, gb.Wo}, x->dtype, x->device()));
      hipStream_t st = current_stream(x->device());
      if (igemm_conv_fwd_pair(xc.get(), wa.get(), ba.get(), ya.get(), ga, wb.get(), bb.get(), yb.get(), gb, st) ||
          narrow_conv_fwd_pair(xc.get(), wa.get(), ba.get(), ya.get(), ga, wb.get(), bb.get(), yb.get(), gb, st)) {
        out2[0] = ya.take(); out2[1] = yb.take();
        fused = true;
      }
    }
  }
  if (!fused) {                                       // the two calls (each validates its own arguments)
    lamp_tensor* a = nullptr;
    if (lamp_convolution(&a, x, w_a, bias_a, stride_a, padding_a, dilation_a, nspatial, 0, zero2, groups) != 0) throw Error(lamp_last_error());
    Hold ha(a);
    lamp_tensor* b = nullptr;
    if (lamp_convolution(&b, x, w_b, bias_b, stride_b, padding_b, dilation_b, nspatial, 0, zero2, groups) != 0) throw Error(lamp_last_error());
    out2[0] = ha.take(); out2[1] = b;
  }
  LAMP_API_END
}

int lamp_convolution_chain_pair(lamp_tensor* out3[3], const lamp_tensor* x, const lamp_tensor* w, const lamp_tensor* bias, const int64_t* stride,
                                const int64_t* padding, const int64_t* dilation, const lamp_tensor* w_a, const lamp_tensor* bias_a, const int64_t* stride_a,
                                const int64_t* padding_a, const int64_t* dilation_a, const lamp_tensor* w_b, const lamp_tensor* bias_b,
                                const int64_t* stride_b, const int64_t* padding_b, const int64_t* dilation_b, int nspatial, int64_t groups) {
  LAMP_API_BEGIN
  out3[0] = out3[1] = out3[2] = nullptr;
  check_device_tensor(x, "input"); check_device_tensor(w, "weight"); check_device_tensor(w_a, "weight a"); check_device_tensor(w_b, "weight b");
  const int64_t zero2[2] = {0, 0};
  bool fused = false;
  auto bias_ok = [&](const lamp_tensor* b, int64_t c) { return !b || (b->is_device() && b->numel() == c && b->dtype == x->dtype); };
  if (nspatial == 2 && x->ndim == 4 && x->dtype == kBF16 && w->dtype == kBF16 && w_a->dtype == kBF16 && w_b->dtype == kBF16 && w_a->ndim == 4 && w_b->ndim == 4 &&
      w_a->sizes[1] * groups == w->sizes[0] && w_b->sizes[1] * groups == w->sizes[0]) {
    ConvGeom g0 = make_geom(x, w, stride, padding, dilation, nspatial, 0, zero2, groups);
    if (g0.Ho > 0 && g0.Wo > 0) {
      Hold s(new_tensor({g0.N, g0.Cout, g0.Ho, g0.Wo}, x->dtype, x->device()));
      ConvGeom ga = make_geom(s.get(), w_a, stride_a, padding_a, dilation_a, nspatial, 0, zero2, groups);
      ConvGeom gb = make_geom(s.get(), w_b, stride_b, padding_b, dilation_b, nspatial, 0, zero2, groups);
      if (bias_ok(bias, g0.Cout) && bias_ok(bias_a, ga.Cout) && bias_ok(bias_b, gb.Cout) && ga.Ho == gb.Ho && ga.Wo == gb.Wo && ga.Ho > 0 && ga.Wo > 0) {
        Hold xc(contiguous(x)), w0(contiguous_filter(w)), wa(contiguous_filter(w_a)), wb(contiguous_filter(w_b));
        Hold b0(bias ? contiguous(bias) : nullptr), ba(bias_a ? contiguous(bias_a) : nullptr), bb(bias_b ? contiguous(bias_b) : nullptr);
        Hold ya(new_tensor({ga.N, ga.Cout, ga.Ho, ga.Wo}, x->dtype, x->device())), yb(new_tensor({gb.N, gb.Cout, gb.Ho, gb.Wo}, x->dtype, x->device()));
        hipStream_t st = current_stream(x->device());
        if (narrow_conv_chain_pair(xc.get(), w0.get(), b0.get(), s.get(), g0, wa.get(), ba.get(), ya.get(), ga, wb.get(), bb.get(), yb.get(), gb, st)) {
          out3[0] = s.take(); out3[1] = ya.take(); out3[2] = yb.take();
          fused = true;
        }
      }
    }
  }
  if (!fused) {                                       // the two calls (each validates its own arguments)
    lamp_tensor* s = nullptr;
    if (lamp_convolution(&s, x, w, bias, stride, padding, dilation, nspatial, 0, zero2, groups) != 0) throw Error(lamp_last_error());
    Hold hs(s);
    lamp_tensor* o2[2] = {nullptr, nullptr};
    if (lamp_convolution_pair(o2, s, w_a, bias_a, stride_a, padding_a, dilation_a, w_b, bias_b, stride_b, padding_b, dilation_b, nspatial, groups) != 0)
      throw Error(lamp_last_error());
    out3[0] = hs.take(); out3[1] = o2[0]; out3[2] = o2[1];
  }
  LAMP_API_END
}

int lamp_convolution_backward(lamp_tensor* out3[3], const lamp_tensor* grad_out, const lamp_tensor* x, const lamp_tensor* w,
                              const int64_t* stride, const int64_t* padding, const int64_t* dilation, int nspatial, int transposed,
                              const int64_t* output_padding, int64_t groups, const uint8_t mask[3]) {
  LAMP_API_BEGIN
  check_device_tensor(x, "input"); check_device_tensor(w, "weight"); check_device_tensor(grad_out, "grad_out");
  LAMP_CHECK(x->dtype == w->dtype && grad_out->dtype == x->dtype, "convolution_backward: dtype mismatch");
  ConvGeom g = make_geom(x, w, stride, padding, dilation, nspatial, transposed, output_padding, groups);
  {
    const int64_t oc = transposed ? g.Cin : g.Cout, oh = transposed ? g.H : g.Ho, ow = transposed ? g.W : g.Wo;
    LAMP_CHECK(grad_out->ndim == x->ndim && grad_out->sizes[0] == g.N && grad_out->sizes[1] == oc &&
               grad_out->sizes[grad_out->ndim - 1] == ow && (nspatial == 1 || grad_out->sizes[2] == oh),
               "convolution_backward: grad_out " << grad_out->describe() << " does not match the forward output shape");
  }
  Hold xc(contiguous(x)), wc(contiguous_filter(w)), gc(contiguous(grad_out));
  hipStream_t st = current_stream(x->device());
  Hold dx(mask[0] ? new_like(xc.get()) : nullptr);
  Hold dw(mask[1] ? new_like(wc.get()) : nullptr);
  Hold db;
  if (!transposed) {
    if (dx.get() && !igemm_conv_dgrad(gc.get(), wc.get(), dx.get(), g, st) && !igemm32_conv_dgrad(gc.get(), wc.get(), dx.get(), g, st) &&
        !narrow_conv_dgrad(gc.get(), wc.get(), dx.get(), g, st) && !small_conv_dgrad(gc.get(), wc.get(), dx.get(), g, st) &&
        !(gen_asked(g, nspatial) && gen_conv_dgrad(gc.get(), wc.get(), nullptr, dx.get(), g, st))) {
      LAMP_DISPATCH_FLOAT(x->dtype, T, (launch_dgrad<T>(gc.get(), wc.get(), nullptr, dx.get(), g, st)));
    }
    if (dw.get() && !igemm_conv_wgrad(gc.get(), xc.get(), dw.get(), g, st) && !igemm32_conv_wgrad(gc.get(), xc.get(), dw.get(), g, st) &&
        !narrow_conv_wgrad(gc.get(), xc.get(), dw.get(), g, st) && !small_conv_wgrad(gc.get(), xc.get(), dw.get(), g, st) &&
        !(gen_asked(g, nspatial) && gen_conv_wgrad(gc.get(), xc.get(), dw.get(), g, st))) {
      LAMP_DISPATCH_FLOAT(x->dtype, T, (launch_wgrad<T>(gc.get(), xc.get(), dw.get(), g, st)));
    }
  } else {
    // forward was dgrad(x, w): d/dx is the regular forward conv of grad_out, d/dw swaps the roles of x and grad_out
    if (dx.get() && !(gen_asked(g, nspatial) && gen_conv_fwd(gc.get(), wc.get(), nullptr, dx.get(), g, st))) {
      LAMP_DISPATCH_FLOAT(x->dtype, T, (launch_fwd<T>(gc.get(), wc.get(), nullptr, dx.get(), g, st)));
    }
    if (dw.get() && !(gen_asked(g, nspatial) && gen_conv_wgrad(xc.get(), gc.get(), dw.get(), g, st))) {
      LAMP_DISPATCH_FLOAT(x->dtype, T, (launch_wgrad<T>(xc.get(), gc.get(), dw.get(), g, st)));
    }
  }
  if (mask[2]) {
    std::vector<int64_t> dims = {0};
    for (int i = 2; i < grad_out->ndim; i++) dims.push_back(i);
    db = Hold(reduce_dims(gc.get(), dims.data(), (int)dims.size(), false, 0));
  }
  out3[0] = dx.take(); out3[1] = dw.take(); out3[2] = db.take();
  LAMP_API_END
}

// ---- conv(relu(bn(x))): the batch norm + relu between two convolutions folded into the consumer (round 3) -----------------------------
// `affine` = f32 [C][4] rows (mean, invstd * weight, bias, -) from lamp_batch_norm_affine.  Where the implicit-GEMM kernels can apply it
// while they stage their input (eight-image fprop kernel, eight-wave weight-gradient kernel: the wide 8x8 layers at large batch) the
// normalised tensor is never written; every other geometry materialises it once with the same arithmetic and runs the plain operators.
static void check_affine(const lamp_tensor* affine, const lamp_tensor* x) {
  check_device_tensor(affine, "affine");
  LAMP_CHECK(affine->dtype == kF32 && affine->ndim == 2 && affine->sizes[0] == x->sizes[1] && affine->sizes[1] == 4 && affine->is_contiguous(),
             "affine must be the contiguous f32 [channels, 4] table of lamp_batch_norm_affine, got " << affine->describe());
  LAMP_CHECK(x->dtype == kBF16 || x->dtype == kF16 || x->dtype == kF32, "conv(relu(bn(x))) with a folded batch norm is a reduced-precision path (f32 table): f64 runs the separate operators");
}
// *out = 1 when BOTH the forward and the weight-gradient kernel for this geometry apply the table while staging (the fold saves a pass
// over the activation), 0 when either would materialise relu(bn(x)) first (the fold is then no faster than the separate operators)
int lamp_convolution_bn_relu_input_folds(int* out, const lamp_tensor* x, const lamp_tensor* w, const int64_t* stride, const int64_t* padding,
                                         const int64_t* dilation, int nspatial, int64_t groups) {
  LAMP_API_BEGIN
  *out = 0;
  if (!x->is_device() || !w->is_device() || x->dtype != w->dtype) return 0;
  const int64_t zero2[2] = {0, 0};
  ConvGeom g = make_geom(x, w, stride, padding, dilation, nspatial, 0, zero2, groups);
  *out = igemm_conv_folds_affine(g, x->dtype) ? 1 : 0;
  LAMP_API_END
}
int lamp_convolution_bn_relu_input(lamp_tensor** out, const lamp_tensor* x, const lamp_tensor* affine, const lamp_tensor* w, const lamp_tensor* bias,
                                   const int64_t* stride, const int64_t* padding, const int64_t* dilation, int nspatial, int64_t groups) {
  LAMP_API_BEGIN
  check_device_tensor(x, "input"); check_device_tensor(w, "weight"); check_affine(affine, x);
  LAMP_CHECK(x->dtype == w->dtype, "convolution: input " << x->describe() << " and weight " << w->describe() << " have different dtypes");
  const int64_t zero2[2] = {0, 0};
  ConvGeom g = make_geom(x, w, stride, padding, dilation, nspatial, 0, zero2, groups);
  if (bias) { check_device_tensor(bias, "bias"); LAMP_CHECK(bias->numel() == g.Cout && bias->dtype == x->dtype, "convolution: bias must have " << g.Cout << " elements"); }
  Hold xc(contiguous(x)), wc(contiguous_filter(w));
  Hold bc(bias ? contiguous(bias) : nullptr);
  hipStream_t st = current_stream(x->device());
  std::vector<int64_t> oshape = {g.N, g.Cout};
  if (nspatial == 2) oshape.push_back(g.Ho);
  oshape.push_back(g.Wo);
  Hold y(new_tensor(oshape, x->dtype, x->device()));
  if (!igemm_conv_fwd_affine(xc.get(), affine, wc.get(), bc.get(), y.get(), g, st)) {
    Hold act(bn_relu_materialise(xc.get(), affine, st));
    lamp_tensor* o = nullptr;
    if (lamp_convolution(&o, act.get(), wc.get(), bc.get(), stride, padding, dilation, nspatial, 0, zero2, groups) != 0) throw Error(lamp_last_error());
    *out = o;
    return 0;
  }
  *out = y.take();
  LAMP_API_END
}
// out3 = (gradient w.r.t. relu(bn(x)), dweight, dbias); the caller runs the batch norm + relu backward on out3[0] and x
int lamp_convolution_bn_relu_input_backward(lamp_tensor* out3[3], const lamp_tensor* grad_out, const lamp_tensor* x, const lamp_tensor* affine,
                                            const lamp_tensor* w, const int64_t* stride, const int64_t* padding, const int64_t* dilation, int nspatial,
                                            int64_t groups, const uint8_t mask[3]) {
  LAMP_API_BEGIN
  out3[0] = out3[1] = out3[2] = nullptr;
  check_device_tensor(x, "input"); check_device_tensor(w, "weight"); check_device_tensor(grad_out, "grad_out"); check_affine(affine, x);
  const int64_t zero2[2] = {0, 0};
  ConvGeom g = make_geom(x, w, stride, padding, dilation, nspatial, 0, zero2, groups);
  Hold xc(contiguous(x)), wc(contiguous_filter(w)), gc(contiguous(grad_out));
  hipStream_t st = current_stream(x->device());
  Hold dw;
  bool dw_done = false;
  if (mask[1]) {
    dw = Hold(new_like(wc.get()));
    dw_done = igemm_conv_wgrad(gc.get(), xc.get(), dw.get(), g, st, affine);        // relu(bn(x)) rebuilt while staging
  }
  // everything else through the plain operator: the input gradient never needs the activation, the weight gradient gets a materialised one
  const bool need_act = mask[1] && !dw_done;
  Hold act(need_act ? bn_relu_materialise(xc.get(), affine, st) : nullptr);
  const uint8_t m3[3] = {mask[0], (uint8_t)(mask[1] && !dw_done), mask[2]};
  lamp_tensor* r3[3] = {nullptr, nullptr, nullptr};
  if (m3[0] || m3[1] || m3[2]) {
    if (lamp_convolution_backward(r3, gc.get(), need_act ? act.get() : xc.get(), wc.get(), stride, padding, dilation, nspatial, 0, zero2, groups, m3) != 0)
      throw Error(lamp_last_error());
  }
  out3[0] = r3[0]; out3[1] = dw_done ? dw.take() : r3[1]; out3[2] = r3[2];
  LAMP_API_END
}

int lamp_convolution_backward_input_add(lamp_tensor** out, const lamp_tensor* grad_out, const lamp_tensor* x, const lamp_tensor* w,
                                        const int64_t* stride, const int64_t* padding, const int64_t* dilation, int nspatial,
                                        const int64_t* output_padding, int64_t groups, const lamp_tensor* addend) {
  LAMP_API_BEGIN
  check_device_tensor(x, "input"); check_device_tensor(w, "weight"); check_device_tensor(grad_out, "grad_out"); check_device_tensor(addend, "addend");
  LAMP_CHECK(x->dtype == w->dtype && grad_out->dtype == x->dtype && addend->dtype == x->dtype, "convolution_backward_input_add: dtype mismatch");
  LAMP_CHECK(addend->ndim == x->ndim, "convolution_backward_input_add: addend " << addend->describe() << " does not have the input's shape " << x->describe());
  for (int i = 0; i < x->ndim; i++)
    LAMP_CHECK(addend->sizes[i] == x->sizes[i], "convolution_backward_input_add: addend " << addend->describe() << " does not have the input's shape " << x->describe());
  ConvGeom g = make_geom(x, w, stride, padding, dilation, nspatial, 0, output_padding, groups);
  LAMP_CHECK(grad_out->ndim == x->ndim && grad_out->sizes[0] == g.N && grad_out->sizes[1] == g.Cout &&
             grad_out->sizes[grad_out->ndim - 1] == g.Wo && (nspatial == 1 || grad_out->sizes[2] == g.Ho),
             "convolution_backward_input_add: grad_out " << grad_out->describe() << " does not match the forward output shape");
  Hold wc(contiguous_filter(w)), gc(contiguous(grad_out)), ac(contiguous(addend));
  hipStream_t st = current_stream(x->device());
  Hold dx(new_tensor(std::vector<int64_t>(x->sizes, x->sizes + x->ndim), x->dtype, x->device()));
  bool fused = false;
  if (!igemm_conv_dgrad(gc.get(), wc.get(), dx.get(), g, st, ac.get(), &fused) && !igemm32_conv_dgrad(gc.get(), wc.get(), dx.get(), g, st, ac.get(), &fused) &&
      !narrow_conv_dgrad(gc.get(), wc.get(), dx.get(), g, st, ac.get(), &fused) && !small_conv_dgrad(gc.get(), wc.get(), dx.get(), g, st, ac.get(), &fused) &&
      !(gen_asked(g, nspatial) && gen_conv_dgrad(gc.get(), wc.get(), nullptr, dx.get(), g, st))) {
    LAMP_DISPATCH_FLOAT(x->dtype, T, (launch_dgrad<T>(gc.get(), wc.get(), nullptr, dx.get(), g, st)));
  }
  if (fused) { *out = dx.take(); }
  else {
    lamp_tensor* sum = nullptr;
    if (lamp_add(&sum, ac.get(), dx.get(), 1.0) != 0) throw Error(lamp_last_error());
    *out = sum;
  }
  LAMP_API_END
}

int lamp_convolution_backward_input_pair(lamp_tensor** out, const lamp_tensor* x, const lamp_tensor* grad_out_a, const lamp_tensor* w_a,
                                         const int64_t* stride_a, const int64_t* padding_a, const int64_t* dilation_a,
                                         const lamp_tensor* grad_out_b, const lamp_tensor* w_b, const int64_t* stride_b,
                                         const int64_t* padding_b, const int64_t* dilation_b, int nspatial, int64_t groups,
                                         const lamp_tensor* addend) {
  LAMP_API_BEGIN
  check_device_tensor(x, "input"); check_device_tensor(w_a, "first weight"); check_device_tensor(grad_out_a, "first grad_out");
  check_device_tensor(w_b, "second weight"); check_device_tensor(grad_out_b, "second grad_out");
  LAMP_CHECK(x->dtype == w_a->dtype && x->dtype == w_b->dtype && grad_out_a->dtype == x->dtype && grad_out_b->dtype == x->dtype,
             "convolution_backward_input_pair: dtype mismatch");
  if (addend) {
    check_device_tensor(addend, "addend");
    LAMP_CHECK(addend->dtype == x->dtype, "convolution_backward_input_pair: dtype mismatch");
    LAMP_CHECK(addend->shape() == x->shape(), "convolution_backward_input_pair: addend " << addend->describe() << " does not have the input's shape " << x->describe());
  }
  LAMP_CHECK(nspatial >= 1 && nspatial <= 2, "convolution_backward_input_pair: 1 or 2 spatial dimensions");
  const int64_t zero2[2] = {0, 0};
  ConvGeom ga = make_geom(x, w_a, stride_a, padding_a, dilation_a, nspatial, 0, zero2, groups);
  ConvGeom gb = make_geom(x, w_b, stride_b, padding_b, dilation_b, nspatial, 0, zero2, groups);
  auto check_grad = [&](const lamp_tensor* gy, const ConvGeom& g, const char* which) {
    LAMP_CHECK(gy->ndim == x->ndim && gy->sizes[0] == g.N && gy->sizes[1] == g.Cout && gy->sizes[gy->ndim - 1] == g.Wo && (nspatial == 1 || gy->sizes[2] == g.Ho),
               "convolution_backward_input_pair: the " << which << " grad_out " << gy->describe() << " does not match its forward output shape");
  };
  check_grad(grad_out_a, ga, "first"); check_grad(grad_out_b, gb, "second");
  if (x->dtype == kBF16 && nspatial == 2) {
    Hold wa(contiguous_filter(w_a)), wb(contiguous_filter(w_b)), gya(contiguous(grad_out_a)), gyb(contiguous(grad_out_b)), ac(addend ? contiguous(addend) : nullptr);
    hipStream_t st = current_stream(x->device());
    Hold dx(new_tensor(std::vector<int64_t>(x->sizes, x->sizes + x->ndim), x->dtype, x->device()));
    bool fused = false;
    if (narrow_conv_dgrad_pair(gya.get(), wa.get(), ga, gyb.get(), wb.get(), gb, dx.get(), st, ac.get(), &fused) ||
        igemm_conv_dgrad_pair(gya.get(), wa.get(), ga, gyb.get(), wb.get(), gb, dx.get(), st, ac.get(), &fused)) {
      if (ac.get() && !fused) {
        lamp_tensor* sum = nullptr;
        if (lamp_add(&sum, ac.get(), dx.get(), 1.0) != 0) throw Error(lamp_last_error());
        *out = sum;
      } else *out = dx.take();
      return 0;
    }
  }
  // the chain: the second gradient (+ addend), then the first one added to it (the order backprop reaches lamp's residual block in)
  const uint8_t m3[3] = {1, 0, 0};
  lamp_tensor* part = nullptr;
  if (addend) {
    if (lamp_convolution_backward_input_add(&part, grad_out_b, x, w_b, stride_b, padding_b, dilation_b, nspatial, zero2, groups, addend) != 0) throw Error(lamp_last_error());
  } else {
    lamp_tensor* r3[3] = {nullptr, nullptr, nullptr};
    if (lamp_convolution_backward(r3, grad_out_b, x, w_b, stride_b, padding_b, dilation_b, nspatial, 0, zero2, groups, m3) != 0) throw Error(lamp_last_error());
    part = r3[0];
  }
  Hold ph(part);
  if (lamp_convolution_backward_input_add(out, grad_out_a, x, w_a, stride_a, padding_a, dilation_a, nspatial, zero2, groups, ph.get()) != 0) throw Error(lamp_last_error());
  LAMP_API_END
}

int lamp_convolution_backward_weight_pair(lamp_tensor* out2[2], const lamp_tensor* x, const lamp_tensor* grad_out_a, const lamp_tensor* w_a,
                                          const int64_t* stride_a, const int64_t* padding_a, const int64_t* dilation_a,
                                          const lamp_tensor* grad_out_b, const lamp_tensor* w_b, const int64_t* stride_b,
                                          const int64_t* padding_b, const int64_t* dilation_b, int nspatial, int64_t groups) {
  LAMP_API_BEGIN
  check_device_tensor(x, "input"); check_device_tensor(w_a, "first weight"); check_device_tensor(grad_out_a, "first grad_out");
  check_device_tensor(w_b, "second weight"); check_device_tensor(grad_out_b, "second grad_out");
  LAMP_CHECK(x->dtype == w_a->dtype && x->dtype == w_b->dtype && grad_out_a->dtype == x->dtype && grad_out_b->dtype == x->dtype,
             "convolution_backward_weight_pair: dtype mismatch");
  LAMP_CHECK(nspatial >= 1 && nspatial <= 2, "convolution_backward_weight_pair: 1 or 2 spatial dimensions");
  const int64_t zero2[2] = {0, 0};
  ConvGeom ga = make_geom(x, w_a, stride_a, padding_a, dilation_a, nspatial, 0, zero2, groups);
  ConvGeom gb = make_geom(x, w_b, stride_b, padding_b, dilation_b, nspatial, 0, zero2, groups);
  auto check_grad = [&](const lamp_tensor* gy, const ConvGeom& g, const char* which) {
    LAMP_CHECK(gy->ndim == x->ndim && gy->sizes[0] == g.N && gy->sizes[1] == g.Cout && gy->sizes[gy->ndim - 1] == g.Wo && (nspatial == 1 || gy->sizes[2] == g.Ho),
               "convolution_backward_weight_pair: the " << which << " grad_out " << gy->describe() << " does not match its forward output shape");
  };
  check_grad(grad_out_a, ga, "first"); check_grad(grad_out_b, gb, "second");
  if (x->dtype == kBF16 && nspatial == 2) {
    Hold xc(contiguous(x)), wa(contiguous_filter(w_a)), wb(contiguous_filter(w_b)), gya(contiguous(grad_out_a)), gyb(contiguous(grad_out_b));
    hipStream_t st = current_stream(x->device());
    Hold dwa(new_like(wa.get())), dwb(new_like(wb.get()));
    if (narrow_conv_wgrad_pair(gya.get(), gyb.get(), xc.get(), dwa.get(), dwb.get(), ga, gb, st) ||
        igemm_conv_wgrad_pair(gya.get(), gyb.get(), xc.get(), dwa.get(), dwb.get(), ga, gb, st)) {
      out2[0] = dwa.take(); out2[1] = dwb.take();
      return 0;
    }
  }
  const uint8_t m3[3] = {0, 1, 0};
  lamp_tensor* ra[3] = {nullptr, nullptr, nullptr};
  if (lamp_convolution_backward(ra, grad_out_a, x, w_a, stride_a, padding_a, dilation_a, nspatial, 0, zero2, groups, m3) != 0) throw Error(lamp_last_error());
  Hold ha(ra[1]);
  lamp_tensor* rb[3] = {nullptr, nullptr, nullptr};
  if (lamp_convolution_backward(rb, grad_out_b, x, w_b, stride_b, padding_b, dilation_b, nspatial, 0, zero2, groups, m3) != 0) throw Error(lamp_last_error());
  out2[0] = ha.take(); out2[1] = rb[1];
  LAMP_API_END
}

int lamp_convolution_backward_pair(lamp_tensor* out3[3], const lamp_tensor* x, const lamp_tensor* grad_out_a, const lamp_tensor* w_a,
                                   const int64_t* stride_a, const int64_t* padding_a, const int64_t* dilation_a, const lamp_tensor* grad_out_b,
                                   const lamp_tensor* w_b, const int64_t* stride_b, const int64_t* padding_b, const int64_t* dilation_b, int nspatial,
                                   int64_t groups, const lamp_tensor* addend) {
  LAMP_API_BEGIN
  out3[0] = out3[1] = out3[2] = nullptr;
  check_device_tensor(x, "input"); check_device_tensor(w_a, "first weight"); check_device_tensor(grad_out_a, "first grad_out");
  check_device_tensor(w_b, "second weight"); check_device_tensor(grad_out_b, "second grad_out");
  if (addend) check_device_tensor(addend, "addend");
  const bool bf = x->dtype == kBF16 && w_a->dtype == kBF16 && w_b->dtype == kBF16 && grad_out_a->dtype == kBF16 && grad_out_b->dtype == kBF16 &&
                  (!addend || addend->dtype == kBF16);
  if (bf && nspatial == 2 && x->ndim == 4 && w_a->ndim == 4 && w_b->ndim == 4 && grad_out_a->ndim == 4 && grad_out_b->ndim == 4 &&
      (!addend || addend->shape() == x->shape())) {
    const int64_t zero2[2] = {0, 0};
    ConvGeom ga = make_geom(x, w_a, stride_a, padding_a, dilation_a, nspatial, 0, zero2, groups);
    ConvGeom gb = make_geom(x, w_b, stride_b, padding_b, dilation_b, nspatial, 0, zero2, groups);
    auto grad_ok = [&](const lamp_tensor* gy, const ConvGeom& g) { return gy->sizes[0] == g.N && gy->sizes[1] == g.Cout && gy->sizes[2] == g.Ho && gy->sizes[3] == g.Wo; };
    if (grad_ok(grad_out_a, ga) && grad_ok(grad_out_b, gb)) {
      Hold xc(contiguous(x)), wa(contiguous_filter(w_a)), wb(contiguous_filter(w_b)), gya(contiguous(grad_out_a)), gyb(contiguous(grad_out_b));
      Hold ac(addend ? contiguous(addend) : nullptr);
      hipStream_t st = current_stream(x->device());
      Hold dx(new_tensor(std::vector<int64_t>(x->sizes, x->sizes + x->ndim), x->dtype, x->device())), dwa(new_like(wa.get())), dwb(new_like(wb.get()));
      if (narrow_conv_backward_pair(gya.get(), gyb.get(), xc.get(), wa.get(), wb.get(), ga, gb, dx.get(), dwa.get(), dwb.get(), st, ac.get()) ||
          igemm_conv_backward_pair(gya.get(), gyb.get(), xc.get(), wa.get(), wb.get(), ga, gb, dx.get(), dwa.get(), dwb.get(), st, ac.get())) {
        out3[0] = dx.take(); out3[1] = dwa.take(); out3[2] = dwb.take();
        return 0;
      }
    }
  }
  // the two pair calls (each validates its own arguments)
  lamp_tensor* dxo = nullptr;
  if (lamp_convolution_backward_input_pair(&dxo, x, grad_out_a, w_a, stride_a, padding_a, dilation_a, grad_out_b, w_b, stride_b, padding_b, dilation_b, nspatial,
                                           groups, addend) != 0) throw Error(lamp_last_error());
  Hold hdx(dxo);
  lamp_tensor* o2[2] = {nullptr, nullptr};
  if (lamp_convolution_backward_weight_pair(o2, x, grad_out_a, w_a, stride_a, padding_a, dilation_a, grad_out_b, w_b, stride_b, padding_b, dilation_b, nspatial,
                                            groups) != 0) throw Error(lamp_last_error());
  out3[0] = hdx.take(); out3[1] = o2[0]; out3[2] = o2[1];
  LAMP_API_END
}

}  // extern "C"
