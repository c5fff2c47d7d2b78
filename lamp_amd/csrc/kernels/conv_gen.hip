// General-geometry implicit-GEMM convolution on the gfx950 matrix cores: forward, input gradient and weight gradient in bf16
// (v_mfma_f32_16x16x32_bf16, f32 accumulation, one rounding on the store) and f32 (v_mfma_f32_16x16x4_f32, exact fma chains).
//
// The backend behind Conv1D and Conv2DTransposed (lamp-core nn/Conv1D.scala, nn/Conv2DTransposed.scala; operator ops.scala:1547-1651):
// conv.hip asks it where the direct kernels ran before, for 1-D and transposed geometries.  It takes any kernel size, stride, padding,
// dilation, output padding, channel count and map size in groups == 1; f64 and grouped convolutions are declined (gen_plan says why).
//
// One kernel body serves the three passes.  Each is a product R[u][v] = sum_k P(u, k) Q(v, k), v being the index that is contiguous in the
// result (the D column of the MFMA, so the 16 lanes of a lane group store neighbouring elements):
//
//   pass    u (U)     v (V)                 k (K)                 P(u, k)            Q(v, k)
//   fwd     co Cout   (n, ho, wo) N Ho Wo   (ci, r, s) Cin kh kw  W[co][ci][r][s]    X[n][ci][ho sh - ph + r dh][wo sw - pw + s dw]
//   dgrad   ci Cin    (n, h, w)   N H W     (r, s, co) kh kw Cout W[co][ci][r][s]    dY[n][co][(h + ph - r dh) / sh][(w + pw - s dw) / sw]
//   wgrad   co Cout   (ci, r, s) Cin kh kw  (n, ho, wo) N Ho Wo   dY[n][co][ho][wo]  X[n][ci][ho sh - ph + r dh][wo sw - pw + s dw]
//
// Taps outside the image are zero by predicate (dgrad: also the taps whose position is not on the stride grid - the gather form; at
// stride s it multiplies s^2 times the needed work, decomposing by stride phase is left for later).  Nothing is padded or packed in
// memory: the filter is read as stored on every launch.  dgrad orders K as (r, s, co) so that a tap's validity and position, the
// divisions by the stride included, are worked out once per run of co and not per element (with (co, r, s) that arithmetic bound it).
//
// A workgroup of four waves owns a 64 x 64 tile of R and walks K in stages of 32.  NCHW operands are contiguous along pixels, not along
// K, and the bf16 MFMA wants eight consecutive k per lane: every thread therefore GATHERS the eight consecutive k of one row (u or v)
// of the stage into registers - lanes run along the operand's contiguous index, so the loads of a wave coalesce - and writes them to
// LDS as one 16-byte packet (f32: two) into rows [64][32 + pad].  That register pass is the transposition; the MFMA operands then come
// back as one ds_read_b128 per 16 x 32 fragment (f32: one value per lane and k-step of 4).  The next stage's gathers are issued before
// the MFMAs of the current one, one LDS buffer, two barriers per stage.  Row pads: 80 bytes (bf16) and 144 bytes (f32: the f32
// fragment read is conflict free, 16 rows x 4 k on 64 distinct banks).
//
// wgrad splits K (the pixels) over blockIdx.z; the f32 partial tiles go to a workspace [split][U][V] from the caching allocator on the
// launch stream and conv_gen_reduce_kernel adds them in split order: no floating-point atomics, bit-identical from run to run, every
// launch capturable.  Indices are 32-bit: gen_plan declines any operand or result of more than 2^31 - 1 elements.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include "device_utils.h"
#include "conv_geom.h"
#include "conv_backends.h"

namespace lamp {

constexpr int GEN_B = 64;          // tile edge, U and V
constexpr int GEN_K = 32;          // K per stage
constexpr int GEN_THREADS = 256;
constexpr int GEN_MAX_SPLITS = 128;
template <class T> constexpr int gen_ldk() { return sizeof(T) == 2 ? 40 : 36; }   // LDS row length in elements (32 + pad)

GenPlan gen_plan(int pass, int dtype, const ConvGeom& g, int cus) {
  GenPlan p{};
  p.pass = pass; p.dtype = dtype; p.BU = GEN_B; p.BV = GEN_B; p.BK = GEN_K; p.threads = GEN_THREADS; p.splits = 1;
  auto decline = [&](const char* why) { p.accepted = false; p.reason = why; return p; };
  if (pass < kGenFwd || pass > kGenWgrad) return decline("unknown pass");
  if (dtype != kBF16 && dtype != kF32) return decline("dtype: bf16 and f32 only, other types keep the direct kernels");
  if (g.groups != 1) return decline("groups: grouped convolutions keep the direct kernels");
  const int64_t khkw = (int64_t)g.kh * g.kw;
  const int64_t lim = INT32_MAX;
  // 32-bit indexing: every extent below is a factor of one of these three products
  if (g.N < 1 || g.Cin < 1 || g.Cout < 1 || g.H < 1 || g.W < 1 || g.Ho < 1 || g.Wo < 1 || khkw < 1) return decline("empty operand");
  auto numel_ok = [&](int64_t a, int64_t b, int64_t c, int64_t d) {
    return a <= lim && b <= lim / a && c <= lim / (a * b) && d <= lim / (a * b * c);
  };
  if (!numel_ok(g.N, g.Cin, g.H, g.W) || !numel_ok(g.N, g.Cout, g.Ho, g.Wo) || !numel_ok(g.Cout, g.Cin, g.kh, g.kw))
    return decline("size: an operand of more than 2^31 - 1 elements (the kernels index in 32 bits)");
  switch (pass) {
    case kGenFwd:   p.U = g.Cout; p.V = g.N * g.Ho * g.Wo; p.K = g.Cin * khkw; break;
    case kGenDgrad: p.U = g.Cin;  p.V = g.N * g.H * g.W;   p.K = g.Cout * khkw; break;
    default:        p.U = g.Cout; p.V = g.Cin * khkw;      p.K = g.N * g.Ho * g.Wo; break;
  }
  const int64_t tu = (p.U + GEN_B - 1) / GEN_B, tv = (p.V + GEN_B - 1) / GEN_B;
  if (tu > 65535) return decline("size: more than 65535 tiles of 64 channels");
  p.klen = (p.K + GEN_K - 1) / GEN_K * GEN_K;
  if (pass == kGenWgrad) {
    // enough workgroups for two per compute unit, no split shorter than four stages, at most GEN_MAX_SPLITS partial tiles per element
    const int64_t tiles = tu * tv;
    int64_t want = (2 * (int64_t)cus + tiles - 1) / tiles;
    want = std::max<int64_t>(1, std::min<int64_t>(want, GEN_MAX_SPLITS));
    int64_t klen = ((p.K + want - 1) / want + GEN_K - 1) / GEN_K * GEN_K;
    klen = std::max<int64_t>(klen, 4 * GEN_K);
    p.klen = klen;
    p.splits = (int)((p.K + klen - 1) / klen);
    // the workspace is indexed in 64 bits, but keep it a sane size: fall back to one pass over K
    if (p.splits > 1 && (double)p.splits * (double)p.U * (double)p.V * 4.0 > 1024.0 * 1024.0 * 1024.0) { p.splits = 1; p.klen = (p.K + GEN_K - 1) / GEN_K * GEN_K; }
  }
  p.ws_bytes = p.splits > 1 ? (size_t)p.splits * (size_t)p.U * (size_t)p.V * 4 : 0;
  p.lds_bytes = 2 * GEN_B * (dtype == kBF16 ? gen_ldk<bf16_t>() * 2 : gen_ldk<float>() * 4);
  p.grid = dim3((unsigned)tv, (unsigned)tu, (unsigned)p.splits);
  p.accepted = true; p.reason = "";
  return p;
}

struct GenArgs {
  const void* p;        // fwd, dgrad: the filter; wgrad: dY
  const void* q;        // fwd: X; dgrad: dY; wgrad: X
  const void* bias;     // [U] or nullptr
  void* out;
  float* ws;            // wgrad with splits > 1: [split][U][V]
  int N, Cin, H, W, Cout, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw;
  int U, V, K, klen, splits;
};

typedef __bf16 gen_bf8 __attribute__((ext_vector_type(8)));
typedef float gen_f4 __attribute__((ext_vector_type(4)));

template <class T> __device__ __forceinline__ T gen_zero();
template <> __device__ __forceinline__ float gen_zero<float>() { return 0.f; }
template <> __device__ __forceinline__ bf16_t gen_zero<bf16_t>() { bf16_t z; z.bits = 0; return z; }

// eight consecutive k of one row -> LDS row[kg * 8 ...]
template <class T> __device__ __forceinline__ void gen_put(T* row, int kg, const T (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    uint4 pk;
    pk.x = (unsigned)v[0].bits | ((unsigned)v[1].bits << 16); pk.y = (unsigned)v[2].bits | ((unsigned)v[3].bits << 16);
    pk.z = (unsigned)v[4].bits | ((unsigned)v[5].bits << 16); pk.w = (unsigned)v[6].bits | ((unsigned)v[7].bits << 16);
    *reinterpret_cast<uint4*>(row + kg * 8) = pk;
  } else {
    *reinterpret_cast<float4*>(row + kg * 8) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(row + kg * 8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

// x / s for the strides that occur (the general division is some forty instructions)
__device__ __forceinline__ int gen_div_stride(int x, int s) { return s == 1 ? x : s == 2 ? x >> 1 : x / s; }

// The operand along u.  u: the row this thread gathers; k0: its first k of the stage; kend: end of this workgroup's K range.
template <class T, int PASS>
__device__ __forceinline__ void gen_gather_p(const GenArgs& a, int u, int k0, int kend, T (&v)[8]) {
  const T* __restrict__ src = static_cast<const T*>(a.p);
  const bool uok = u < a.U;
  if constexpr (PASS == kGenFwd) {                       // W[u][k]
    const int base = u * a.K;
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = (uok && k0 + i < kend) ? src[base + k0 + i] : gen_zero<T>();
  } else if constexpr (PASS == kGenDgrad) {              // W[co][u][rs], k = (rs, co)
    const int khkw = a.kh * a.kw, step = a.Cin * khkw;
    int rs = k0 / a.Cout, co = k0 - rs * a.Cout;
    int idx = (co * a.Cin + u) * khkw + rs;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      v[i] = (uok && k0 + i < kend) ? src[idx] : gen_zero<T>();
      idx += step;
      if (++co == a.Cout) { co = 0; rs++; idx = u * khkw + rs; }
    }
  } else {                                               // dY[n][u][p], k = (n, p)
    const int hw = a.Ho * a.Wo;
    int n = k0 / hw, p = k0 - n * hw;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      v[i] = (uok && k0 + i < kend) ? src[(n * a.Cout + u) * hw + p] : gen_zero<T>();
      if (++p == hw) { p = 0; n++; }
    }
  }
}

// The operand along v.  c0, c1, c2: the row's own coordinates, decoded once per thread by gen_row_q.
struct GenRowQ { int ok, base, hb, wb; };
template <int PASS> __device__ __forceinline__ GenRowQ gen_row_q(const GenArgs& a, int v) {
  GenRowQ r;
  r.ok = v < a.V;
  if constexpr (PASS == kGenFwd) {                       // v = (n, ho, wo)
    const int hw = a.Ho * a.Wo, n = v / hw, p = v - n * hw, ho = p / a.Wo, wo = p - ho * a.Wo;
    r.base = n * a.Cin * a.H * a.W; r.hb = ho * a.sh - a.ph; r.wb = wo * a.sw - a.pw;
  } else if constexpr (PASS == kGenDgrad) {              // v = (n, h, w)
    const int hw = a.H * a.W, n = v / hw, p = v - n * hw, h = p / a.W, w = p - h * a.W;
    r.base = n * a.Cout * a.Ho * a.Wo; r.hb = h + a.ph; r.wb = w + a.pw;
  } else {                                               // v = (ci, r, s)
    const int khkw = a.kh * a.kw, ci = v / khkw, rs = v - ci * khkw, rr = rs / a.kw, ss = rs - rr * a.kw;
    r.base = ci * a.H * a.W; r.hb = rr * a.dh - a.ph; r.wb = ss * a.dw - a.pw;
  }
  if (!r.ok) { r.base = 0; r.hb = 0; r.wb = 0; }
  return r;
}
template <class T, int PASS>
__device__ __forceinline__ void gen_gather_q(const GenArgs& a, const GenRowQ& row, int k0, int kend, T (&v)[8]) {
  const T* __restrict__ src = static_cast<const T*>(a.q);
  if constexpr (PASS == kGenFwd) {                       // k = (ci, r, s)
    const int khkw = a.kh * a.kw;
    int ci = k0 / khkw, rs = k0 - ci * khkw, r = rs / a.kw, s = rs - r * a.kw;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int h = row.hb + r * a.dh, w = row.wb + s * a.dw;
      const bool ok = row.ok && k0 + i < kend && h >= 0 && h < a.H && w >= 0 && w < a.W;
      v[i] = ok ? src[row.base + (ci * a.H + h) * a.W + w] : gen_zero<T>();
      if (++s == a.kw) { s = 0; if (++r == a.kh) { r = 0; ci++; } }
    }
  } else if constexpr (PASS == kGenDgrad) {              // k = (r, s, co): the tap, its divisions by the stride included, once per run of co
    const int hw = a.Ho * a.Wo;
    int rs = k0 / a.Cout, co = k0 - rs * a.Cout, r = rs / a.kw, s = rs - r * a.kw;
    bool tap;                                            // this row meets an output position under tap (r, s) ...
    int off;                                             // ... at [ho][wo] = off
    auto set_tap = [&]() {
      const int hn = row.hb - r * a.dh, wn = row.wb - s * a.dw;
      const int ho = gen_div_stride(hn, a.sh), wo = gen_div_stride(wn, a.sw);
      tap = row.ok && hn >= 0 && wn >= 0 && ho * a.sh == hn && wo * a.sw == wn && ho < a.Ho && wo < a.Wo;
      off = ho * a.Wo + wo;
    };
    set_tap();
    int idx = row.base + co * hw;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      v[i] = (tap && k0 + i < kend) ? src[idx + off] : gen_zero<T>();
      idx += hw;
      if (++co == a.Cout) {
        co = 0; idx = row.base;
        if (++s == a.kw) { s = 0; r++; }
        set_tap();
      }
    }
  } else {                                               // k = (n, ho, wo)
    const int hw = a.Ho * a.Wo, chw = a.Cin * a.H * a.W;
    int n = k0 / hw, p = k0 - n * hw, ho = p / a.Wo, wo = p - ho * a.Wo;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int h = ho * a.sh + row.hb, w = wo * a.sw + row.wb;
      const bool ok = row.ok && k0 + i < kend && h >= 0 && h < a.H && w >= 0 && w < a.W;
      v[i] = ok ? src[n * chw + row.base + h * a.W + w] : gen_zero<T>();
      if (++wo == a.Wo) { wo = 0; if (++ho == a.Ho) { ho = 0; n++; } }
    }
  }
}

// Which index the lanes of a wave run along while gathering: the operand's contiguous one.  Row-major ("along rows"): thread t takes
// row t & 63 and k group t >> 6; k-major: row t >> 2 and k group t & 3 (four neighbouring lanes cover the 32 k of a stage).
template <int PASS> constexpr bool gen_p_kmajor() { return PASS != kGenDgrad; }
template <int PASS> constexpr bool gen_q_kmajor() { return PASS == kGenWgrad; }

template <class T, int PASS>
__global__ __launch_bounds__(GEN_THREADS) void conv_gen_kernel(GenArgs a) {
  constexpr int LDK = gen_ldk<T>();
  __shared__ __attribute__((aligned(16))) T ps[GEN_B * LDK];
  __shared__ __attribute__((aligned(16))) T qs[GEN_B * LDK];
  const int t = threadIdx.x;
  const int ub = blockIdx.y * GEN_B, vb = blockIdx.x * GEN_B;
  const int kbeg = blockIdx.z * a.klen, kend = min(a.K, kbeg + a.klen);
  const int prow = gen_p_kmajor<PASS>() ? t >> 2 : t & 63, pkg = gen_p_kmajor<PASS>() ? t & 3 : t >> 6;
  const int qrow = gen_q_kmajor<PASS>() ? t >> 2 : t & 63, qkg = gen_q_kmajor<PASS>() ? t & 3 : t >> 6;
  const GenRowQ rq = gen_row_q<PASS>(a, vb + qrow);

  const int lane = t & 63, wave = t >> 6, r = lane & 15, q = lane >> 4;
  // a wave owns 2 x 2 MFMA tiles (32 u x 32 v); where the workgroup holds at most 16 rows of u (few channels), one tile each, the four
  // waves side by side along v: no MFMA on rows that do not exist
  const bool narrow = a.U - ub <= 16;
  const int nt = narrow ? 1 : 2;
  const int wu = narrow ? 0 : (wave >> 1) * 32, wv = narrow ? wave * 16 : (wave & 1) * 32;
  gen_f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = gen_f4{0.f, 0.f, 0.f, 0.f};

  T pv[8], qv[8];
  gen_gather_p<T, PASS>(a, ub + prow, kbeg + pkg * 8, kend, pv);
  gen_gather_q<T, PASS>(a, rq, kbeg + qkg * 8, kend, qv);
  for (int k0 = kbeg; k0 < kend; k0 += GEN_K) {
    __syncthreads();                                     // the previous stage's fragment reads are done
    gen_put<T>(ps + prow * LDK, pkg, pv);
    gen_put<T>(qs + qrow * LDK, qkg, qv);
    __syncthreads();
    if (k0 + GEN_K < kend) {                             // in flight under the MFMAs below
      gen_gather_p<T, PASS>(a, ub + prow, k0 + GEN_K + pkg * 8, kend, pv);
      gen_gather_q<T, PASS>(a, rq, k0 + GEN_K + qkg * 8, kend, qv);
    }
    if constexpr (sizeof(T) == 2) {
      gen_bf8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        if (i < nt) {
          fa[i] = *reinterpret_cast<const gen_bf8*>(ps + (wu + i * 16 + r) * LDK + q * 8);
          fb[i] = *reinterpret_cast<const gen_bf8*>(qs + (wv + i * 16 + r) * LDK + q * 8);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
          if (i < nt && j < nt) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int kk = 0; kk < GEN_K / 4; kk++) {
        float fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
          if (i < nt) {
            fa[i] = ps[(wu + i * 16 + r) * LDK + kk * 4 + q];
            fb[i] = qs[(wv + i * 16 + r) * LDK + kk * 4 + q];
          }
        }
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++)
            if (i < nt && j < nt) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  // D[row = 4 q + reg][col = r]: rows are u, columns v
  T* __restrict__ out = static_cast<T*>(a.out);
  const T* __restrict__ bias = static_cast<const T*>(a.bias);
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int v = vb + wv + j * 16 + r;
    if (j >= nt || v >= a.V) continue;
    int vn = 0, vp = v, hw = 0, cu = 0;                  // fwd / dgrad: v = (n, pixel); the result is [n][u][pixel]
    if constexpr (PASS != kGenWgrad) {
      hw = PASS == kGenFwd ? a.Ho * a.Wo : a.H * a.W;
      cu = a.U;
      vn = v / hw; vp = v - vn * hw;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int u = ub + wu + i * 16 + q * 4 + e;
        if (i >= nt || u >= a.U) continue;
        float val = acc[i][j][e];
        if constexpr (PASS != kGenWgrad) {
          if (bias) val += load_as<float>(bias[u]);
          out[(vn * cu + u) * hw + vp] = store_as<T>(val);
        } else {
          if (a.splits > 1) a.ws[((size_t)blockIdx.z * a.U + u) * (size_t)a.V + v] = val;
          else out[u * a.V + v] = store_as<T>(val);
        }
      }
    }
  }
}

// dw[o] = sum over the splits, in split order
template <class T>
__global__ __launch_bounds__(256) void conv_gen_reduce_kernel(const float* __restrict__ ws, T* __restrict__ dw, int O, int splits) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= O) return;
  float s = 0.f;
  for (int z = 0; z < splits; z++) s += ws[(size_t)z * O + o];
  dw[o] = store_as<T>(s);
}

static GenArgs gen_args(const GenPlan& pl, const ConvGeom& g) {
  GenArgs a{};
  a.N = (int)g.N; a.Cin = (int)g.Cin; a.H = (int)g.H; a.W = (int)g.W; a.Cout = (int)g.Cout; a.Ho = (int)g.Ho; a.Wo = (int)g.Wo;
  a.kh = g.kh; a.kw = g.kw; a.sh = g.sh; a.sw = g.sw; a.ph = g.ph; a.pw = g.pw; a.dh = g.dh; a.dw = g.dw;
  a.U = (int)pl.U; a.V = (int)pl.V; a.K = (int)pl.K; a.klen = (int)pl.klen; a.splits = pl.splits;
  return a;
}

template <class T, int PASS> static void gen_launch(const GenPlan& pl, const GenArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((conv_gen_kernel<T, PASS>), pl.grid, dim3(pl.threads), 0, st, a);
  LAMP_LAUNCH_CHECK();
}
template <int PASS> static void gen_launch(const GenPlan& pl, const GenArgs& a, hipStream_t st) {
  if (pl.dtype == kBF16) gen_launch<bf16_t, PASS>(pl, a, st); else gen_launch<float, PASS>(pl, a, st);
}

bool gen_conv_fwd(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, hipStream_t st) {
  const GenPlan pl = gen_plan(kGenFwd, x->dtype, g, num_cus());
  if (!pl.accepted) return false;
  GenArgs a = gen_args(pl, g);
  a.p = w->raw(); a.q = x->raw(); a.bias = bias ? bias->raw() : nullptr; a.out = y->data();
  KernelTimer kt("conv_gen_fwd", conv_flops(g), conv_bytes(g, dtype_size(x->dtype)), st);
  gen_launch<kGenFwd>(pl, a, st);
  return true;
}

bool gen_conv_dgrad(const Tensor* dy, const Tensor* w, const Tensor* bias, Tensor* dx, const ConvGeom& g, hipStream_t st) {
  const GenPlan pl = gen_plan(kGenDgrad, dy->dtype, g, num_cus());
  if (!pl.accepted) return false;
  GenArgs a = gen_args(pl, g);
  a.p = w->raw(); a.q = dy->raw(); a.bias = bias ? bias->raw() : nullptr; a.out = dx->data();
  KernelTimer kt("conv_gen_dgrad", conv_flops(g), conv_bytes(g, dtype_size(dy->dtype)), st);
  gen_launch<kGenDgrad>(pl, a, st);
  return true;
}

bool gen_conv_wgrad(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st) {
  const GenPlan pl = gen_plan(kGenWgrad, dy->dtype, g, num_cus());
  if (!pl.accepted) return false;
  GenArgs a = gen_args(pl, g);
  a.p = dy->raw(); a.q = x->raw(); a.out = dw->data();
  Hold partial;
  if (pl.splits > 1) {
    int64_t ps[1] = {(int64_t)(pl.ws_bytes / 4)};
    partial = Hold(new_tensor(ps, 1, kF32, dy->device()));
    a.ws = partial->ptr<float>();
  }
  {
    KernelTimer kt("conv_gen_wgrad", conv_flops(g), conv_bytes(g, dtype_size(dy->dtype)), st);
    gen_launch<kGenWgrad>(pl, a, st);
  }
  if (pl.splits > 1) {
    const int O = (int)(pl.U * pl.V);
    KernelTimer kt("conv_gen_wgrad_reduce", (double)pl.splits * O, (double)pl.ws_bytes + (double)O * dtype_size(dy->dtype), st);
    if (pl.dtype == kBF16) hipLaunchKernelGGL((conv_gen_reduce_kernel<bf16_t>), dim3((O + 255) / 256), dim3(256), 0, st, a.ws, dw->ptr<bf16_t>(), O, pl.splits);
    else hipLaunchKernelGGL((conv_gen_reduce_kernel<float>), dim3((O + 255) / 256), dim3(256), 0, st, a.ws, dw->ptr<float>(), O, pl.splits);
    LAMP_LAUNCH_CHECK();
  }
  return true;
}

}  // namespace lamp

using namespace lamp;

extern "C" {

// Test tool, needs no GPU: the plan gen_conv_fwd / _dgrad / _wgrad (pass 0 / 1 / 2) would launch for this geometry, in ConvGeom's regular
// terms, on a device of `cus` compute units.  dims = {N, Cin, H, W, Cout, Ho, Wo}; taps = {kh, kw, sh, sw, ph, pw, dh, dw}.  key=value
// lines into buf; a declined plan has accepted=0 and its reason.
int lamp_debug_conv_gen_plan(int pass, int dtype, const int64_t* dims, const int* taps, int64_t groups, int cus, char* buf, int buflen) {
  LAMP_API_BEGIN
  LAMP_CHECK(dims && taps && buf && buflen > 0 && cus > 0, "lamp_debug_conv_gen_plan: bad arguments");
  ConvGeom g{};
  g.N = dims[0]; g.Cin = dims[1]; g.H = dims[2]; g.W = dims[3]; g.Cout = dims[4]; g.Ho = dims[5]; g.Wo = dims[6];
  g.kh = taps[0]; g.kw = taps[1]; g.sh = taps[2]; g.sw = taps[3]; g.ph = taps[4]; g.pw = taps[5]; g.dh = taps[6]; g.dw = taps[7];
  g.groups = groups;
  const GenPlan p = gen_plan(pass, dtype, g, cus);
  char text[768];
  const int n = snprintf(text, sizeof(text),
                         "accepted=%d\nreason=%s\npass=%d\ndtype=%d\nU=%lld\nV=%lld\nK=%lld\ntile_u=%d\ntile_v=%d\ntile_k=%d\ngrid_x=%u\ngrid_y=%u\ngrid_z=%u\n"
                         "threads=%d\nsplits=%d\nk_per_split=%lld\nworkspace_bytes=%zu\nlds_bytes=%d\nindex_bits=32\n",
                         p.accepted ? 1 : 0, p.reason, p.pass, p.dtype, (long long)p.U, (long long)p.V, (long long)p.K, p.BU, p.BV, p.BK, p.grid.x, p.grid.y,
                         p.grid.z, p.threads, p.splits, (long long)p.klen, p.ws_bytes, p.lds_bytes);
  LAMP_CHECK(n > 0 && n < buflen && n < (int)sizeof(text), "lamp_debug_conv_gen_plan: buffer too small");
  memcpy(buf, text, n + 1);
  LAMP_API_END
}

}  // extern "C"
