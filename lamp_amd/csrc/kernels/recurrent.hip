// Fused cell kernels of the recurrent modules (lamp-core/src/main/scala/lamp/nn/{LSTM,GRU,RNN}.scala), f32 and f64.
//
// The reference writes one time step as a chain of element-wise operators over [B, H] tensors (LSTM.scala:65-78: 9 adds,
// 3 sigmoids, 2 tanh, 3 multiplies; about twice that in its backward closures).  Here the host layer (host/recurrent.cpp) runs one
// GEMM for x.Wx + bias over all time steps, one GEMM per step for h.Wh accumulated onto it, and ONE of these kernels per step and
// direction (GRU: two, its candidate needs (r*h).Whh in between).
//
// All of them are bandwidth-bound maps over [B, H]: every operand is read once and every result written once, 16-byte packets
// where H and the row pitches allow it (a scalar form otherwise), no LDS, grid-stride loops bounded by B * H.  The gate buffer
// `G` is [B, nG * H] with row pitch ldg, the gates of one cell side by side (LSTM i | f | o | c, GRU r | z | h); everything else is
// [B, H] with its own row pitch.  Arithmetic is in the tensor's own type.
#include "device_utils.h"

namespace lamp {
namespace {

template <class T> __device__ __forceinline__ T rc_exp(T x);
template <> __device__ __forceinline__ float rc_exp(float x) { return expf(x); }
template <> __device__ __forceinline__ double rc_exp(double x) { return exp(x); }
template <class T> __device__ __forceinline__ T rc_tanh(T x);
template <> __device__ __forceinline__ float rc_tanh(float x) { return tanhf(x); }
template <> __device__ __forceinline__ double rc_tanh(double x) { return tanh(x); }
template <class T> __device__ __forceinline__ T rc_sigmoid(T x) { return T(1) / (T(1) + rc_exp<T>(-x)); }

template <class T, int V> __device__ __forceinline__ Vec<T, V> rc_load(const T* p) { return *reinterpret_cast<const Vec<T, V>*>(p); }
template <class T, int V> __device__ __forceinline__ Vec<T, V> rc_load_or_zero(const T* p, int64_t off) {
  if (p) return rc_load<T, V>(p + off);
  Vec<T, V> z;
#pragma unroll
  for (int k = 0; k < V; k++) z.v[k] = T(0);
  return z;
}
template <class T, int V> __device__ __forceinline__ void rc_store(T* p, const Vec<T, V>& x) { *reinterpret_cast<Vec<T, V>*>(p) = x; }

// one work item = V neighbouring columns of one row; hv = H / V
#define RC_ITEMS(b, j)                                                                                                        \
  const int64_t items = B * hv;                                                                                               \
  for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x)        \
    for (int64_t b = it / hv, j = (it - b * hv) * V, once = 1; once; once = 0)

// ---- LSTM (LSTM.scala:67-74) -----------------------------------------------------------------------------------------
// G: pre-activations in, activated gates i, f, o, c^ out (backward reads them).  c = f * c_prev + i * c^ ; h = o * tanh(c)
template <class T, int V>
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(T* __restrict__ G, int64_t ldg, const T* __restrict__ cprev, int64_t ldcp, T* __restrict__ h,
                                                            int64_t ldh, T* __restrict__ c, int64_t ldc, int64_t B, int64_t H, int64_t hv) {
  RC_ITEMS(b, j) {
    T* g = G + b * ldg + j;
    Vec<T, V> gi = rc_load<T, V>(g), gf = rc_load<T, V>(g + H), go = rc_load<T, V>(g + 2 * H), gc = rc_load<T, V>(g + 3 * H);
    const Vec<T, V> cp = rc_load<T, V>(cprev + b * ldcp + j);
    Vec<T, V> hn, cn;
#pragma unroll
    for (int k = 0; k < V; k++) {
      gi.v[k] = rc_sigmoid<T>(gi.v[k]);
      gf.v[k] = rc_sigmoid<T>(gf.v[k]);
      go.v[k] = rc_sigmoid<T>(go.v[k]);
      gc.v[k] = rc_tanh<T>(gc.v[k]);
      cn.v[k] = gf.v[k] * cp.v[k] + gi.v[k] * gc.v[k];
      hn.v[k] = go.v[k] * rc_tanh<T>(cn.v[k]);
    }
    rc_store<T, V>(g, gi); rc_store<T, V>(g + H, gf); rc_store<T, V>(g + 2 * H, go); rc_store<T, V>(g + 3 * H, gc);
    rc_store<T, V>(c + b * ldc + j, cn);
    rc_store<T, V>(h + b * ldh + j, hn);
  }
}
// dh = dout + dh_carry ; dc = dc_carry + dh * o * (1 - tanh(c)^2) ; dG = gate derivatives ; dc_prev = dc * f.
// dc_prev may alias dc_carry (every element is read before it is written, by the same thread).
template <class T, int V>
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(T* __restrict__ dG, int64_t lddg, T* dcprev, int64_t lddcp, const T* __restrict__ G, int64_t ldg,
                                                            const T* __restrict__ cprev, int64_t ldcp, const T* __restrict__ c, int64_t ldc,
                                                            const T* __restrict__ dout, int64_t lddo, const T* __restrict__ dh, int64_t lddh, const T* dc,
                                                            int64_t lddc, int64_t B, int64_t H, int64_t hv) {
  RC_ITEMS(b, j) {
    const T* g = G + b * ldg + j;
    const Vec<T, V> gi = rc_load<T, V>(g), gf = rc_load<T, V>(g + H), go = rc_load<T, V>(g + 2 * H), gc = rc_load<T, V>(g + 3 * H);
    const Vec<T, V> cp = rc_load<T, V>(cprev + b * ldcp + j), cv = rc_load<T, V>(c + b * ldc + j);
    const Vec<T, V> d1 = rc_load_or_zero<T, V>(dout, b * lddo + j), d2 = rc_load_or_zero<T, V>(dh, b * lddh + j), d3 = rc_load_or_zero<T, V>(dc, b * lddc + j);
    Vec<T, V> di, df, dO, dcc, dcp;
#pragma unroll
    for (int k = 0; k < V; k++) {
      const T dht = d1.v[k] + d2.v[k];
      const T tc = rc_tanh<T>(cv.v[k]);
      const T dct = d3.v[k] + dht * go.v[k] * (T(1) - tc * tc);
      dO.v[k] = dht * tc * go.v[k] * (T(1) - go.v[k]);
      di.v[k] = dct * gc.v[k] * gi.v[k] * (T(1) - gi.v[k]);
      df.v[k] = dct * cp.v[k] * gf.v[k] * (T(1) - gf.v[k]);
      dcc.v[k] = dct * gi.v[k] * (T(1) - gc.v[k] * gc.v[k]);
      dcp.v[k] = dct * gf.v[k];
    }
    T* d = dG + b * lddg + j;
    rc_store<T, V>(d, di); rc_store<T, V>(d + H, df); rc_store<T, V>(d + 2 * H, dO); rc_store<T, V>(d + 3 * H, dcc);
    rc_store<T, V>(dcprev + b * lddcp + j, dcp);
  }
}

// ---- GRU (GRU.scala:52-56) ---------------------------------------------------------------------------------------------
// first half: r, z = sigmoid (in place over G's first two blocks), rh = r * h_prev
template <class T, int V>
__global__ __launch_bounds__(256) void gru_gates_fwd_kernel(T* __restrict__ G, int64_t ldg, const T* __restrict__ hprev, int64_t ldhp, T* __restrict__ rh,
                                                            int64_t ldrh, int64_t B, int64_t H, int64_t hv) {
  RC_ITEMS(b, j) {
    T* g = G + b * ldg + j;
    Vec<T, V> gr = rc_load<T, V>(g), gz = rc_load<T, V>(g + H);
    const Vec<T, V> hp = rc_load<T, V>(hprev + b * ldhp + j);
    Vec<T, V> o;
#pragma unroll
    for (int k = 0; k < V; k++) {
      gr.v[k] = rc_sigmoid<T>(gr.v[k]);
      gz.v[k] = rc_sigmoid<T>(gz.v[k]);
      o.v[k] = gr.v[k] * hp.v[k];
    }
    rc_store<T, V>(g, gr); rc_store<T, V>(g + H, gz);
    rc_store<T, V>(rh + b * ldrh + j, o);
  }
}
// second half: h^ = tanh (in place over G's third block), h = z * h_prev + (1 - z) * h^
template <class T, int V>
__global__ __launch_bounds__(256) void gru_out_fwd_kernel(T* __restrict__ G, int64_t ldg, const T* __restrict__ hprev, int64_t ldhp, T* __restrict__ h,
                                                          int64_t ldh, int64_t B, int64_t H, int64_t hv) {
  RC_ITEMS(b, j) {
    T* g = G + b * ldg + j;
    const Vec<T, V> gz = rc_load<T, V>(g + H);
    Vec<T, V> gh = rc_load<T, V>(g + 2 * H);
    const Vec<T, V> hp = rc_load<T, V>(hprev + b * ldhp + j);
    Vec<T, V> o;
#pragma unroll
    for (int k = 0; k < V; k++) {
      gh.v[k] = rc_tanh<T>(gh.v[k]);
      o.v[k] = gz.v[k] * hp.v[k] + (gz.v[k] * T(-1) + T(1)) * gh.v[k];
    }
    rc_store<T, V>(g + 2 * H, gh);
    rc_store<T, V>(h + b * ldh + j, o);
  }
}
// backward, first half: dh = dout + dh_carry ; dG_h = dh (1 - z)(1 - h^2) ; dG_z = dh (h_prev - h^) z (1 - z) ; dh_prev = dh * z.
// dh_prev may alias dh_carry.
template <class T, int V>
__global__ __launch_bounds__(256) void gru_out_bwd_kernel(T* __restrict__ dG, int64_t lddg, T* dhprev, int64_t lddhp, const T* __restrict__ G, int64_t ldg,
                                                          const T* __restrict__ hprev, int64_t ldhp, const T* __restrict__ dout, int64_t lddo, const T* dh,
                                                          int64_t lddh, int64_t B, int64_t H, int64_t hv) {
  RC_ITEMS(b, j) {
    const T* g = G + b * ldg + j;
    const Vec<T, V> gz = rc_load<T, V>(g + H), gh = rc_load<T, V>(g + 2 * H);
    const Vec<T, V> hp = rc_load<T, V>(hprev + b * ldhp + j);
    const Vec<T, V> d1 = rc_load_or_zero<T, V>(dout, b * lddo + j), d2 = rc_load_or_zero<T, V>(dh, b * lddh + j);
    Vec<T, V> dz, dhh, dp;
#pragma unroll
    for (int k = 0; k < V; k++) {
      const T dht = d1.v[k] + d2.v[k];
      dhh.v[k] = dht * (T(1) - gz.v[k]) * (T(1) - gh.v[k] * gh.v[k]);
      dz.v[k] = dht * (hp.v[k] - gh.v[k]) * gz.v[k] * (T(1) - gz.v[k]);
      dp.v[k] = dht * gz.v[k];
    }
    T* d = dG + b * lddg + j;
    rc_store<T, V>(d + H, dz); rc_store<T, V>(d + 2 * H, dhh);
    rc_store<T, V>(dhprev + b * lddhp + j, dp);
  }
}
// backward, second half, after drh = dG_h . Whh^T: dG_r = drh * h_prev * r (1 - r) ; dh_prev += drh * r
template <class T, int V>
__global__ __launch_bounds__(256) void gru_gates_bwd_kernel(T* __restrict__ dG, int64_t lddg, T* __restrict__ dhprev, int64_t lddhp, const T* __restrict__ G,
                                                            int64_t ldg, const T* __restrict__ hprev, int64_t ldhp, const T* __restrict__ drh, int64_t lddrh,
                                                            int64_t B, int64_t H, int64_t hv) {
  RC_ITEMS(b, j) {
    const Vec<T, V> gr = rc_load<T, V>(G + b * ldg + j);
    const Vec<T, V> hp = rc_load<T, V>(hprev + b * ldhp + j), dr = rc_load<T, V>(drh + b * lddrh + j);
    Vec<T, V> dp = rc_load<T, V>(dhprev + b * lddhp + j);
    Vec<T, V> dgr;
#pragma unroll
    for (int k = 0; k < V; k++) {
      dgr.v[k] = dr.v[k] * hp.v[k] * gr.v[k] * (T(1) - gr.v[k]);
      dp.v[k] += dr.v[k] * gr.v[k];
    }
    rc_store<T, V>(dG + b * lddg + j, dgr);
    rc_store<T, V>(dhprev + b * lddhp + j, dp);
  }
}

// ---- RNN (RNN.scala:40) --------------------------------------------------------------------------------------------------
template <class T, int V>
__global__ __launch_bounds__(256) void rnn_cell_fwd_kernel(const T* __restrict__ G, int64_t ldg, T* __restrict__ h, int64_t ldh, int64_t B, int64_t H, int64_t hv) {
  RC_ITEMS(b, j) {
    Vec<T, V> g = rc_load<T, V>(G + b * ldg + j);
#pragma unroll
    for (int k = 0; k < V; k++) g.v[k] = rc_tanh<T>(g.v[k]);
    rc_store<T, V>(h + b * ldh + j, g);
  }
}
template <class T, int V>
__global__ __launch_bounds__(256) void rnn_cell_bwd_kernel(T* __restrict__ dG, int64_t lddg, const T* __restrict__ h, int64_t ldh, const T* __restrict__ dout,
                                                           int64_t lddo, const T* __restrict__ dh, int64_t lddh, int64_t B, int64_t H, int64_t hv) {
  RC_ITEMS(b, j) {
    const Vec<T, V> hv_ = rc_load<T, V>(h + b * ldh + j);
    const Vec<T, V> d1 = rc_load_or_zero<T, V>(dout, b * lddo + j), d2 = rc_load_or_zero<T, V>(dh, b * lddh + j);
    Vec<T, V> o;
#pragma unroll
    for (int k = 0; k < V; k++) o.v[k] = (d1.v[k] + d2.v[k]) * (T(1) - hv_.v[k] * hv_.v[k]);
    rc_store<T, V>(dG + b * lddg + j, o);
  }
}
#undef RC_ITEMS

// ---- host side: shape checks and the choice of the packet width -----------------------------------------------------------
struct Rows {              // a [B, cols] operand with unit column stride
  const Tensor* t;
  int64_t ld;
};
// every operand: 2-D, on the device of the first, of its dtype, unit column stride, B rows and `cols` columns
Rows rc_rows(const Tensor* t, const Tensor* first, int64_t B, int64_t cols, const char* what) {
  check_device_tensor(t, what);
  check_same_device(t, first);
  LAMP_CHECK(t->dtype == first->dtype, what << " " << t->describe() << " has another dtype than " << first->describe());
  LAMP_CHECK(t->ndim == 2 && t->sizes[0] == B && t->sizes[1] == cols, what << " " << t->describe() << " must be [" << B << ", " << cols << "]");
  LAMP_CHECK(t->strides[1] == 1 || cols == 1, what << " " << t->describe() << " must have unit column stride");
  LAMP_CHECK(t->strides[0] >= cols || B == 1, what << " " << t->describe() << ": rows overlap");
  return Rows{t, B == 1 ? cols : t->strides[0]};
}
template <class T> bool rc_packets_ok(int64_t H, std::initializer_list<Rows> ops) {
  constexpr int64_t W = 16 / sizeof(T);
  if (H % W) return false;
  for (const Rows& r : ops) {
    if (!r.t) continue;
    if (r.ld % W || ((uintptr_t)r.t->raw() & 15)) return false;
  }
  return true;
}
void rc_check_dtype(const Tensor* t, const char* fn) {
  LAMP_CHECK(t->dtype == kF32 || t->dtype == kF64, fn << ": f32 and f64 only, got " << t->describe() << " (other types take the composed chain)");
}
#define RC_DISPATCH(DT, T, ...)                      \
  if ((DT) == kF32) { using T = float; __VA_ARGS__; } \
  else { using T = double; __VA_ARGS__; }
#define RC_LAUNCH(KERNEL, TAG, NBYTES_PER_ELEM, PACKED, ...)                                                                      \
  do {                                                                                                                            \
    constexpr int W = 16 / sizeof(T);                                                                                             \
    KernelTimer kt(TAG, 0, (double)B * H * (NBYTES_PER_ELEM) * sizeof(T), st);                                                    \
    if (PACKED) { const int64_t hv = H / W; hipLaunchKernelGGL((KERNEL<T, W>), dim3(grid_for(B * hv, 256)), dim3(256), 0, st, __VA_ARGS__, B, H, hv); } \
    else { const int64_t hv = H; hipLaunchKernelGGL((KERNEL<T, 1>), dim3(grid_for(B * hv, 256)), dim3(256), 0, st, __VA_ARGS__, B, H, hv); }            \
    LAMP_LAUNCH_CHECK();                                                                                                          \
  } while (0)
const Rows kNone{nullptr, 0};

}  // namespace
}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_lstm_cell_forward(lamp_tensor* gates, const lamp_tensor* c_prev, lamp_tensor* h_out, lamp_tensor* c_out) {
  LAMP_API_BEGIN
  check_device_tensor(gates, "gates");
  rc_check_dtype(gates, "lamp_lstm_cell_forward");
  LAMP_CHECK(gates->ndim == 2 && gates->sizes[1] % 4 == 0, "gates " << gates->describe() << " must be [B, 4 * H]");
  const int64_t B = gates->sizes[0], H = gates->sizes[1] / 4;
  const Rows g = rc_rows(gates, gates, B, 4 * H, "gates"), cp = rc_rows(c_prev, gates, B, H, "c_prev"), h = rc_rows(h_out, gates, B, H, "h_out"),
             c = rc_rows(c_out, gates, B, H, "c_out");
  if (B * H == 0) return 0;
  hipStream_t st = current_stream(gates->device());
  RC_DISPATCH(gates->dtype, T, {
    const bool pk = rc_packets_ok<T>(H, {g, cp, h, c});
    RC_LAUNCH(lstm_cell_fwd_kernel, "lstm_cell_fwd", 11, pk, gates->ptr<T>(), g.ld, c_prev->ptr<T>(), cp.ld, h_out->ptr<T>(), h.ld, c_out->ptr<T>(), c.ld);
  })
  LAMP_API_END
}

int lamp_lstm_cell_backward(lamp_tensor* dgates, lamp_tensor* dc_prev, const lamp_tensor* gates, const lamp_tensor* c_prev, const lamp_tensor* c,
                            const lamp_tensor* dout_or_null, const lamp_tensor* dh_or_null, const lamp_tensor* dc_or_null) {
  LAMP_API_BEGIN
  check_device_tensor(gates, "gates");
  rc_check_dtype(gates, "lamp_lstm_cell_backward");
  LAMP_CHECK(gates->ndim == 2 && gates->sizes[1] % 4 == 0, "gates " << gates->describe() << " must be [B, 4 * H]");
  const int64_t B = gates->sizes[0], H = gates->sizes[1] / 4;
  const Rows g = rc_rows(gates, gates, B, 4 * H, "gates"), dg = rc_rows(dgates, gates, B, 4 * H, "dgates"), dcp = rc_rows(dc_prev, gates, B, H, "dc_prev"),
             cp = rc_rows(c_prev, gates, B, H, "c_prev"), cc = rc_rows(c, gates, B, H, "c");
  const Rows dO = dout_or_null ? rc_rows(dout_or_null, gates, B, H, "dout") : kNone, dh = dh_or_null ? rc_rows(dh_or_null, gates, B, H, "dh") : kNone,
             dc = dc_or_null ? rc_rows(dc_or_null, gates, B, H, "dc") : kNone;
  if (B * H == 0) return 0;
  hipStream_t st = current_stream(gates->device());
  RC_DISPATCH(gates->dtype, T, {
    const bool pk = rc_packets_ok<T>(H, {g, dg, dcp, cp, cc, dO, dh, dc});
    RC_LAUNCH(lstm_cell_bwd_kernel, "lstm_cell_bwd", 11 + (dO.t ? 1 : 0) + (dh.t ? 1 : 0) + (dc.t ? 1 : 0), pk, dgates->ptr<T>(), dg.ld, dc_prev->ptr<T>(),
              dcp.ld, gates->ptr<T>(), g.ld, c_prev->ptr<T>(), cp.ld, c->ptr<T>(), cc.ld, dO.t ? dO.t->ptr<T>() : nullptr, dO.ld,
              dh.t ? dh.t->ptr<T>() : nullptr, dh.ld, dc.t ? dc.t->ptr<T>() : nullptr, dc.ld);
  })
  LAMP_API_END
}

int lamp_gru_gates_forward(lamp_tensor* gates, const lamp_tensor* h_prev, lamp_tensor* rh_out) {
  LAMP_API_BEGIN
  check_device_tensor(gates, "gates");
  rc_check_dtype(gates, "lamp_gru_gates_forward");
  LAMP_CHECK(gates->ndim == 2 && gates->sizes[1] % 3 == 0, "gates " << gates->describe() << " must be [B, 3 * H]");
  const int64_t B = gates->sizes[0], H = gates->sizes[1] / 3;
  const Rows g = rc_rows(gates, gates, B, 3 * H, "gates"), hp = rc_rows(h_prev, gates, B, H, "h_prev"), rh = rc_rows(rh_out, gates, B, H, "rh_out");
  if (B * H == 0) return 0;
  hipStream_t st = current_stream(gates->device());
  RC_DISPATCH(gates->dtype, T, {
    const bool pk = rc_packets_ok<T>(H, {g, hp, rh});
    RC_LAUNCH(gru_gates_fwd_kernel, "gru_gates_fwd", 6, pk, gates->ptr<T>(), g.ld, h_prev->ptr<T>(), hp.ld, rh_out->ptr<T>(), rh.ld);
  })
  LAMP_API_END
}

int lamp_gru_output_forward(lamp_tensor* gates, const lamp_tensor* h_prev, lamp_tensor* h_out) {
  LAMP_API_BEGIN
  check_device_tensor(gates, "gates");
  rc_check_dtype(gates, "lamp_gru_output_forward");
  LAMP_CHECK(gates->ndim == 2 && gates->sizes[1] % 3 == 0, "gates " << gates->describe() << " must be [B, 3 * H]");
  const int64_t B = gates->sizes[0], H = gates->sizes[1] / 3;
  const Rows g = rc_rows(gates, gates, B, 3 * H, "gates"), hp = rc_rows(h_prev, gates, B, H, "h_prev"), h = rc_rows(h_out, gates, B, H, "h_out");
  if (B * H == 0) return 0;
  hipStream_t st = current_stream(gates->device());
  RC_DISPATCH(gates->dtype, T, {
    const bool pk = rc_packets_ok<T>(H, {g, hp, h});
    RC_LAUNCH(gru_out_fwd_kernel, "gru_output_fwd", 5, pk, gates->ptr<T>(), g.ld, h_prev->ptr<T>(), hp.ld, h_out->ptr<T>(), h.ld);
  })
  LAMP_API_END
}

int lamp_gru_output_backward(lamp_tensor* dgates, lamp_tensor* dh_prev, const lamp_tensor* gates, const lamp_tensor* h_prev, const lamp_tensor* dout_or_null,
                             const lamp_tensor* dh_or_null) {
  LAMP_API_BEGIN
  check_device_tensor(gates, "gates");
  rc_check_dtype(gates, "lamp_gru_output_backward");
  LAMP_CHECK(gates->ndim == 2 && gates->sizes[1] % 3 == 0, "gates " << gates->describe() << " must be [B, 3 * H]");
  const int64_t B = gates->sizes[0], H = gates->sizes[1] / 3;
  const Rows g = rc_rows(gates, gates, B, 3 * H, "gates"), dg = rc_rows(dgates, gates, B, 3 * H, "dgates"), dhp = rc_rows(dh_prev, gates, B, H, "dh_prev"),
             hp = rc_rows(h_prev, gates, B, H, "h_prev");
  const Rows dO = dout_or_null ? rc_rows(dout_or_null, gates, B, H, "dout") : kNone, dh = dh_or_null ? rc_rows(dh_or_null, gates, B, H, "dh") : kNone;
  if (B * H == 0) return 0;
  hipStream_t st = current_stream(gates->device());
  RC_DISPATCH(gates->dtype, T, {
    const bool pk = rc_packets_ok<T>(H, {g, dg, dhp, hp, dO, dh});
    RC_LAUNCH(gru_out_bwd_kernel, "gru_output_bwd", 6 + (dO.t ? 1 : 0) + (dh.t ? 1 : 0), pk, dgates->ptr<T>(), dg.ld, dh_prev->ptr<T>(), dhp.ld, gates->ptr<T>(),
              g.ld, h_prev->ptr<T>(), hp.ld, dO.t ? dO.t->ptr<T>() : nullptr, dO.ld, dh.t ? dh.t->ptr<T>() : nullptr, dh.ld);
  })
  LAMP_API_END
}

int lamp_gru_gates_backward(lamp_tensor* dgates, lamp_tensor* dh_prev, const lamp_tensor* gates, const lamp_tensor* h_prev, const lamp_tensor* drh) {
  LAMP_API_BEGIN
  check_device_tensor(gates, "gates");
  rc_check_dtype(gates, "lamp_gru_gates_backward");
  LAMP_CHECK(gates->ndim == 2 && gates->sizes[1] % 3 == 0, "gates " << gates->describe() << " must be [B, 3 * H]");
  const int64_t B = gates->sizes[0], H = gates->sizes[1] / 3;
  const Rows g = rc_rows(gates, gates, B, 3 * H, "gates"), dg = rc_rows(dgates, gates, B, 3 * H, "dgates"), dhp = rc_rows(dh_prev, gates, B, H, "dh_prev"),
             hp = rc_rows(h_prev, gates, B, H, "h_prev"), dr = rc_rows(drh, gates, B, H, "drh");
  if (B * H == 0) return 0;
  hipStream_t st = current_stream(gates->device());
  RC_DISPATCH(gates->dtype, T, {
    const bool pk = rc_packets_ok<T>(H, {g, dg, dhp, hp, dr});
    RC_LAUNCH(gru_gates_bwd_kernel, "gru_gates_bwd", 6, pk, dgates->ptr<T>(), dg.ld, dh_prev->ptr<T>(), dhp.ld, gates->ptr<T>(), g.ld, h_prev->ptr<T>(), hp.ld,
              drh->ptr<T>(), dr.ld);
  })
  LAMP_API_END
}

int lamp_rnn_cell_forward(const lamp_tensor* gates, lamp_tensor* h_out) {
  LAMP_API_BEGIN
  check_device_tensor(gates, "gates");
  rc_check_dtype(gates, "lamp_rnn_cell_forward");
  LAMP_CHECK(gates->ndim == 2, "gates " << gates->describe() << " must be [B, H]");
  const int64_t B = gates->sizes[0], H = gates->sizes[1];
  const Rows g = rc_rows(gates, gates, B, H, "gates"), h = rc_rows(h_out, gates, B, H, "h_out");
  if (B * H == 0) return 0;
  hipStream_t st = current_stream(gates->device());
  RC_DISPATCH(gates->dtype, T, {
    const bool pk = rc_packets_ok<T>(H, {g, h});
    RC_LAUNCH(rnn_cell_fwd_kernel, "rnn_cell_fwd", 2, pk, gates->ptr<T>(), g.ld, h_out->ptr<T>(), h.ld);
  })
  LAMP_API_END
}

int lamp_rnn_cell_backward(lamp_tensor* dgates, const lamp_tensor* h, const lamp_tensor* dout_or_null, const lamp_tensor* dh_or_null) {
  LAMP_API_BEGIN
  check_device_tensor(h, "h");
  rc_check_dtype(h, "lamp_rnn_cell_backward");
  LAMP_CHECK(h->ndim == 2, "h " << h->describe() << " must be [B, H]");
  const int64_t B = h->sizes[0], H = h->sizes[1];
  const Rows hh = rc_rows(h, h, B, H, "h"), dg = rc_rows(dgates, h, B, H, "dgates");
  const Rows dO = dout_or_null ? rc_rows(dout_or_null, h, B, H, "dout") : kNone, dh = dh_or_null ? rc_rows(dh_or_null, h, B, H, "dh") : kNone;
  if (B * H == 0) return 0;
  hipStream_t st = current_stream(h->device());
  RC_DISPATCH(h->dtype, T, {
    const bool pk = rc_packets_ok<T>(H, {hh, dg, dO, dh});
    RC_LAUNCH(rnn_cell_bwd_kernel, "rnn_cell_bwd", 2 + (dO.t ? 1 : 0) + (dh.t ? 1 : 0), pk, dgates->ptr<T>(), dg.ld, h->ptr<T>(), hh.ld,
              dO.t ? dO.t->ptr<T>() : nullptr, dO.ld, dh.t ? dh.t->ptr<T>() : nullptr, dh.ld);
  })
  LAMP_API_END
}

}  // extern "C"
