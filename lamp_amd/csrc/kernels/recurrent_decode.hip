// Recurrent text generation: one new token per row through Embedding -> RNN | GRU | LSTM (host/text.cpp; the reference runs the module's
// sequence-shaped forward at T = 1 for every token, lamp-core/src/main/scala/lamp/nn/FreeRunningRNN.scala, lamp-data/.../Text.scala:18-135).
// f32 and f64, R <= 16 rows: as in decode.hip every product is a weight-streaming problem, so the weights go from memory to registers in
// 16-byte packets and the cell is the epilogue of the product.
//
//   recurrent_decode_pack_kernel   once per generation: Wx over Wh as one [E + H, nG * H] matrix whose columns are gate-interleaved (column
//                                  j * nG + g is gate g of hidden unit j; LSTM i f o c, GRU r z h^, RNN h), the biases in the same order.  GRU:
//                                  the candidate's rows below E are zero, its Whh goes to a matrix of its own for the second phase.
//   recurrent_decode_step_kernel   gates[r] = bias + table[tokens[r]] . Wx + state[parent[r]] . Wh, then the cell of kernels/recurrent.hip: an
//                                  operation of the body decode_stream_body.h (which holds the stream loop, the wave and slab
//                                  reductions and the ticket protocol).  The operation checks the rows' tokens and parents, gives the image
//                                  (the gathered embedding row, then the state row) and applies the cell to a lane's CL neighbouring columns =
//                                  whole hidden units (LSTM 4 = one unit, GRU 3 = one unit, RNN one packet of units).  GRU takes two launches:
//                                  the first produces z, r * h and the candidate's x . Wxh + bh, the second adds (r * h) . Whh and produces h.
//   log_softmax_argmax_rows_kernel a workgroup per row: maximum, sum of exp, logits - max - log(sum) stored (or the logits passed through),
//                                  then the index of the largest STORED value, lowest index among equals, NaN first as lamp_argmax has it.
// No kernel uses a floating atomic and every sum has a fixed order: the results are functions of the inputs, bit for bit.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), recurrent_decode_step_kernel at 1 / 2 .. 4 / 5 .. 16 rows:
//   LSTM (a unit = one f32 packet, two f64 packets)   f32  64 /  76 / 132 VGPRs     f64 104 / 128 / 232
//   GRU, first launch (three columns, element loads)  f32  68 /  74 / 106           f64  86 / 104 / 182
//   RNN and GRU's second launch, packet form          f32  64 /  76 / 128           f64  67 /  76 / 128 (126 in the second launch)
//   the same, element form                            f32  44 /  68 /  72           f64  59 /  66 /  80
// log_softmax_argmax_rows_kernel 22 (f32) and 51 (f64), the pack kernel 21.  No kernel of this file uses scratch memory.
#include "decode_stream.h"

namespace lamp {
namespace {

// ---- pack -----------------------------------------------------------------------------------------------------------------------------------
template <class T> struct RdPack {
  const T* wx[4]; const T* wh[4]; const T* b[4];   // per gate; a null wh: zeros (GRU's candidate)
  T* w; T* bias;
  int64_t E, H;
  int nG;
};
template <class T>
__global__ __launch_bounds__(256) void recurrent_decode_pack_kernel(RdPack<T> p) {
  const int64_t N = p.nG * p.H, total = (p.E + p.H + 1) * N;   // the last "row" is the bias
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = i / N, n = i - k * N, j = n / p.nG;
    const int g = (int)(n - j * p.nG);
    if (k < p.E) p.w[i] = p.wx[g][k * p.H + j];
    else if (k < p.E + p.H) p.w[i] = p.wh[g] ? p.wh[g][(k - p.E) * p.H + j] : T(0);
    else p.bias[n] = p.b[g][j];
  }
}

// ---- step -----------------------------------------------------------------------------------------------------------------------------------
template <class T> struct RdStep {
  const T* table; const int64_t* tokens; const int64_t* parent;
  const T* src;                       // the rows multiplied by the lower part of w: h_prev [Rp, H] through parent; second phase: r * h [R, H]
  const T* w; const T* bias;          // [E + H, N], [N]
  const T* hprev; const T* cprev;     // the cell's previous state [Rp, H], rows through parent
  const T* z; const T* pre;           // second phase: z and the candidate's x . Wxh + bh of the first, [R, H]
  T* h; T* c; T* relu;                // [R, H]; relu may be null
  T* zo; T* rho; T* preo;             // first phase of GRU
  T* slab; unsigned* ticket; int* assert_word;
  int64_t tstride, Vt, E, H, N;
  int R, Rp, Kc, S;
};

// the cell on the sums `a` of the lane's CL columns n0 .. n0 + CL - 1 of row r; pr: the row of the previous state (-1: reads as zeros)
template <class T, int CELL, int CL>
__device__ __forceinline__ void rd_cell(const T (&a)[CL], int r, int pr, int64_t n0, const RdStep<T>& p) {
  const int64_t H = p.H;
  if constexpr (CELL == LAMP_RECURRENT_LSTM) {          // CL == 4: i f o c of unit j (LSTM.scala:67-74, lstm_cell_fwd_kernel)
    const int64_t j = n0 / 4;
    const T gi = dec_sigmoid(a[0] + p.bias[n0]), gf = dec_sigmoid(a[1] + p.bias[n0 + 1]), go = dec_sigmoid(a[2] + p.bias[n0 + 2]);
    const T gc = dec_tanh(a[3] + p.bias[n0 + 3]);
    const T cp = pr >= 0 ? p.cprev[(int64_t)pr * H + j] : T(0);
    const T cn = gf * cp + gi * gc;
    const T hn = go * dec_tanh(cn);
    p.c[(int64_t)r * H + j] = cn;
    p.h[(int64_t)r * H + j] = hn;
    if (p.relu) p.relu[(int64_t)r * H + j] = hn > T(0) ? hn : T(0);
  } else if constexpr (CELL == LAMP_RECURRENT_GRU) {    // CL == 3: r z h^ of unit j (GRU.scala:52-54, gru_gates_fwd_kernel)
    const int64_t j = n0 / 3;
    const T gr = dec_sigmoid(a[0] + p.bias[n0]), gz = dec_sigmoid(a[1] + p.bias[n0 + 1]);
    const T hp = pr >= 0 ? p.hprev[(int64_t)pr * H + j] : T(0);
    p.zo[(int64_t)r * H + j] = gz;
    p.rho[(int64_t)r * H + j] = gr * hp;
    p.preo[(int64_t)r * H + j] = a[2] + p.bias[n0 + 2];
  } else {
#pragma unroll
    for (int u = 0; u < CL; u++) {
      const int64_t j = n0 + u;
      T hn;
      if constexpr (CELL == kDecFormGru2) {                  // GRU.scala:54-56, gru_out_fwd_kernel
        const T gz = p.z[(int64_t)r * H + j], gh = dec_tanh(p.pre[(int64_t)r * H + j] + a[u]);
        const T hp = pr >= 0 ? p.hprev[(int64_t)pr * H + j] : T(0);
        hn = gz * hp + (gz * T(-1) + T(1)) * gh;
      } else {                                // RNN.scala:40
        hn = dec_tanh(a[u] + p.bias[j]);
      }
      p.h[(int64_t)r * H + j] = hn;
      if (p.relu) p.relu[(int64_t)r * H + j] = hn > T(0) ? hn : T(0);
    }
  }
}

// the operation of decode_stream_body.h: the image is the gathered embedding row over the state row, the finished sums of a lane's
// CL columns (whole hidden units, N % CL == 0) go through rd_cell.  CL columns in CL / V packets; V > 1 only when N % V == 0 and w is
// 16-byte aligned.
template <class T, int CELL, int CL, int RT> struct RdStepOp {
  const RdStep<T>& p;
  long long* tok;                     // LDS [RT]: the row's token, -1 outside the table
  int* irow; int* prow;               // LDS [RT]: the row of src for the image, the row of the previous state for the cell; -1 outside
  __device__ __forceinline__ void prepare(int tid, int, int) {
    if (tid < RT) {
      long long t = -1;
      int pr = -1;
      if (tid < p.R) {
        if (p.E > 0) {
          t = p.tokens[(int64_t)tid * p.tstride];
          if (t < 0 || t >= p.Vt) { t = -1; *(volatile int*)p.assert_word = kAssertIndexRange; }   // the bound is tested before an address is formed
        }
        const int64_t q = p.parent ? p.parent[tid] : (int64_t)tid;
        if (q < 0 || q >= p.Rp) *(volatile int*)p.assert_word = kAssertIndexRange;
        else pr = (int)q;
      }
      tok[tid] = t;
      prow[tid] = pr;
      irow[tid] = CELL == kDecFormGru2 ? (tid < p.R ? tid : -1) : pr;
    }
    __syncthreads();
  }
  __device__ __forceinline__ T image(int r, int64_t k) const {
    T v = T(0);
    if (k < p.E) { if (tok[r] >= 0) v = p.table[(int64_t)tok[r] * p.E + k]; }
    else if (irow[r] >= 0) v = p.src[(int64_t)irow[r] * p.H + (k - p.E)];
    return v;
  }
  __device__ __forceinline__ void finish(const T (&a)[CL], int r, int64_t n0) const { rd_cell<T, CELL, CL>(a, r, prow[r], n0, p); }
};
template <class T, int CELL, int CL, int V, int RT>
__global__ __launch_bounds__(64 * kDecWaves) void recurrent_decode_step_kernel(RdStep<T> p) {
  __shared__ long long tok[RT];
  __shared__ int irow[RT], prow[RT];
  RdStepOp<T, CELL, CL, RT> op{p, tok, irow, prow};
  const int64_t K = p.E + p.H;
#include "decode_stream_body.h"
}

// ---- log-softmax + argmax -------------------------------------------------------------------------------------------------------------------
// grid R, 256 threads.  LSM: out = x - max - log(sum exp(x - max)) with the roundings of softmax_fwd_kernel (a NaN in the row makes the sum
// and so every output a NaN); otherwise out = x.  The token is the argmax of what was stored: the first NaN if there is one (lamp_argmax),
// else the largest value's lowest index.
template <class T, bool LSM>
__global__ __launch_bounds__(256) void log_softmax_argmax_rows_kernel(const T* __restrict__ x, int64_t xstride, T* __restrict__ out, int64_t ostride,
                                                                      int64_t* __restrict__ token, int64_t tstride, int64_t V) {
  __shared__ T red[4];
  __shared__ T bestv[256];
  __shared__ long long besti[256];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const T* xr = x + row * xstride;
  T* orow = out + row * ostride;
  T m = T(0), ls = T(0);
  if (LSM) {
    m = -INFINITY;
    for (int64_t i = tid; i < V; i += 256) { const T v = xr[i]; m = v > m ? v : m; }
    m = block_max(m, red);
    T s = T(0);
    for (int64_t i = tid; i < V; i += 256) s += dec_exp(xr[i] - m);
    s = block_sum(s, red);
    ls = dec_log(s);
  }
  // ascending indices per thread, lamp_argmax's rule: a larger value or the first NaN replaces the best
  T best = T(0);
  long long bi = -1;
  for (int64_t i = tid; i < V; i += 256) {
    const T v = LSM ? (T)(xr[i] - m - ls) : xr[i];
    orow[i] = v;
    if (bi < 0 || v > best || (v != v && best == best)) { best = v; bi = i; }
  }
  bestv[tid] = best; besti[tid] = bi;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      const T a = bestv[tid], b = bestv[tid + off];
      const long long ia = besti[tid], ib = besti[tid + off];
      bool take = false;                     // does b replace a?
      if (ib >= 0) {
        if (ia < 0) take = true;
        else if (b != b) take = a == a || ib < ia;                  // a NaN beats a number, the earlier of two NaNs wins
        else if (a == a) take = b > a || (b == a && ib < ia);
      }
      if (take) { bestv[tid] = b; besti[tid] = ib; }
    }
    __syncthreads();
  }
  if (tid == 0) token[row * tstride] = besti[0];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
template <class T, int CELL, int CL, int V>
void rd_launch(const RdStep<T>& p, const DecForm& f, const DecPlan& pl, hipStream_t st) {
  LAMP_CHECK(f.CL == CL && f.V == V, "the step kernel <" << CL << ", " << V << "> is not the planned form <" << f.CL << ", " << f.V << ">");
  dec_rt_ladder(p.R, [&](auto rt) {
    hipLaunchKernelGGL((recurrent_decode_step_kernel<T, CELL, CL, V, decltype(rt)::value>), pl.grid, pl.block, 0, st, p);
  });
}

// p holds the operands, R, E, H and N; the form is dec_form's, the tiling dec_plan's.  `slab` keeps the slabs alive for the caller.
template <class T>
void rd_step_run(RdStep<T> p, int cell, int dev, hipStream_t st, Hold& slab) {
  constexpr int VW = 16 / (int)sizeof(T);
  const DecForm f = dec_form(cell, p.N, sizeof(T), dec_aligned({p.w}));
  const DecPlan pl = dec_plan(p.E + p.H, p.N, p.R, f.CL, sizeof(T), sizeof(acc_t<T>), num_cus());
  dec_plan_apply<acc_t<T>>(p, pl, dev, st, slab);
  const bool vec = f.V > 1;
  switch (cell) {
    case LAMP_RECURRENT_LSTM:
      if (vec) rd_launch<T, LAMP_RECURRENT_LSTM, 4, VW>(p, f, pl, st); else rd_launch<T, LAMP_RECURRENT_LSTM, 4, 1>(p, f, pl, st);
      break;
    case LAMP_RECURRENT_GRU: rd_launch<T, LAMP_RECURRENT_GRU, 3, 1>(p, f, pl, st); break;
    case kDecFormGru2:
      if (vec) rd_launch<T, kDecFormGru2, VW, VW>(p, f, pl, st); else rd_launch<T, kDecFormGru2, 1, 1>(p, f, pl, st);
      break;
    default:
      if (vec) rd_launch<T, LAMP_RECURRENT_RNN, VW, VW>(p, f, pl, st); else rd_launch<T, LAMP_RECURRENT_RNN, 1, 1>(p, f, pl, st);
      break;
  }
}

int rd_gates(int kind) { return kind == LAMP_RECURRENT_LSTM ? 4 : kind == LAMP_RECURRENT_GRU ? 3 : 1; }
void rd_check_kind(int kind) {
  LAMP_CHECK(kind == LAMP_RECURRENT_RNN || kind == LAMP_RECURRENT_GRU || kind == LAMP_RECURRENT_LSTM,
             "kind must be LAMP_RECURRENT_RNN, _GRU or _LSTM, got " << kind);
}

}  // namespace
}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_recurrent_decode_pack(lamp_tensor** w_out, lamp_tensor** bias_out, lamp_tensor** wh2_out_or_null, int kind, lamp_tensor* const* tensors, int n) {
  LAMP_API_BEGIN
  rd_check_kind(kind);
  LAMP_CHECK(n == (kind == LAMP_RECURRENT_LSTM ? 12 : kind == LAMP_RECURRENT_GRU ? 9 : 3), "the module's " << (kind == LAMP_RECURRENT_LSTM ? 12 : kind == LAMP_RECURRENT_GRU ? 9 : 3)
                                                                                                   << " state tensors in `state` order, got " << n);
  for (int i = 0; i < n; i++) { LAMP_CHECK(tensors[i], "NULL state tensor"); check_device_tensor(tensors[i], "state tensor"); }
  const int dt = tensors[0]->dtype, dev = tensors[0]->device();
  LAMP_CHECK(dt == kF32 || dt == kF64, "f32 or f64, got " << tensors[0]->describe());
  // per gate: the indices of Wx, Wh (-1: none) and the bias in `state` order (LSTM.scala:28-42, GRU.scala:27-38, RNN.scala:20-25)
  static const int lstm[4][3] = {{0, 3, 8}, {1, 4, 9}, {2, 5, 10}, {6, 7, 11}};
  static const int gru[3][3] = {{2, 4, 6}, {3, 5, 7}, {0, -1, 8}};
  static const int rnn[1][3] = {{0, 1, 2}};
  const int (*map)[3] = kind == LAMP_RECURRENT_LSTM ? lstm : kind == LAMP_RECURRENT_GRU ? gru : rnn;
  const int nG = rd_gates(kind);
  LAMP_CHECK(tensors[map[0][0]]->ndim == 2, "the input weights must be [in, hidden], got " << tensors[map[0][0]]->describe());
  const int64_t E = tensors[map[0][0]]->sizes[0], H = tensors[map[0][0]]->sizes[1];
  LAMP_CHECK(E >= 1 && H >= 1, "empty weights " << tensors[map[0][0]]->describe());
  LAMP_CHECK(wh2_out_or_null || kind != LAMP_RECURRENT_GRU, "GRU: wh2_out receives the candidate's recurrent weights");
  std::vector<Hold> keep;
  auto dense = [&](int idx, int64_t rows, int64_t cols, bool vector_ok) {
    const lamp_tensor* t = tensors[idx];
    const bool ok = t->dtype == dt && t->device() == dev &&
                    ((t->ndim == 2 && t->sizes[0] == rows && t->sizes[1] == cols) || (vector_ok && t->ndim == 1 && t->sizes[0] == cols));
    LAMP_CHECK(ok, "state tensor " << idx << " must be [" << rows << ", " << cols << "] of the first one's type and device, got " << t->describe());
    keep.emplace_back(contiguous(t));
    return keep.back().get();
  };
  int64_t ws[2] = {E + H, nG * H}, bs[1] = {nG * H};
  Hold w(new_tensor(ws, 2, dt, dev)), b(new_tensor(bs, 1, dt, dev));
  hipStream_t st = current_stream(dev);
  const int64_t total = (E + H + 1) * nG * H;
  KernelTimer kt("recurrent_decode_pack", 0.0, 2.0 * (double)total * (double)dtype_size(dt), st);
#define RD_PACK(T)                                                                                                        \
  {                                                                                                                       \
    RdPack<T> p{};                                                                                                        \
    for (int g = 0; g < nG; g++) {                                                                                        \
      p.wx[g] = dense(map[g][0], E, H, false)->ptr<T>();                                                                  \
      p.wh[g] = map[g][1] >= 0 ? dense(map[g][1], H, H, false)->ptr<T>() : nullptr;                                       \
      p.b[g] = dense(map[g][2], 1, H, true)->ptr<T>();                                                                    \
    }                                                                                                                     \
    p.w = w->ptr<T>(); p.bias = b->ptr<T>(); p.E = E; p.H = H; p.nG = nG;                                                 \
    hipLaunchKernelGGL((recurrent_decode_pack_kernel<T>), dim3(grid_for(total, 256)), dim3(256), 0, st, p);               \
  }
  if (dt == kF32) RD_PACK(float) else RD_PACK(double)
#undef RD_PACK
  LAMP_LAUNCH_CHECK();
  if (kind == LAMP_RECURRENT_GRU) *wh2_out_or_null = contiguous(dense(1, H, H, false));
  else if (wh2_out_or_null) *wh2_out_or_null = nullptr;
  *w_out = w.take();
  *bias_out = b.take();
  LAMP_API_END
}

int lamp_recurrent_decode_step(int kind, const lamp_tensor* table, const lamp_tensor* tokens, const lamp_tensor* parent_or_null, const lamp_tensor* w,
                               const lamp_tensor* bias, const lamp_tensor* wh2_or_null, const lamp_tensor* h_prev, const lamp_tensor* c_prev_or_null,
                               lamp_tensor* h_out, lamp_tensor* c_out_or_null, lamp_tensor* relu_out_or_null) {
  LAMP_API_BEGIN
  rd_check_kind(kind);
  check_device_tensor(table, "table"); check_device_tensor(tokens, "tokens"); check_device_tensor(w, "w"); check_device_tensor(bias, "bias");
  check_device_tensor(h_prev, "h_prev"); check_device_tensor(h_out, "h_out");
  const int dt = table->dtype, dev = table->device();
  LAMP_CHECK(dt == kF32 || dt == kF64, "f32 or f64, got " << table->describe());
  LAMP_CHECK(table->ndim == 2 && table->is_contiguous(), "table must be contiguous [vocabulary, E], got " << table->describe());
  const int nG = rd_gates(kind);
  const int64_t Vt = table->sizes[0], E = table->sizes[1];
  LAMP_CHECK(tokens->dtype == kI64 && tokens->device() == dev, "tokens must be int64 on the table's device, got " << tokens->describe());
  const int64_t R = tokens->numel();
  LAMP_CHECK(R >= 1 && R <= kDecMaxRows, R << " rows: this is the kernel of 1 .. " << kDecMaxRows << " rows, longer inputs are the module's forward");
  const int64_t tstride = dec_vector_stride(tokens, "tokens must be a vector or one row or column of a matrix");
  LAMP_CHECK(w->ndim == 2 && w->dtype == dt && w->device() == dev && w->is_contiguous() && w->sizes[0] > E && w->sizes[1] % nG == 0 &&
                 w->sizes[1] / nG == w->sizes[0] - E && E >= 1,
             "w must be the packed [E + H, " << nG << " H] of lamp_recurrent_decode_pack for a table " << table->describe() << ", got " << w->describe());
  const int64_t H = w->sizes[0] - E, N = nG * H;
  LAMP_CHECK(bias->dtype == dt && bias->device() == dev && bias->numel() == N && bias->is_contiguous(), "bias must hold " << N << " elements, got " << bias->describe());
  LAMP_CHECK(h_prev->dtype == dt && h_prev->device() == dev && h_prev->ndim == 2 && h_prev->sizes[1] == H && h_prev->is_contiguous() && h_prev->sizes[0] >= 1,
             "h_prev must be contiguous [rows, " << H << "], got " << h_prev->describe());
  const int64_t Rp = h_prev->sizes[0];
  if (parent_or_null) {
    check_device_tensor(parent_or_null, "parent");
    LAMP_CHECK(parent_or_null->dtype == kI64 && parent_or_null->device() == dev && parent_or_null->numel() == R && parent_or_null->is_contiguous(),
               "parent must be contiguous int64 [" << R << "], got " << parent_or_null->describe());
  } else {
    LAMP_CHECK(Rp == R, "without parent the previous state has the tokens' " << R << " rows, got " << h_prev->describe());
  }
  auto state_out = [&](const lamp_tensor* t, const char* what) {
    check_device_tensor(t, what);
    LAMP_CHECK(t->dtype == dt && t->device() == dev && t->ndim == 2 && t->sizes[0] == R && t->sizes[1] == H && t->is_contiguous(),
               what << " must be contiguous [" << R << ", " << H << "], got " << t->describe());
    LAMP_CHECK(t->raw() != h_prev->raw() && (!c_prev_or_null || t->raw() != c_prev_or_null->raw()), what << " must not be the previous state's buffer");
  };
  state_out(h_out, "h_out");
  if (relu_out_or_null) state_out(relu_out_or_null, "relu_out");
  LAMP_CHECK((kind == LAMP_RECURRENT_LSTM) == (c_prev_or_null != nullptr) && (kind == LAMP_RECURRENT_LSTM) == (c_out_or_null != nullptr),
             "c_prev and c_out come with LAMP_RECURRENT_LSTM and with it alone");
  if (kind == LAMP_RECURRENT_LSTM) {
    check_device_tensor(c_prev_or_null, "c_prev");
    LAMP_CHECK(c_prev_or_null->dtype == dt && c_prev_or_null->device() == dev && c_prev_or_null->ndim == 2 && c_prev_or_null->sizes[0] == Rp &&
                   c_prev_or_null->sizes[1] == H && c_prev_or_null->is_contiguous(), "c_prev must be contiguous [" << Rp << ", " << H << "], got " << c_prev_or_null->describe());
    state_out(c_out_or_null, "c_out");
  }
  LAMP_CHECK((kind == LAMP_RECURRENT_GRU) == (wh2_or_null != nullptr), "wh2 comes with LAMP_RECURRENT_GRU and with it alone");
  if (kind == LAMP_RECURRENT_GRU) {
    check_device_tensor(wh2_or_null, "wh2");
    LAMP_CHECK(wh2_or_null->dtype == dt && wh2_or_null->device() == dev && wh2_or_null->ndim == 2 && wh2_or_null->sizes[0] == H && wh2_or_null->sizes[1] == H &&
                   wh2_or_null->is_contiguous(), "wh2 must be contiguous [" << H << ", " << H << "], got " << wh2_or_null->describe());
  }
  hipStream_t st = current_stream(dev);
  const double sz = (double)dtype_size(dt);
  Hold slab1, slab2, scratch;
#define RD_STEP(T)                                                                                                                          \
  {                                                                                                                                         \
    RdStep<T> p{};                                                                                                                          \
    p.table = table->ptr<T>(); p.tokens = tokens->ptr<int64_t>(); p.parent = parent_or_null ? parent_or_null->ptr<int64_t>() : nullptr;     \
    p.src = h_prev->ptr<T>(); p.w = w->ptr<T>(); p.bias = bias->ptr<T>(); p.hprev = h_prev->ptr<T>();                                       \
    p.cprev = c_prev_or_null ? c_prev_or_null->ptr<T>() : nullptr;                                                                          \
    p.h = h_out->ptr<T>(); p.c = c_out_or_null ? c_out_or_null->ptr<T>() : nullptr;                                                         \
    p.relu = relu_out_or_null ? relu_out_or_null->ptr<T>() : nullptr;                                                                       \
    p.assert_word = device_assert_word(dev);                                                                                                \
    p.tstride = tstride; p.Vt = Vt; p.E = E; p.H = H; p.N = N; p.R = (int)R; p.Rp = (int)Rp;                                                \
    if (kind != LAMP_RECURRENT_GRU) {                                                                                                       \
      KernelTimer kt("recurrent_decode_step", 2.0 * R * (E + H) * N, ((double)(E + H) * N + (double)R * (E + 3 * H)) * sz, st);             \
      rd_step_run<T>(p, kind, dev, st, slab1);                                                                                              \
    } else {                                                                                                                                \
      int64_t ss[3] = {3, R, H};                                                                                                            \
      scratch = Hold(new_tensor(ss, 3, dt, dev));                                                                                           \
      T* sp = scratch->ptr<T>();                                                                                                            \
      p.zo = sp; p.rho = sp + R * H; p.preo = sp + 2 * R * H;                                                                               \
      {                                                                                                                                     \
        KernelTimer kt("recurrent_decode_step", 2.0 * R * (E + H) * N, ((double)(E + H) * N + (double)R * (E + 4 * H)) * sz, st);           \
        rd_step_run<T>(p, LAMP_RECURRENT_GRU, dev, st, slab1);                                                                              \
      }                                                                                                                                     \
      RdStep<T> q = p;                                                                                                                      \
      q.table = nullptr; q.tokens = nullptr; q.E = 0; q.N = H; q.src = p.rho; q.w = wh2_or_null->ptr<T>(); q.bias = nullptr;                \
      q.z = p.zo; q.pre = p.preo; q.slab = nullptr; q.ticket = nullptr;                                                                     \
      KernelTimer kt("recurrent_decode_gru_out", 2.0 * R * H * H, ((double)H * H + 5.0 * R * H) * sz, st);                                  \
      rd_step_run<T>(q, kDecFormGru2, dev, st, slab2);                                                                                           \
    }                                                                                                                                       \
  }
  if (dt == kF32) RD_STEP(float) else RD_STEP(double)
#undef RD_STEP
  LAMP_LAUNCH_CHECK();
  LAMP_API_END
}

int lamp_log_softmax_argmax_rows(lamp_tensor* out, lamp_tensor* tokens_out, const lamp_tensor* logits, int log_softmax) {
  LAMP_API_BEGIN
  check_device_tensor(logits, "logits"); check_device_tensor(out, "out"); check_device_tensor(tokens_out, "tokens_out");
  const int dt = logits->dtype, dev = logits->device();
  LAMP_CHECK(dt == kF32 || dt == kF64, "f32 or f64 logits, got " << logits->describe());
  LAMP_CHECK(logits->ndim == 2 && logits->sizes[1] >= 1 && logits->strides[1] == 1, "logits must be [R, V] with unit column stride, got " << logits->describe());
  const int64_t R = logits->sizes[0], V = logits->sizes[1];
  LAMP_CHECK(out->dtype == dt && out->device() == dev && out->ndim == 2 && out->sizes[0] == R && out->sizes[1] == V && out->strides[1] == 1,
             "out must be [" << R << ", " << V << "] of the logits' type with unit column stride, got " << out->describe());
  LAMP_CHECK(tokens_out->dtype == kI64 && tokens_out->device() == dev && tokens_out->numel() == R,
             "tokens_out must hold " << R << " int64 elements on the logits' device, got " << tokens_out->describe());
  const int64_t tstride = dec_vector_stride(tokens_out, "tokens_out must be a vector or one row or column of a matrix");
  if (R == 0) return 0;
  LAMP_CHECK(R <= 65535 * 32768LL, R << " rows are more than a grid holds");
  hipStream_t st = current_stream(dev);
  KernelTimer kt("log_softmax_argmax_rows", 4.0 * R * V, (log_softmax ? 4.0 : 2.0) * R * V * (double)dtype_size(dt) + 8.0 * R, st);
#define RD_LSM(T, L) hipLaunchKernelGGL((log_softmax_argmax_rows_kernel<T, L>), dim3((unsigned)R), dim3(256), 0, st, logits->ptr<T>(), logits->strides[0], \
                                        out->ptr<T>(), out->strides[0], tokens_out->ptr<int64_t>(), tstride, V)
  if (dt == kF32) { if (log_softmax) RD_LSM(float, true); else RD_LSM(float, false); }
  else { if (log_softmax) RD_LSM(double, true); else RD_LSM(double, false); }
#undef RD_LSM
  LAMP_LAUNCH_CHECK();
  LAMP_API_END
}

}  // extern "C"
