// Dense linear algebra of the symmetric positive-definite family (STen.scala:348-359, :1594-1601; ops.scala:2186-2285): batched Cholesky
// factorisation, triangular solve, Cholesky solve and Cholesky inverse in f32 and f64, each computed and accumulated in its own type.
// Leading dimensions are a batch; a launch serves many matrices, carried as base pointer + leading dimension + batch stride.
//
// Factorisation, n <= LINALG_LDS_SIDE: the named triangle is read into LDS as a lower triangle W (row stride odd: a column walk touches
// every bank once), then a right-looking column sweep with ONE workgroup barrier per column.  Column j stays unscaled in LDS: a thread
// that needs l_ij takes W[i][j] / sqrt(W[j][j]) itself - the same correctly rounded quotient wherever it is formed, so the result is the
// textbook algorithm's bit for bit, and nobody writes column j while others read it.  The scaling happens once more at the store.
// Small matrices share a workgroup: 16 threads per matrix up to side 8, a wavefront up to 32, 256 threads up to 64, 1024 above.
// Pivot rule: !(d > 0) at column j (a NaN too) sets the matrix's status word to j + 1 (LAPACK's info) and that matrix stops updating;
// the column loop and its barriers run to n regardless.  No trip count and no address depends on data.
//
// Factorisation, larger n: right-looking over block columns of LINALG_NB in a lower-triangular workspace W (the named triangle copied,
// transposed for `upper`): (a) the diagonal block by the LDS kernel in place, (b) the panel below it, L21 = A21 L11^-T, by the
// triangular-solve kernel with a thread per panel row, (c) the trailing update A22 -= L21 L21^T by the library's batched product on
// views (K = NB: below the split-K threshold, one FMA chain per output whatever the batch).  The update also writes W's other triangle;
// the last kernel writes the result's named triangle from W and exact zeros into the other.
//
// Triangular solve: op(T) X = B for the eight (upper, transpose, unitriangular) combinations is one forward substitution: the effective
// matrix (T or T^T) is read - named triangle only, diagonal not at all when unitriangular - into LDS as a lower triangle, an effective
// upper one with rows and columns reversed.  A thread owns a right-hand-side column and walks it in row blocks of 8 held in registers;
// the part of the solution already finished is read back from the output.  B = I (Cholesky inverse) is formed in the kernel.
// Larger n: the same kernel on diagonal blocks of LINALG_NB and a product on views for the remaining rows.
//
// linalg_plan() is the one place that decides form, threads, grid, LDS, block size, launches and workspace, from the arguments and a
// compute-unit count alone (lamp_debug_linalg_plan and tests/test_linalg_plan.py ask it without a device).
#include "device_utils.h"

#include <cstring>

namespace lamp {

constexpr int LINALG_LDS_SIDE = 128;       // largest side whose triangle lives in LDS (128 x 129 f64 = 129 KiB of the CU's 160)
constexpr int LINALG_NB = 64;              // block column of the blocked forms
constexpr int LINALG_RB = 8;               // rows of a right-hand side a solve thread holds in registers
constexpr int LINALG_SOLVE_THREADS = 256;
constexpr int LINALG_SHARED_LDS = 64 * 1024;   // several small matrices share a workgroup up to this much LDS
constexpr int64_t LINALG_MAX_ELEMS = 2147483647LL;

enum LinalgOp { kLinalgCholesky = 0, kLinalgCholeskySolve = 1, kLinalgCholeskyInverse = 2, kLinalgTriangularSolve = 3 };
enum LinalgForm { kLinalgLds = 0, kLinalgBlocked = 1 };

// one kernel geometry: the factorisation's (threads per matrix `tpm`, a tside x tside thread grid per matrix) or the solve's
// (`cpw` right-hand-side columns per workgroup)
struct LinalgLaunch {
  int threads = 0, mpw = 0, tpm = 0, tside = 0, cpw = 0, ld = 0, lds_bytes = 0;
  unsigned grid_x = 0, grid_y = 1;
};

struct LinalgPlan {
  bool accepted = false;
  const char* reason = "";
  int op = 0, dtype = 0, form = 0;
  int64_t batch = 0, n = 0, nrhs = 0;
  int nb = 0, steps = 0, launches = 0;
  size_t ws_bytes = 0;
  LinalgLaunch potrf;    // Cholesky: the whole matrix (LDS form) or a diagonal block (blocked form)
  LinalgLaunch solve;    // the solves: the whole triangle or a diagonal block; Cholesky's blocked form: the panel solve
};

static int linalg_round8(int64_t n) { return (int)((n + LINALG_RB - 1) / LINALG_RB * LINALG_RB); }

static LinalgLaunch potrf_launch(int64_t batch, int n, size_t es) {
  LinalgLaunch l;
  l.tpm = n <= 8 ? 16 : (n <= 32 ? 64 : (n <= 64 ? 256 : 1024));
  l.tside = n <= 8 ? 4 : (n <= 32 ? 8 : (n <= 64 ? 16 : 32));
  l.ld = n | 1;
  l.mpw = (int)std::min<int64_t>(std::max(1, 256 / l.tpm), batch);
  l.threads = std::max(64, (l.mpw * l.tpm + 63) / 64 * 64);
  l.lds_bytes = (int)((size_t)l.mpw * n * l.ld * es);
  l.grid_x = (unsigned)((batch + l.mpw - 1) / l.mpw);
  return l;
}

// `n` rows of a triangle against `nrhs` columns; few workgroups on many compute units: narrower workgroups
static LinalgLaunch solve_launch(int64_t batch, int n, int64_t nrhs, size_t es, int64_t cus) {
  LinalgLaunch l;
  const int n8 = linalg_round8(n);
  l.ld = n8 | 1;
  const int64_t per = (int64_t)n8 * l.ld * (int64_t)es;
  auto shape = [&](int cpw) {
    l.cpw = cpw;
    l.mpw = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(LINALG_SOLVE_THREADS / cpw, LINALG_SHARED_LDS / per), batch));
    l.grid_x = (unsigned)((batch + l.mpw - 1) / l.mpw);
    l.grid_y = (unsigned)((nrhs + cpw - 1) / cpw);
  };
  shape((int)std::min<int64_t>(nrhs, LINALG_SOLVE_THREADS));
  if (nrhs > 64 && (int64_t)l.grid_x * l.grid_y < cus) shape(64);
  l.threads = std::max(64, (l.mpw * l.cpw + 63) / 64 * 64);
  l.lds_bytes = (int)((int64_t)l.mpw * per);
  return l;
}

static LinalgPlan linalg_plan(int op, int dtype, int64_t batch, int64_t n, int64_t nrhs, int64_t cus) {
  LinalgPlan p;
  p.op = op; p.dtype = dtype; p.batch = batch; p.n = n; p.nrhs = nrhs;
  auto decline = [&](const char* why) { p.accepted = false; p.reason = why; return p; };
  if (op < kLinalgCholesky || op > kLinalgTriangularSolve) return decline("unknown operation");
  if (dtype != kF32 && dtype != kF64) return decline("f32 and f64 only (as ATen's CPU kernels: no bf16 / f16 factorisation or solve)");
  if (batch < 1 || n < 1) return decline("empty input");
  if (n * n > LINALG_MAX_ELEMS) return decline("a matrix has more than 2^31 - 1 elements");
  if (op == kLinalgCholesky) nrhs = p.nrhs = 0;
  if (op == kLinalgCholeskyInverse) nrhs = p.nrhs = n;
  if (op != kLinalgCholesky && (nrhs < 1 || n * nrhs > LINALG_MAX_ELEMS)) return decline(nrhs < 1 ? "empty right-hand side" : "a right-hand side has more than 2^31 - 1 elements");
  if (batch > LINALG_MAX_ELEMS) return decline("more than 2^31 - 1 matrices");
  const size_t es = dtype_size(dtype);
  const int solves = op == kLinalgTriangularSolve ? 1 : 2;
  if (n <= LINALG_LDS_SIDE) {
    p.form = kLinalgLds; p.nb = (int)n; p.steps = 1; p.ws_bytes = 0;
    if (op == kLinalgCholesky) { p.potrf = potrf_launch(batch, (int)n, es); p.launches = 1; }
    else { p.solve = solve_launch(batch, (int)n, nrhs, es, cus); p.launches = solves; }
  } else {
    p.form = kLinalgBlocked; p.nb = LINALG_NB; p.steps = (int)((n + LINALG_NB - 1) / LINALG_NB);
    if (op == kLinalgCholesky) {
      // copy in, then per block column: diagonal block, and (all but the last) panel solve + trailing product; copy out
      p.potrf = potrf_launch(batch, LINALG_NB, es);
      p.solve = solve_launch(batch, LINALG_NB, n - LINALG_NB, es, cus);
      p.launches = 2 + p.steps + 2 * (p.steps - 1);
      p.ws_bytes = (size_t)batch * n * n * es;
    } else {
      // per solve and block row: diagonal-block solve, and (all but the last) a product; the inverse writes its identity first
      p.solve = solve_launch(batch, LINALG_NB, nrhs, es, cus);
      p.launches = solves * (2 * p.steps - 1) + (op == kLinalgCholeskyInverse ? 1 : 0);
      p.ws_bytes = 0;
    }
  }
  if (p.solve.grid_y > 65535u) return decline("more than 65535 * 64 right-hand-side columns");
  p.accepted = true;
  return p;
}

// the (batch, n, nrhs) of a call from its operand shapes, or the reason there is none.  a: the matrix / factor / triangle; b: the
// right-hand side (null for the one-operand calls).  Batch rule: equal batch shapes, or one operand 2-D and broadcast over the other's.
struct LinalgProblem { const char* reason = nullptr; int64_t batch = 1, n = 0, nrhs = 0; bool a_bcast = false, b_bcast = false; };
static LinalgProblem linalg_problem(const int64_t* as, int and_, const int64_t* bs, int bnd) {
  LinalgProblem q;
  if (and_ < 2) { q.reason = "the matrix must have at least 2 dimensions"; return q; }
  if (as[and_ - 1] != as[and_ - 2]) { q.reason = "the matrix must be square (batches of square matrices)"; return q; }
  q.n = as[and_ - 1];
  const int64_t* lead = as; int nlead = and_ - 2;
  if (bs) {
    if (bnd < 2) { q.reason = "the right-hand side must have at least 2 dimensions"; return q; }
    if (bs[bnd - 2] != q.n) { q.reason = "mismatched sizes: the right-hand side's rows are not the matrix's side"; return q; }
    q.nrhs = bs[bnd - 1];
    if (and_ == 2 && bnd > 2) { q.a_bcast = true; lead = bs; nlead = bnd - 2; }
    else if (bnd == 2 && and_ > 2) q.b_bcast = true;
    else {
      bool same = and_ == bnd;
      for (int d = 0; same && d < and_ - 2; d++) same = as[d] == bs[d];
      if (!same) { q.reason = "batch shapes must be equal, or one operand 2-D (broadcast over the other's batch)"; return q; }
    }
  }
  for (int d = 0; d < nlead; d++) q.batch *= lead[d];
  return q;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
struct PotrfArgs {
  const void* src; void* dst; int* status;
  int64_t src_ld, src_bs, dst_ld, dst_bs, batch;
  int n, ld, tpm, tside, mpw;
  int src_upper;    // read the upper triangle (as the transposed lower one)
  int dst_upper;    // write the factor transposed
  int zero_other;   // write zeros into the other triangle (0: leave it alone - a diagonal block of the blocked form)
  int chained;      // blocked form: a matrix whose status word is set already does nothing; info counts from col0
  int col0;
};

template <class T> __device__ __forceinline__ T linalg_sqrt(T v);
template <> __device__ __forceinline__ float linalg_sqrt<float>(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double linalg_sqrt<double>(double v) { return sqrt(v); }

extern __shared__ __align__(16) unsigned char linalg_lds[];

template <class T>
__global__ __launch_bounds__(1024) void linalg_potrf_kernel(PotrfArgs a) {
  T* lds = (T*)linalg_lds;
  const int tid = threadIdx.x, slot = tid / a.tpm, t = tid - slot * a.tpm;
  const int64_t m = (int64_t)blockIdx.x * a.mpw + slot;
  const bool live = slot < a.mpw && m < a.batch;               // (a workgroup is whole wavefronts: the spare threads only meet the barriers)
  const int n = a.n, ld = a.ld;
  T* W = lds + (size_t)(live ? slot : 0) * n * ld;
  const T* S = (const T*)a.src + (live ? m : 0) * a.src_bs;
  T* D = (T*)a.dst + (live ? m : 0) * a.dst_bs;
  bool stop = false;
  if (live) {
    if (a.chained) stop = a.status[m] != 0;
    for (int e = t; e < n * n; e += a.tpm) {                   // consecutive threads read consecutive addresses of a row
      const int r = e / n, c = e - r * n;
      if (a.src_upper ? c >= r : c <= r) {
        const T v = S[(int64_t)r * a.src_ld + c];
        if (a.src_upper) W[c * ld + r] = v; else W[r * ld + c] = v;
      }
    }
  }
  __syncthreads();
  const int tx = t % a.tside, ty = t / a.tside;
  int info = 0;
  for (int j = 0; j < n; j++) {
    if (live && !stop) {
      const T d = W[j * ld + j];
      if (!(d > (T)0)) { info = a.col0 + j + 1; stop = true; }   // every thread of the matrix reads the same d
      else {
        const T l = linalg_sqrt<T>(d);
        for (int i = j + 1 + ty; i < n; i += a.tside) {
          const T lij = W[i * ld + j] / l;
          for (int k = j + 1 + tx; k <= i; k += a.tside) W[i * ld + k] -= lij * (W[k * ld + j] / l);
        }
      }
    }
    __syncthreads();                                           // column j + 1 is complete; column j is never written
  }
  if (!live) return;
  if (t == 0 && (info != 0 || !a.chained)) a.status[m] = info;
  for (int e = t; e < n * n; e += a.tpm) {
    const int r = e / n, c = e - r * n;
    const int i = a.dst_upper ? c : r, j = a.dst_upper ? r : c;   // the factor's element (i, j), i >= j, lands at (r, c)
    if (i >= j) {
      const T l = linalg_sqrt<T>(W[j * ld + j]);
      D[(int64_t)r * a.dst_ld + c] = i == j ? l : W[i * ld + j] / l;
    } else if (a.zero_other) {
      D[(int64_t)r * a.dst_ld + c] = (T)0;
    }
  }
}

struct SolveArgs {
  const void* tri; void* x;
  int64_t t_ld, t_bs;             // the triangle: row stride, batch stride (0: one triangle for the whole batch)
  int64_t x_rs, x_cs, x_bs;       // the right-hand sides / solution: stride between the rows of the system, between columns, batch
  int64_t batch, nrhs;
  int n, n8, ld, mpw, cpw;
  int upper, trans, unit;
  int identity;                   // the right-hand side is I: formed here, x is only written
};

template <class T>
__global__ __launch_bounds__(LINALG_SOLVE_THREADS) void linalg_solve_kernel(SolveArgs a) {
  T* lds = (T*)linalg_lds;
  const int tid = threadIdx.x, n = a.n, n8 = a.n8, ld = a.ld;
  const bool lower = a.upper == a.trans;                       // the effective matrix op(T) is lower triangular
  const int64_t m0 = (int64_t)blockIdx.x * a.mpw;
  const int here = a.batch - m0 < a.mpw ? (int)(a.batch - m0) : a.mpw;     // matrices of this workgroup
  // padding rows n .. n8 of the identity, then the named triangle as the lower triangle E'[i][j], i >= j
  for (int e = tid; e < here * n8 * n8; e += blockDim.x) {
    const int s = e / (n8 * n8), q = e - s * n8 * n8, i = q / n8, j = q - i * n8;
    if (i >= n && j <= i) lds[(size_t)s * n8 * ld + i * ld + j] = i == j ? (T)1 : (T)0;
  }
  for (int e = tid; e < here * n * n; e += blockDim.x) {
    const int s = e / (n * n), q = e - s * n * n, r = q / n, c = q - r * n;
    if (a.upper ? c >= r : c <= r) {
      const T* Tm = (const T*)a.tri + (m0 + s) * a.t_bs;
      const T v = (a.unit && r == c) ? (T)1 : Tm[(int64_t)r * a.t_ld + c];
      int i = a.trans ? c : r, j = a.trans ? r : c;
      if (!lower) { i = n - 1 - i; j = n - 1 - j; }
      lds[(size_t)s * n8 * ld + i * ld + j] = v;
    }
  }
  __syncthreads();
  const int slot = tid / a.cpw;
  const int64_t col = (int64_t)blockIdx.y * a.cpw + (tid - slot * a.cpw);
  if (slot >= here || col >= a.nrhs) return;
  const T* L = lds + (size_t)slot * n8 * ld;
  T* X = (T*)a.x + (m0 + slot) * a.x_bs + col * a.x_cs;
  for (int i0 = 0; i0 < n8; i0 += LINALG_RB) {
    T acc[LINALG_RB];
#pragma unroll
    for (int r = 0; r < LINALG_RB; r++) {
      const int row = i0 + r, mr = lower ? row : n - 1 - row;   // row `row` of the substitution is row `mr` of the system
      acc[r] = row < n ? (a.identity ? (mr == col ? (T)1 : (T)0) : X[(int64_t)mr * a.x_rs]) : (T)0;
    }
    for (int k = 0; k < i0; k++) {
      const T xk = X[(int64_t)(lower ? k : n - 1 - k) * a.x_rs];  // written by this thread in an earlier block
#pragma unroll
      for (int r = 0; r < LINALG_RB; r++) acc[r] -= L[(i0 + r) * ld + k] * xk;
    }
#pragma unroll
    for (int r = 0; r < LINALG_RB; r++) {
      acc[r] = acc[r] / L[(i0 + r) * ld + i0 + r];
#pragma unroll
      for (int r2 = r + 1; r2 < LINALG_RB; r2++) acc[r2] -= L[(i0 + r2) * ld + i0 + r] * acc[r];
    }
#pragma unroll
    for (int r = 0; r < LINALG_RB; r++) {
      const int row = i0 + r;
      if (row < n) X[(int64_t)(lower ? row : n - 1 - row) * a.x_rs] = acc[r];
    }
  }
}

// blocked Cholesky, first and last launch.  in: W = the named triangle of A as a lower triangle, zeros above it, status words cleared.
// out: the result's named triangle from W's lower one, exact zeros in the other.
template <class T>
__global__ __launch_bounds__(256) void linalg_triangle_kernel(const T* __restrict__ src, T* __restrict__ dst, int* status, int64_t batch, int n, int upper) {
  const int64_t nn = (int64_t)n * n, total = batch * nn;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = e / nn, q = e - m * nn;
    const int r = (int)(q / n), c = (int)(q - (int64_t)r * n);
    if (status && q == 0) status[m] = 0;
    // in (status != null): dst is W, its (r, c) with c <= r comes from A's (r, c) or, upper, (c, r).  out: dst's named triangle from W.
    const bool named = status ? c <= r : (upper ? c >= r : c <= r);
    dst[e] = named ? (upper ? src[m * nn + (int64_t)c * n + r] : src[e]) : (T)0;
  }
}

template <class T>
__global__ __launch_bounds__(256) void linalg_eye_kernel(T* __restrict__ dst, int64_t batch, int n) {
  const int64_t nn = (int64_t)n * n, total = batch * nn;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = e % nn;
    dst[e] = q / n == q % n ? (T)1 : (T)0;
  }
}

// ---- host drivers ----------------------------------------------------------------------------------------------------------------
namespace {

template <class K> void linalg_lds_opt_in(K kernel, int lds_bytes) {
  if (lds_bytes > 64 * 1024) allow_big_lds((const void*)kernel);
}

void launch_potrf(const LinalgLaunch& l, PotrfArgs a, int dtype, hipStream_t st) {
  a.ld = l.ld; a.tpm = l.tpm; a.tside = l.tside; a.mpw = l.mpw;
  if (dtype == kF32) {
    linalg_lds_opt_in(linalg_potrf_kernel<float>, l.lds_bytes);
    hipLaunchKernelGGL(linalg_potrf_kernel<float>, dim3(l.grid_x), dim3(l.threads), l.lds_bytes, st, a);
  } else {
    linalg_lds_opt_in(linalg_potrf_kernel<double>, l.lds_bytes);
    hipLaunchKernelGGL(linalg_potrf_kernel<double>, dim3(l.grid_x), dim3(l.threads), l.lds_bytes, st, a);
  }
  LAMP_LAUNCH_CHECK();
}

void launch_solve(const LinalgLaunch& l, SolveArgs a, int dtype, hipStream_t st) {
  a.n8 = linalg_round8(a.n); a.ld = l.ld; a.mpw = l.mpw; a.cpw = l.cpw;
  if (dtype == kF32) {
    linalg_lds_opt_in(linalg_solve_kernel<float>, l.lds_bytes);
    hipLaunchKernelGGL(linalg_solve_kernel<float>, dim3(l.grid_x, l.grid_y), dim3(l.threads), l.lds_bytes, st, a);
  } else {
    linalg_lds_opt_in(linalg_solve_kernel<double>, l.lds_bytes);
    hipLaunchKernelGGL(linalg_solve_kernel<double>, dim3(l.grid_x, l.grid_y), dim3(l.threads), l.lds_bytes, st, a);
  }
  LAMP_LAUNCH_CHECK();
}

// rows [r0, r0 + nr) x columns [c0, c0 + nc) of every matrix of t [batch, R, C] (any batch stride, 0 included), or its transpose
Tensor* block_view(const Tensor* t, int64_t r0, int64_t nr, int64_t c0, int64_t nc, bool transposed = false) {
  int64_t sizes[3] = {t->sizes[0], nr, nc}, strides[3] = {t->strides[0], t->strides[1], t->strides[2]};
  if (transposed) { std::swap(sizes[1], sizes[2]); std::swap(strides[1], strides[2]); }
  return new_view(t, sizes, strides, 3, t->offset + r0 * t->strides[1] + c0 * t->strides[2]);
}

#define LINALG_CALL(expr) do { if ((expr) != 0) throw Error(lamp_last_error()); } while (0)

void linalg_cholesky_blocked(const LinalgPlan& p, const Tensor* a3, Tensor* out3, Tensor* status, int upper, hipStream_t st) {
  const int64_t batch = p.batch, n = p.n;
  Hold W(new_like(out3));
  const int grid = grid_for(batch * n * n, 256);
  if (p.dtype == kF32) hipLaunchKernelGGL(linalg_triangle_kernel<float>, dim3(grid), dim3(256), 0, st, a3->ptr<float>(), W->ptr<float>(), status->ptr<int>(), batch, (int)n, upper);
  else hipLaunchKernelGGL(linalg_triangle_kernel<double>, dim3(grid), dim3(256), 0, st, a3->ptr<double>(), W->ptr<double>(), status->ptr<int>(), batch, (int)n, upper);
  LAMP_LAUNCH_CHECK();
  const size_t es = dtype_size(p.dtype);
  for (int s = 0; s < p.steps; s++) {
    const int64_t j0 = (int64_t)s * p.nb, nb = std::min<int64_t>(p.nb, n - j0), below = n - j0 - nb;
    char* diag = (char*)W->data() + (j0 * n + j0) * es;
    PotrfArgs pa{};
    pa.src = diag; pa.dst = diag; pa.status = status->ptr<int>();
    pa.src_ld = pa.dst_ld = n; pa.src_bs = pa.dst_bs = n * n; pa.batch = batch;
    pa.n = (int)nb; pa.chained = 1; pa.col0 = (int)j0;
    launch_potrf(nb == p.nb ? p.potrf : potrf_launch(batch, (int)nb, es), pa, p.dtype, st);
    if (below == 0) break;
    // L21 = A21 L11^-T: row r of the panel solves L11 x = a_r^T, so the panel is the right-hand side with its rows as columns
    SolveArgs sa{};
    sa.tri = diag; sa.t_ld = n; sa.t_bs = n * n;
    sa.x = (char*)W->data() + ((j0 + nb) * n + j0) * es; sa.x_rs = 1; sa.x_cs = n; sa.x_bs = n * n;
    sa.batch = batch; sa.nrhs = below; sa.n = (int)nb;
    launch_solve(solve_launch(batch, (int)nb, below, es, num_cus()), sa, p.dtype, st);
    Hold l21(block_view(W.get(), j0 + nb, below, j0, nb)), a22(block_view(W.get(), j0 + nb, below, j0 + nb, below));
    LINALG_CALL(lamp_baddbmm_out_transposed2(a22.get(), a22.get(), l21.get(), l21.get(), 1.0, -1.0));
  }
  if (p.dtype == kF32) hipLaunchKernelGGL(linalg_triangle_kernel<float>, dim3(grid), dim3(256), 0, st, W->ptr<float>(), out3->ptr<float>(), (int*)nullptr, batch, (int)n, upper);
  else hipLaunchKernelGGL(linalg_triangle_kernel<double>, dim3(grid), dim3(256), 0, st, W->ptr<double>(), out3->ptr<double>(), (int*)nullptr, batch, (int)n, upper);
  LAMP_LAUNCH_CHECK();
}

// op(T) X = B in place in x3 [batch, n, nrhs] (contiguous); t3 [batch, n, n] row-major, batch stride 0 for one triangle
void linalg_solve_inplace(const LinalgPlan& p, const Tensor* t3, Tensor* x3, int upper, int trans, int unit, int identity, hipStream_t st) {
  const int64_t batch = p.batch, n = p.n, nrhs = p.nrhs;
  const size_t es = dtype_size(p.dtype);
  SolveArgs sa{};
  sa.t_ld = t3->strides[1]; sa.t_bs = t3->strides[0];
  sa.x_rs = nrhs; sa.x_cs = 1; sa.x_bs = n * nrhs;
  sa.batch = batch; sa.nrhs = nrhs; sa.upper = upper; sa.trans = trans; sa.unit = unit;
  if (p.form == kLinalgLds) {
    sa.tri = t3->raw(); sa.x = x3->data(); sa.n = (int)n; sa.identity = identity;
    launch_solve(p.solve, sa, p.dtype, st);
    return;
  }
  if (identity) {
    const int grid = grid_for(batch * n * n, 256);
    if (p.dtype == kF32) hipLaunchKernelGGL(linalg_eye_kernel<float>, dim3(grid), dim3(256), 0, st, x3->ptr<float>(), batch, (int)n);
    else hipLaunchKernelGGL(linalg_eye_kernel<double>, dim3(grid), dim3(256), 0, st, x3->ptr<double>(), batch, (int)n);
    LAMP_LAUNCH_CHECK();
  }
  const bool lower = upper == trans;
  for (int s = 0; s < p.steps; s++) {
    const int k = lower ? s : p.steps - 1 - s;                 // forward over the block rows, or backward
    const int64_t r0 = (int64_t)k * p.nb, nb = std::min<int64_t>(p.nb, n - r0);
    sa.tri = (const char*)t3->raw() + (r0 * sa.t_ld + r0) * es;
    sa.x = (char*)x3->data() + r0 * nrhs * es;
    sa.n = (int)nb;
    launch_solve(nb == p.nb ? p.solve : solve_launch(batch, (int)nb, nrhs, es, num_cus()), sa, p.dtype, st);
    const int64_t rest0 = lower ? r0 + nb : 0, rest = lower ? n - r0 - nb : r0;
    if (rest == 0) continue;
    // X[rest] -= E[rest, block] X[block], E = op(T); the product takes E[rest, block]^T: T's own block when transposed, a strided view of it otherwise
    Hold et(trans ? block_view(t3, r0, nb, rest0, rest) : block_view(t3, rest0, rest, r0, nb, true));
    Hold xk(block_view(x3, r0, nb, 0, nrhs)), xr(block_view(x3, rest0, rest, 0, nrhs));
    LINALG_CALL(lamp_baddbmm_out_transposed1(xr.get(), xr.get(), et.get(), xk.get(), 1.0, -1.0));
  }
}

// a as [batch, n, n] with unit column stride and a regular batch stride (0 when it is broadcast): a view, or a contiguous copy
Tensor* as_batch3(const Tensor* a, int64_t batch, int64_t rows, int64_t cols, bool bcast) {
  Hold c(contiguous(a));
  int64_t sizes[3] = {batch, rows, cols}, strides[3] = {bcast ? 0 : rows * cols, cols, 1};
  return new_view(c.get(), sizes, strides, 3, c->offset);
}

// b expanded over the batch, as a fresh contiguous [batch, n, nrhs] the solve overwrites
Tensor* rhs_copy(const Tensor* b, const std::vector<int64_t>& out_shape, int64_t batch, int64_t n, int64_t nrhs, bool bcast) {
  Hold x(new_tensor(out_shape, b->dtype, b->device()));
  Hold b3(as_batch3(b, batch, n, nrhs, bcast));
  int64_t s3[3] = {batch, n, nrhs}, st3[3] = {n * nrhs, nrhs, 1};
  Hold x3(new_view(x.get(), s3, st3, 3, x->offset));
  copy_into(x3.get(), b3.get());
  return x.take();
}

std::vector<int64_t> batch_shape_of(const Tensor* a, const Tensor* b, const LinalgProblem& q, int64_t rows, int64_t cols) {
  const Tensor* lead = (b && q.a_bcast) ? b : a;
  std::vector<int64_t> s(lead->sizes, lead->sizes + lead->ndim - 2);
  s.push_back(rows); s.push_back(cols);
  return s;
}

// the shared body of the three solves: checks, plan, copy of the right-hand side, one or two substitutions
Tensor* linalg_solve_call(int op, const Tensor* b, const Tensor* tri, int upper, int trans, int unit, const char* what) {
  check_device_tensor(tri, what);
  if (b) { check_device_tensor(b, "b"); check_same_device(b, tri); }
  LAMP_CHECK(!b || b->dtype == tri->dtype, "b is " << dtype_name(b->dtype) << ", " << what << " is " << dtype_name(tri->dtype));
  const LinalgProblem q = linalg_problem(tri->sizes, tri->ndim, b ? b->sizes : nullptr, b ? b->ndim : 0);
  LAMP_CHECK(!q.reason, q.reason << ": " << what << " " << tri->describe() << (b ? ", b " + b->describe() : std::string()));
  const int64_t n = q.n, nrhs = b ? q.nrhs : n;
  const std::vector<int64_t> shape = batch_shape_of(tri, b, q, n, nrhs);
  if (q.batch == 0 || n == 0 || nrhs == 0) {
    LAMP_CHECK(tri->dtype == kF32 || tri->dtype == kF64, "f32 and f64 only, got " << tri->describe());
    return new_tensor(shape, tri->dtype, tri->device());
  }
  const LinalgPlan p = linalg_plan(op, tri->dtype, q.batch, n, nrhs, num_cus());
  LAMP_CHECK(p.accepted, p.reason << ": " << what << " " << tri->describe());
  hipStream_t st = current_stream(tri->device());
  Hold t3(as_batch3(tri, q.batch, n, n, q.a_bcast));
  Hold x(b ? rhs_copy(b, shape, q.batch, n, nrhs, q.b_bcast) : new_tensor(shape, tri->dtype, tri->device()));
  int64_t s3[3] = {q.batch, n, nrhs}, st3[3] = {n * nrhs, nrhs, 1};
  Hold x3(new_view(x.get(), s3, st3, 3, x->offset));
  if (op == kLinalgTriangularSolve) {
    linalg_solve_inplace(p, t3.get(), x3.get(), upper, trans, unit, 0, st);
  } else {
    // A = L L^T: L y = b, L^T x = y.  A = U^T U: U^T y = b, U x = y.
    linalg_solve_inplace(p, t3.get(), x3.get(), upper, upper ? 1 : 0, 0, b ? 0 : 1, st);
    linalg_solve_inplace(p, t3.get(), x3.get(), upper, upper ? 0 : 1, 0, 0, st);
  }
  return x.take();
}

}  // namespace
}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_linalg_cholesky(lamp_tensor** out, const lamp_tensor* a, int upper) {
  LAMP_API_BEGIN
  check_device_tensor(a, "a");
  const LinalgProblem q = linalg_problem(a->sizes, a->ndim, nullptr, 0);
  LAMP_CHECK(!q.reason, q.reason << ": a " << a->describe());
  if (q.batch == 0 || q.n == 0) {
    LAMP_CHECK(a->dtype == kF32 || a->dtype == kF64, "f32 and f64 only, got " << a->describe());
    *out = new_tensor(a->shape(), a->dtype, a->device());
    return 0;
  }
  const LinalgPlan p = linalg_plan(kLinalgCholesky, a->dtype, q.batch, q.n, 0, num_cus());
  LAMP_CHECK(p.accepted, p.reason << ": a " << a->describe());
  const int dev = a->device();
  hipStream_t st = current_stream(dev);
  const int64_t batch = q.batch, n = q.n;
  Hold a3(as_batch3(a, batch, n, n, false));
  Hold r(new_tensor(a->shape(), a->dtype, dev));
  int64_t s3[3] = {batch, n, n}, st3[3] = {n * n, n, 1}, sb[1] = {batch};
  Hold r3(new_view(r.get(), s3, st3, 3, r->offset));
  Hold status(new_tensor(sb, 1, kI32, dev));
  const int up = upper != 0;
  if (p.form == kLinalgLds) {
    PotrfArgs pa{};
    pa.src = a3->raw(); pa.dst = r3->data(); pa.status = status->ptr<int>();
    pa.src_ld = pa.dst_ld = n; pa.src_bs = pa.dst_bs = n * n; pa.batch = batch;
    pa.n = (int)n; pa.src_upper = up; pa.dst_upper = up; pa.zero_other = 1;
    launch_potrf(p.potrf, pa, p.dtype, st);
  } else {
    linalg_cholesky_blocked(p, a3.get(), r3.get(), status.get(), up, st);
  }
  // the one synchronisation of the call: ATen raises for a matrix that is not positive-definite, and names the first one
  std::vector<int> info((size_t)batch);
  HIP_CHECK(hipMemcpyAsync(info.data(), status->raw(), sizeof(int) * (size_t)batch, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  for (int64_t m = 0; m < batch; m++) {
    if (info[(size_t)m] == 0) continue;
    std::ostringstream os;
    os << "linalg.cholesky: ";
    if (a->ndim > 2) os << "(Batch element " << m << "): ";
    os << "The factorization could not be completed because the input is not positive-definite (the leading minor of order " << info[(size_t)m]
       << " is not positive-definite).";
    throw Error(os.str());
  }
  *out = r.take();
  LAMP_API_END
}

int lamp_cholesky_solve(lamp_tensor** out, const lamp_tensor* b, const lamp_tensor* factor, int upper) {
  LAMP_API_BEGIN
  LAMP_CHECK(b != nullptr, "b is null");
  *out = linalg_solve_call(kLinalgCholeskySolve, b, factor, upper != 0, 0, 0, "factor");
  LAMP_API_END
}

int lamp_cholesky_inverse(lamp_tensor** out, const lamp_tensor* factor, int upper) {
  LAMP_API_BEGIN
  *out = linalg_solve_call(kLinalgCholeskyInverse, nullptr, factor, upper != 0, 0, 0, "factor");
  LAMP_API_END
}

int lamp_triangular_solve(lamp_tensor** solution, lamp_tensor** cloned_a, const lamp_tensor* b, const lamp_tensor* a, int upper, int transpose,
                          int unitriangular) {
  LAMP_API_BEGIN
  LAMP_CHECK(b != nullptr && solution != nullptr, "b or solution is null");
  Hold x(linalg_solve_call(kLinalgTriangularSolve, b, a, upper != 0, transpose != 0, unitriangular != 0, "a"));
  if (cloned_a) {                                              // ATen's second result: the coefficient, copied (over the batch when it was broadcast)
    const LinalgProblem q = linalg_problem(a->sizes, a->ndim, b->sizes, b->ndim);
    Hold c(new_tensor(batch_shape_of(a, b, q, q.n, q.n), a->dtype, a->device()));
    if (c->numel() > 0) {
      int64_t s3[3] = {q.batch, q.n, q.n}, st3[3] = {q.n * q.n, q.n, 1};
      Hold c3(new_view(c.get(), s3, st3, 3, c->offset)), a3(as_batch3(a, q.batch, q.n, q.n, q.a_bcast));
      copy_into(c3.get(), a3.get());
    }
    *cloned_a = c.take();
  }
  *solution = x.take();
  LAMP_API_END
}

// Test tool, needs no GPU: the plan the four calls would run for operands of these shapes on a device of `cus` compute units.  op: 0
// linalg_cholesky, 1 cholesky_solve, 2 cholesky_inverse, 3 triangular_solve; a_sizes: the matrix / factor / triangle; b_sizes: the
// right-hand side (b_ndim = 0 for the one-operand calls).  key=value lines into buf; a declined plan has accepted=0 and its reason.
int lamp_debug_linalg_plan(int op, int dtype, const int64_t* a_sizes, int a_ndim, const int64_t* b_sizes, int b_ndim, int cus, char* buf, int buflen) {
  LAMP_API_BEGIN
  LAMP_CHECK(a_sizes && buf && buflen > 0 && cus > 0 && a_ndim >= 0 && a_ndim <= kMaxDims && b_ndim >= 0 && b_ndim <= kMaxDims, "lamp_debug_linalg_plan: bad arguments");
  const bool two = op == kLinalgCholeskySolve || op == kLinalgTriangularSolve;
  LinalgPlan p;
  p.op = op; p.dtype = dtype;
  LinalgProblem q;
  if (two && !(b_sizes && b_ndim > 0)) q.reason = "this call takes a right-hand side";
  else q = linalg_problem(a_sizes, a_ndim, two ? b_sizes : nullptr, two ? b_ndim : 0);
  if (q.reason) p.reason = q.reason;
  else p = linalg_plan(op, dtype, q.batch, q.n, q.nrhs, cus);
  const LinalgLaunch& l = op == kLinalgCholesky ? p.potrf : p.solve;
  char text[1536];
  const int w = snprintf(text, sizeof(text),
                         "accepted=%d\nreason=%s\nop=%d\ndtype=%d\nbatch=%lld\nn=%lld\nnrhs=%lld\nform=%s\nlds_side=%d\nnb=%d\nsteps=%d\nlaunches=%d\n"
                         "workspace_bytes=%zu\nthreads=%d\ngrid_x=%u\ngrid_y=%u\nlds_bytes=%d\n"
                         "potrf_threads=%d\npotrf_grid_x=%u\npotrf_lds_bytes=%d\npotrf_matrices_per_workgroup=%d\npotrf_threads_per_matrix=%d\npotrf_ld=%d\n"
                         "solve_threads=%d\nsolve_grid_x=%u\nsolve_grid_y=%u\nsolve_lds_bytes=%d\nsolve_matrices_per_workgroup=%d\n"
                         "solve_columns_per_workgroup=%d\nsolve_ld=%d\n",
                         p.accepted ? 1 : 0, p.reason, p.op, p.dtype, (long long)p.batch, (long long)p.n, (long long)p.nrhs,
                         p.form == kLinalgLds ? "lds" : "blocked", LINALG_LDS_SIDE, p.nb, p.steps, p.launches, p.ws_bytes, l.threads, l.grid_x, l.grid_y,
                         l.lds_bytes, p.potrf.threads, p.potrf.grid_x, p.potrf.lds_bytes, p.potrf.mpw, p.potrf.tpm, p.potrf.ld, p.solve.threads,
                         p.solve.grid_x, p.solve.grid_y, p.solve.lds_bytes, p.solve.mpw, p.solve.cpw, p.solve.ld);
  LAMP_CHECK(w > 0 && w < buflen && w < (int)sizeof(text), "lamp_debug_linalg_plan: buffer too small");
  memcpy(buf, text, w + 1);
  LAMP_API_END
}

}  // extern "C"
