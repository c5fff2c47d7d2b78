// Batched symmetric eigendecomposition in f64 for Shampoo's preconditioners (nn/Shampoo.scala:142-146 calls svd on the f64 copy of a
// statistics matrix of side <= 512): one-sided (Hestenes) Jacobi, one workgroup per matrix, one launch for every matrix of a form.
//
// W is an f64 copy of the whole matrix (both triangles: f32 statistics are not bit-symmetric), stored column-major.  A sweep is
// m - 1 rounds of a round-robin pairing of the columns (m = n rounded up to even; with an odd n one column has a bye per round).  A
// wave owns a pair (i, j) - or, for sides up to 256, two or four pairs on 32 or 16 lanes each: the lanes stride down the rows, the three
// dot products a = wi.wi, b = wj.wj, c = wi.wj are reductions over those lanes, and the two columns are rotated in registers unless
// |c| <= tol * sqrt(a) * sqrt(b).  One workgroup barrier per round; the sweep that rotates nothing is the last one.  Then the column norms are the singular values (= eigenvalues of a PSD matrix) and the
// normalised columns are U; V is never accumulated.  The values are ranked by counting and written in descending order, U with its
// columns in that order.
//
// Two residencies: n <= 128 keeps W in LDS (128 KiB of the CU's 160; a column is contiguous, so the 64 lanes of a wave read 64
// consecutive f64), 128 < n <= 512 keeps it in a global workspace (2 MiB at 512: L2-resident) with the same structure.
// Every loop is bounded: EIG_MAX_SWEEPS sweeps at the most, and nothing waits on data.  status[m] = sweeps used, or a negative code.
#include "device_utils.h"

namespace lamp {

constexpr int EIG_MAX_SIDE = 512;
constexpr int EIG_LDS_SIDE = 128;
constexpr int EIG_MAX_SWEEPS = 30;
constexpr int EIG_THREADS = 1024;          // 16 waves: 16 to 64 pairs in flight per round
constexpr int EIG_BATCH = 64;              // matrices per launch (the descriptor is a by-value kernel argument)
constexpr int EIG_NOT_CONVERGED = -1;
constexpr int EIG_NON_FINITE = -2;

struct EigArgs {
  int count;                     // matrices of this launch
  int total;                     // status words of the whole call (a failed finiteness check anywhere stops every workgroup)
  int side[EIG_BATCH];
  int f32[EIG_BATCH];            // source dtype
  int slot[EIG_BATCH];           // index of the matrix in the call = its status word
  const void* src[EIG_BATCH];    // [n, n] row-major, f32 or f64
  double* work[EIG_BATCH];       // global form: n * n f64
  double* values[EIG_BATCH];     // [n]
  double* vectors[EIG_BATCH];    // [n, n] row-major or null
  int* status;
};
static_assert(sizeof(EigArgs) <= 4096, "EigArgs is passed by value: HIP kernel arguments are limited to 4 KB");

__device__ __forceinline__ double eig_load(const void* src, int f32, int64_t i) {
  return f32 ? (double)((const float*)src)[i] : ((const double*)src)[i];
}

// status[slot] = EIG_NON_FINITE for a matrix with a NaN or an infinity, 0 otherwise: the decomposition kernels write nothing when
// any matrix of the call failed this check
__global__ __launch_bounds__(256) void eig_check_kernel(EigArgs a) {
  const int m = blockIdx.x, n = a.side[m];
  int bad = 0;
  for (int64_t e = threadIdx.x; e < (int64_t)n * n; e += blockDim.x) {
    const double v = eig_load(a.src[m], a.f32[m], e);
    bad |= !(fabs(v) <= 1.79769313486231570815e308);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) a.status[a.slot[m]] = bad ? EIG_NON_FINITE : 0;
}

// the sum over the LP lanes that share a pair (LP a power of two <= 64; every lane of the wave takes part in the exchange)
template <int LP, class T> __device__ __forceinline__ T eig_group_sum(T v) {
#pragma unroll
  for (int off = LP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// LP = lanes per pair (a wave holds 64 / LP pairs at a time: a small matrix has few rows and many pairs), R = rows per lane (n <= LP * R)
template <bool IN_LDS, int LP, int R>
__global__ __launch_bounds__(EIG_THREADS) void eig_jacobi_kernel(EigArgs a) {
  extern __shared__ double eig_lds[];
  __shared__ double sig[EIG_MAX_SIDE];
  __shared__ int perm[EIG_MAX_SIDE];
  const int m = blockIdx.x, n = a.side[m];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = EIG_THREADS / 64;
  constexpr int GROUPS = 64 / LP;                                      // pairs per wave
  const int sub = lane / LP, gl = lane % LP;
  int bad = 0;
  for (int k = tid; k < a.total; k += EIG_THREADS) bad |= a.status[k] < 0;
  if (__syncthreads_or(bad)) return;                                   // (uniform: every thread gets the same answer)
  double* W = IN_LDS ? eig_lds : a.work[m];
  for (int e = tid; e < n * n; e += EIG_THREADS) {                     // coalesced read of row i; W[j * n + i] = A[i][j]
    const int i = e / n, j = e - i * n;
    W[j * n + i] = eig_load(a.src[m], a.f32[m], e);
  }
  __syncthreads();
  const int me = (n + 1) & ~1, half = me >> 1, rounds = me - 1;
  // relative to sqrt(a b): sqrt(n) * 2^-52 is the rounding of the dot product itself; never below 4 * 2^-52, which a pair that has just
  // been rotated in f64 reaches (a tighter one rotates on its own rounding error).  Both are within the 4 n 2^-52 orthogonality bound.
  const double tol = fmax(sqrt((double)n), 4.0) * 2.220446049250313e-16;
  int sweeps = 0, converged = 0;
  for (int sweep = 0; sweep < EIG_MAX_SWEEPS && n > 1; sweep++) {
    int rotated = 0;
    for (int r = 0; r < rounds; r++) {
      for (int k0 = wave * GROUPS; k0 < half; k0 += nwaves * GROUPS) {  // (wave-uniform trip count: the exchanges below need every lane)
        // circle method: me - 1 stays, the others turn; every column meets every other one once per sweep
        const int k = k0 + sub;
        const int ci = (r + k) % rounds, cj = k == 0 ? me - 1 : (r - k + rounds) % rounds;
        const bool pair = k < half && ci < n && cj < n;                // (false: past the last pair, or the bye of an odd n)
        double* wi = W + ci * n;
        double* wj = W + cj * n;
        double x[R], y[R], aa = 0, bb = 0, cc = 0;
#pragma unroll
        for (int q = 0; q < R; q++) {
          const int row = gl + LP * q;
          x[q] = pair && row < n ? wi[row] : 0.0;
          y[q] = pair && row < n ? wj[row] : 0.0;
          aa += x[q] * x[q]; bb += y[q] * y[q]; cc += x[q] * y[q];
        }
        aa = eig_group_sum<LP>(aa); bb = eig_group_sum<LP>(bb); cc = eig_group_sum<LP>(cc);
        if (fabs(cc) > tol * sqrt(aa) * sqrt(bb)) {                    // not orthogonal enough (false for a zero column and for no pair)
          const double zeta = (bb - aa) / (2.0 * cc);
          const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
          for (int q = 0; q < R; q++) {
            const int row = gl + LP * q;
            if (row < n) { wi[row] = cs * x[q] - sn * y[q]; wj[row] = sn * x[q] + cs * y[q]; }
          }
          rotated = 1;
        }
      }
      __syncthreads();                                                 // the round's columns are disjoint; the next round regroups them
    }
    sweeps = sweep + 1;
    if (!__syncthreads_or(rotated)) { converged = 1; break; }
  }
  if (n <= 1) { sweeps = 1; converged = 1; }
  for (int j = wave; j < n; j += nwaves) {
    double s = 0;
    for (int row = lane; row < n; row += 64) { const double v = W[j * n + row]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) sig[j] = sqrt(s);
  }
  __syncthreads();
  if (tid < n) {                                                       // descending rank by counting; ties keep their column order
    const double s = sig[tid];
    int rank = 0;
    for (int k = 0; k < n; k++) rank += (sig[k] > s) || (sig[k] == s && k < tid);
    perm[rank] = tid;
    a.values[m][rank] = s;
  }
  __syncthreads();
  if (a.vectors[m]) {
    double* U = a.vectors[m];
    for (int e = tid; e < n * n; e += EIG_THREADS) {
      const int i = e / n, c = e - i * n, j = perm[c];
      const double s = sig[j];
      U[e] = s > 0 ? W[j * n + i] / s : 0.0;                           // a zero column of a singular matrix stays zero
    }
  }
  if (tid == 0) a.status[a.slot[m]] = converged ? sweeps : EIG_NOT_CONVERGED;
}

}  // namespace lamp

using namespace lamp;

extern "C" {

int lamp_symmetric_eig(lamp_tensor* const* matrices, int n, lamp_tensor* const* values_out, lamp_tensor* const* vectors_out_or_null,
                       lamp_tensor* status_out_or_null) {
  LAMP_API_BEGIN
  if (n == 0) return 0;
  LAMP_CHECK(matrices && values_out, "matrices and values_out are arrays of n tensors");
  check_device_tensor(matrices[0], "matrix");                          // host matrices: the staging layer runs the call on GPU copies
  const int dev = matrices[0]->device();
  std::vector<Hold> keep;                                              // contiguous copies of strided inputs, workspaces
  std::vector<const lamp_tensor*> src(n);
  for (int i = 0; i < n; i++) {
    const lamp_tensor* t = matrices[i];
    check_device_tensor(t, "matrix");
    check_device_tensor(values_out[i], "values_out");
    LAMP_CHECK(t->device() == dev && values_out[i]->device() == dev, "matrix " << i << " or its values are on another device");
    LAMP_CHECK(t->ndim == 2 && t->sizes[0] == t->sizes[1] && t->sizes[0] >= 1, "matrix " << i << " is " << t->describe() << ", expected a square matrix");
    LAMP_CHECK(t->sizes[0] <= EIG_MAX_SIDE, "matrix " << i << " has side " << t->sizes[0] << ", the limit is " << EIG_MAX_SIDE);
    LAMP_CHECK(t->dtype == kF32 || t->dtype == kF64, "matrix " << i << " is " << dtype_name(t->dtype) << ", expected f32 or f64");
    const lamp_tensor* v = values_out[i];
    LAMP_CHECK(v->dtype == kF64 && v->ndim == 1 && v->sizes[0] == t->sizes[0] && v->is_contiguous(), "values_out " << i << " is " << v->describe() << ", expected f64[" << t->sizes[0] << "]");
    if (vectors_out_or_null) {
      const lamp_tensor* u = vectors_out_or_null[i];
      check_device_tensor(u, "vectors_out");
      LAMP_CHECK(u->device() == dev && u->dtype == kF64 && u->ndim == 2 && u->sizes[0] == t->sizes[0] && u->sizes[1] == t->sizes[0] && u->is_contiguous(),
                 "vectors_out " << i << " is " << u->describe() << ", expected f64[" << t->sizes[0] << "," << t->sizes[0] << "]");
    }
  }
  for (int i = 0; i < n; i++) {
    src[i] = matrices[i];
    if (!(matrices[i]->strides[1] == 1 && matrices[i]->strides[0] == matrices[i]->sizes[1]) && matrices[i]->sizes[0] > 1) {
      keep.emplace_back(contiguous(matrices[i]));
      src[i] = keep.back().get();
    }
  }
  hipStream_t st = current_stream(dev);
  int64_t ns[1] = {n};
  if (status_out_or_null) {
    const lamp_tensor* s = status_out_or_null;
    check_device_tensor(s, "status_out");
    LAMP_CHECK(s->device() == dev && s->dtype == kI32 && s->ndim == 1 && s->sizes[0] == n && s->is_contiguous(), "status_out is " << s->describe() << ", expected i32[" << n << "]");
  }
  Hold status(status_out_or_null ? retain(status_out_or_null) : new_tensor(ns, 1, kI32, dev));
  auto fill = [&](EigArgs& a, int i) {
    const int k = a.count++;
    a.side[k] = (int)src[i]->sizes[0];
    a.f32[k] = src[i]->dtype == kF32;
    a.slot[k] = i;
    a.src[k] = src[i]->raw();
    a.work[k] = nullptr;
    a.values[k] = values_out[i]->ptr<double>();
    a.vectors[k] = vectors_out_or_null ? vectors_out_or_null[i]->ptr<double>() : nullptr;
  };
  for (int base = 0; base < n; base += EIG_BATCH) {
    EigArgs a{};
    a.total = n; a.status = status->ptr<int>();
    for (int i = base; i < std::min(n, base + EIG_BATCH); i++) fill(a, i);
    hipLaunchKernelGGL(eig_check_kernel, dim3(a.count), dim3(256), 0, st, a);
  }
  LAMP_LAUNCH_CHECK();
  for (int form = 0; form < 2; form++) {                               // 0: W in LDS, 1: W in a global workspace
    std::vector<int> sel;
    for (int i = 0; i < n; i++) if ((src[i]->sizes[0] > EIG_LDS_SIDE) == (form == 1)) sel.push_back(i);
    for (size_t base = 0; base < sel.size(); base += EIG_BATCH) {
      EigArgs a{};
      a.total = n; a.status = status->ptr<int>();
      int max_side = 0;
      for (size_t k = base; k < std::min(sel.size(), base + EIG_BATCH); k++) {
        fill(a, sel[k]);
        const int side = a.side[a.count - 1];
        max_side = std::max(max_side, side);
        if (form == 1) {
          int64_t ws[1] = {(int64_t)side * side};
          keep.emplace_back(new_tensor(ws, 1, kF64, dev));
          a.work[a.count - 1] = keep.back()->ptr<double>();
        }
      }
      if (form == 0) {
        const size_t lds = (size_t)max_side * max_side * sizeof(double);
        if (max_side <= 64) {
          hipLaunchKernelGGL((eig_jacobi_kernel<true, 16, 4>), dim3(a.count), dim3(EIG_THREADS), lds, st, a);
        } else {
          // up to 128 KiB of dynamic LDS next to the kernel's 6.25 KiB of static LDS (allow_big_lds asks for all 160 KiB as dynamic, which
          // a kernel with static LDS cannot be given)
          HIP_CHECK(hipFuncSetAttribute((const void*)eig_jacobi_kernel<true, 32, 4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        EIG_LDS_SIDE * EIG_LDS_SIDE * (int)sizeof(double)));
          hipLaunchKernelGGL((eig_jacobi_kernel<true, 32, 4>), dim3(a.count), dim3(EIG_THREADS), lds, st, a);
        }
      } else {
        if (max_side <= 256) hipLaunchKernelGGL((eig_jacobi_kernel<false, 32, 8>), dim3(a.count), dim3(EIG_THREADS), 0, st, a);
        else hipLaunchKernelGGL((eig_jacobi_kernel<false, 64, 8>), dim3(a.count), dim3(EIG_THREADS), 0, st, a);
      }
      LAMP_LAUNCH_CHECK();
    }
  }
  // the one synchronisation of the call: the status words decide whether the results mean anything
  std::vector<int> host_status(n);
  HIP_CHECK(hipMemcpyAsync(host_status.data(), status->raw(), sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < n; i++)
    LAMP_CHECK(host_status[i] != EIG_NON_FINITE, "matrix " << i << " has a NaN or an infinity (nothing was written)");
  for (int i = 0; i < n; i++)
    LAMP_CHECK(host_status[i] > 0, "matrix " << i << " did not converge in " << EIG_MAX_SWEEPS << " sweeps");
  LAMP_API_END
}

}  // extern "C"
