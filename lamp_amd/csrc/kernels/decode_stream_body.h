// The body of the split-K weight-streaming kernels (decode_stream.h has the description).  Textually included, once, inside each of the
// two kernels: a kernel compiled from this text goes through the optimiser as one function, where the same text in a device function
// is optimised on its own first and then inlined, which with this compiler merges the two finishes and changes one contraction in GRU's
// cell and the stores of the 16-row epilogues (EXPERIMENTS.md, "Decode kernels: one skeleton, one host plan").  In scope where it is
// included: the types T, the constants CL, V (CL % V == 0), RT, the kernel's argument struct p (w [K, N], N, R, Kc, S and, with S > 1,
// slab [S, R, N] and the stream's ticket), int64_t K, and the operation op (prepare, image, finish).  It returns from the kernel.
  using A = acc_t<T>;
  static_assert(CL % V == 0, "a lane's columns are whole packets");
  constexpr int RW = (RT + kDecWaves - 1) / kDecWaves;
  constexpr int NP = CL / V;
  constexpr int UN = dec_unroll(CL, sizeof(T));
  __shared__ A xs[kDecKcMax * RT];                     // [k - k0][row]
  __shared__ A red[(kDecWaves - 1) * 64 * CL];         // one row's sums of the waves 1 ..
  __shared__ unsigned lastFlag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t N = p.N;
  const int R = p.R;
  const int64_t n0 = ((int64_t)blockIdx.x * 64 + lane) * CL;
  const int64_t k0 = (int64_t)blockIdx.y * p.Kc;
  const int kn = (int)(min(k0 + (int64_t)p.Kc, K) - k0);
  op.prepare(tid, lane, wave);
  for (int i = tid; i < kn * RT; i += 64 * kDecWaves) {
    const int kk = i / RT, r = i - kk * RT;
    xs[i] = r < R ? op.image(r, k0 + kk) : A(0);
  }
  __syncthreads();

  A acc[RT][CL];
#pragma unroll
  for (int r = 0; r < RT; r++)
#pragma unroll
    for (int j = 0; j < CL; j++) acc[r][j] = A(0);
  const bool mine = n0 < N;            // N % CL == 0: a lane's columns are inside or outside together
  if (mine) {
    const int kw = (kn + kDecWaves - 1) / kDecWaves, ke = min(kn, (wave + 1) * kw);
    const T* wp = p.w + k0 * N + n0;
    int kk = wave * kw;
    for (; kk + UN <= ke; kk += UN) {
      Vec<T, V> wv[UN][NP];
#pragma unroll
      for (int u = 0; u < UN; u++)
#pragma unroll
        for (int q = 0; q < NP; q++) wv[u][q] = load_packet<T, V>(wp + (int64_t)(kk + u) * N + q * V);
#pragma unroll
      for (int u = 0; u < UN; u++)
#pragma unroll
        for (int r = 0; r < RT; r++) {
          const A xv = xs[(kk + u) * RT + r];
#pragma unroll
          for (int q = 0; q < NP; q++)
#pragma unroll
            for (int j = 0; j < V; j++) acc[r][q * V + j] += xv * load_as<A>(wv[u][q].v[j]);
        }
    }
    for (; kk < ke; kk++) {
      Vec<T, V> wv[NP];
#pragma unroll
      for (int q = 0; q < NP; q++) wv[q] = load_packet<T, V>(wp + (int64_t)kk * N + q * V);
#pragma unroll
      for (int r = 0; r < RT; r++) {
        const A xv = xs[kk * RT + r];
#pragma unroll
        for (int q = 0; q < NP; q++)
#pragma unroll
          for (int j = 0; j < V; j++) acc[r][q * V + j] += xv * load_as<A>(wv[q].v[j]);
      }
    }
  }
  // the waves' sums, row by row through LDS, added in wave order into wave 0
#pragma unroll
  for (int r = 0; r < RT; r++) {
    if (r < R) {
      if (wave > 0)
#pragma unroll
        for (int j = 0; j < CL; j++) red[((wave - 1) * 64 + lane) * CL + j] = acc[r][j];
      __syncthreads();
      if (wave == 0)
        for (int w = 0; w < kDecWaves - 1; w++)
#pragma unroll
          for (int j = 0; j < CL; j++) acc[r][j] += red[(w * 64 + lane) * CL + j];
      __syncthreads();
    }
  }
  if (p.S == 1) {
    if (wave == 0 && mine)
#pragma unroll
      for (int r = 0; r < RT; r++)
        if (r < R) op.finish(acc[r], r, n0);
    return;
  }
  // publish this slice's sums, draw a ticket; the workgroup that draws the last one adds the slabs in slice order
  if (wave == 0 && mine) {
#pragma unroll
    for (int r = 0; r < RT; r++)
      if (r < R)
#pragma unroll
        for (int j = 0; j < CL; j++) p.slab[((int64_t)blockIdx.y * R + r) * N + n0 + j] = acc[r][j];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old = __hip_atomic_fetch_add(&p.ticket[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned last = old == (unsigned)(p.S - 1) ? 1u : 0u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(&p.ticket[blockIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the stream's next launch
    }
    lastFlag = last;
  }
  __syncthreads();
  if (!lastFlag || !mine) return;
  // the rows wave, wave + 4, ...: kDecSlabBatch slabs' loads in flight, added in slice order
#pragma unroll
  for (int q = 0; q < RW; q++) {
    const int r = wave + kDecWaves * q;
    if (r >= R) continue;
    A t[CL];
#pragma unroll
    for (int j = 0; j < CL; j++) t[j] = A(0);
    for (int s = 0; s < p.S; s += kDecSlabBatch) {
      A b[kDecSlabBatch][CL];
#pragma unroll
      for (int i = 0; i < kDecSlabBatch; i++)
#pragma unroll
        for (int j = 0; j < CL; j++) b[i][j] = s + i < p.S ? p.slab[((int64_t)(s + i) * R + r) * N + n0 + j] : A(0);
#pragma unroll
      for (int i = 0; i < kDecSlabBatch; i++)
#pragma unroll
        for (int j = 0; j < CL; j++) t[j] += b[i][j];
    }
    op.finish(t, r, n0);
  }
