// Matrix-core convolution for the NARROW bf16 layers of the CIFAR ResNet (3..16 channels on 32x32 / 16x16 / 8x8
// maps: stem 3->6 5x5, res1 6->6 (stride 2), res2 6->16 (stride 2) and their 1x1 projections; reference
// workload example-cifar100/.../cnn.scala:89-131, op ops.scala:1547-1651).
//
// These layers are bound by activation traffic (a few FLOPs per byte), but a scalar-FMA direct convolution
// still needs ~100 VALU instructions per output pixel and ends up 3-10x above the HBM time.  Here the
// multiply-accumulates go to v_mfma_f32_16x16x32_bf16 with a formulation that needs NO im2col gather:
//
//   fprop / dgrad:   D[pixel][co] = sum_{(c, r)} sum_{j = 0..7} X[c][ho*sh + r][wo*sw + j] * Wk[(c, r)][j][co]
//     the K dimension is (channel, filter row) x an 8-wide window of the image row; Wk is the filter row
//     zero-padded from kw to 8 taps.  The A fragment of a lane (8 consecutive k of one pixel) is then 16
//     CONTIGUOUS bytes of the LDS image, one ds_read_b128 at 2-byte alignment (gfx950 has unaligned DS
//     access), the B fragments (packed weights) live in registers for the whole kernel.  The padding costs
//     MFMA work only, of which there is plenty to spare.  dgrad = fprop over the stride-dilated dy image
//     (zeros inserted while staging) with the filter mirrored and Cin/Cout swapped.
//   wgrad:           D[co][(ci, r, s)] = sum_{pixels} dY[co][p] * X[ci][ho*sh - ph + r][wo*sw - pw + s]
//     K runs over output pixels (8 consecutive pixels of a row per lane): A = 16 aligned bytes of dY,
//     B = 16 contiguous bytes of the shifted image row (stride 2: of its even / odd column plane).
//
// One workgroup stages one image (or a few 8x8 ones) in LDS with coalesced 16-byte loads and walks a strided
// range of images; every kernel reads each activation once and writes each result once.
// Accumulation is fp32 in a fixed order: results are bitwise reproducible.
#include "device_utils.h"
#include "conv_geom.h"
#include "conv_backends.h"
#include "../core/pack_cache.h"
#include "wgrad_reduce.h"
#include <type_traits>
#include <vector>
#include "conv_narrow_pack.h"
#include "../core/switches.h"

namespace lamp {

typedef nv_s8 __attribute__((aligned(2))) nv_s8_u;      // 16-byte LDS read at 2-byte alignment
typedef float nv_f4 __attribute__((ext_vector_type(4)));

struct NcvGeom {
  int N, C, CO;          // images, loop (K-side) channels, output channels
  int H, W;              // staged tensor [C][H][W]
  int Hs, Ws;            // LDS image [C][Hs][Ws]
  int top, left, dil;    // staged pixel (a, b) lands at (top + a*dil, left + b*dil)
  int Ho, Wo;            // output map
  int sh, sw, wx;        // window of output (ho, wo), filter row r: LDS row ho*sh + r, columns wo*sw + wx + [0, 8)
  int kh;
  int kh_inv;            // 65536 / kh + 1: pair / kh == (pair * kh_inv) >> 16 for pair < 4096 (no integer division in the prologue)
  int pf;                // the image fits the register prefetch (W % 8 == 0 and at most NCV_PF 16-byte packets per thread)
  // ncv_fwd2_kernel, dgrad of a PAIR (round 5): channels [0, C1) of the staged image come from the first tensor and take part with all kh
  // filter rows, channels [C1, C) come from a second tensor (the gradient of a sibling 1x1 convolution of the same input) and take part with
  // the centre row only: K pairs (c, r) = C1 * kh + (C - C1).  C1 = C: one source.
  int C1;
};

constexpr int NCV_LEFT = 8;   // staged images start at column 8: 16-byte aligned rows for the vector copy

// (the weight-fragment layout, ncv_weight_frag and NcvPackMany live in conv_narrow_pack.h: conv_igemm.hip packs these images in its own launch)
__global__ __launch_bounds__(256) void ncv_pack_kernel(NcvPackMany a) { ncv_pack_body(a, blockIdx.y, blockIdx.x * 256 + threadIdx.x); }

// Image staging in two halves, so that the NEXT image's global loads are in flight while the current one is multiplied: the image
// [C][H][W] is read as consecutive 16-byte packets (W % 8 == 0), packet tid + k * nthreads into register k of the thread, and
// written to the LDS image [C][Hs][Ws] at (top + a*dil, left + b*dil) once the previous image's reads are done.  A thread handles
// the same packets of every image, so their LDS destinations are computed once (ncv_stage_plan): -1 = no packet.
constexpr int NCV_PF = 4;
// (compile-time loop: the index reaches the body as a constant, so register arrays indexed by it never turn into scratch memory)
template <int I0, int I1, class F> __device__ __forceinline__ void ncv_static_for(F&& f) {
  if constexpr (I0 < I1) { f(std::integral_constant<int, I0>{}); ncv_static_for<I0 + 1, I1>(f); }
}
// (NPF: packets per thread; ncv_chain_kernel, whose first image is small and whose registers are scarce, holds 2)
template <int NPF> struct NcvPreT { uint4 v[NPF]; };
template <int NPF> struct NcvPlanT { int dst[NPF]; int src[NPF]; };      // src: element offset in the image's source tensor, + (1 << 30) for the second one
typedef NcvPreT<NCV_PF> NcvPre;
typedef NcvPlanT<NCV_PF> NcvPlan;
template <int NPF = NCV_PF>
__device__ __forceinline__ NcvPlanT<NPF> ncv_stage_plan(const NcvGeom& q, int tid, int nthreads) {
  NcvPlanT<NPF> pl;
  const int rc = q.W >> 3, total = q.C * q.H * rc, first = q.C1 * q.H * rc;
#pragma unroll
  for (int k = 0; k < NPF; k++) {
    const int i = tid + k * nthreads;
    const int b = i % rc, a = (i / rc) % q.H, c = i / (rc * q.H);
    pl.dst[k] = (q.pf && i < total) ? (c * q.Hs + q.top + a * q.dil) * q.Ws + q.left + b * 8 * q.dil : -1;
    pl.src[k] = i < first ? i * 8 : ((i - first) * 8) | (1 << 30);
  }
  return pl;
}
template <int NPF>
__device__ __forceinline__ void ncv_stage_load(NcvPreT<NPF>& r, const NcvPlanT<NPF>& pl, const bf16_t* __restrict__ sp, const bf16_t* __restrict__ sp2) {
  ncv_static_for<0, NPF>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if (pl.dst[k] >= 0) r.v[k] = *reinterpret_cast<const uint4*>(((pl.src[k] >> 30) ? sp2 : sp) + (pl.src[k] & ((1 << 30) - 1)));
  });
}
// the 8 values of a packet, `dil` elements apart (the zero-dilated image of an input gradient)
__device__ __forceinline__ void ncv_scatter8(unsigned short* d, const uint4& v, int dil) {
  const unsigned int u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; j++) { d[(2 * j) * dil] = (unsigned short)(u[j] & 0xffffu); d[(2 * j + 1) * dil] = (unsigned short)(u[j] >> 16); }
}
template <int NPF>
__device__ __forceinline__ void ncv_stage_store(unsigned short* xs, const NcvPreT<NPF>& r, const NcvPlanT<NPF>& pl, int dil) {
  ncv_static_for<0, NPF>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if (pl.dst[k] < 0) return;
    // (member-wise: a whole-struct copy is a memcpy, and a register array that only memcpys touch - dil a compile-time 1 - stays in scratch memory)
    if (dil == 1) *reinterpret_cast<uint4*>(xs + pl.dst[k]) = make_uint4(r.v[k].x, r.v[k].y, r.v[k].z, r.v[k].w);
    else ncv_scatter8(xs + pl.dst[k], r.v[k], dil);
  });
}

__device__ __forceinline__ void ncv_stage(unsigned short* xs, const bf16_t* __restrict__ sp, const NcvGeom& q, int tid, int nthreads) {
  if (q.dil == 1) {
    const int rc = q.W >> 3, total = q.C * q.H * rc;
    for (int i = tid; i < total; i += nthreads) {
      const int b = i % rc, a = (i / rc) % q.H, c = i / (rc * q.H);
      const uint4 v = *reinterpret_cast<const uint4*>(sp + (c * q.H + a) * q.W + b * 8);
      *reinterpret_cast<uint4*>(xs + (c * q.Hs + q.top + a) * q.Ws + q.left + b * 8) = v;
    }
  } else {
    const int total = q.C * q.H * q.W;
    for (int i = tid; i < total; i += nthreads) {
      const int b = i % q.W, a = (i / q.W) % q.H, c = i / (q.W * q.H);
      xs[(c * q.Hs + q.top + a * q.dil) * q.Ws + q.left + b * q.dil] = sp[i].bits;
    }
  }
}

template <int NK>
__global__ __launch_bounds__(256) void ncv_fwd_kernel(const bf16_t* __restrict__ src, const nv_bf8* __restrict__ wpk, const bf16_t* __restrict__ bias,
                                                      bf16_t* __restrict__ dst, NcvGeom q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* xs = reinterpret_cast<unsigned short*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int co = lane & 15;
  nv_bf8 wfr[NK];
  int koff[NK];
#pragma unroll
  for (int ks = 0; ks < NK; ks++) {
    wfr[ks] = wpk[ks * 64 + lane];
    int pair = ks * 4 + (lane >> 4);
    if (pair >= q.C * q.kh) pair = 0;                    // padded k: weights are zero, any valid address will do
    const int c = (pair * q.kh_inv) >> 16, r = pair - c * q.kh;
    koff[ks] = (c * q.Hs + r) * q.Ws * 2;
  }
  const float bv = (bias && co < q.CO) ? (float)bias[co] : 0.f;
  const int HoWo = q.Ho * q.Wo, ntiles = (HoWo + 15) >> 4;
  const int img_elems = q.C * q.Hs * q.Ws;
  for (int o = tid * 8; o < img_elems; o += 256 * 8) *reinterpret_cast<uint4*>(xs + o) = make_uint4(0, 0, 0, 0);   // img_elems % 8 == 0
  for (int n = blockIdx.x; n < q.N; n += gridDim.x) {
    __syncthreads();                                     // zero fill / previous image's reads are done
    ncv_stage(xs, src + (int64_t)n * q.C * q.H * q.W, q, tid, 256);
    __syncthreads();
    bf16_t* yp = dst + (int64_t)n * q.CO * HoWo;
    for (int tile = wid; tile < ntiles; tile += 4) {
      const int p = min(tile * 16 + (lane & 15), HoWo - 1);
      const int ho = p / q.Wo, wo = p - ho * q.Wo;
      const char* base = smem + ((ho * q.sh) * q.Ws + wo * q.sw + q.wx) * 2;
      nv_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NK; ks++) {
        const nv_s8 a = *reinterpret_cast<const nv_s8_u*>(base + koff[ks]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(nv_bf8, a), wfr[ks], acc, 0, 0, 0);
      }
      // D: column = output channel (lane & 15), rows = 4 consecutive pixels
      const int p4 = tile * 16 + (lane >> 4) * 4;
      if (co < q.CO && p4 < HoWo) {
        const bf16_t o0(acc[0] + bv), o1(acc[1] + bv), o2(acc[2] + bv), o3(acc[3] + bv);
        uint2 pk;
        pk.x = (unsigned)o0.bits | ((unsigned)o1.bits << 16);
        pk.y = (unsigned)o2.bits | ((unsigned)o3.bits << 16);
        *reinterpret_cast<uint2*>(yp + co * HoWo + p4) = pk;
      }
    }
  }
}

// Aligned-window variant.  An unaligned ds_read_b128 runs at ~1/11 of the aligned rate on gfx950
// (scripts/microbench/lds_unaligned.hip), and the windows of neighbouring pixels start 2 (stride 1) or 4 bytes
// apart.  So one MFMA tile takes 16 pixels whose windows have the SAME phase inside a 16-byte segment: columns
// cg*P + d with a fixed d (P = 8 / stride phases), from TR = 16 / (Wo / P) image rows.  The P tiles d = 0..P-1 of
// such a "super-tile" (TR full output rows) read the SAME two or three aligned segments per lane, which are loaded
// once and funnel-shifted in registers by a compile-time amount; a lane ends up holding P consecutive output
// pixels per accumulator register, stored as one 16- or 8-byte write.
//   PH0 = (window origin wx) & 7.
// -DNCV_STAMP (diagnostic builds only; scripts/ncv_stamp_probe.py): s_memtime stamps of thread 0 of the first 1024 workgroups
#if defined(NCV_SKIP) && (NCV_SKIP & 2)
#define NCV_STORE_COND && pk[0] == 0x12345678u
#else
#define NCV_STORE_COND
#endif
#ifdef NCV_STAMP
__device__ unsigned long long ncv_stamps[1024 * 8];
#define NCV_STAMP_AT(k) do { if (threadIdx.x == 0 && blockIdx.x < 1024) ncv_stamps[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define NCV_STAMP_ONCE(k) do { if (n == (int)blockIdx.x) NCV_STAMP_AT(k); } while (0)
#else
#define NCV_STAMP_AT(k) do { } while (0)
#define NCV_STAMP_ONCE(k) do { } while (0)
#endif
//   NS = shifts per MFMA (see NcvW): NS = 2 halves the P window phases an MFMA has to be issued for.
//   ADD: dst = round(round(conv) + add) - a separate instantiation (dgrad only: SW = 1) because the addend's registers cost the plain
//   kernels a wave of occupancy
struct NcvWf { float n, mean, m2; };
__device__ __forceinline__ NcvWf ncv_wf_merge(const NcvWf& a, const NcvWf& b) {   // Chan's merge; either side may be empty
  NcvWf r;
  r.n = a.n + b.n;
  if (r.n == 0.f) { r.mean = 0.f; r.m2 = 0.f; return r; }
  const float d = b.mean - a.mean, f = b.n / r.n;
  r.mean = a.mean + d * f;
  r.m2 = a.m2 + b.m2 + d * d * a.n * f;
  return r;
}
//   STATS (fprop): the batch-norm statistics of the output leave with it, as Welford triples (count, mean, M2) over the ROUNDED values as
//   they are stored: stats[channel][part][3], part = image (stats_per_wg == 0) or workgroup (every workgroup walks the same number of images) -
//   the layout bn_merge_channel takes from the implicit-GEMM kernels (equal counts), so the batch norm behind a narrow convolution launches
//   no statistics pass (5 launches of the ResNet step).  The sums are taken by the matrix cores, which idle here: a lane's packed output
//   row IS a B fragment (8 bf16 of column j = lane & 15), so  ones . Y  accumulates sum y per column and  Y^T . Y  accumulates sum y^2 on its
//   diagonal - exact products, f32 accumulation, no VALU work per value (as shifted VALU sums the statistics cost the B = 2048 step what the
//   five statistics launches had cost).  Unshifted sums over at most a few thousand values: M2 loses ~1e-6 (mean / std)^2 relative.
//   The epilogue must not cost the kernel a wave of occupancy: hence the second launch bound.  What it still costs (scripts/ncv_stats_probe.py,
//   stem / 6 -> 6 / 6 -> 16 layer at N = 2048: 11.3 / 5.5 / 4.8 us without, 14.2 / 7.4 / 6.3 us with): 1.3 - 2.2 us for the end of the workgroup
//   (barrier, the waves' sums through LDS, one more store round trip behind the last output store) and, on the stem, 1.5 us of matrix-core time.
//   PAR (round 6; input gradients of stride-2 convolutions, kh = 3, NK even): the staged image is zero-dilated, so an output row meets non-zero
//   image rows under ONE parity of the filter row r only.  The K pairs are packed by that parity (NcvW::nke = NK / 2) and a super-tile takes TR
//   rows of one parity (rows blk * 2 TR + 2 tr + par): it runs the NK / 2 k-steps of its class instead of all NK - the other half multiplied
//   structural zeros (EXPERIMENTS 66: the two such launches of the step spent 12 and 9 us in their k-loops).  Same products, same order per
//   output element as far as non-zero terms go; the skipped terms were exact zeros.
// The pieces of the aligned-window kernel as device functions: ncv_fwd2_kernel runs them for one convolution (or a 3x3 with its sibling 1x1),
// ncv_chain_kernel runs them twice per image, the second time over the first one's output in LDS.
//   this lane's k-steps: B fragments (in registers for the whole kernel) and the byte offset of their (channel, filter row) in the LDS image
template <int NK, bool PAR>
__device__ __forceinline__ void ncv_frag_setup(const NcvGeom& q, const nv_bf8* __restrict__ wpk, int lane, nv_bf8 (&wfr)[NK], int (&koff)[NK]) {
  ncv_static_for<0, NK>([&](auto ksc) {
    constexpr int ks = decltype(ksc)::value;
    wfr[ks] = wpk[ks * 64 + lane];
    int pair = ks * 4 + (lane >> 4);
    const int pairs1 = q.C1 * q.kh;
    if (pair >= pairs1 + (q.C - q.C1)) pair = 0;
    int c = (pair * q.kh_inv) >> 16, r = pair - c * q.kh;
    if (pair >= pairs1) { c = q.C1 + (pair - pairs1); r = q.kh >> 1; }   // second source: centre row only
    if constexpr (PAR) {                                  // the packed image's parity order (NcvW::nke = NK / 2, kh == 3)
      const int pr = ks * 4 + (lane >> 4);
      if (ks < NK / 2) { c = pr >> 1; r = 2 * (pr & 1); if (c >= q.C1) { c = 0; r = 0; } }
      else {
        const int p2 = pr - (NK / 2) * 4;
        if (p2 < q.C1) { c = p2; r = 1; }
        else if (p2 < q.C) { c = p2; r = 1; }            // second source: channels [C1, C) of the staged image, centre row
        else { c = 0; r = 0; }                            // (padded pairs: zero weights, any valid address)
      }
    }
    koff[ks] = (c * q.Hs + r) * q.Ws * 2;
  });
}
//   ... of ONE parity class of the packed image only (PAR; cls 0: filter rows 0 and 2, k-steps [0, NK / 2); cls 1: the centre row and the
//   second source, k-steps [NK / 2, NK)): what a wave needs whose super-tiles all start on rows of one parity
template <int NK>
__device__ __forceinline__ void ncv_frag_setup_class(const NcvGeom& q, const nv_bf8* __restrict__ wpk, int lane, int cls, nv_bf8 (&wfr)[NK / 2], int (&koff)[NK / 2]) {
  ncv_static_for<0, NK / 2>([&](auto ksc) {
    constexpr int i = decltype(ksc)::value;
    wfr[i] = wpk[((cls ? NK / 2 : 0) + i) * 64 + lane];
    const int p2 = i * 4 + (lane >> 4);
    int c = cls ? p2 : p2 >> 1, r = cls ? 1 : 2 * (p2 & 1);
    if (c >= (cls ? q.C : q.C1)) { c = 0; r = 0; }        // (padded pairs: zero weights, any valid address)
    koff[i] = (c * q.Hs + r) * q.Ws * 2;
  });
}
//   sum y (every row of st1 alike) and sum y^2 (diagonal of st2: row j of column j = lane & 15 is register j & 3 of lane group j >> 2) of a
//   wave's `tiles` super-tiles
struct NcvStatAcc { nv_f4 st1, st2; int tiles; };
__device__ __forceinline__ void ncv_stats_take(NcvStatAcc& s, unsigned a, unsigned b, unsigned c, unsigned d) {
  typedef unsigned int nv_u4 __attribute__((ext_vector_type(4)));
  const unsigned ones2 = 0x3f803f80u;                      // two bf16 ones
  const nv_bf8 ones = __builtin_bit_cast(nv_bf8, nv_u4{ones2, ones2, ones2, ones2});
  const nv_bf8 y = __builtin_bit_cast(nv_bf8, nv_u4{a, b, c, d});
  s.st1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, y, s.st1, 0, 0, 0);
  s.st2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y, y, s.st2, 0, 0, 0);
}
//   ... -> sst[wave][column] = (count, sum y, sum y^2); VPT = output values per column and super-tile
template <int VPT>
__device__ __forceinline__ void ncv_stats_leave(NcvStatAcc& s, float (*sst)[16][3], int lane, int wid) {
  const int j = lane & 15, r = j & 3;
  const float sq = r == 0 ? s.st2[0] : r == 1 ? s.st2[1] : r == 2 ? s.st2[2] : s.st2[3];
  if ((lane >> 4) == (j >> 2)) { sst[wid][j][0] = (float)(s.tiles * VPT); sst[wid][j][1] = s.st1[0]; sst[wid][j][2] = sq; }
  s.st1 = nv_f4{0.f, 0.f, 0.f, 0.f}; s.st2 = nv_f4{0.f, 0.f, 0.f, 0.f}; s.tiles = 0;
}
//   the waves' sums of one part (left in sst before the barrier the caller has just passed) -> stats[channel][part] = (count, mean, M2),
//   added in wave order; NS = 2: channel co sits in columns co and co + 8
template <int NS>
__device__ __forceinline__ void ncv_stats_flush(float (*sst)[16][3], int lane, int wid, int nwaves, int CO, int co_a, float* __restrict__ stats,
                                                float* __restrict__ stats2, int part, int nparts) {
  if (wid == 0 && lane < (NS == 2 ? 8 : 16) && lane < CO) {
    float cnt = 0.f, sy = 0.f, sq = 0.f;
    for (int h = 0; h < NS; h++)
      for (int k = 0; k < nwaves; k++) { cnt += sst[k][lane + 8 * h][0]; sy += sst[k][lane + 8 * h][1]; sq += sst[k][lane + 8 * h][2]; }
    const float mean = sy / cnt;                         // (cnt > 0: every image has at least one super-tile)
    float* o = lane < co_a ? stats + ((int64_t)lane * nparts + part) * 3 : stats2 + ((int64_t)(lane - co_a) * nparts + part) * 3;
    o[0] = cnt; o[1] = mean; o[2] = fmaxf(sq - sy * mean, 0.f);
  }
}
//   The super-tiles of ONE staged image (this wave's share): window reads, MFMAs, epilogue, stores to this lane's output plane yc.
//   smem: the LDS image; ap (ADD): this lane's plane of the addend; sa (STATS): the wave's running sums.
//   MIRROR (stride 1, plain tiles): every 16-byte packet stored to yc also goes to row (h, column cg * 8) of the lane's channel plane mc (row
//   pitch mws elements) of a second LDS image - the staged input of the convolution that reads this output next (ncv_chain_kernel)
//   NW = NK / 2 (PAR, an even number of waves): a wave's super-tiles all have the parity of its index, so wfr / koff hold its class alone
//   (ncv_frag_setup_class), k-step ks at index ks % NW
//   KGRP > 0: the scheduler keeps the window reads of at most KGRP k-steps ahead of their MFMAs (a fence behind every KGRP-th k-step).  Left
//   alone it hoists a whole class's reads - 8 k-steps of 8 to 12 registers with 16 k-steps - which a kernel that holds other state across
//   the super-tiles (ncv_bwd_pair_kernel: the weight gradient's accumulators and the next round's packets) pays for in scratch memory
template <int NK, int SW, int PH0, int NS, bool ADD, bool STATS, bool PAR, bool MIRROR, int NW = NK, int KGRP = 0>
__device__ __forceinline__ void ncv_super_tiles(const char* smem, const NcvGeom& q, const nv_bf8 (&wfr)[NW], const int (&koff)[NW], int a_off, float bv, int co,
                                                bf16_t* yc, const bf16_t* ap, NcvStatAcc& sa, unsigned short* mc, int mws, int lane, int wid, int nwaves) {
  constexpr int P = 8 / SW;
  constexpr int ND = P / NS;                               // accumulators (MFMAs per k-step) of a super-tile
  constexpr int NSEG = (PH0 + (ND - 1) * NS * SW + 7) < 16 ? 2 : 3;
  static_assert(!MIRROR || (P == 8 && !PAR), "the LDS copy takes whole 16-byte packets of plain tiles");
  static_assert(NW == NK || (PAR && NW * 2 == NK), "all k-steps, or one parity class of them");
  const int ncg = q.Wo / P, TR = 16 / ncg;
  const int nsuper = q.Ho / TR;
  for (int st = wid; st < nsuper; st += nwaves) {
    // rows of the super-tile: h0 + RS * tr (PAR: super-tiles 2 b and 2 b + 1 share the 2 TR rows of block b, one parity each)
    constexpr int RS = PAR ? 2 : 1;
    const int h0 = PAR ? (st >> 1) * (2 * TR) + (st & 1) : st * TR;
    const char* base = smem + a_off + h0 * q.sh * q.Ws * 2;
    nv_f4 acc[ND];
#pragma unroll
    for (int d = 0; d < ND; d++) acc[d] = nv_f4{0.f, 0.f, 0.f, 0.f};
#ifdef NCV_SKIP                      // diagnostic builds only (scripts/build_variant.sh): 1 = no k-loop, 2 = no output stores, 4 = no image staging
    if (NCV_SKIP & 1) { acc[0][0] = (float)lane; }
    else
#endif
    {
    auto kstep = [&](auto ksc) {
      constexpr int ks = decltype(ksc)::value;
      unsigned int sg[NSEG * 4 + 1];
#pragma unroll
      for (int e = 0; e < NSEG; e++) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + koff[ks % NW] + e * 16);
        sg[e * 4 + 0] = v.x; sg[e * 4 + 1] = v.y; sg[e * 4 + 2] = v.z; sg[e * 4 + 3] = v.w;
      }
      sg[NSEG * 4] = 0;
#pragma unroll
      for (int d = 0; d < ND; d++) {
        const int o = PH0 + d * NS * SW;                 // compile-time after unrolling: window origin of phase d * NS
        const int dq = o >> 1;
        unsigned int f[4];
#pragma unroll
        for (int j = 0; j < 4; j++) f[j] = (o & 1) ? __builtin_amdgcn_alignbit(sg[dq + j + 1], sg[dq + j], 16) : sg[dq + j];
        typedef unsigned int u4v __attribute__((ext_vector_type(4)));
        const u4v fv = {f[0], f[1], f[2], f[3]};
        acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(nv_bf8, fv), wfr[ks % NW], acc[d], 0, 0, 0);
      }
      if constexpr (KGRP > 0) { if ((ks % NW) % KGRP == KGRP - 1) __builtin_amdgcn_sched_barrier(0); }
    };
    if constexpr (PAR) {
      // rows h0 + 2 tr of the dilated image hold values iff (row + r - top) is even: the class of k-steps whose r has the parity of (h0 + top)
      if (((h0 + q.top) & 1) == 0) ncv_static_for<0, NK / 2>(kstep);          // r in {0, 2}
      else ncv_static_for<NK / 2, NK>(kstep);                                  // r = 1 (and the second source's centre row)
    } else ncv_static_for<0, NK>(kstep);
    }
    // ap != nullptr: dst = round(round(conv) + add) (see ig_conv8d_kernel); the rows this lane stores.  Requested after the MFMAs:
    // held across them they cost 12 - 20 registers and a wave of occupancy
    constexpr int NROW = NS == 1 ? 4 : 2;
    const int row0 = (lane >> 4) * 4 + (NS == 1 ? 0 : ((lane >> 3) & 1) * 2);
    uint4 addv[NROW];
    if (ADD && co < q.CO) {
#pragma unroll
      for (int k = 0; k < NROW; k++) {
        const int i = row0 + k, tr = i / ncg, cg = i - tr * ncg;
        const bf16_t* a = ap + (h0 + RS * tr) * q.Wo + cg * P;
        if (P == 8) addv[k] = *reinterpret_cast<const uint4*>(a);
        else { const uint2 t = *reinterpret_cast<const uint2*>(a); addv[k] = make_uint4(t.x, t.y, 0, 0); }
      }
    }
    if (STATS) sa.tiles++;
    if (NS == 1) {
      unsigned int prev[P / 2];                          // P = 4: two rows make one fragment
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int i = (lane >> 4) * 4 + rr;
        const int tr = i / ncg, cg = i - tr * ncg;
        bf16_t* o = yc + (h0 + RS * tr) * q.Wo + cg * P;
        unsigned int pk[P / 2];
#pragma unroll
        for (int d = 0; d < P; d += 2) {
          const bf16_t lo(acc[d % ND][rr] + bv), hi(acc[(d + 1) % ND][rr] + bv);
          pk[d >> 1] = (unsigned)lo.bits | ((unsigned)hi.bits << 16);
        }
        if (ADD) {
#pragma unroll
          for (int j = 0; j < P / 2; j++) pk[j] = add_bf16x2(pk[j], (&addv[rr % NROW].x)[j]);
        }
        if (STATS) {                                     // (every lane: the columns beyond CO carry zeros)
          if (P == 8) ncv_stats_take(sa, pk[0], pk[1], pk[2 % (P / 2)], pk[3 % (P / 2)]);
          else if (rr & 1) ncv_stats_take(sa, prev[0], prev[1], pk[0], pk[1]);
          else { prev[0] = pk[0]; prev[1] = pk[1]; }
        }
        if (co < q.CO NCV_STORE_COND) {
          if (P == 8) *reinterpret_cast<uint4*>(o) = make_uint4(pk[0], pk[1], pk[2 % (P / 2)], pk[3 % (P / 2)]);
          else *reinterpret_cast<uint2*>(o) = make_uint2(pk[0], pk[1]);
          if constexpr (MIRROR) *reinterpret_cast<uint4*>(mc + (h0 + tr) * mws + cg * 8) = make_uint4(pk[0], pk[1], pk[2 % (P / 2)], pk[3 % (P / 2)]);
        }
      }
    } else {
      // lane (s, co, g) holds phases 2d + s of rows 4g .. 4g+3; its partner lane ^ 8 holds the other parity.  The s = 0 lane
      // completes rows 4g, 4g+1 and the s = 1 lane rows 4g+2, 4g+3: each sends the two rows it does not store.
      const int sft = (lane >> 3) & 1;
      unsigned int keep[2][ND], got[2][ND];
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int d = 0; d < ND; d++) {
          const bf16_t mine(acc[d][sft * 2 + h] + bv), theirs(acc[d][(1 - sft) * 2 + h] + bv);    // rows this lane stores / sends
          keep[h][d] = mine.bits;
          got[h][d] = (unsigned)__shfl_xor((int)theirs.bits, 8, 64);
        }
      unsigned int prev[ND];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int i = (lane >> 4) * 4 + sft * 2 + h;
        const int tr = i / ncg, cg = i - tr * ncg;
        bf16_t* o = yc + (h0 + RS * tr) * q.Wo + cg * P;
        unsigned int pk[ND];
#pragma unroll
        for (int d = 0; d < ND; d++) {
          const unsigned int even = sft ? got[h][d] : keep[h][d], odd = sft ? keep[h][d] : got[h][d];
          pk[d] = even | (odd << 16);
        }
        if (ADD) {
#pragma unroll
          for (int d = 0; d < ND; d++) pk[d] = add_bf16x2(pk[d], (&addv[h % NROW].x)[d]);
        }
        if (STATS) {
          if (P == 8) ncv_stats_take(sa, pk[0], pk[1], pk[2 % ND], pk[3 % ND]);
          else if (h) ncv_stats_take(sa, prev[0], prev[1], pk[0], pk[1]);
          else { prev[0] = pk[0]; prev[1] = pk[1]; }
        }
        if (co < q.CO NCV_STORE_COND) {
          if (P == 8) *reinterpret_cast<uint4*>(o) = make_uint4(pk[0], pk[1], pk[2 % ND], pk[3 % ND]);
          else *reinterpret_cast<uint2*>(o) = make_uint2(pk[0], pk[1]);
          if constexpr (MIRROR) *reinterpret_cast<uint4*>(mc + (h0 + tr) * mws + cg * 8) = make_uint4(pk[0], pk[1], pk[2 % ND], pk[3 % ND]);
        }
      }
    }
  }
}

template <int NK, int SW, int PH0, int NS, bool ADD, bool STATS, bool PAR = false>
__global__ __launch_bounds__(256, (STATS && NK <= 5) ? 3 : 1) void ncv_fwd2_kernel(const bf16_t* __restrict__ src, const nv_bf8* __restrict__ wpk, const bf16_t* __restrict__ bias,
                                                       bf16_t* dst, NcvGeom q, const bf16_t* add, bf16_t* dst2, const bf16_t* __restrict__ bias2, int co_a,
                                                       float* __restrict__ stats, float* __restrict__ stats2, int stats_per_wg,
                                                       const bf16_t* __restrict__ src2) {
  // src2 (dgrad of a pair): the second source of the staged image, channels [q.C1, q.C)
  // co_a: output columns [0, co_a) belong to dst, [co_a, q.CO) to dst2 (the sibling 1x1 of NcvW; co_a = q.CO and dst2 = nullptr otherwise)
  __shared__ float sst[STATS ? 2 : 1][4][16][3];           // [image parity][wave][MFMA column]: the waves' triples of one image
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* xs = reinterpret_cast<unsigned short*>(smem);
  NCV_STAMP_AT(0);
  constexpr int P = 8 / SW;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
  const int co = NS == 2 ? (lane & 7) : (lane & 15);
  const int ncg = q.Wo / P;
  // The first image's packets are requested before anything else: a workgroup lives for two or three images, and in-kernel stamps
  // (scripts/ncv_stamp_probe.py) showed 3800 - 6300 of its 11 - 20 k cycles between "weights in registers" and "first image in LDS" -
  // the HBM round trip of that first load, started only after the weights had arrived and the LDS was zeroed.
  const int64_t img_in = (int64_t)q.C1 * q.H * q.W, img_in2 = (int64_t)(q.C - q.C1) * q.H * q.W;
  NcvPre pre;
  const NcvPlan plan = ncv_stage_plan(q, tid, nthreads);
  if (q.pf && (int)blockIdx.x < q.N) ncv_stage_load(pre, plan, src + blockIdx.x * img_in, src2 + blockIdx.x * img_in2);
  nv_bf8 wfr[NK];
  int koff[NK];
  ncv_frag_setup<NK, PAR>(q, wpk, lane, wfr, koff);
  const float bv = co < co_a ? (bias ? (float)bias[co] : 0.f) : ((bias2 && co < q.CO) ? (float)bias2[co - co_a] : 0.f);
#ifdef NCV_STAMP
  __builtin_amdgcn_s_waitcnt(0);
  NCV_STAMP_AT(1);
#endif
  const int HoWo = q.Ho * q.Wo;
  const int img_elems = q.C * q.Hs * q.Ws;
  for (int o = tid * 8; o < img_elems; o += nthreads * 8) *reinterpret_cast<uint4*>(xs + o) = make_uint4(0, 0, 0, 0);
  // A-side lane -> (row within the super-tile, column group)
  const int a_tr = (lane & 15) / ncg, a_cg = (lane & 15) - a_tr * ncg;
  const int a_off = ((PAR ? 2 : 1) * a_tr * q.sh * q.Ws + a_cg * 8 + (q.wx - PH0)) * 2;      // PAR: a tile's rows are two apart
  constexpr int VPT = 16 * P / NS;
  NcvStatAcc sa{nv_f4{0.f, 0.f, 0.f, 0.f}, nv_f4{0.f, 0.f, 0.f, 0.f}, 0};
  int it = 0;
  for (int n = blockIdx.x; n < q.N; n += gridDim.x, it++) {
    __syncthreads();                                     // zero fill / the previous image's reads are done
    NCV_STAMP_ONCE(2);
    if (STATS && !stats_per_wg && it > 0) ncv_stats_flush<NS>(sst[(it - 1) & 1], lane, wid, nwaves, q.CO, co_a, stats, stats2, n - (int)gridDim.x, q.N);
#if defined(NCV_SKIP) && (NCV_SKIP & 4)
    if (n < 0)
#endif
    {
    if (q.pf) ncv_stage_store(xs, pre, plan, q.dil);
    else ncv_stage(xs, src + n * img_in, q, tid, nthreads);
    }
    __syncthreads();
    NCV_STAMP_ONCE(3);
#if defined(NCV_SKIP) && (NCV_SKIP & 4)
    if (n < 0)
#endif
    if (q.pf && n + (int)gridDim.x < q.N)                 // in flight during the MFMAs
      ncv_stage_load(pre, plan, src + (n + (int)gridDim.x) * img_in, src2 + (n + (int)gridDim.x) * img_in2);
    // this lane's output plane: channel co of dst, or channel co - co_a of the sibling's tensor
    bf16_t* yc = co < co_a ? dst + ((int64_t)n * co_a + co) * HoWo : dst2 + ((int64_t)n * (q.CO - co_a) + (co - co_a)) * HoWo;
    const bf16_t* ap = ADD ? add + (int64_t)n * q.CO * HoWo + co * HoWo : nullptr;
    ncv_super_tiles<NK, SW, PH0, NS, ADD, STATS, PAR, false>(smem, q, wfr, koff, a_off, bv, co, yc, ap, sa, nullptr, 0, lane, wid, nwaves);
    if (STATS && !stats_per_wg) ncv_stats_leave<VPT>(sa, sst[it & 1], lane, wid);
    NCV_STAMP_ONCE(4);
  }
  if (STATS && it > 0) {
    if (stats_per_wg) ncv_stats_leave<VPT>(sa, sst[0], lane, wid);
    __syncthreads();
    if (stats_per_wg) ncv_stats_flush<NS>(sst[0], lane, wid, nwaves, q.CO, co_a, stats, stats2, (int)blockIdx.x, (int)gridDim.x);
    else ncv_stats_flush<NS>(sst[(it - 1) & 1], lane, wid, nwaves, q.CO, co_a, stats, stats2, (int)blockIdx.x + (it - 1) * (int)gridDim.x, q.N);
  }
#ifdef NCV_STAMP
  NCV_STAMP_AT(5);
  __builtin_amdgcn_s_waitcnt(0);
  NCV_STAMP_AT(6);
#endif
}

// A stride-1 convolution and the 3x3 + 1x1 pair that reads its output (the stem of Cnn.resnet and the two branches of the first residual block,
// cnn.scala:95-109: no batch norm between them, so nothing between x and (a, b) needs the whole batch) in ONE launch.  Per image: the first
// convolution's super-tiles run as in ncv_fwd2_kernel; each rounded 16-byte packet goes to s in global memory (the pair's weight gradient reads
// it in backward) AND into a second LDS image laid out as the pair's staged input (q1's top / left / pitch); after a barrier the pair's
// super-tiles run from that image, with the statistics epilogue of a and b.  Same MFMA chains over the same rounded values: s, a, b and the
// statistics are bitwise those of ncv_fwd2_kernel twice; what goes away is one launch and the 25 MB read of s (B = 2048).
// The first convolution is the two-shift form (NS = 2), the pair the one-shift form at stride 2: the geometries of the ResNet's entry.
constexpr int NCV_CHAIN_PF = 2;
template <int NK0, int PH00, int NK1, int PH01, bool STATS>
__global__ __launch_bounds__(256, NK1 <= 5 ? 3 : 1) void ncv_chain_kernel(const bf16_t* __restrict__ x, const nv_bf8* __restrict__ wpk0, const bf16_t* __restrict__ bias0,
                                                                          bf16_t* s, NcvGeom q0, const nv_bf8* __restrict__ wpk1, const bf16_t* __restrict__ bias1,
                                                                          const bf16_t* __restrict__ bias1b, bf16_t* ya, bf16_t* yb, int co_a, NcvGeom q1,
                                                                          float* __restrict__ stats, float* __restrict__ stats2, int stats_per_wg) {
  __shared__ float sst[STATS ? 2 : 1][4][16][3];
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int img0 = q0.C * q0.Hs * q0.Ws, img1 = q1.C * q1.Hs * q1.Ws;         // elements, multiples of 8
  unsigned short* xs0 = reinterpret_cast<unsigned short*>(smem);
  unsigned short* xs1 = xs0 + img0;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int co0 = lane & 7, co1 = lane & 15;
  const int64_t img_in = (int64_t)q0.C * q0.H * q0.W;
  NcvPreT<NCV_CHAIN_PF> pre;
  const NcvPlanT<NCV_CHAIN_PF> plan = ncv_stage_plan<NCV_CHAIN_PF>(q0, tid, 256);      // (the launcher fuses only images that fit the prefetch)
  if ((int)blockIdx.x < q0.N) ncv_stage_load(pre, plan, x + blockIdx.x * img_in, x);
  // The pair's fragments stay in registers; the first convolution's are read again for every image (the pair's phase alone needs all but five of
  // the 168 registers that three workgroups per CU leave a thread, and keeping both sets spilled 15 of them)
  nv_bf8 wfr1[NK1];
  int koff1[NK1];
  ncv_frag_setup<NK1, false>(q1, wpk1, lane, wfr1, koff1);
  const float bv0 = (bias0 && co0 < q0.CO) ? (float)bias0[co0] : 0.f;
  const float bv1 = co1 < co_a ? (bias1 ? (float)bias1[co1] : 0.f) : ((bias1b && co1 < q1.CO) ? (float)bias1b[co1 - co_a] : 0.f);
  for (int o = tid * 8; o < img0 + img1; o += 256 * 8) *reinterpret_cast<uint4*>(xs0 + o) = make_uint4(0, 0, 0, 0);
  const int ncg0 = q0.Wo / 8, ncg1 = q1.Wo / 4;
  const int a_tr0 = (lane & 15) / ncg0, a_cg0 = (lane & 15) - a_tr0 * ncg0;
  const int a_off0 = (a_tr0 * q0.sh * q0.Ws + a_cg0 * 8 + (q0.wx - PH00)) * 2;
  const int a_tr1 = (lane & 15) / ncg1, a_cg1 = (lane & 15) - a_tr1 * ncg1;
  const int a_off1 = (a_tr1 * q1.sh * q1.Ws + a_cg1 * 8 + (q1.wx - PH01)) * 2;
  const int HoWo0 = q0.Ho * q0.Wo, HoWo1 = q1.Ho * q1.Wo;
  // this lane's channel plane of the pair's image: pixel (h, w) of s at (top + h, left + w), as ncv_stage_store places a staged one
  unsigned short* mc = xs1 + (co0 * q1.Hs + q1.top) * q1.Ws + q1.left;
  constexpr int VPT = 16 * 4;
  NcvStatAcc sa{nv_f4{0.f, 0.f, 0.f, 0.f}, nv_f4{0.f, 0.f, 0.f, 0.f}, 0}, none = sa;
  int it = 0;
  for (int n = blockIdx.x; n < q0.N; n += gridDim.x, it++) {
    __syncthreads();                                     // zero fill / the previous image's reads of both LDS images are done
    if (STATS && !stats_per_wg && it > 0) ncv_stats_flush<1>(sst[(it - 1) & 1], lane, wid, 4, q1.CO, co_a, stats, stats2, n - (int)gridDim.x, q1.N);
    ncv_stage_store(xs0, pre, plan, 1);
    __syncthreads();
    if (n + (int)gridDim.x < q0.N) ncv_stage_load(pre, plan, x + (n + (int)gridDim.x) * img_in, x);      // in flight during both phases' MFMAs
    nv_bf8 wfr0[NK0];
    int koff0[NK0];
    int lane0 = lane;
    asm volatile("" : "+v"(lane0));                      // (opaque: keeps these loads inside the loop, out of the pair's phase)
    ncv_frag_setup<NK0, false>(q0, wpk0, lane0, wfr0, koff0);
    ncv_super_tiles<NK0, 1, PH00, 2, false, false, false, true>(smem, q0, wfr0, koff0, a_off0, bv0, co0, s + ((int64_t)n * q0.CO + co0) * HoWo0, nullptr, none,
                                                                mc, q1.Ws, lane, wid, 4);
    __syncthreads();                                     // s of this image is complete in the second LDS image
    bf16_t* yc = co1 < co_a ? ya + ((int64_t)n * co_a + co1) * HoWo1 : yb + ((int64_t)n * (q1.CO - co_a) + (co1 - co_a)) * HoWo1;
    ncv_super_tiles<NK1, 2, PH01, 1, false, STATS, false, false>(reinterpret_cast<const char*>(xs1), q1, wfr1, koff1, a_off1, bv1, co1, yc, nullptr, sa, nullptr, 0,
                                                                 lane, wid, 4);
    if (STATS && !stats_per_wg) ncv_stats_leave<VPT>(sa, sst[it & 1], lane, wid);
  }
  if (STATS && it > 0) {
    if (stats_per_wg) ncv_stats_leave<VPT>(sa, sst[0], lane, wid);
    __syncthreads();
    if (stats_per_wg) ncv_stats_flush<1>(sst[0], lane, wid, 4, q1.CO, co_a, stats, stats2, (int)blockIdx.x, (int)gridDim.x);
    else ncv_stats_flush<1>(sst[(it - 1) & 1], lane, wid, 4, q1.CO, co_a, stats, stats2, (int)blockIdx.x + (it - 1) * (int)gridDim.x, q1.N);
  }
}
#ifdef NCV_STAMP
extern "C" int lamp_debug_ncv_stamps(unsigned long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(ncv_stamps), sizeof(ncv_stamps)) == hipSuccess ? 0 : 1; }
#endif

// ---- wgrad ---------------------------------------------------------------------------------------------
struct NcvWGeom {
  int N, Cin, Cout, H, W, Ho, Wo;
  int kh, kw, ph, pw;
  int Hs, Ws;            // SW == 1: LDS x image [Cin][Hs][Ws]; SW == 2: [Cin][Hs][2 parities][Ws]
  int ncol;              // Cin * kh * kw
  int IG;                // images staged per round
  // ncv_wgrad2_kernel, weight gradients of a PAIR (round 5): rows [Cout, Cout + Cout2) of the staged gradient image come from a second tensor,
  // the output gradient of a sibling 1x1 convolution of the same x (same stride and output map); of their products only the centre tap is
  // its weight gradient [Cout2][Cin] (the other taps are computed and dropped: the MFMA's 16 rows were 6 of 16 used).  0: none.
  int Cout2;
};
constexpr int NCV_OFF2 = 4;   // stride 2: column w lives at plane (w & 1), position (w >> 1) + NCV_OFF2

template <int NT, int SW>
__global__ __launch_bounds__(256) void ncv_wgrad_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, float* __restrict__ partial, NcvWGeom q,
                                                        int images_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int HoWo = q.Ho * q.Wo;
  const int ximg = q.Cin * q.Hs * q.Ws * (SW == 2 ? 2 : 1);        // elements per staged image
  unsigned short* xs = reinterpret_cast<unsigned short*>(smem);      // [IG][ximg]
  unsigned short* ds = xs + q.IG * ximg;                             // [IG][16][HoWo]  (rows >= Cout stay zero)
  float* red = reinterpret_cast<float*>(ds + q.IG * 16 * HoWo);      // [4 waves][16][NT * 16]
  {
    const int tot = q.IG * (ximg + 16 * HoWo);                       // multiple of 8 (host guarantees)
    for (int o = tid * 8; o < tot; o += 256 * 8) *reinterpret_cast<uint4*>(xs + o) = make_uint4(0, 0, 0, 0);
  }
  // per-lane column (ci, r, s) of each n-tile -> byte offset of its shifted row inside a staged image
  int coff[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    int cidx = nt * 16 + (lane & 15);
    if (cidx >= q.ncol) cidx = 0;                                     // padded columns: computed, never written
    const int s = cidx % q.kw, r = (cidx / q.kw) % q.kh, ci = cidx / (q.kw * q.kh);
    if (SW == 1) coff[nt] = ((ci * q.Hs + r) * q.Ws + s - q.pw + NCV_LEFT) * 2;
    else {
      const int t = s - q.pw, par = t & 1, half = (t - par) >> 1;
      coff[nt] = (((ci * q.Hs + r) * 2 + par) * q.Ws + half + NCV_OFF2) * 2;
    }
  }
  nv_f4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) acc[nt] = nv_f4{0.f, 0.f, 0.f, 0.f};

  const int64_t n0 = (int64_t)blockIdx.x * images_per_block, n1 = min<int64_t>(n0 + images_per_block, q.N);
  const int chunks_per_img = HoWo >> 5;
  for (int64_t nb = n0; nb < n1; nb += q.IG) {
    const int ig = (int)min<int64_t>(q.IG, n1 - nb);
    __syncthreads();
    for (int im = 0; im < ig; im++) {
      const bf16_t* xp = x + (nb + im) * q.Cin * q.H * q.W;
      unsigned short* xi = xs + im * ximg;
      const int rc = q.W >> 3, total = q.Cin * q.H * rc;
      for (int i = tid; i < total; i += 256) {
        const int b = i % rc, a = (i / rc) % q.H, c = i / (rc * q.H);
        const uint4 v = *reinterpret_cast<const uint4*>(xp + (c * q.H + a) * q.W + b * 8);
        if (SW == 1) {
          *reinterpret_cast<uint4*>(xi + (c * q.Hs + q.ph + a) * q.Ws + NCV_LEFT + b * 8) = v;
        } else {
          // de-interleave even / odd columns
          uint2 ev, od;
          ev.x = (v.x & 0xffffu) | (v.y << 16); ev.y = (v.z & 0xffffu) | (v.w << 16);
          od.x = (v.x >> 16) | (v.y & 0xffff0000u); od.y = (v.z >> 16) | (v.w & 0xffff0000u);
          unsigned short* row = xi + ((c * q.Hs + q.ph + a) * 2) * q.Ws + NCV_OFF2 + b * 4;
          *reinterpret_cast<uint2*>(row) = ev;
          *reinterpret_cast<uint2*>(row + q.Ws) = od;
        }
      }
      const bf16_t* dp = dy + (nb + im) * q.Cout * HoWo;
      unsigned short* di = ds + im * 16 * HoWo;
      const int dtot = q.Cout * HoWo >> 3;
      for (int i = tid; i < dtot; i += 256) *reinterpret_cast<uint4*>(di + i * 8) = *reinterpret_cast<const uint4*>(dp + i * 8);
    }
    __syncthreads();
    const int nchunks = ig * chunks_per_img;
    for (int ch = wid; ch < nchunks; ch += 4) {
      const int pg = ch * 32 + (lane >> 4) * 8;                      // this lane's 8 consecutive output pixels
      const int im = pg / HoWo, pp = pg - im * HoWo;
      const int ho = pp / q.Wo, wo0 = pp - ho * q.Wo;
      const nv_s8 a = *reinterpret_cast<const nv_s8*>(ds + (im * 16 + (lane & 15)) * HoWo + pp);
      const char* xb = reinterpret_cast<const char*>(xs + im * ximg) +
                       (SW == 1 ? (ho * q.Ws + wo0) * 2 : ((ho * 2) * 2 * q.Ws + wo0) * 2);
#pragma unroll
      for (int nt = 0; nt < NT; nt++) {
        const nv_s8 b = *reinterpret_cast<const nv_s8_u*>(xb + coff[nt]);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(nv_bf8, a), __builtin_bit_cast(nv_bf8, b), acc[nt], 0, 0, 0);
      }
    }
  }
  // D: column = (ci, r, s) index, rows = 4 output channels; combine the 4 waves in a fixed order
#pragma unroll
  for (int nt = 0; nt < NT; nt++)
#pragma unroll
    for (int rr = 0; rr < 4; rr++) red[(wid * 16 + (lane >> 4) * 4 + rr) * (NT * 16) + nt * 16 + (lane & 15)] = acc[nt][rr];
  __syncthreads();
  const int O = q.Cout * q.ncol;
  for (int i = tid; i < O; i += 256) {
    const int co = i / q.ncol, cidx = i - co * q.ncol;
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < 4; w++) a += red[(w * 16 + co) * (NT * 16) + cidx];
    partial[(int64_t)blockIdx.x * O + i] = a;
  }
}

// Aligned-read wgrad.  The MFMA columns of one tile are 16 (ci, r) pairs at ONE filter column s, so the window shift s - pw is
// the same for the whole wave: per (32-pixel chunk, pair tile) a lane reads two or three ALIGNED 16-byte segments of its image
// row and cuts the KW shifted fragments out of them with compile-time funnel shifts (an unaligned ds_read_b128 costs 11 aligned
// ones, see ncv_fwd2_kernel).  Stride 2: even / odd column planes, filter column s reads plane (s - pw) & 1 at offset
// (s - pw) >> 1 in {-1, 0} (KW <= 3).  acc[pair tile][s] holds dW[co][(ci, r)][s].
constexpr int NCV_OFFA = 8;   // column origin of the staged rows (both strides): 16-byte aligned segments
constexpr int NCV_WPF = 6;    // 16-byte packets per thread the image-group prefetch holds
// The pieces of the aligned-read kernel as device functions: ncv_wgrad2_kernel runs them for one weight gradient (or a 3x3's with its sibling
// 1x1's), ncv_bwd_pair_kernel runs them beside the input gradient's super-tiles over the same staged gradients.
//   Staging in two halves (as in ncv_fwd2_kernel): the x and dy packets of the NEXT image group are loaded into registers while this group is
//   multiplied, and written to LDS after the barrier.  A group is [image][x packets | dy packets | second dy packets] of 16 bytes.  A thread
//   handles the same packets of every group: source offsets (elements, from the group's first image; negative: a dy packet, below -2^30: a
//   packet of the second gradient tensor) and LDS destinations (elements from xs) are computed once; im = image index within the group, or
//   -1 (no packet).  The staged gradient image of one input image is [drows][HoWo], the second tensor's rows start at row2.
//   DIL: dst2 = where the packet's 8 values go in the input gradient's zero-dilated image qd (ncv_stage_plan's placement; the group's first
//   image only, -1 otherwise)
template <int WPF> struct NcvWPlan { int src[WPF], dst[WPF], im[WPF], dst2[WPF]; };
template <int SW, int WPF, bool DIL>
__device__ __forceinline__ bool ncv_wg_plan(NcvWPlan<WPF>& pl, const NcvWGeom& q, int ximg, int drows, int row2, int tid, int nthreads, const NcvGeom& qd) {
  const int HoWo = q.Ho * q.Wo;
  const int xpk = (q.Cin * q.H * q.W) >> 3, dpk = (q.Cout * HoWo) >> 3, dpk2 = (q.Cout2 * HoWo) >> 3, per = xpk + dpk + dpk2;
  const int rc = q.W >> 3, rcd = q.Wo >> 3;
  const bool pf = q.IG * per <= WPF * nthreads;
#pragma unroll
  for (int k = 0; k < WPF; k++) {
    const int idx = tid + k * nthreads;
    const int im = idx / per, j = idx - im * per;
    pl.im[k] = (pf && im < q.IG) ? im : -1;
    pl.dst2[k] = -1;
    if (j < xpk) {
      const int b = j % rc, a = (j / rc) % q.H, c = j / (rc * q.H);
      pl.src[k] = im * q.Cin * q.H * q.W + j * 8;
      pl.dst[k] = im * ximg + (SW == 1 ? (c * q.Hs + q.ph + a) * q.Ws + NCV_OFFA + b * 8 : ((c * q.Hs + q.ph + a) * 2) * q.Ws + NCV_OFFA + b * 4);
    } else {
      const bool second = j >= xpk + dpk;
      const int e = j - xpk - (second ? dpk : 0);
      if (!second) {
        pl.src[k] = -(im * q.Cout * HoWo + e * 8) - 1;
        pl.dst[k] = q.IG * ximg + im * drows * HoWo + e * 8;
      } else {
        pl.src[k] = -(im * q.Cout2 * HoWo + e * 8) - 1 - (1 << 30);
        pl.dst[k] = q.IG * ximg + im * drows * HoWo + row2 * HoWo + e * 8;
      }
      if (DIL && im == 0) {
        const int b = e % rcd, a = (e / rcd) % q.Ho, c = e / (rcd * q.Ho) + (second ? qd.C1 : 0);
        pl.dst2[k] = (c * qd.Hs + qd.top + a * qd.dil) * qd.Ws + qd.left + b * 8 * qd.dil;
      }
    }
  }
  return pf;
}
template <int WPF>
__device__ __forceinline__ void ncv_wg_load(uint4 (&pre)[WPF], const NcvWPlan<WPF>& pl, const NcvWGeom& q, const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                            const bf16_t* __restrict__ dy2, int64_t nb, int ig) {
  const int HoWo = q.Ho * q.Wo;
  const bf16_t* xg = x + nb * q.Cin * q.H * q.W;
  const bf16_t* dg = dy + nb * q.Cout * HoWo;
  const bf16_t* dg2 = dy2 + nb * q.Cout2 * HoWo;
#pragma unroll
  for (int k = 0; k < WPF; k++)
    if (pl.im[k] >= 0 && pl.im[k] < ig) {
      const bf16_t* sp = pl.src[k] >= 0 ? xg + pl.src[k] : pl.src[k] >= -(1 << 30) ? dg + (-pl.src[k] - 1) : dg2 + (-pl.src[k] - 1 - (1 << 30));
      pre[k] = *reinterpret_cast<const uint4*>(sp);
    }
}
//   one 16-byte packet of an x row; stride 2: de-interleaved into the row's even / odd column planes (Ws apart)
template <int SW>
__device__ __forceinline__ void ncv_wg_stage_x(unsigned short* dst, const uint4 v, int Ws) {
  if (SW == 1) {
    *reinterpret_cast<uint4*>(dst) = v;
  } else {
    uint2 ev, od;
    ev.x = (v.x & 0xffffu) | (v.y << 16); ev.y = (v.z & 0xffffu) | (v.w << 16);
    od.x = (v.x >> 16) | (v.y & 0xffff0000u); od.y = (v.z >> 16) | (v.w & 0xffff0000u);
    *reinterpret_cast<uint2*>(dst) = ev;
    *reinterpret_cast<uint2*>(dst + Ws) = od;
  }
}
template <int SW, int WPF, bool DIL>
__device__ __forceinline__ void ncv_wg_store(unsigned short* xs, unsigned short* xd, const uint4 (&pre)[WPF], const NcvWPlan<WPF>& pl, int ig, int Ws, int dil) {
#pragma unroll
  for (int k = 0; k < WPF; k++) {
    if (pl.im[k] < 0 || pl.im[k] >= ig) continue;
    const uint4 v = pre[k];
    if (SW == 1 || pl.src[k] < 0) *reinterpret_cast<uint4*>(xs + pl.dst[k]) = v;      // stride 1 rows and dy packets: one 16-byte write
    else ncv_wg_stage_x<SW>(xs + pl.dst[k], v, Ws);
    if (DIL && pl.dst2[k] >= 0) ncv_scatter8(xd + pl.dst2[k], v, dil);
  }
}
//   per-lane row offset (bytes) of pair tile pt: pair = pt*16 + (lane & 15) -> (ci, r)
template <int SW, int NPT>
__device__ __forceinline__ void ncv_wg_pair_offsets(const NcvWGeom& q, int lane, int (&poff)[NPT]) {
  const int npairs = q.Cin * q.kh;
#pragma unroll
  for (int pt = 0; pt < NPT; pt++) {
    int pair = pt * 16 + (lane & 15);
    if (pair >= npairs) pair = 0;                                    // padded columns: computed, never written
    const int ci = pair / q.kh, r = pair - ci * q.kh;
    poff[pt] = (SW == 1 ? (ci * q.Hs + r) * q.Ws : (ci * q.Hs + r) * 2 * q.Ws) * 2;
  }
}
//   The k-loop over the `nchunks` 32-pixel chunks of a staged image group, this wave's share (chunk wid, wid + 4, ...: four waves).
//   W2: a second A fragment, rows [16, 32) of the staged gradient image (a sibling 1x1's output gradient that does not fit beside the
//   3x3's in the 16 MFMA rows), multiplied with the centre-tap fragment only: acc2[pair tile] holds its dW[co2][(ci, r)] at s = KW / 2
template <int KW, int PW, int SW, int NPT, bool W2>
__device__ __forceinline__ void ncv_wg_chunks(const unsigned short* xs, const unsigned short* ds, int drows, const NcvWGeom& q, int ximg, const int (&poff)[NPT],
                                              nv_f4 (&acc)[NPT][KW], nv_f4 (&acc2)[NPT], int nchunks, int wid, int lane) {
  const int HoWo = q.Ho * q.Wo;
  for (int ch = wid; ch < nchunks; ch += 4) {
    const int pg = ch * 32 + (lane >> 4) * 8;
    const int im = pg / HoWo, pp = pg - im * HoWo;
    const int ho = pp / q.Wo, wo0 = pp - ho * q.Wo;
    const nv_s8 a = *reinterpret_cast<const nv_s8*>(ds + (im * drows + (lane & 15)) * HoWo + pp);
    const nv_bf8 af = __builtin_bit_cast(nv_bf8, a);
    nv_bf8 af2 = af;
    if constexpr (W2) af2 = __builtin_bit_cast(nv_bf8, *reinterpret_cast<const nv_s8*>(ds + (im * drows + 16 + (lane & 15)) * HoWo + pp));
    // byte address of element column (wo0 + NCV_OFFA - 8) of this lane's group row: segment -1
    const char* xb = reinterpret_cast<const char*>(xs + im * ximg) +
                     (SW == 1 ? (ho * q.Ws + wo0 + NCV_OFFA - 8) * 2 : ((ho * 2) * 2 * q.Ws + wo0 + NCV_OFFA - 8) * 2);
#pragma unroll
    for (int pt = 0; pt < NPT; pt++) {
      const char* rowp = xb + poff[pt];
      if (SW == 1) {
        // 24 elements around the aligned window: [seg-1 | seg0 | seg+1]
        constexpr bool need_m = PW > 0, need_p = (KW - 1 - PW) > 0;
        unsigned int sg[13];
        const uint4 z = make_uint4(0, 0, 0, 0);
        const uint4 v0 = need_m ? *reinterpret_cast<const uint4*>(rowp) : z;
        const uint4 v1 = *reinterpret_cast<const uint4*>(rowp + 16);
        const uint4 v2 = need_p ? *reinterpret_cast<const uint4*>(rowp + 32) : z;
        sg[0] = v0.x; sg[1] = v0.y; sg[2] = v0.z; sg[3] = v0.w; sg[4] = v1.x; sg[5] = v1.y; sg[6] = v1.z; sg[7] = v1.w;
        sg[8] = v2.x; sg[9] = v2.y; sg[10] = v2.z; sg[11] = v2.w; sg[12] = 0;
#pragma unroll
        for (int s = 0; s < KW; s++) {
          const int o = 8 + s - PW;                              // compile-time element offset of the window
          const int dq = o >> 1;
          typedef unsigned int u4v __attribute__((ext_vector_type(4)));
          u4v f;
#pragma unroll
          for (int j = 0; j < 4; j++) f[j] = (o & 1) ? __builtin_amdgcn_alignbit(sg[dq + j + 1], sg[dq + j], 16) : sg[dq + j];
          acc[pt][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(nv_bf8, f), acc[pt][s], 0, 0, 0);
          if (W2 && s == KW / 2) acc2[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af2, __builtin_bit_cast(nv_bf8, f), acc2[pt], 0, 0, 0);
        }
      } else {
        // per parity plane: [seg-1 | seg0]; filter column s -> plane (s - PW) & 1, element offset 8 + ((s - PW) >> 1)
        unsigned int sg[2][9];
#pragma unroll
        for (int par = 0; par < 2; par++) {
          const uint4 v0 = *reinterpret_cast<const uint4*>(rowp + par * q.Ws * 2);
          const uint4 v1 = *reinterpret_cast<const uint4*>(rowp + par * q.Ws * 2 + 16);
          sg[par][0] = v0.x; sg[par][1] = v0.y; sg[par][2] = v0.z; sg[par][3] = v0.w;
          sg[par][4] = v1.x; sg[par][5] = v1.y; sg[par][6] = v1.z; sg[par][7] = v1.w; sg[par][8] = 0;
        }
#pragma unroll
        for (int s = 0; s < KW; s++) {
          const int t = s - PW, par = t & 1, half = (t - par) >> 1;   // compile time
          const int o = 8 + half, dq = o >> 1;
          typedef unsigned int u4v __attribute__((ext_vector_type(4)));
          u4v f;
#pragma unroll
          for (int j = 0; j < 4; j++) f[j] = (o & 1) ? __builtin_amdgcn_alignbit(sg[par][dq + j + 1], sg[par][dq + j], 16) : sg[par][dq + j];
          acc[pt][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(nv_bf8, f), acc[pt][s], 0, 0, 0);
          if (W2 && s == KW / 2) acc2[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af2, __builtin_bit_cast(nv_bf8, f), acc2[pt], 0, 0, 0);
        }
      }
    }
  }
}
//   The end of a workgroup: the four k-loop waves' sums through red ([4 waves][16][NPT * KW * 16]; W2: and red2, [4 waves][16][NPT * 16]),
//   added in wave order by all `nthreads` threads -> this workgroup's partial sums.  D: column = pair within the tile, rows = 4 output channels.
template <int KW, int NPT, bool W2>
__device__ __forceinline__ void ncv_wg_finish(float* red, float* red2, const nv_f4 (&acc)[NPT][KW], const nv_f4 (&acc2)[NPT], const NcvWGeom& q,
                                              float* __restrict__ partial, float* __restrict__ partial2, int tid, int nthreads, int wid, int lane) {
  constexpr int NCOLT = NPT * KW * 16;                               // accumulator columns per output channel
  if (wid < 4) {
#pragma unroll
    for (int pt = 0; pt < NPT; pt++)
#pragma unroll
      for (int s = 0; s < KW; s++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) red[(wid * 16 + (lane >> 4) * 4 + rr) * NCOLT + (pt * KW + s) * 16 + (lane & 15)] = acc[pt][s][rr];
    if constexpr (W2) {
#pragma unroll
      for (int pt = 0; pt < NPT; pt++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) red2[(wid * 16 + (lane >> 4) * 4 + rr) * (NPT * 16) + pt * 16 + (lane & 15)] = acc2[pt][rr];
    }
  }
  __syncthreads();
  const int O = q.Cout * q.ncol;
  for (int i = tid; i < O; i += nthreads) {
    const int co = i / q.ncol, cidx = i - co * q.ncol;              // cidx = (ci*kh + r)*kw + s
    const int pair = cidx / KW, s = cidx - pair * KW;
    const int col = ((pair >> 4) * KW + s) * 16 + (pair & 15);
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < 4; w++) a += red[(w * 16 + co) * NCOLT + col];
    partial[(int64_t)blockIdx.x * O + i] = a;
  }
  // the sibling 1x1's weight gradient [Cout2][Cin]: the centre tap of rows Cout ... (W2: of the second fragment's rows)
  const int O2 = q.Cout2 * q.Cin;
  for (int i = tid; i < O2; i += nthreads) {
    const int co2 = i / q.Cin, ci = i - co2 * q.Cin;
    const int pair = ci * q.kh + (q.kh >> 1), s = KW >> 1;
    float a = 0.f;
    if constexpr (W2) {
      const int col = (pair >> 4) * 16 + (pair & 15);
#pragma unroll
      for (int w = 0; w < 4; w++) a += red2[(w * 16 + co2) * (NPT * 16) + col];
    } else {
      const int col = ((pair >> 4) * KW + s) * 16 + (pair & 15);
#pragma unroll
      for (int w = 0; w < 4; w++) a += red[(w * 16 + q.Cout + co2) * NCOLT + col];
    }
    partial2[(int64_t)blockIdx.x * O2 + i] = a;
  }
}
template <int KW, int PW, int SW, int NPT>
__global__ __launch_bounds__(256) void ncv_wgrad2_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, float* __restrict__ partial, NcvWGeom q,
                                                         int images_per_block, const bf16_t* __restrict__ dy2, float* __restrict__ partial2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int HoWo = q.Ho * q.Wo;
  const int ximg = q.Cin * q.Hs * q.Ws * (SW == 2 ? 2 : 1);
  unsigned short* xs = reinterpret_cast<unsigned short*>(smem);
  unsigned short* ds = xs + q.IG * ximg;
  float* red = reinterpret_cast<float*>(ds + q.IG * 16 * HoWo);      // [4 waves][16][NPT * KW * 16]
  {
    const int tot = q.IG * (ximg + 16 * HoWo);
    for (int o = tid * 8; o < tot; o += 256 * 8) *reinterpret_cast<uint4*>(xs + o) = make_uint4(0, 0, 0, 0);
  }
  int poff[NPT];
  ncv_wg_pair_offsets<SW, NPT>(q, lane, poff);
  nv_f4 acc[NPT][KW], none[NPT];
#pragma unroll
  for (int pt = 0; pt < NPT; pt++)
#pragma unroll
    for (int s = 0; s < KW; s++) acc[pt][s] = nv_f4{0.f, 0.f, 0.f, 0.f};

  const int64_t n0 = (int64_t)blockIdx.x * images_per_block, n1 = min<int64_t>(n0 + images_per_block, q.N);
  const int chunks_per_img = HoWo >> 5;
  const int xpk = (q.Cin * q.H * q.W) >> 3, dpk = (q.Cout * HoWo) >> 3, dpk2 = (q.Cout2 * HoWo) >> 3;
  const int rc = q.W >> 3;
  uint4 pre[NCV_WPF];
  NcvWPlan<NCV_WPF> plan;
  const bool pf = ncv_wg_plan<SW, NCV_WPF, false>(plan, q, ximg, 16, q.Cout, tid, 256, NcvGeom{});
  auto x_dst = [&](unsigned short* xi, int j) {
    const int b = j % rc, a = (j / rc) % q.H, c = j / (rc * q.H);
    return xi + (SW == 1 ? (c * q.Hs + q.ph + a) * q.Ws + NCV_OFFA + b * 8 : ((c * q.Hs + q.ph + a) * 2) * q.Ws + NCV_OFFA + b * 4);
  };

  if (pf && n0 < n1) ncv_wg_load(pre, plan, q, x, dy, dy2, n0, (int)min<int64_t>(q.IG, n1 - n0));
  for (int64_t nb = n0; nb < n1; nb += q.IG) {
    const int ig = (int)min<int64_t>(q.IG, n1 - nb);
    __syncthreads();
#if defined(NCV_WSKIP) && (NCV_WSKIP & 4)   // diagnostic builds only: 1 = no k-loop, 4 = no staging (requests and LDS writes)
    if (nb < 0)
#endif
    if (pf) ncv_wg_store<SW, NCV_WPF, false>(xs, nullptr, pre, plan, ig, q.Ws, 1);
    else for (int im = 0; im < ig; im++) {
      const bf16_t* xp = x + (nb + im) * q.Cin * q.H * q.W;
      unsigned short* xi = xs + im * ximg;
      for (int i = tid; i < xpk; i += 256) ncv_wg_stage_x<SW>(x_dst(xi, i), *reinterpret_cast<const uint4*>(xp + i * 8), q.Ws);
      const bf16_t* dp = dy + (nb + im) * q.Cout * HoWo;
      unsigned short* di = ds + im * 16 * HoWo;
      for (int i = tid; i < dpk; i += 256) *reinterpret_cast<uint4*>(di + i * 8) = *reinterpret_cast<const uint4*>(dp + i * 8);
      const bf16_t* dp2 = dy2 + (nb + im) * q.Cout2 * HoWo;
      for (int i = tid; i < dpk2; i += 256) *reinterpret_cast<uint4*>(di + q.Cout * HoWo + i * 8) = *reinterpret_cast<const uint4*>(dp2 + i * 8);
    }
    __syncthreads();
#if defined(NCV_WSKIP) && (NCV_WSKIP & 4)
    if (nb < 0)
#endif
    if (pf && nb + q.IG < n1) ncv_wg_load(pre, plan, q, x, dy, dy2, nb + q.IG, (int)min<int64_t>(q.IG, n1 - nb - q.IG));      // in flight during the MFMAs
#if defined(NCV_WSKIP) && (NCV_WSKIP & 1)
    if (nb < 0)
#endif
    ncv_wg_chunks<KW, PW, SW, NPT, false>(xs, ds, 16, q, ximg, poff, acc, none, ig * chunks_per_img, wid, lane);
  }
  ncv_wg_finish<KW, NPT, false>(red, nullptr, acc, none, q, partial, partial2, tid, 256, wid, lane);
}

// A block's whole backward over its entry pair in ONE launch: dx = round(dgrad3x3(dy, w) + dgrad1x1(dy2, w2)) [+ addend], dW of the 3x3 and
// dW of the 1x1 (stride 2, 3x3 pad 1 + 1x1 pad 0 of the same x; the geometries narrow_conv_dgrad_pair and ncv_wgrad2_kernel<3, 1, 2, .> take).
// The paired input gradient and the weight gradients read the same two output gradients: per round of IG images a workgroup requests x
// and both gradients ONCE (the register prefetch of ncv_wgrad2_kernel) and writes the gradients into LDS twice from the same registers -
// as the plain [drows][Ho*Wo] image the weight gradient's k-loop reads and (the round's first image; the others are copied over from the
// plain image when their turn comes) as the zero-dilated, padded image the parity super-tiles of ncv_fwd2_kernel<.., PAR> read.  Then
// ncv_wg_chunks and ncv_super_tiles run as in the kernels they come from: same MFMA chains over the same values, same partition of the
// images over workgroups as the weight gradient's own launch where two workgroups fit a CU, so dx and (then) dW keep their bits.
// `red` lies over the dilated image: it is only used after the last round.
// 256 threads run the k-loop and then the super-tiles of a staged round.  (The form with 512 threads - waves 0-3 in the k-loop while waves 4-7
// run the super-tiles - needs four waves per SIMD for two workgroups per CU, 128 registers: it spilled 100 - 215 of them in every
// instantiation, the k-loop's side alone holds 127 and the super-tiles' 153.  Not kept.)
// A wave's super-tiles all start on rows of one parity (four waves, super-tile st = wid + 4 k), so it keeps the weight fragments of that
// parity class only: NK / 2 of them.
//   W2: see ncv_wg_chunks (6 -> 16 + 6 -> 16: the 1x1's 16 rows are a second A fragment).  WPF: packets per thread of the prefetch.
template <int NK, bool ADD, int NPT, bool W2, int WPF>
__global__ __launch_bounds__(256, 2) void ncv_bwd_pair_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ dy2, const bf16_t* __restrict__ x,
                                                               const nv_bf8* __restrict__ wpk, bf16_t* dx, const bf16_t* add, float* __restrict__ partial,
                                                               float* __restrict__ partial2, NcvWGeom q, NcvGeom qd, int images_per_block) {
  constexpr int KW = 3, PW = 1, SW = 2, PH0 = 7, NS = 2;
  constexpr int NCOLT = NPT * KW * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int HoWo = q.Ho * q.Wo;
  const int ximg = q.Cin * q.Hs * q.Ws * 2;
  const int drows = W2 ? 32 : 16;
  unsigned short* xs = reinterpret_cast<unsigned short*>(smem);      // [IG][ximg]
  unsigned short* ds = xs + q.IG * ximg;                             // [IG][drows][HoWo]
  unsigned short* xd = ds + q.IG * drows * HoWo;                     // the dilated image of ONE input image [qd.C][qd.Hs][qd.Ws]
  float* red = reinterpret_cast<float*>(xd);
  float* red2 = red + 4 * 16 * NCOLT;
  const int64_t n0 = (int64_t)blockIdx.x * images_per_block, n1 = min<int64_t>(n0 + images_per_block, q.N);
  uint4 pre[WPF];
  NcvWPlan<WPF> plan;
  ncv_wg_plan<SW, WPF, true>(plan, q, ximg, drows, W2 ? 16 : q.Cout, tid, 256, qd);      // (the launcher takes only groups that fit the prefetch)
  if (n0 < n1) ncv_wg_load(pre, plan, q, x, dy, dy2, n0, (int)min<int64_t>(q.IG, n1 - n0));
  nv_bf8 wfr[NK / 2];
  int koff[NK / 2];
  ncv_frag_setup_class<NK>(qd, wpk, lane, (wid + qd.top) & 1, wfr, koff);
  {
    const int tot = q.IG * (ximg + drows * HoWo) + qd.C * qd.Hs * qd.Ws;
    for (int o = tid * 8; o < tot; o += 256 * 8) *reinterpret_cast<uint4*>(xs + o) = make_uint4(0, 0, 0, 0);
  }
  int poff[NPT];
  ncv_wg_pair_offsets<SW, NPT>(q, lane, poff);
  nv_f4 acc[NPT][KW], acc2[NPT];
#pragma unroll
  for (int pt = 0; pt < NPT; pt++) {
    acc2[pt] = nv_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KW; s++) acc[pt][s] = nv_f4{0.f, 0.f, 0.f, 0.f};
  }
  // the input gradient's lane constants (as ncv_fwd2_kernel, parity tiles)
  const int co = lane & 7;
  const int ncg = qd.Wo / 8;
  const int a_tr = (lane & 15) / ncg, a_cg = (lane & 15) - a_tr * ncg;
  const int a_off = (2 * a_tr * qd.sh * qd.Ws + a_cg * 8 + (qd.wx - PH0)) * 2;
  const int HoWo_d = qd.Ho * qd.Wo;
  NcvStatAcc none{nv_f4{0.f, 0.f, 0.f, 0.f}, nv_f4{0.f, 0.f, 0.f, 0.f}, 0};
  const int chunks_per_img = HoWo >> 5;
  for (int64_t nb = n0; nb < n1; nb += q.IG) {
    const int ig = (int)min<int64_t>(q.IG, n1 - nb);
    __syncthreads();                                     // zero fill / the previous round's reads are done
    ncv_wg_store<SW, WPF, true>(xs, xd, pre, plan, ig, q.Ws, qd.dil);
    __syncthreads();
    if (nb + q.IG < n1) ncv_wg_load(pre, plan, q, x, dy, dy2, nb + q.IG, (int)min<int64_t>(q.IG, n1 - nb - q.IG));      // in flight during the MFMAs
    ncv_wg_chunks<KW, PW, SW, NPT, W2>(xs, ds, drows, q, ximg, poff, acc, acc2, ig * chunks_per_img, wid, lane);
    for (int im = 0; im < ig; im++) {
      if (im > 0) {
        // images 1 .. IG-1 of a round reach the dilated image from the plain one: ncv_stage_plan's packets, read from LDS
        __syncthreads();                                 // the super-tiles of image im - 1 are done
        const NcvPlanT<2> dplan = ncv_stage_plan<2>(qd, tid, 256);
        const bf16_t* pa = reinterpret_cast<const bf16_t*>(ds + im * drows * HoWo);
        NcvPreT<2> t;
        ncv_stage_load(t, dplan, pa, pa + (W2 ? 16 : q.Cout) * HoWo);
        ncv_stage_store(xd, t, dplan, qd.dil);
        __syncthreads();
      }
      const int64_t n = nb + im;
      bf16_t* yc = dx + (n * qd.CO + co) * HoWo_d;
      const bf16_t* ap = ADD ? add + (n * qd.CO + co) * HoWo_d : nullptr;
      ncv_super_tiles<NK, 1, PH0, NS, ADD, false, true, false, NK / 2, (NK >= 8 ? 2 : 0)>(reinterpret_cast<const char*>(xd), qd, wfr, koff, a_off, 0.f, co, yc, ap, none, nullptr, 0, lane, wid, 4);
    }
  }
  __syncthreads();                                       // the last super-tiles are done: red lies over their image
  ncv_wg_finish<KW, NPT, W2>(red, red2, acc, acc2, q, partial, partial2, tid, 256, wid, lane);
}

// (the reduction of the per-block partial sums lives in wgrad_reduce.h: it runs batched with the other layers' reductions)

// ---- host ------------------------------------------------------------------------------------------------
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

static bool ncv_common(const ConvGeom& g, int dtype) {
  if (dtype != kBF16) return false;
  if (g.groups != 1 || g.transposed || g.dh != 1 || g.dw != 1) return false;
  if (g.Cin > 16 || g.Cout > 16 || g.N < 1) return false;
  if (g.sh != g.sw || g.sh < 1 || g.sh > 2) return false;
  if (g.kw > 8 || g.ph > g.kh - 1 || g.pw > g.kw - 1 || g.pw > 8) return false;
  return true;
}

// g a 3x3 pad 1 and g1 a 1x1 pad 0 convolution of one input: same stride, input map, output map, channels in and batch (the two branches of
// lamp's residual block on its input, cnn.scala:16-20).  Every pair launch below starts here and adds only what is its own.
static bool ncv_pair_shapes(const ConvGeom& g, const ConvGeom& g1) {
  if (g.kh != 3 || g.kw != 3 || g.ph != 1 || g.pw != 1 || g1.kh != 1 || g1.kw != 1 || g1.ph != 0 || g1.pw != 0) return false;
  if (g.sh != g1.sh || g.sw != g1.sw || g.Ho != g1.Ho || g.Wo != g1.Wo || g.H != g1.H || g.W != g1.W || g.Cin != g1.Cin || g.N != g1.N) return false;
  return g.groups == 1 && g1.groups == 1 && g.dh == 1 && g.dw == 1 && g1.dh == 1 && g1.dw == 1;
}
// the work and traffic a sibling 1x1 of cout2 output channels adds to g's launch (its input is the one already counted)
static double ncv_sibling_flops(const ConvGeom& g, int cout2) { return 2.0 * (double)g.N * cout2 * (double)g.Ho * g.Wo * (double)g.Cin; }
static double ncv_sibling_bytes(const ConvGeom& g, int cout2) { return ((double)g.N * cout2 * g.Ho * g.Wo + (double)cout2 * g.Cin) * 2.0; }

constexpr size_t NCV_LDS_BUDGET = 150 * 1024;      // LDS the workgroups of a CU share (of its 160 KiB)
constexpr size_t NCV_LDS_DEFAULT = 64 * 1024;      // dynamic LDS a kernel may ask for without allow_big_lds
constexpr int NCV_PER_CU_MAX = 4;                  // most workgroups per CU (A/B on one device: 4 beats 8 and 2)
// workgroups per CU the LDS image allows, and of those the ones that are really co-resident (registers)
static int ncv_lds_per_cu(size_t lds) { return (int)std::max<size_t>(1, std::min<size_t>(NCV_PER_CU_MAX, NCV_LDS_BUDGET / std::max<size_t>(lds, 1))); }
static int ncv_per_cu(const void* kfn, int threads, size_t lds) { return std::min(ncv_lds_per_cu(lds), kernel_occupancy(kfn, threads, lds)); }
// every convolution launch of this file: more than the default LDS has to be asked for (once per kernel and device)
static void ncv_launch(const void* kfn, int blocks, int threads, size_t lds, void** args, hipStream_t st) {
  if (lds > NCV_LDS_DEFAULT) allow_big_lds(kfn);
  HIP_CHECK(hipLaunchKernel(kfn, dim3(blocks), dim3(threads), args, lds, st));
  LAMP_LAUNCH_CHECK();
}
// Per-slice batch-norm statistics of a launch's one or two outputs ([parts][C][3] f32, written by the kernel's epilogue): allocated where
// the launch takes them, handed to the consuming batch norm behind it.
struct NcvStats {
  Hold t, t2;
  int parts;
  NcvStats(bool on, int parts_, int64_t C, int64_t C2, int device) : parts(parts_) {
    if (!on) return;
    t = Hold(new_tensor({parts * C * 3}, kF32, device));
    if (C2 > 0) t2 = Hold(new_tensor({parts * C2 * 3}, kF32, device));
  }
  float* ptr() { return t.get() ? t->ptr<float>() : nullptr; }
  float* ptr2() { return t2.get() ? t2->ptr<float>() : nullptr; }
  void publish(const Tensor* y, uint64_t producer, const Tensor* y2) {
    if (t.get()) conv_stats_publish(y, t.get(), parts, producer);
    if (t2.get()) conv_stats_publish(y2, t2.get(), parts);
  }
};

// ---- packed weight-fragment images, one per (filter [and sibling], geometry, direction, stream): cached and re-packed in place by the
// optimiser's hook (core/pack_cache.h).  An entry keeps no data pointers: the hook resolves both filters among the parameters it is handed.
static PackCache g_ncv_packs;
constexpr int64_t NCV_PACK_ELEMS = (int64_t)NCV_NKMAX * 64 * 8;
// the key's geometry tag
enum { NCV_T_COUT, NCV_T_CIN, NCV_T_KH, NCV_T_KW, NCV_T_DGRAD, NCV_T_NS, NCV_T_SW, NCV_T_COUT2 };    // NS: ns + 16 * nke

void narrow_pack_launch(const NcvPackMany& a, int cnt, hipStream_t st) {
  hipLaunchKernelGGL(ncv_pack_kernel, dim3((NCV_NKMAX * 64 + 255) / 256, (unsigned)cnt), dim3(256), 0, st, a);
  LAMP_LAUNCH_CHECK();
}

// returns a +1 handle on the fragment image of `w` (and its sibling w2) for this direction
static Tensor* ncv_packed_weights(const Tensor* w, const NcvW& wq, hipStream_t st, const Tensor* w2 = nullptr) {
  const bool cacheable = PackCache::cacheable(w, w2);
  const PackKey key{w->st->uid, w->offset, {wq.Cout, wq.Cin, wq.kh, wq.kw, wq.dgrad, wq.ns + 16 * wq.nke, wq.sw, w2 ? wq.Cout2 : 0}, st,
                    w2 ? w2->st->uid : 0, w2 ? w2->offset : 0};
  const uint64_t ver = PackCache::version_of(w), ver2 = PackCache::version_of(w2);
  if (cacheable) if (Tensor* hit = g_ncv_packs.find(key, ver, ver2)) return hit;
  int64_t ps[1] = {NCV_PACK_ELEMS};
  Hold wp(new_tensor(ps, 1, kBF16, w->device()));
  NcvPackMany a;
  a.w[0] = wq; a.dst[0] = reinterpret_cast<nv_bf8*>(wp->ptr<bf16_t>());
  narrow_pack_launch(a, 1, st);
  if (cacheable) g_ncv_packs.insert(key, ver, ver2, wp.get());
  return wp.take();
}

// The narrow half of the optimisers' hook (called by igemm_repack_cached): every cached fragment image of these parameters on this stream
// is packed again IN PLACE (a captured HIP graph keeps the address), NCV_PACK_MAX per launch.
// `fill` (optional): instead of launching, hand the LAST batch of at most NCV_PACK_MAX images to the caller (*fill, *fill_cnt), which packs them
// in the launch that packs the implicit-GEMM images; earlier full batches are still launched here
void narrow_repack_cached(lamp_tensor* const* params, int n, hipStream_t st, NcvPackMany* fill, int* fill_cnt) {
  if (fill_cnt) *fill_cnt = 0;
  // the narrow filters among the parameters just written: an image is packed again ONLY from tensors the caller holds right now (ADVICE r5:
  // the entry used to keep raw data pointers of both filters of a pair and read the absent one's after its storage could be gone)
  std::vector<const Tensor*> cand;
  for (int i = 0; i < n; i++) {
    const Tensor* w = params[i];
    if (!w || !w->is_device() || w->dtype != kBF16 || w->ndim != 4 || !w->st->owned || !w->is_contiguous()) continue;
    if (w->sizes[0] > 16 || w->sizes[1] > 16) continue;
    cand.push_back(w);
  }
  if (cand.empty()) return;
  auto find = [&](uint64_t uid, int64_t offset, int co, int ci, int kh, int kw) -> const Tensor* {
    for (const Tensor* w : cand)
      if (w->st->uid == uid && w->offset == offset && (int)w->sizes[0] == co && (int)w->sizes[1] == ci && (int)w->sizes[2] == kh && (int)w->sizes[3] == kw)
        return w;
    return nullptr;
  };
  NcvPackMany a;
  int cnt = 0;
  g_ncv_packs.walk(st,
      [&](const PackKey& k, PackEntry& v) {
        const int* t = k.tag.data();
        const Tensor* w1 = find(k.uid, k.offset, t[NCV_T_COUT], t[NCV_T_CIN], t[NCV_T_KH], t[NCV_T_KW]);
        const Tensor* w2 = t[NCV_T_COUT2] > 0 ? find(k.uid2, k.offset2, t[NCV_T_COUT2], t[NCV_T_CIN], 1, 1) : nullptr;
        if (!w1 && !w2) return true;                                 // none of this call's parameters
        // a pair image with only ONE of its filters among the parameters (the other was a temporary, or its layer was rebuilt): it cannot be
        // brought up to date here.  Drop it - the next convolution packs a fresh image from the tensors it is given - unless a captured graph
        // reads this address; that entry stays, stale by its versions, exactly as when a parameter is written outside the optimiser.
        if (!w1 || (t[NCV_T_COUT2] > 0 && !w2)) return false;
        if (cnt == NCV_PACK_MAX) { narrow_pack_launch(a, cnt, st); cnt = 0; }
        a.w[cnt] = NcvW{w1->ptr<bf16_t>(), t[NCV_T_COUT], t[NCV_T_CIN], t[NCV_T_KH], t[NCV_T_KW], t[NCV_T_DGRAD], t[NCV_T_NS] & 15, t[NCV_T_SW],
                        w2 ? w2->ptr<bf16_t>() : nullptr, t[NCV_T_COUT2], t[NCV_T_NS] >> 4};
        a.dst[cnt] = static_cast<nv_bf8*>(v.packed->raw());
        g_ncv_packs.touch(v, PackCache::version_of(w1), PackCache::version_of(w2));
        cnt++;
        return true;
      },
      [&] {
        if (cnt == 0) return;
        if (fill) { *fill = a; *fill_cnt = cnt; }
        else narrow_pack_launch(a, cnt, st);
      });
}

// sibling (fprop, optional): a 1x1 convolution of the same input, same stride and output map, whose Cout2 channels fit beside w's in the
// MFMA's 16 columns: both outputs from one launch of the aligned kernel (false, nothing launched, when that kernel does not take the pair)
struct NcvSibling { const Tensor* w; const Tensor* bias; Tensor* out; };
// second (dgrad, optional): the output gradient and the filter of a sibling 1x1 convolution of the same input (same stride and output map): both
// input gradients, summed in f32, from one launch of the aligned kernel (false, nothing launched, when that kernel does not take the pair)
struct NcvSecondGrad { const Tensor* dy; const Tensor* w; };
// What a narrow forward / input-gradient launch looks like for a geometry: the LDS image, the kernel form and its template arguments.
// sib / second: a sibling 1x1's cout2 output channels (fprop) or its output gradient as extra image channels (dgrad) take part.
// own_stage: the launch is not ncv_fwd_kernel's / ncv_fwd2_kernel's own but that of a kernel which always stages this image through a register
// prefetch of its own (ncv_chain_kernel, ncv_bwd_pair_kernel): q.pf is set, and whether the image fits THAT prefetch is the launcher's check.
// false: the narrow kernels do not take it.  true: the launch is taken, with exactly these parameters.
struct NcvLaunchPlan {
  NcvGeom q;
  bool aligned;          // the aligned-window kernel (ncv_fwd2_kernel); else ncv_fwd_kernel
  int ncg, ph0;          // aligned: column groups per output row, window phase
  int NK;                // the kernel's k-steps (its template argument)
  int nke;               // > 0: parity tiles, nke k-steps per class
  int NS;                // output phases per MFMA
  size_t lds;
  int threads;
};
static bool ncv_plan(const ConvGeom& g, int dtype, bool dgrad, bool sib, bool second, int cout2, bool own_stage, NcvLaunchPlan& lp) {
  if (!ncv_common(g, dtype)) return false;
  if (sib && (dgrad || g.Cout + cout2 > 16)) return false;
  if (second && (!dgrad || sib || cout2 > 16)) return false;
  NcvGeom& q = lp.q;
  q.N = (int)g.N; q.kh = g.kh; q.pf = 0; q.kh_inv = 65536 / g.kh + 1;
  if (!dgrad) {
    if (g.W % 8 != 0) return false;
    q.C = (int)g.Cin; q.C1 = q.C; q.CO = (int)g.Cout + cout2; q.H = (int)g.H; q.W = (int)g.W; q.dil = 1;
    q.top = g.ph; q.left = NCV_LEFT;
    q.Ho = (int)g.Ho; q.Wo = (int)g.Wo; q.sh = g.sh; q.sw = g.sw; q.wx = NCV_LEFT - g.pw;
    q.Hs = std::max((int)g.H + 2 * g.ph, (q.Ho - 1) * g.sh + g.kh);
    q.Ws = round_up(std::max(NCV_LEFT + (int)g.W, (q.Wo - 1) * g.sw + q.wx + 8), 8);
  } else {
    // dx = stride-1 correlation of the dilated dy image with the mirrored filter, padding k-1-p
    const int pt = g.kh - 1 - g.ph, pl = g.kw - 1 - g.pw;
    q.C1 = (int)g.Cout; q.C = q.C1 + (second ? cout2 : 0); q.CO = (int)g.Cin; q.H = (int)g.Ho; q.W = (int)g.Wo; q.dil = g.sh;
    if (q.dil == 1 && q.W % 8 != 0) return false;
    q.top = pt; q.left = NCV_LEFT;
    q.Ho = (int)g.H; q.Wo = (int)g.W; q.sh = 1; q.sw = 1; q.wx = NCV_LEFT - pl;
    q.Hs = std::max(pt + ((int)g.Ho - 1) * g.sh + 1, (int)g.H + g.kh - 1);
    q.Ws = round_up(std::max(NCV_LEFT + ((int)g.Wo - 1) * g.sw + 1, (int)g.W - 1 + q.wx + 8), 8);
  }
  if ((q.Ho * q.Wo) % 4 != 0) return false;
  // aligned-window kernel: Wo a multiple of the P = 8/stride phases, 16 pixels = TR full-phase rows
  const int P = 8 / q.sw, ph0 = q.wx & 7;
  bool aligned = q.Wo % P == 0 && (ph0 == 0 || ph0 == 6 || ph0 == 7);
  int ncg = aligned ? q.Wo / P : 0;
  if (aligned && !(ncg == 2 || ncg == 4 || ncg == 8 || ncg == 16)) aligned = false;
  if (aligned && q.Ho % (16 / ncg) != 0) aligned = false;
  if (aligned) q.Ws = round_up(std::max(q.Ws, q.Wo * q.sw + (q.wx - ph0) + 16), 8);
  if ((sib || second) && !aligned) return false;
  const int pairs = q.C1 * q.kh + (q.C - q.C1);
  const int nk_real = (pairs + 3) / 4;
  static const int nk_opts[] = {1, 2, 4, 5, 6, 8, 12, 16};
  int NK = 0;
  for (int o : nk_opts) if (o >= nk_real) { NK = o; break; }
  if (!NK) return false;
  // round 6: the input gradient of a stride-2 pair runs its super-tiles by row parity over K pairs packed by the parity of the filter row
  // (ncv_fwd2_kernel<.., PAR>; LAMP_NCV_DGRAD_PARITY=0: the plain form): half the k-steps per super-tile
  int nke = 0;
  const bool par_on = sw().ncv_dgrad_parity;
  if (par_on && aligned && dgrad && second && q.dil == 2 && g.kh == 3 && NK > 5) {
    const int nk2 = NK <= 6 ? 6 : NK <= 8 ? 8 : 16;
    const int need_e = (q.C1 * 2 + 3) / 4, need_o = (q.C + 3) / 4;      // pairs (c, r even) / (c, 1) and the second source's centre rows
    if (need_e <= nk2 / 2 && need_o <= nk2 / 2 && q.Ho % (2 * (16 / ncg)) == 0) nke = nk2 / 2;
  }
  // The row pitch of the LDS image decides the bank conflicts of the fragment reads: the 16 lanes of a quarter-wave read 16 bytes each at
  // (row a_tr, column group a_cg) = a_tr * RS * sh * pitch + a_cg * 16 (RS = 2 with the parity tiles), TR x ncg = 16 of them; they are 16
  // DIFFERENT 16-byte bank slots iff (RS * sh * Ws / 8) mod 16 is an odd multiple of ncg.  (Round 6: the res2 pair's image had a 64-byte pitch -
  // rows a_tr and a_tr + 4 on the same banks, and with the parity tiles' two-apart rows a_tr and a_tr + 2: the halved k-loop read twice as slowly
  // and the launch gained nothing.)  The pitch is widened by at most 15 x 16 bytes to the next such value.
  if (aligned) {
    const int rs = (nke > 0 ? 2 : 1) * q.sh;
    for (int k = 0; k < 16; k++) {
      const int step = (rs * ((q.Ws >> 3) + k)) & 15;
      if (step % ncg == 0 && ((step / ncg) & 1) == 1 && (size_t)q.C * q.Hs * (q.Ws + 8 * k) * 2 <= NCV_LDS_DEFAULT) { q.Ws += 8 * k; break; }
    }
  }
  const size_t lds = (size_t)q.C * q.Hs * q.Ws * 2;
  if (lds > NCV_LDS_DEFAULT) return false;
  lp.aligned = aligned; lp.ncg = ncg; lp.ph0 = ph0; lp.nke = nke; lp.lds = lds;
  if (!aligned) {
    // ncv_fwd_kernel: one output phase per MFMA, 1, 2, 4, 5, 8 or 12 k-steps
    if (NK > 12) return false;
    lp.NK = NK == 6 ? 8 : NK; lp.NS = 1; lp.threads = 256;
    return true;
  }
  // two output phases per MFMA where the columns allow it (see NcvW)
  lp.NS = (q.CO <= 8 && g.kw + q.sw <= 8) ? 2 : 1;
  const int nsuper = q.Ho / (16 / ncg);
  lp.threads = 64 * std::min(4, nsuper);
  q.pf = (own_stage || (q.W % 8 == 0 && (int64_t)q.C * q.H * q.W <= (int64_t)NCV_PF * lp.threads * 8)) ? 1 : 0;
  if (second && !q.pf) return false;                     // (two sources are staged through the register prefetch only)
  // ncv_fwd2_kernel: 2, 4, 5 or 12 k-steps; 6, 8 and 16 for the pairs' input gradients only.  (Parity tiles: the kernel's k-steps are the packed
  // image's two halves - 2 nke, whatever the plain form would have taken: 12 k-steps of pairs are 16 there)
  if (NK > 12 && !second) return false;
  lp.NK = nke > 0 ? 2 * nke : NK <= 2 ? 2 : (NK <= 4 ? 4 : (NK <= 5 ? 5 : (NK <= 6 && second ? 6 : (NK <= 8 && second ? 8 : (NK <= 12 ? 12 : 16)))));
  return true;
}
// the packed image's description for a planned launch (second: the sibling's / the second gradient's filter)
static NcvW ncv_weights_of(const Tensor* w, const ConvGeom& g, bool dgrad, const NcvLaunchPlan& lp, const Tensor* wsecond, int cout2) {
  return NcvW{w->ptr<bf16_t>(), (int)g.Cout, (int)g.Cin, g.kh, g.kw, dgrad ? 1 : 0, lp.NS, lp.q.sw, wsecond ? wsecond->ptr<bf16_t>() : (const bf16_t*)nullptr, cout2, lp.nke};
}
// the fragment image of a planned launch's filter(s), as the kernels take it (the handle keeps it alive)
static const nv_bf8* ncv_fragments(const Hold& wpk) { return reinterpret_cast<const nv_bf8*>(static_cast<const Tensor*>(wpk.get())->ptr<bf16_t>()); }
// Per-image batch-norm statistics of the output(s) from a forward launch's epilogue (LAMP_CONV_BN_STATS=0 turns the hand-off off,
// LAMP_NCV_BN_STATS=0 the narrow kernels' alone, A/B).  A filter whose output's statistics nobody took last time - the stem of Cnn.resnet feeds
// res1's convolutions directly - stops paying for them; a pair's are always taken.
static bool ncv_takes_stats(const NcvGeom& q, bool dgrad, bool addend, bool sib, const Tensor* w) {
  return sw().conv_bn_stats && sw().ncv_bn_stats && !dgrad && !addend && q.N >= 2 && (int64_t)q.Ho * q.Wo >= 64 && (sib || conv_stats_wanted(w->st->uid));
}
// the instantiation of ncv_fwd_kernel for the plan's k-steps
static const void* ncv_fwd_fn(int NK) {
  switch (NK) {
    case 1: return (const void*)ncv_fwd_kernel<1>;
    case 2: return (const void*)ncv_fwd_kernel<2>;
    case 4: return (const void*)ncv_fwd_kernel<4>;
    case 5: return (const void*)ncv_fwd_kernel<5>;
    case 8: return (const void*)ncv_fwd_kernel<8>;
    default: return (const void*)ncv_fwd_kernel<12>;
  }
}
// the instantiation of ncv_fwd2_kernel for (k-steps, phases per MFMA, window phase, stride, addend, statistics, parity tiles)
static const void* ncv_fwd2_fn(int NK2, int NS, int ph0, int sw, bool with_add, bool with_stats, int nke) {
  const void* kfn = nullptr;
#define NCV_F2(NKv, SWv, PHv, ADDv, STv) kfn = NS == 2 ? (const void*)ncv_fwd2_kernel<NKv, SWv, PHv, 2, ADDv, STv> : (const void*)ncv_fwd2_kernel<NKv, SWv, PHv, 1, ADDv, STv>
#define NCV_F2_PH(NKv, SWv, ADDv, STv) do { if (ph0 == 0) NCV_F2(NKv, SWv, 0, ADDv, STv); else if (ph0 == 6) NCV_F2(NKv, SWv, 6, ADDv, STv); else NCV_F2(NKv, SWv, 7, ADDv, STv); } while (0)
#define NCV_F2_SW(NKv) do { if (with_stats) { if (sw == 1) NCV_F2_PH(NKv, 1, false, true); else NCV_F2_PH(NKv, 2, false, true); }                \
                            else if (sw == 1) { if (with_add) NCV_F2_PH(NKv, 1, true, false); else NCV_F2_PH(NKv, 1, false, false); }                \
                            else NCV_F2_PH(NKv, 2, false, false); } while (0)
    // (6, 8 and 16 k-steps: the pairs' input gradients only - stride-1 correlations without statistics)
#define NCV_F2P(NKv, PHv, ADDv) kfn = NS == 2 ? (const void*)ncv_fwd2_kernel<NKv, 1, PHv, 2, ADDv, false, true> : (const void*)ncv_fwd2_kernel<NKv, 1, PHv, 1, ADDv, false, true>
#define NCV_F2P_PH(NKv, ADDv) do { if (ph0 == 0) NCV_F2P(NKv, 0, ADDv); else if (ph0 == 6) NCV_F2P(NKv, 6, ADDv); else NCV_F2P(NKv, 7, ADDv); } while (0)
#define NCV_F2_PAIR(NKv) do { if (nke > 0) { if (with_add) NCV_F2P_PH(NKv, true); else NCV_F2P_PH(NKv, false); }                                   \
                              else if (with_add) NCV_F2_PH(NKv, 1, true, false); else NCV_F2_PH(NKv, 1, false, false); } while (0)
    switch (NK2) {
      case 2: NCV_F2_SW(2); break;
      case 4: NCV_F2_SW(4); break;
      case 5: NCV_F2_SW(5); break;
      case 6: NCV_F2_PAIR(6); break;
      case 8: NCV_F2_PAIR(8); break;
      case 16: NCV_F2_PAIR(16); break;
      default: NCV_F2_SW(12); break;
    }
#undef NCV_F2_PAIR
#undef NCV_F2P_PH
#undef NCV_F2P
#undef NCV_F2_SW
#undef NCV_F2_PH
#undef NCV_F2
  return kfn;
}
// persistent grids: at most as many workgroups as are co-resident, each walks a strided range of images
static int ncv_grid(int64_t N, int per_cu) { return (int)std::min<int64_t>(N, (int64_t)num_cus() * per_cu); }
// a planned launch of ncv_fwd_kernel
static void ncv_run_generic(const NcvLaunchPlan& lp, const Tensor* in, const nv_bf8* wpk, const Tensor* bias, Tensor* out, hipStream_t st) {
  const bf16_t* srcp = in->ptr<bf16_t>();
  const bf16_t* bp = bias ? bias->ptr<bf16_t>() : (const bf16_t*)nullptr;
  bf16_t* dstp = out->ptr<bf16_t>();
  void* args[] = {(void*)&srcp, (void*)&wpk, (void*)&bp, (void*)&dstp, (void*)&lp.q};
  ncv_launch(ncv_fwd_fn(lp.NK), ncv_grid(lp.q.N, ncv_lds_per_cu(lp.lds)), 256, lp.lds, args, st);
}
// a planned launch of ncv_fwd2_kernel
static void ncv_run_aligned(const NcvLaunchPlan& lp, bool dgrad, const Tensor* in, const Tensor* w, const nv_bf8* wpk, const Tensor* bias, Tensor* out,
                            hipStream_t st, const Tensor* addend, bool* addend_fused, const NcvSibling* sib, const NcvSecondGrad* second) {
  const NcvGeom& q = lp.q;
  const bool with_add = addend != nullptr && q.sw == 1;
  const bool with_stats = ncv_takes_stats(q, dgrad, addend != nullptr, sib != nullptr, w);
  const void* kfn = ncv_fwd2_fn(lp.NK, lp.NS, lp.ph0, q.sw, with_add, with_stats, lp.nke);
  const int blocks = ncv_grid(q.N, ncv_per_cu(kfn, lp.threads, lp.lds));
  // one triple per workgroup where every workgroup walks the same number of images (equal counts), else one per image
  int stats_per_wg = q.N % blocks == 0 ? 1 : 0;
  int co_a = q.CO - (sib ? (int)sib->w->sizes[0] : 0);   // the sibling's output channels are the columns behind w's
  NcvStats stats(with_stats, stats_per_wg ? blocks : q.N, co_a, q.CO - co_a, in->device());
  const bf16_t* srcp = in->ptr<bf16_t>();
  const bf16_t* src2p = second ? second->dy->ptr<bf16_t>() : (const bf16_t*)nullptr;
  const bf16_t* bp = bias ? bias->ptr<bf16_t>() : (const bf16_t*)nullptr;
  bf16_t* dstp = out->ptr<bf16_t>();
  const bf16_t* addp = with_add ? addend->ptr<bf16_t>() : (const bf16_t*)nullptr;
  if (addend_fused) *addend_fused = with_add;
  bf16_t* dst2p = sib ? sib->out->ptr<bf16_t>() : (bf16_t*)nullptr;
  const bf16_t* bias2p = (sib && sib->bias) ? sib->bias->ptr<bf16_t>() : (const bf16_t*)nullptr;
  float* statp = stats.ptr();
  float* stat2p = stats.ptr2();
  void* args[] = {(void*)&srcp, (void*)&wpk, (void*)&bp, (void*)&dstp, (void*)&q, (void*)&addp, (void*)&dst2p, (void*)&bias2p, (void*)&co_a,
                  (void*)&statp, (void*)&stat2p, (void*)&stats_per_wg, (void*)&src2p};
  ncv_launch(kfn, blocks, lp.threads, lp.lds, args, st);
  stats.publish(out, sib ? 0 : w->st->uid, sib ? sib->out : nullptr);
}
static bool ncv_run(const Tensor* in, const Tensor* w, const Tensor* bias, Tensor* out, const ConvGeom& g, bool dgrad, hipStream_t st,
                    const Tensor* addend = nullptr, bool* addend_fused = nullptr, const NcvSibling* sib = nullptr,
                    const NcvSecondGrad* second = nullptr) {
  if (addend_fused) *addend_fused = false;
  const Tensor* wsecond = sib ? sib->w : second ? second->w : nullptr;
  const int cout2 = wsecond ? (int)wsecond->sizes[0] : 0;
  NcvLaunchPlan lp;
  if (!ncv_plan(g, in->dtype, dgrad, sib != nullptr, second != nullptr, cout2, false, lp)) return false;
  Hold wpk(ncv_packed_weights(w, ncv_weights_of(w, g, dgrad, lp, wsecond, cout2), st, wsecond));
  // (a sibling's or second gradient's work is declared with the launch)
  KernelTimer kt(dgrad ? "conv_dgrad_narrow" : "conv_fwd_narrow", conv_flops(g) + ncv_sibling_flops(g, cout2), conv_bytes(g, 2) + ncv_sibling_bytes(g, cout2), st);
  if (lp.aligned) ncv_run_aligned(lp, dgrad, in, w, ncv_fragments(wpk), bias, out, st, addend, addend_fused, sib, second);
  else ncv_run_generic(lp, in, ncv_fragments(wpk), bias, out, st);
  return true;
}

bool narrow_conv_fwd(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, hipStream_t st) {
  return ncv_run(x, w, bias, y, g, false, st);
}
// the 3x3 pad 1 + 1x1 pad 0 pairs the sibling launch is for (LAMP_CONV_SIBLING=0: none)
static bool ncv_fwd_pair_shapes(const Tensor* x, const ConvGeom& g, const ConvGeom& g1) {
  return sw().conv_sibling && x->dtype == kBF16 && ncv_pair_shapes(g, g1);
}
// y = conv3x3(x, w) and y1 = conv1x1(x, w1), same stride and output map (the two branches of lamp's residual block on its input,
// cnn.scala:16-20), Cout + Cout1 <= 16: one launch, the values of the two separate ones (the second filter is the centre tap of extra
// output columns); false = nothing launched
bool narrow_conv_fwd_pair(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, const Tensor* w1, const Tensor* bias1,
                          Tensor* y1, const ConvGeom& g1, hipStream_t st) {
  if (!ncv_fwd_pair_shapes(x, g, g1)) return false;
  const NcvSibling sb{w1, bias1, y1};
  return ncv_run(x, w, bias, y, g, false, st, nullptr, nullptr, &sb);
}
// s = conv(x, w0), y = conv3x3(s, w) and y1 = conv1x1(s, w1): a stride-1 convolution and the pair that reads its output, in one launch of
// ncv_chain_kernel - bitwise the values, and the statistics hand-off of y and y1, of narrow_conv_fwd followed by narrow_conv_fwd_pair.
// false = nothing launched: the caller runs those two.  Taken when both are the aligned-window form the chain kernel is built for (the first
// in the two-shift form with 4 k-steps and window phase 6: up to 8 output channels from up to 3 x 5 (channel, row) pairs of a 5-wide filter;
// the pair at stride 2 in the one-shift form, 5 or 12 k-steps), one image of each fits the LDS together, and the pair's statistics keep the
// partition they have in a launch of their own.
bool narrow_conv_chain_pair(const Tensor* x, const Tensor* w0, const Tensor* bias0, Tensor* s, const ConvGeom& g0, const Tensor* w, const Tensor* bias,
                            Tensor* y, const ConvGeom& g, const Tensor* w1, const Tensor* bias1, Tensor* y1, const ConvGeom& g1, hipStream_t st) {
  if (!ncv_fwd_pair_shapes(x, g, g1)) return false;
  if (g0.groups != 1 || g0.sh != 1 || g0.sw != 1 || g0.N != g.N || g0.Cout != g.Cin || g0.Ho != g.H || g0.Wo != g.W) return false;
  const int cout2 = (int)w1->sizes[0];
  NcvLaunchPlan p0, p1;
  // (x reaches the first image through the chain kernel's own register prefetch, the pair's image is written by the first convolution)
  if (!ncv_plan(g0, x->dtype, false, false, false, 0, true, p0) || !ncv_plan(g, x->dtype, false, true, false, cout2, false, p1)) return false;
  if (!p0.aligned || !p1.aligned || p0.threads != 256 || p1.threads != 256) return false;
  if ((int64_t)p0.q.C * p0.q.H * p0.q.W > (int64_t)NCV_CHAIN_PF * 256 * 8) return false;      // (the chain kernel's register prefetch of x)
  if (p0.NS != 2 || p0.NK != 4 || p0.ph0 != 6) return false;
  if (p1.NS != 1 || p1.q.sw != 2 || p1.ph0 != 7 || !(p1.NK == 5 || p1.NK == 12)) return false;
  const size_t lds = p0.lds + p1.lds;
  if (lds > NCV_LDS_BUDGET) return false;
  const NcvGeom& q0 = p0.q;
  const NcvGeom& q1 = p1.q;
  const bool with_stats = ncv_takes_stats(q1, false, false, true, w);
  const void* kfn = nullptr;
  if (p1.NK == 5) kfn = with_stats ? (const void*)ncv_chain_kernel<4, 6, 5, 7, true> : (const void*)ncv_chain_kernel<4, 6, 5, 7, false>;
  else kfn = with_stats ? (const void*)ncv_chain_kernel<4, 6, 12, 7, true> : (const void*)ncv_chain_kernel<4, 6, 12, 7, false>;
  // the grid of the pair's own launch decides how its statistics are partitioned (per workgroup when every workgroup walks the same number
  // of images): this launch takes that grid, or a smaller one where per-image triples are what the pair's launch would have written too
  const void* kpair = ncv_fwd2_fn(p1.NK, p1.NS, p1.ph0, q1.sw, false, with_stats, p1.nke);
  const int pair_per_cu = ncv_per_cu(kpair, 256, p1.lds);
  const int pair_blocks = ncv_grid(g.N, pair_per_cu);
  const int blocks = ncv_grid(g.N, std::min(pair_per_cu, ncv_per_cu(kfn, 256, lds)));
  const bool pair_per_wg = g.N % pair_blocks == 0;
  if (with_stats && blocks != pair_blocks && pair_per_wg && g.N > pair_blocks) return false;
  int stats_per_wg = (blocks == pair_blocks && pair_per_wg) ? 1 : 0;
  Hold wpk0_h(ncv_packed_weights(w0, ncv_weights_of(w0, g0, false, p0, nullptr, 0), st));
  Hold wpk1_h(ncv_packed_weights(w, ncv_weights_of(w, g, false, p1, w1, cout2), st, w1));
  const nv_bf8* wpk0 = ncv_fragments(wpk0_h);
  const nv_bf8* wpk1 = ncv_fragments(wpk1_h);
  NcvStats stats(with_stats, stats_per_wg ? blocks : (int)g.N, g.Cout, cout2, x->device());
  {
    // both convolutions' work and traffic, less the read of s that the LDS image replaces
    const double fl = conv_flops(g0) + conv_flops(g) + ncv_sibling_flops(g, cout2);
    const double by = conv_bytes(g0, 2) + conv_bytes(g, 2) + ncv_sibling_bytes(g, cout2) - (double)g.N * g.Cin * g.H * g.W * 2.0;
    KernelTimer kt("conv_fwd_narrow", fl, by, st);
    const bf16_t* xp = x->ptr<bf16_t>();
    const bf16_t* b0p = bias0 ? bias0->ptr<bf16_t>() : (const bf16_t*)nullptr;
    const bf16_t* bp = bias ? bias->ptr<bf16_t>() : (const bf16_t*)nullptr;
    const bf16_t* b1p = bias1 ? bias1->ptr<bf16_t>() : (const bf16_t*)nullptr;
    bf16_t* sp = s->ptr<bf16_t>();
    bf16_t* yp = y->ptr<bf16_t>();
    bf16_t* y1p = y1->ptr<bf16_t>();
    int co_a = (int)g.Cout;
    float* statp = stats.ptr();
    float* stat2p = stats.ptr2();
    void* args[] = {(void*)&xp, (void*)&wpk0, (void*)&b0p, (void*)&sp, (void*)&q0, (void*)&wpk1, (void*)&bp, (void*)&b1p, (void*)&yp, (void*)&y1p,
                    (void*)&co_a, (void*)&q1, (void*)&statp, (void*)&stat2p, (void*)&stats_per_wg};
    ncv_launch(kfn, blocks, 256, lds, args, st);
  }
  stats.publish(y, 0, y1);
  return true;
}
bool narrow_conv_dgrad(const Tensor* dy, const Tensor* w, Tensor* dx, const ConvGeom& g, hipStream_t st, const Tensor* addend, bool* addend_fused) {
  return ncv_run(dy, w, nullptr, dx, g, true, st, addend, addend_fused);
}
// dx = round(dgrad3x3(dy, w) + dgrad1x1(dy1, w1) [then round(. + addend)]: the input gradient of the two branches of lamp's residual block
// (cnn.scala:16-20; autograd.scala:66-84 accumulates the two partial derivatives) from ONE launch - the second gradient tensor is staged
// as extra channels of the image, the second filter is their centre tap - summed in f32 before the one rounding (the two-launch chain
// rounds each contribution first); false = nothing launched
bool narrow_conv_dgrad_pair(const Tensor* dy, const Tensor* w, const ConvGeom& g, const Tensor* dy1, const Tensor* w1, const ConvGeom& g1, Tensor* dx,
                            hipStream_t st, const Tensor* addend, bool* addend_fused) {
  if (addend_fused) *addend_fused = false;
  if (!sw().conv_dgrad_pair || dy->dtype != kBF16 || dy1->dtype != kBF16) return false;
  if (!ncv_pair_shapes(g, g1) || g1.Cout > 16) return false;
  const NcvSecondGrad sg{dy1, w1};
  return ncv_run(dy, w, nullptr, dx, g, true, st, addend, addend_fused, nullptr, &sg);
}

// the instantiation of ncv_wgrad_kernel for (16-column tiles of the Cin x kh x kw filter columns, stride)
static const void* ncv_wgrad_fn(int NT, int SW) {
#define NCV_WG(NTv) return SW == 1 ? (const void*)ncv_wgrad_kernel<NTv, 1> : (const void*)ncv_wgrad_kernel<NTv, 2>
  switch (NT) {
    case 1: NCV_WG(1);
    case 2: NCV_WG(2);
    case 4: NCV_WG(4);
    case 5: NCV_WG(5);
    default: NCV_WG(9);
  }
#undef NCV_WG
}
// the instantiation of ncv_wgrad2_kernel for (filter width, stride, pair tiles)
static const void* ncv_wgrad2_fn(int kw, int SW, int npt) {
  const void* kfn = nullptr;
#define NCV_WG2(KWv, PWv, SWv, NPTv) kfn = (const void*)ncv_wgrad2_kernel<KWv, PWv, SWv, NPTv>
#define NCV_WG2_NPT(KWv, PWv, SWv) do { if (npt == 1) NCV_WG2(KWv, PWv, SWv, 1); else if (npt == 2) NCV_WG2(KWv, PWv, SWv, 2); else NCV_WG2(KWv, PWv, SWv, 3); } while (0)
  if (kw == 5) NCV_WG2_NPT(5, 2, 1);
  else if (kw == 3 && SW == 1) NCV_WG2_NPT(3, 1, 1);
  else if (kw == 3) NCV_WG2_NPT(3, 1, 2);
  else if (SW == 1) NCV_WG2_NPT(1, 0, 1);
  else NCV_WG2_NPT(1, 0, 2);
#undef NCV_WG2_NPT
#undef NCV_WG2
  return kfn;
}
// the partition of N images in rounds of IG over at most per_cu workgroups per CU: the number of workgroups, ipb = images per workgroup
static int ncv_partition(int per_cu, int64_t N, int IG, int& ipb) {
  const int64_t rounds = (N + IG - 1) / IG;
  const int nb = (int)std::min<int64_t>(rounds, (int64_t)num_cus() * per_cu);
  ipb = (int)((rounds + nb - 1) / nb) * IG;
  return (int)((N + ipb - 1) / ipb);
}
// One weight-gradient launch: the staged geometry, the kernel, its LDS and the partition of the images over the workgroups.
struct NcvWgradPlan {
  NcvWGeom q;
  const void* kfn;
  int npt;               // aligned-read form: pair tiles
  size_t lds;
  int nblocks, ipb;      // workgroups, images per workgroup
};
// The form of a geometry's weight-gradient launch, without its partition.  aligned: ncv_wgrad2_kernel, for the filter shapes of the CIFAR ResNet
// (x parity planes / rows at column NCV_OFFA; it alone takes a sibling's cout2 gradient rows); else ncv_wgrad_kernel.  The two stage x alike but
// for the row pitch.  false: the geometry has no such form
static bool ncv_wgrad_form(const ConvGeom& g, int dtype, int cout2, bool aligned, NcvWgradPlan& wp) {
  if (!ncv_common(g, dtype)) return false;
  if (g.W % 8 != 0 || g.Wo % 8 != 0 || (g.Ho * g.Wo) % 32 != 0) return false;
  NcvWGeom& q = wp.q;
  q.N = (int)g.N; q.Cin = (int)g.Cin; q.Cout = (int)g.Cout; q.H = (int)g.H; q.W = (int)g.W; q.Ho = (int)g.Ho; q.Wo = (int)g.Wo;
  q.kh = g.kh; q.kw = g.kw; q.ph = g.ph; q.pw = g.pw; q.Cout2 = cout2;
  q.ncol = (int)g.Cin * g.kh * g.kw;
  q.Hs = std::max((int)g.H + 2 * g.ph, ((int)g.Ho - 1) * g.sh + g.kh);
  const int SW = g.sh, HoWo = (int)(g.Ho * g.Wo);
  q.IG = std::max(1, 256 / HoWo);                                    // >= 8 chunks of 32 pixels per round
  int red_cols = 0;                                                  // columns of the four waves' 16-row sums
  if (aligned) {
    wp.npt = (int)((g.Cin * g.kh + 15) / 16);
    if (!(g.kh == g.kw && wp.npt <= 3 && ((g.kw == 5 && g.pw == 2 && SW == 1) || (g.kw == 3 && g.pw == 1) || (g.kw == 1 && g.pw == 0)))) return false;
    q.Ws = SW == 1 ? round_up(NCV_OFFA + std::max((int)g.W, (int)g.Wo + 8) + 8, 8) : round_up(NCV_OFFA + std::max((int)g.W / 2, (int)g.Wo) + 8, 8);
    wp.kfn = ncv_wgrad2_fn(g.kw, SW, wp.npt);
    red_cols = wp.npt * g.kw * 16;
  } else {
    if (cout2 > 0) return false;
    const int nt_real = (q.ncol + 15) / 16;
    static const int nt_opts[] = {1, 2, 4, 5, 9};
    int NT = 0;
    for (int o : nt_opts) if (o >= nt_real) { NT = o; break; }
    if (!NT) return false;
    const int half_max = (g.kw - 1 - g.pw) >> 1;
    q.Ws = SW == 1 ? round_up(std::max(NCV_LEFT + (int)g.W, (int)g.Wo - 1 + g.kw - 1 - g.pw + NCV_LEFT + 1), 8)
                   : round_up(std::max((int)g.W / 2, (int)g.Wo + half_max) + NCV_OFF2 + 1, 8);
    wp.kfn = ncv_wgrad_fn(NT, SW);
    red_cols = NT * 16;
  }
  const int ximg = q.Cin * q.Hs * q.Ws * (SW == 2 ? 2 : 1);
  if (!aligned && (q.IG * (ximg + 16 * HoWo)) % 8 != 0) return false;
  wp.lds = (size_t)q.IG * (ximg + 16 * HoWo) * 2 + (size_t)4 * 16 * red_cols * 4;
  return true;
}
// The planned launch in that form: a workgroup's images fit the LDS, and the N images go in rounds of IG over the workgroups that are
// co-resident.  The partition fixes the order of the partial sums, and with it the bits of dw: the aligned form counts the workgroups that
// LDS and registers allow, the generic form those the LDS allows.
static bool ncv_wgrad_plan(const ConvGeom& g, int dtype, int cout2, bool aligned, NcvWgradPlan& wp) {
  if (!ncv_wgrad_form(g, dtype, cout2, aligned, wp) || wp.lds > NCV_LDS_BUDGET) return false;
  const int per_cu = aligned ? ncv_per_cu(wp.kfn, 256, wp.lds) : ncv_lds_per_cu(wp.lds);
  wp.nblocks = ncv_partition(per_cu, g.N, wp.q.IG, wp.ipb);
  return true;
}
// second (optional): the output gradient of a sibling 1x1 convolution of the same x and ITS weight gradient: both from the one launch of the
// aligned kernel (false, nothing launched, when that kernel does not take the pair)
struct NcvSecondWgrad { const Tensor* dy; Tensor* dw; };
static void ncv_wgrad_launch(const NcvWgradPlan& wp, const ConvGeom& g, const Tensor* dy, const Tensor* x, Tensor* dw, const NcvSecondWgrad* second,
                             hipStream_t st) {
  const NcvWGeom& q = wp.q;
  const int O = q.Cout * q.ncol, O2 = q.Cout2 * q.Cin;
  Hold partial(new_tensor({(int64_t)wp.nblocks * O}, kF32, dy->device()));
  Hold partial2(second ? new_tensor({(int64_t)wp.nblocks * O2}, kF32, dy->device()) : nullptr);
  {
    // (the sibling's work is declared with the launch; x is the one already counted)
    KernelTimer kt("conv_wgrad_narrow", conv_flops(g) + ncv_sibling_flops(g, q.Cout2), conv_bytes(g, 2) + ncv_sibling_bytes(g, q.Cout2), st);
    const bf16_t* dp = dy->ptr<bf16_t>(); const bf16_t* xp = x->ptr<bf16_t>(); float* pp = partial->ptr<float>();
    const bf16_t* dp2 = second ? second->dy->ptr<bf16_t>() : (const bf16_t*)nullptr;
    float* pp2 = second ? partial2->ptr<float>() : (float*)nullptr;
    int ipb = wp.ipb;
    void* args[] = {(void*)&dp, (void*)&xp, (void*)&pp, (void*)&q, (void*)&ipb, (void*)&dp2, (void*)&pp2};      // (ncv_wgrad_kernel: the first five)
    ncv_launch(wp.kfn, wp.nblocks, 256, wp.lds, args, st);
  }
  wgrad_reduce_flat(O, wp.nblocks, partial.get(), dw, st);
  if (second) wgrad_reduce_flat(O2, wp.nblocks, partial2.get(), second->dw, st);
}
static bool ncv_wgrad_run(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st, const NcvSecondWgrad* second) {
  const int cout2 = second ? (int)second->dy->sizes[1] : 0;
  if (second && (g.Cout + cout2 > 16 || g.kh != 3 || g.kw != 3 || g.ph != 1 || g.pw != 1)) return false;
  NcvWgradPlan wp;
  if (!ncv_wgrad_plan(g, x->dtype, cout2, true, wp) && !ncv_wgrad_plan(g, x->dtype, cout2, false, wp)) return false;
  ncv_wgrad_launch(wp, g, dy, x, dw, second, st);
  return true;
}


bool narrow_conv_wgrad(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st) { return ncv_wgrad_run(dy, x, dw, g, st, nullptr); }
// dw = wgrad3x3(dy, x) and dw1 = wgrad1x1(dy1, x) - the weight gradients of the two convolutions lamp's residual block applies to its input
// (cnn.scala:16-20) - from one launch that stages x once: the values of the two separate launches (the second gradient tensor rides in the
// spare rows of the MFMA tile, its weight gradient is the centre tap of those rows); false = nothing launched
bool narrow_conv_wgrad_pair(const Tensor* dy, const Tensor* dy1, const Tensor* x, Tensor* dw, Tensor* dw1, const ConvGeom& g, const ConvGeom& g1, hipStream_t st) {
  if (!sw().conv_wgrad_pair || x->dtype != kBF16 || dy->dtype != kBF16 || dy1->dtype != kBF16) return false;
  if (!ncv_pair_shapes(g, g1)) return false;
  const NcvSecondWgrad sg{dy1, dw1};
  return ncv_wgrad_run(dy, x, dw, g, st, &sg);
}

// dx, dw and dw1 of a block's 3x3 pad 1 + 1x1 pad 0 stride-2 pair from ONE launch of ncv_bwd_pair_kernel: the values of narrow_conv_dgrad_pair
// and of the weight-gradient launches (narrow_conv_wgrad_pair, or two narrow_conv_wgrad where the two gradients do not share the 16 MFMA rows).
// false = nothing launched: the caller runs those.  Taken when the input gradient is the parity form of the aligned-window kernel (two-shift,
// window phase 7), the weight gradient the aligned-read form with two pair tiles, a round fits the register prefetch and one workgroup's images
// fit the LDS.  The workgroups and their images are those of the 3x3 weight gradient's own launch wherever as many workgroups fit a CU.
bool narrow_conv_backward_pair(const Tensor* dy, const Tensor* dy1, const Tensor* x, const Tensor* w, const Tensor* w1, const ConvGeom& g, const ConvGeom& g1,
                               Tensor* dx, Tensor* dw, Tensor* dw1, hipStream_t st, const Tensor* addend) {
  if (!sw().conv_bwd_pair || !sw().conv_dgrad_pair || !sw().conv_wgrad_pair) return false;
  if (x->dtype != kBF16 || dy->dtype != kBF16 || dy1->dtype != kBF16 || w->dtype != kBF16 || w1->dtype != kBF16) return false;
  if (!ncv_pair_shapes(g, g1) || g.sh != 2 || g.sw != 2 || g1.Cout > 16) return false;
  const int cout2 = (int)g1.Cout;
  // the input gradient: the plan of narrow_conv_dgrad_pair, staged through this kernel's image-group prefetch (its fit is checked below)
  NcvLaunchPlan lp;
  if (!ncv_plan(g, x->dtype, true, false, true, cout2, true, lp)) return false;
  if (!lp.aligned || lp.nke <= 0 || lp.NS != 2 || lp.ph0 != 7 || lp.q.sw != 1 || lp.q.W % 8 != 0) return false;
  if (!(lp.NK == 6 || lp.NK == 8 || lp.NK == 16)) return false;
  const NcvGeom& qd = lp.q;
  // the weight gradients: the geometry of ncv_wgrad2_kernel<3, 1, 2, .>, the reference launch whose partition this one takes
  const bool w2 = g.Cout + cout2 > 16;
  NcvWgradPlan ref;
  if (!ncv_wgrad_form(g, x->dtype, cout2, true, ref) || ref.npt != 2) return false;
  NcvWGeom q = ref.q;
  const int HoWo = q.Ho * q.Wo, cpi = HoWo >> 5;
  const int ximg = q.Cin * q.Hs * q.Ws * 2, drows = w2 ? 32 : 16;
  const int ncolt = 2 * 3 * 16;
  const size_t red_bytes = (size_t)4 * 16 * ncolt * 4 + (w2 ? (size_t)4 * 16 * 32 * 4 : 0);
  auto lds_of = [&](int IG) { return (size_t)IG * (ximg + drows * HoWo) * 2 + std::max(lp.lds, red_bytes); };
  // the reference launch's rounds decide the partition; this kernel's rounds may be shorter (a wave meets the same chunks in the same order
  // as long as a round is a multiple of four chunks), which is what lets two workgroups share a CU beside the dilated image
  while (lds_of(q.IG) * 2 > NCV_LDS_BUDGET && q.IG % 2 == 0 && ((q.IG / 2) * cpi) % 4 == 0) q.IG /= 2;
  const size_t lds = lds_of(q.IG);
  if (lds > NCV_LDS_BUDGET) return false;
  const int per = (q.Cin * q.H * q.W + (q.Cout + cout2) * HoWo) >> 3;
  if (q.IG * per > NCV_WPF * 256) return false;                      // (the kernel stages through the register prefetch only)
  const int threads = 256;
  if (q.IG > 1 && (int64_t)qd.C * qd.H * qd.W > (int64_t)2 * threads * 8) return false;      // (an image's copy from the plain to the dilated image: two packets per thread)
  const bool with_add = addend != nullptr;
  // (the 16-k-step forms hold four packets per thread: with six their registers do not fit two workgroups per CU)
  const void* kfn = nullptr;
#define NCV_BP(NKv, W2v, WPFv) kfn = with_add ? (const void*)ncv_bwd_pair_kernel<NKv, true, 2, W2v, WPFv> : (const void*)ncv_bwd_pair_kernel<NKv, false, 2, W2v, WPFv>
  if (lp.NK == 6 && !w2) NCV_BP(6, false, NCV_WPF);
  else if (lp.NK == 8 && !w2) NCV_BP(8, false, NCV_WPF);
  else if (lp.NK == 16 && q.IG * per <= 4 * 256) { if (w2) NCV_BP(16, true, 4); else NCV_BP(16, false, 4); }
  else return false;
#undef NCV_BP
  // the partition of the 3x3 weight gradient's own launch (its rounds, its workgroups per CU), unless fewer of these workgroups fit a CU
  const int per_cu = std::min(ncv_per_cu(ref.kfn, 256, ref.lds), ncv_per_cu(kfn, threads, lds));
  int ipb = 0;
  const int nblocks = ncv_partition(per_cu, g.N, ref.q.IG, ipb);
  Hold wpk_h(ncv_packed_weights(w, ncv_weights_of(w, g, true, lp, w1, cout2), st, w1));
  const nv_bf8* wpk = ncv_fragments(wpk_h);
  const int O = q.Cout * q.ncol, O2 = cout2 * q.Cin;
  Hold partial(new_tensor({(int64_t)nblocks * O}, kF32, dy->device())), partial2(new_tensor({(int64_t)nblocks * O2}, kF32, dy->device()));
  {
    // the three parts' work and traffic, less the second read of the two gradients
    const double dy_by = (double)g.N * (g.Cout + cout2) * HoWo * 2.0;
    KernelTimer kt("conv_bwd_narrow", 2.0 * (conv_flops(g) + ncv_sibling_flops(g, cout2)), 2.0 * (conv_bytes(g, 2) + ncv_sibling_bytes(g, cout2)) - dy_by, st);
    const bf16_t* dp = dy->ptr<bf16_t>(); const bf16_t* dp2 = dy1->ptr<bf16_t>(); const bf16_t* xp = x->ptr<bf16_t>();
    bf16_t* dxp = dx->ptr<bf16_t>();
    const bf16_t* addp = with_add ? addend->ptr<bf16_t>() : (const bf16_t*)nullptr;
    float* pp = partial->ptr<float>(); float* pp2 = partial2->ptr<float>();
    void* args[] = {(void*)&dp, (void*)&dp2, (void*)&xp, (void*)&wpk, (void*)&dxp, (void*)&addp, (void*)&pp, (void*)&pp2, (void*)&q, (void*)&qd, (void*)&ipb};
    ncv_launch(kfn, nblocks, threads, lds, args, st);
  }
  wgrad_reduce_flat(O, nblocks, partial.get(), dw, st);
  wgrad_reduce_flat(O2, nblocks, partial2.get(), dw1, st);
  return true;
}

}  // namespace lamp
