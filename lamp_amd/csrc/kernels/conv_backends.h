// Host entry points of the convolution backends that conv_dispatch (conv.hip) tries in turn.  The bool ones return true when they
// handled the request and false with nothing launched.
#pragma once
#include "../core/tensor.h"
#include "conv_geom.h"

namespace lamp {
struct NcvPackMany;   // conv_narrow_pack.h

// ---- conv_igemm.hip: bf16 implicit GEMM on the matrix cores, the wide 3x3 / 1x1 layers on 8 x 8 maps
bool igemm_conv_fwd(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, hipStream_t st);
bool igemm_conv_fwd_pair(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, const Tensor* w1, const Tensor* bias1,
                         Tensor* y1, const ConvGeom& g1, hipStream_t st);
// addend (optional): dx = round(round(dgrad) + addend) when the kernel chosen has that epilogue; *addend_fused reports whether it was used
bool igemm_conv_dgrad(const Tensor* dy, const Tensor* w, Tensor* dx, const ConvGeom& g, hipStream_t st, const Tensor* addend = nullptr,
                      bool* addend_fused = nullptr);
bool igemm_conv_dgrad_pair(const Tensor* dy, const Tensor* w, const ConvGeom& g, const Tensor* dy1, const Tensor* w1, const ConvGeom& g1, Tensor* dx,
                           hipStream_t st, const Tensor* addend, bool* addend_fused);
bool igemm_conv_wgrad(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st, const Tensor* affine = nullptr);
bool igemm_conv_wgrad_pair(const Tensor* dy, const Tensor* dy1, const Tensor* x, Tensor* dw, Tensor* dw1, const ConvGeom& g, const ConvGeom& g1, hipStream_t st);
// dx (+ addend), dw and dw1 of a stride-1 3x3 + 1x1 pair with at most 16 input channels on 8x8 maps from one launch (false: nothing launched)
bool igemm_conv_backward_pair(const Tensor* dy, const Tensor* dy1, const Tensor* x, const Tensor* w, const Tensor* w1, const ConvGeom& g, const ConvGeom& g1,
                              Tensor* dx, Tensor* dw, Tensor* dw1, hipStream_t st, const Tensor* addend = nullptr);
bool igemm_conv_folds_affine(const ConvGeom& g, int dtype);
bool igemm_conv_fwd_affine(const Tensor* x, const Tensor* affine, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, hipStream_t st);

// ---- conv_igemm_f32.hip: the same layers in f32 / f64, on the f32 / f64 matrix instructions
bool igemm32_conv_fwd(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, hipStream_t st);
bool igemm32_conv_dgrad(const Tensor* dy, const Tensor* w, Tensor* dx, const ConvGeom& g, hipStream_t st, const Tensor* addend = nullptr,
                        bool* addend_fused = nullptr);
bool igemm32_conv_wgrad(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st);

// ---- conv_narrow.hip: bf16 layers of at most 16 channels on the matrix cores
bool narrow_conv_fwd(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, hipStream_t st);
bool narrow_conv_fwd_pair(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, const Tensor* w1, const Tensor* bias1,
                          Tensor* y1, const ConvGeom& g1, hipStream_t st);
// s = conv(x, w0) (stride 1), y = conv3x3(s, w), y1 = conv1x1(s, w1) from one launch (false: nothing launched)
bool narrow_conv_chain_pair(const Tensor* x, const Tensor* w0, const Tensor* bias0, Tensor* s, const ConvGeom& g0, const Tensor* w, const Tensor* bias,
                            Tensor* y, const ConvGeom& g, const Tensor* w1, const Tensor* bias1, Tensor* y1, const ConvGeom& g1, hipStream_t st);
bool narrow_conv_dgrad(const Tensor* dy, const Tensor* w, Tensor* dx, const ConvGeom& g, hipStream_t st, const Tensor* addend = nullptr,
                       bool* addend_fused = nullptr);
bool narrow_conv_dgrad_pair(const Tensor* dy, const Tensor* w, const ConvGeom& g, const Tensor* dy1, const Tensor* w1, const ConvGeom& g1, Tensor* dx,
                            hipStream_t st, const Tensor* addend, bool* addend_fused);
bool narrow_conv_wgrad(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st);
// dx (+ addend), dw and dw1 of a stride-2 3x3 + 1x1 pair of the same x from one launch (false: nothing launched)
bool narrow_conv_backward_pair(const Tensor* dy, const Tensor* dy1, const Tensor* x, const Tensor* w, const Tensor* w1, const ConvGeom& g, const ConvGeom& g1,
                               Tensor* dx, Tensor* dw, Tensor* dw1, hipStream_t st, const Tensor* addend = nullptr);
bool narrow_conv_wgrad_pair(const Tensor* dy, const Tensor* dy1, const Tensor* x, Tensor* dw, Tensor* dw1, const ConvGeom& g, const ConvGeom& g1, hipStream_t st);

// ---- conv_small.hip: narrow layers, image-per-workgroup LDS kernels (bf16 / f32 / f64)
bool small_conv_fwd(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, hipStream_t st);
bool small_conv_dgrad(const Tensor* dy, const Tensor* w, Tensor* dx, const ConvGeom& g, hipStream_t st, const Tensor* addend = nullptr,
                      bool* addend_fused = nullptr);
bool small_conv_wgrad(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st);

// ---- conv_gen.hip: any geometry of groups == 1 in bf16 / f32 on the matrix cores, asked for 1-D and transposed convolutions where the
// direct kernels would run.  The bias of gen_conv_dgrad serves the transposed forward only.
bool gen_conv_fwd(const Tensor* x, const Tensor* w, const Tensor* bias, Tensor* y, const ConvGeom& g, hipStream_t st);
bool gen_conv_dgrad(const Tensor* dy, const Tensor* w, const Tensor* bias, Tensor* dx, const ConvGeom& g, hipStream_t st);
bool gen_conv_wgrad(const Tensor* dy, const Tensor* x, Tensor* dw, const ConvGeom& g, hipStream_t st);
// ... its launch plan: a function of the arguments and the CU count alone, it touches no device (lamp_debug_conv_gen_plan and
// tests/test_conv_gen_plan.py ask it without one).  The product is R[U][V] over K (conv_gen.hip's table); K is cut into `splits` ranges
// of `klen` (a multiple of BK; the last one may be shorter), split z owning [z klen, min(K, (z + 1) klen)).
enum GenPass : int { kGenFwd = 0, kGenDgrad = 1, kGenWgrad = 2 };
struct GenPlan {
  bool accepted;
  const char* reason;      // why it declined ("" when accepted)
  int pass, dtype;
  int64_t U, V, K;
  int BU, BV, BK;          // tile
  dim3 grid;               // (V tiles, U tiles, splits)
  int threads;
  int splits;
  int64_t klen;
  size_t ws_bytes;         // f32 partial tiles [splits][U][V] when splits > 1, else 0
  int lds_bytes;
};
GenPlan gen_plan(int pass, int dtype, const ConvGeom& g, int cus);
// lamp_convolution_matrix_path: off = the dispatch never asks conv_gen.hip
bool conv_matrix_path();

// ---- the optimisers' hook (optim.hip calls it right after it has written the parameters; conv.hip): every packed image of these parameters
// that is cached on this stream is packed again, in place, and its entry moved to the new storage version (core/pack_cache.h)
void conv_repack_cached(lamp_tensor* const* params, int n, hipStream_t st);
// ... its per-backend parts; igemm's takes the narrow images' last batch along in its launch: with `fill`, narrow's hands that batch of at most
// NCV_PACK_MAX images to the caller (*fill, *fill_cnt) instead of launching it
void igemm_repack_cached(lamp_tensor* const* params, int n, hipStream_t st);
void igemm32_repack_cached(lamp_tensor* const* params, int n, hipStream_t st);
void small_repack_cached(lamp_tensor* const* params, int n, hipStream_t st);
void narrow_repack_cached(lamp_tensor* const* params, int n, hipStream_t st, NcvPackMany* fill, int* fill_cnt);
void narrow_pack_launch(const NcvPackMany& a, int cnt, hipStream_t st);

}  // namespace lamp
