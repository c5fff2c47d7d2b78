// The LAMP_* run-time switches: every one the library reads from the environment, in one table.  Nothing else under csrc reads the environment.
//
// A row is  X(member, "NAME", KIND, default, lower clamp, "what it selects")  - one switch per line (tests/test_switches.py reads the rows).
//   BOOL,   default 1: on unless the value's first character is '0'
//   BOOL,   default 0: off unless the value's first character is '1'
//   INT:    unset -> the default as written; set -> max(lower clamp, value)   (SW_NO_CLAMP: the value as given)
//   LETTER: the value's first character, 0 when unset
// The table says WHAT a switch selects; WHY its default won (measurements, EXPERIMENTS.md) stands where the decision is taken.
#pragma once
#include <cstdint>

namespace lamp {

constexpr int64_t SW_NO_CLAMP = INT64_MIN;

// ---- read once per process, at the first call of sw() ------------------------------------------------------------------------------
#define LAMP_SWITCHES_ONCE(X)                                                                                                             \
  /* model level (host/nn.cpp, host/ops.cpp, host/transformer.cpp, host/data.cpp) */                                                      \
  X(conv_sibling, "LAMP_CONV_SIBLING", BOOL, 1, 0, "a residual block's 3x3 and its sibling 1x1 of the same input as one forward launch") \
  X(conv_chain, "LAMP_CONV_CHAIN", BOOL, 1, 0, "a convolution directly in front of a residual block and the block's 3x3 + 1x1 as one forward call (0: two)") \
  X(fuse_bn_pair, "LAMP_FUSE_BN_PAIR", BOOL, 1, 0, "relu(bn(right) + bn(left)) at a block's end as one op (0: the chain)")                \
  X(fuse_pool_logsoftmax, "LAMP_FUSE_POOL_LOGSOFTMAX", BOOL, 1, 0, "average pool -> flatten -> log-softmax tail as one node")             \
  X(fuse_block_tail, "LAMP_FUSE_BLOCK_TAIL", BOOL, 1, 0, "the last residual block and the pooled log-softmax tail as one node")          \
  X(fuse_bn_conv, "LAMP_FUSE_BN_CONV", BOOL, 1, 0, "batch norm -> relu -> convolution: the convolution applies the norm while staging")  \
  X(fuse_loss_accumulate, "LAMP_FUSE_LOSS_ACCUMULATE", BOOL, 1, 0, "acc += n * loss inside the NLL loss kernel")                          \
  X(fuse_loss_backward, "LAMP_FUSE_LOSS_BACKWARD", BOOL, 1, 0, "the NLL loss backward goes straight to the pooled log-softmax node's input in one launch")                      \
  X(fuse_loss_tail, "LAMP_FUSE_LOSS_TAIL", BOOL, 1, 0, "the loss launch also writes the pooled log-softmax's input gradient per plane")  \
  X(conv_dgrad_accumulate, "LAMP_CONV_DGRAD_ACCUMULATE", BOOL, 1, 0, "a convolution's input gradient adds into the existing one in its epilogue") \
  X(conv_dgrad_pair, "LAMP_CONV_DGRAD_PAIR", BOOL, 1, 0, "input gradients of a block's 3x3 and sibling 1x1 from one launch")             \
  X(conv_wgrad_pair, "LAMP_CONV_WGRAD_PAIR", BOOL, 1, 0, "weight gradients of a block's 3x3 and sibling 1x1 from one launch")            \
  X(conv_bwd_pair, "LAMP_CONV_BWD_PAIR", BOOL, 1, 0, "a block's paired input gradient and its two weight gradients from one call (0: the two pair calls)") \
  X(linear_bias_fused, "LAMP_LINEAR_BIAS_FUSED", BOOL, 1, 0, "a linear layer's bias in the GEMM epilogue (0: mm then add)")               \
  X(mult_add_fused, "LAMP_MULT_ADD_FUSED", BOOL, 1, 0, "x * scale + residual in one pass (0: mult then add)")                             \
  X(attention_as_written_for_cuda, "LAMP_ATTENTION_AS_WRITTEN_FOR_CUDA", BOOL, 0, 0, "multi-head attention as the reference's op chain instead of the fused kernels") \
  X(recurrent_fused, "LAMP_RECURRENT_FUSED", BOOL, 1, 0, "RNN / GRU / LSTM as one node per sequence with fused cell kernels (0: the fold over time steps)") \
  X(fuse_qkv, "LAMP_FUSE_QKV", BOOL, 1, 0, "self-attention's three projections as one product (0: three)")                                \
  X(host_stream_side, "LAMP_HOST_STREAM_SIDE", BOOL, 0, 0, "batch streams gather on a side stream instead of the consumer's")             \
  /* tensors and indexing (core/tensor.hip, kernels/index.hip) */                                                                         \
  X(pinned_cache_mb, "LAMP_PINNED_CACHE_MB", INT, 2048, 0, "upper bound of the cache of freed pinned host buffers, MiB")                  \
  X(pinned_gather_wgs, "LAMP_PINNED_GATHER_WGS", INT, 48, 1, "workgroups of a gather that reads pinned host memory")                      \
  /* attention and nearest neighbours */                                                                                                  \
  X(flash_attention, "LAMP_FLASH_ATTENTION", BOOL, 1, 0, "the flash attention kernels, forward and backward")                             \
  X(small_attention, "LAMP_SMALL_ATTENTION", BOOL, 1, 0, "the short-sequence attention kernels")                                          \
  X(knn_fused, "LAMP_KNN_FUSED", BOOL, 1, 0, "the fused distance + top-k nearest-neighbour kernel")                                       \
  X(knn_split, "LAMP_KNN_SPLIT", INT, -1, SW_NO_CLAMP, "f16-plane k-NN filter: 0 off, 1 where it pays, 2 forced; negative: the mode set through the API") \
  X(knn_split_planes, "LAMP_KNN_SPLIT_PLANES", INT, 0, SW_NO_CLAMP, "f16 planes per coordinate of that filter: 3, anything else 2")      \
  X(umap_pairs2, "LAMP_UMAP_PAIRS2", BOOL, 1, 0, "the UMAP loss's two-dimensional pair kernel")                                            \
  /* GEMM (kernels/gemm.hip) */                                                                                                           \
  X(gemm_shape_tags, "LAMP_GEMM_SHAPE_TAGS", BOOL, 0, 0, "profiling aid: one kernel-timer class per GEMM shape and layout")               \
  X(gemm_splitk, "LAMP_GEMM_SPLITK", BOOL, 1, 0, "split-K for products with few output tiles (bf16 and f32 / f64)")                       \
  X(gemm_tail_split, "LAMP_GEMM_TAIL_SPLIT", BOOL, 1, 0, "an almost empty last round of 256 x 256 tiles becomes a second, split-K product") \
  X(gemm_fp_split_wgs, "LAMP_GEMM_FP_SPLIT_WGS", INT, 512, 1, "workgroups an f32 / f64 split-K product aims at")                          \
  /* batch norm backward (kernels/norm.hip) */                                                                                            \
  X(bn_fused_bwd, "LAMP_BN_FUSED_BWD", BOOL, 1, 0, "one-pass batch-norm backward (workgroups exchange their sums) where no mode is set through the API") \
  X(bn_fused_fp, "LAMP_BN_FUSED_FP", BOOL, 1, 0, "... its f32 / f64 form")                                                               \
  X(bn_fused_np_mask, "LAMP_BN_FUSED_NP_MASK", INT, 24, SW_NO_CLAMP, "bit mask of packets per thread (1 .. 16) at which the one-pass form runs") \
  X(bn_fused_per_cu, "LAMP_BN_FUSED_PER_CU", INT, 1, 1, "workgroups per CU the one-pass form aims at first")                              \
  X(bn_fused_small_bytes, "LAMP_BN_FUSED_SMALL_BYTES", INT, (4 << 20) + 1, SW_NO_CLAMP, "bf16 activations below this many bytes take the one-pass form whatever the mask") \
  /* convolutions: small, f32 / f64 implicit GEMM, narrow (conv_small.hip, conv_igemm_f32.hip, conv_narrow.hip) */                        \
  X(conv_small2, "LAMP_CONV_SMALL2", BOOL, 1, 0, "the small-map direct convolution kernels (second generation)")                          \
  X(conv_small2_wgrad, "LAMP_CONV_SMALL2_WGRAD", BOOL, 1, 0, "... their weight gradient")                                                 \
  X(igemm_f32, "LAMP_IGEMM_F32", BOOL, 1, 0, "implicit-GEMM convolution for f32")                                                          \
  X(igemm_f64, "LAMP_IGEMM_F64", BOOL, 1, 0, "implicit-GEMM convolution for f64")                                                          \
  X(conv_bn_stats, "LAMP_CONV_BN_STATS", BOOL, 1, 0, "forward convolutions hand per-image batch-norm statistics of their output on")     \
  X(ncv_bn_stats, "LAMP_NCV_BN_STATS", BOOL, 1, 0, "... the narrow kernels' alone (needs LAMP_CONV_BN_STATS on as well)")                 \
  X(ncv_dgrad_parity, "LAMP_NCV_DGRAD_PARITY", BOOL, 1, 0, "narrow stride-2 pair input gradient: super-tiles by row parity (0: the plain form)") \
  X(pack_cache, "LAMP_PACK_CACHE", BOOL, 1, 0, "packed filter images are cached per parameter and storage version (all four packing backends: core/pack_cache.h)") \
  X(pack_after_step, "LAMP_PACK_AFTER_STEP", BOOL, 1, 0, "the optimiser repacks every cached filter image of all four backends in place (0: lazily at first use)") \
  /* bf16 implicit GEMM, forward and input gradient (kernels/conv_igemm.hip: ig_form) */                                                  \
  X(ig_small_d, "LAMP_IG_SMALL_D", BOOL, 1, 0, "the eight-image kernel for at most 64 output channels too")                               \
  X(ig_w8, "LAMP_IG_W8", BOOL, 1, 0, "two-image 128-row kernel: eight waves per image pair at one workgroup per CU or fewer (0: four)")  \
  X(ig_one_image, "LAMP_IG_ONE_IMAGE", BOOL, 1, 0, "... one image per workgroup at one image per CU or fewer (0: pairs)")                 \
  X(ig_bwd_pair, "LAMP_IG_BWD_PAIR", BOOL, 1, 0, "a wide block's short-K entry pair: input gradient and both weight gradients from one eight-image launch (0: the two pair calls)") \
  X(ig_fwd_pair, "LAMP_IG_FWD_PAIR", BOOL, 1, 0, "a wide block's short-K entry pair, forward: the barrier-free eight-image kernel with both filters resident in LDS (0: the eight-image kernel's sibling form)") \
  /* bf16 implicit GEMM, weight gradient */                                                                                               \
  X(wgrad_group, "LAMP_WGRAD_GROUP", BOOL, 1, 0, "two layers' eight-wave weight gradients parked and launched as one (0: every layer at once)") \
  X(wgrad_min_ips, "LAMP_WGRAD_MIN_IPS", INT, 0, 2, "fewest images per weight-gradient workgroup; unset (0): 2 up to 512 images, 8 above") \
  X(wg8h_dma, "LAMP_WG8H_DMA", BOOL, 1, 0, "eight-wave weight-gradient kernel: dY tiles by LDS-DMA (0: through registers, the bitwise reference of the DMA's hand-counted waits)") \
  X(defer_wgrad_reduce, "LAMP_DEFER_WGRAD_REDUCE", BOOL, 1, 0, "weight-gradient partial sums are reduced in batches, deferred until someone reads them")

// ---- read at EVERY call of sw_now(): a test flips these inside one process -----------------------------------------------------------
#define LAMP_SWITCHES_PER_CALL(X)                                                                                                         \
  X(ig_variant, "LAMP_IG_VARIANT", LETTER, 0, 0, "bf16 implicit GEMM kernel form: b two-image 128-row, d eight-image at any batch; unset or any other letter: by geometry") \
  X(ig_ktail, "LAMP_IG_KTAIL", BOOL, 1, 0, "a 3x3's 1 .. 8 channels beyond the last whole K chunk from their own packed image (0: the padded chunk)") \
  X(knn_split_dbg, "LAMP_KNN_SPLIT_DBG", INT, 0, SW_NO_CLAMP, "3: the k-NN filter's kernel counts visits, candidates and selection cycles per wave and prints them")

using SwType_BOOL = bool;
using SwType_INT = int64_t;
using SwType_LETTER = char;
#define LAMP_SWITCH_MEMBER(member, name, kind, dflt, lo, doc) SwType_##kind member;
struct Switches { LAMP_SWITCHES_ONCE(LAMP_SWITCH_MEMBER) };
struct SwitchesNow { LAMP_SWITCHES_PER_CALL(LAMP_SWITCH_MEMBER) };
#undef LAMP_SWITCH_MEMBER

const Switches& sw();       // filled once, thread-safe
SwitchesNow sw_now();       // read now

}  // namespace lamp
