// Backward chain kernels of the training step (internal; nsr_train_chain.hip).  The forward side of the chain path -- the
// TRAIN instantiation of the inference kernel, its packer and the range check -- is declared with the inference units:
#pragma once
#include "nsr_mlp_units.h"

// backward chain: transposed weight stream, then d(rgb_pre) (P, stride) / d(sigma) (P, stride) -> gradient panels;
// gmax[10] (device): float bits of the largest TRUE magnitude of each gradient panel (zeroed, then atomicMax);
// pscale (10, ceil(P / 128) * 128): per panel and point the power of two that turns the stored fp16 values into true gradients
extern "C" NSR_INTERNAL size_t nsr_chain_bwd_packed_bytes(void);
// terms (round 6): MFMAs per product of the chain -- 3 = W_hi g_hi + W_hi g_lo + W_lo g_hi (fp32-grade), 2 = W_hi g_hi + W_lo g_hi,
// 1 = W_hi g_hi (the stream then carries the hi pieces only); pack and run must agree
extern "C" NSR_INTERNAL int nsr_chain_bwd_pack(const float* const* w, void* packed_dev, int stop_grad, int terms, void* stream);
extern "C" NSR_INTERNAL int nsr_chain_bwd(const void* packed, const unsigned* sgn, void* dpan, const float* d_rgb, int d_rgb_stride,
                                          const float* d_sigma, int d_sigma_stride, int64_t P, unsigned* gmax,
                                          float* pscale, int terms, int gmax_is_zero, void* stream);
// round 6, the step's launch count: both networks per launch; the backward pack also clears `n_zero` doubles at `zero` and
// writes `value` to `word` (the step's loss carries and its option word: two memset launches less)
extern "C" NSR_INTERNAL int nsr_chain_bwd_pack2(const float* const* w0, void* packed0, const float* const* w1, void* packed1, int stop_grad,
                                                int terms, double* zero, int n_zero, unsigned* word, unsigned value, void* stream);
