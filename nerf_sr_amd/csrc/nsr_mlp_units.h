// Internal interface of the inference MLP units: the fp32 unit (nsr_mlp.hip), the split-fp16 unit (nsr_mlp_f16.hip) and the
// single 16-bit operand unit (nsr_mlp_h1.hip) on one side, their callers on the other -- the precision dispatcher of the
// public ABI (nsr_api.hip), the training step (nsr_train.hip through nsr_train_chain.h) and the test hooks (tests/csrc/).
// Every function here is declared ONCE, and the defining unit includes this header too: with C linkage the signature is not
// part of the symbol, so only the compiler, seeing declaration and definition together, can tell that they disagree
// (tests/test_internal_interface_cpu.py).  No launcher checks its arguments beyond null weight tensors: that is the
// dispatcher's work, done before anything is enqueued.  Host-only: this header must not reach nsr_lds_dma.h.
#pragma once
#include "nsr_common.h"
#include "nsr_composite.h"   // NsrCompOut

// ---- the precisions of a packed blob -----------------------------------------------------------------------------------------
// (nsr_payload_bytes and nsr_blob_tail: nsr_common.h, next to the tail's layout)
// largest weight magnitude whose operand encoding is still finite: fp16 rounds to inf from 65,520 on
static inline float nsr_weight_limit(int precision) {
  if (precision == NSR_F16X3) return 65519.996f / 64.0f;   // the stream carries 2^6 w (nsr_f16x3_core.h, kWScale)
  if (precision == NSR_F16) return 65519.996f;
  return 3.402823466e38f;
}
// The fused launch (D2 + V1, nsr_render_rays_composited) exists for these sample counts: 128-point tiles of whole rays
// (fp32), ray groups walking N / 32 windows (split fp16).  Everything else -- any other precision, -1 included -- takes the
// network launch followed by the stand-alone compositor and needs the (R, N, 4) raw tensors: the entry point and the
// workspace carve of nsr_forward_rays both ask here.
static inline bool nsr_fused_samples(int precision, int n_samples) {
  if (n_samples == 64 || n_samples == 128) return precision == NSR_FP32 || precision == NSR_F16X3;
  return precision == NSR_F16X3 && (n_samples == 192 || n_samples == 256);
}

// ---- fp32 MFMA (nsr_mlp.hip) ---------------------------------------------------------------------------------------------------
extern "C" NSR_INTERNAL size_t nsr_fp32_packed_bytes(void);
extern "C" NSR_INTERNAL int nsr_fp32_pack(const float* const* w, void* packed_dev, void* stream);
// x (P, 90) embedded rows -> out (P, 4) = (rgb, sigma), or (P) sigma.  tail: the blob's tail (status and option words)
extern "C" NSR_INTERNAL int nsr_fp32_mlp_forward(const void* packed, const float* x, int64_t P, int sigma_only, float* out,
                                                 unsigned* tail, void* stream);
extern "C" NSR_INTERNAL int nsr_fp32_render_rays(const void* packed, const float* rays, int ray_stride, const float* z, int64_t R,
                                                 int N, float* out, unsigned* tail, void* stream);
// network + compositing in one launch, N = 64 or 128; raw (R * N, 4) optional
extern "C" NSR_INTERNAL int nsr_fp32_render_composite(const void* packed, const float* rays, int ray_stride, const float* z,
                                                      int64_t R, int N, float* raw, const NsrCompOut* co, unsigned* tail, void* stream);
// NSR_FLAG_WEIGHT_RANGE into *word if one of the 24 tensors cannot be carried at `precision` (nsr_weight_limit; biases only
// have to be finite); the word is cleared by whoever owns it, in front of this launch
extern "C" NSR_INTERNAL int nsr_check_weights_range(const float* const* w, int precision, unsigned* word, void* stream);
// ... of both networks of a training step in one launch
extern "C" NSR_INTERNAL int nsr_check_weights_range2(const float* const* w0, const float* const* w1, int precision, unsigned* word, void* stream);

// ---- split fp16 (nsr_mlp_f16.hip) -------------------------------------------------------------------------------------------
extern "C" NSR_INTERNAL size_t nsr_f16x3_packed_bytes(void);
// folds xyz_encoding_final into dir_encoding first.  tail: the blob's status word (NSR_FLAG_WEIGHT_RANGE of the folded
// matrix); limit: the weights' range limit
extern "C" NSR_INTERNAL int nsr_f16x3_pack(const float* const* w, void* packed_dev, float limit, unsigned* tail, void* stream);
// both networks of a training step in one launch, unfolded (no tail: the step's blobs are private)
extern "C" NSR_INTERNAL int nsr_f16x3_pack2(const float* const* w0, void* packed0, const float* const* w1, void* packed1, void* stream);
extern "C" NSR_INTERNAL int nsr_f16x3_mlp_forward(const void* packed, const float* x, int64_t P, int sigma_only, float* out,
                                                  unsigned* tail, void* stream);
extern "C" NSR_INTERNAL int nsr_f16x3_render_rays(const void* packed, const float* rays, int ray_stride, const float* z, int64_t R,
                                                  int N, float* out, unsigned* tail, void* stream);
// network + compositing in one launch (N = 64, 128, 192 or 256; early ray termination, co->ert_tau > 0: 64 or 128);
// raw (R * N, 4) optional
extern "C" NSR_INTERNAL int nsr_f16x3_render_composite(const void* packed, const float* rays, int ray_stride, const float* z,
                                                       int64_t R, int N, float* raw, const NsrCompOut* co, unsigned* tail, void* stream);
// the density-only pass of the same launch: depth / opacity / weights, no colours
extern "C" NSR_INTERNAL int nsr_f16x3_render_density(const void* packed, const float* rays, int ray_stride, const float* z,
                                                     int64_t R, int N, const NsrCompOut* co, unsigned* tail, void* stream);
// bytes of one panel set (twelve fp16 panels, see nsr_f16x3_core.h) for P sample points
extern "C" NSR_INTERNAL int64_t nsr_f16x3_train_panel_bytes(int64_t P);
// dwords of the sign panels (one bit per pre-activation) for P sample points
extern "C" NSR_INTERNAL int64_t nsr_f16x3_train_sign_words(int64_t P);
// forward pass of the training step: raw (R N, 4) = (rgb, sigma) + the activation panels; `packed` = nsr_f16x3_pack2 of the
// weights; status: the step's sticky NSR_FLAG_* word (input / activation range, non-finite outputs) or null
extern "C" NSR_INTERNAL int nsr_f16x3_train_forward(const void* packed, const float* rays, int ray_stride, const float* z, int64_t R,
                                                    int N, float* raw, void* pan, unsigned* sgn, unsigned* status, void* stream);

// ---- single 16-bit operand (nsr_mlp_h1.hip); bf = 1: bf16, 0: fp16 ------------------------------------------------------------
extern "C" NSR_INTERNAL size_t nsr_h1_packed_bytes(void);
extern "C" NSR_INTERNAL int nsr_h1_pack(int bf, const float* const* w, void* packed_dev, void* stream);
extern "C" NSR_INTERNAL int nsr_h1_mlp_forward(int bf, const void* packed, const float* x, int64_t P, int sigma_only,
                                               float* out, unsigned* tail, void* stream);
extern "C" NSR_INTERNAL int nsr_h1_render_rays(int bf, const void* packed, const float* rays, int ray_stride,
                                               const float* z, int64_t R, int N, float* out, unsigned* tail, void* stream);
