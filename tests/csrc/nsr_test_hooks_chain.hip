// Test hooks of the backward-chain unit layer (tests/test_gpu_chain_units.py, reference: tests/chain_ref.py): the internal entry
// points of csrc/nsr_train_chain.h -- the transposed weight stream's packer, the chain launch for every term setting, and the
// three size queries a caller needs to carve its buffers.  Like nsr_test_hooks.hip the wrappers marshal arguments and do no
// arithmetic; there is no kernel here.
#include "nsr_train_chain.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

// w: HOST array of NSR_N_STATE_TENSORS device pointers (state_dict order); terms: 1, 2, 3 or 12
NSR_TEST_API int nsr_test_chain_bwd_pack(const float* const* w, void* packed_dev, int stop_grad, int terms, void* stream) {
  if (!w || !packed_dev) return NSR_ERR_INVALID_ARG;
  return nsr_chain_bwd_pack(w, packed_dev, stop_grad, terms, stream);
}

NSR_TEST_API int nsr_test_chain_bwd(const void* packed, const unsigned* sgn, void* dpan, const float* d_rgb, int d_rgb_stride,
                                    const float* d_sigma, int d_sigma_stride, int64_t P, unsigned* gmax, float* pscale, int terms,
                                    int gmax_is_zero, void* stream) {
  if (!packed || !sgn || !dpan || !d_rgb || !d_sigma || !gmax || !pscale) return NSR_ERR_INVALID_ARG;
  return nsr_chain_bwd(packed, sgn, dpan, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, P, gmax, pscale, terms, gmax_is_zero, stream);
}

NSR_TEST_API int64_t nsr_test_chain_bwd_packed_bytes(void) { return (int64_t)nsr_chain_bwd_packed_bytes(); }

NSR_TEST_API int64_t nsr_test_train_panel_bytes(int64_t P) { return nsr_f16x3_train_panel_bytes(P); }

NSR_TEST_API int64_t nsr_test_train_sign_words(int64_t P) { return nsr_f16x3_train_sign_words(P); }
