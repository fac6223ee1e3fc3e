// Test hooks of the unit layer over what feeds the network's backward (tests/test_gpu_train_heads.py, reference:
// tests/train_heads_ref.py): the launchers of csrc/nsr_train_work.h for the compositing backward, the loss head (lr_loss,
// loss_finish), the density noise and the per-sample gamma.  One entry per launcher.  Like nsr_test_hooks_chain.hip the wrappers
// marshal arguments and do no arithmetic; there is no kernel here.
#include "nsr_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

// gmax, bias_part, g_depth, g_opacity, g_weights may be null
NSR_TEST_API int nsr_test_composite_bwd(const float* rgb4, const float* sigma, const float* z, const float* g_comp, int64_t R, int N,
                                        int flags, float* d4, unsigned* gmax, float* bias_part, const float* g_depth,
                                        const float* g_opacity, const float* g_weights, void* stream) {
  if (!rgb4 || !sigma || !z || !g_comp || !d4) return NSR_ERR_INVALID_ARG;
  return nsr::composite_bwd(nsr_stream(stream), rgb4, sigma, z, g_comp, R, N, flags, d4, gmax, bias_part, g_depth, g_opacity,
                            g_weights);
}

// depth and g_depth may be null
NSR_TEST_API int nsr_test_lr_loss(const float* comp, const float* target, int64_t n_lr, int s2, double scale, float lambda,
                                  float* lr_out, float* g_comp, double* block_sums, float lambda_var, float lambda_dvar, float far,
                                  const float* depth, float* g_depth, void* stream) {
  if (!comp || !target || !lr_out || !g_comp || !block_sums) return NSR_ERR_INVALID_ARG;
  return nsr::lr_loss(nsr_stream(stream), comp, target, n_lr, s2, scale, lambda, lr_out, g_comp, block_sums, lambda_var, lambda_dvar,
                      far, depth, g_depth);
}

// var_losses may be null
NSR_TEST_API int nsr_test_loss_finish(const double* block_sums, int n, double scale, float lambda, float* losses, int slot,
                                      double* carry, float lambda_var, float lambda_dvar, float* var_losses, void* stream) {
  if (!block_sums || !losses || !carry) return NSR_ERR_INVALID_ARG;
  return nsr::loss_finish(nsr_stream(stream), block_sums, n, scale, lambda, losses, slot, carry, lambda_var, lambda_dvar, var_losses);
}

// noise may be null
NSR_TEST_API int nsr_test_sigma_noise(const float* sigma, int sigma_stride, const float* noise, float std_, int64_t P, float* out,
                                      void* stream) {
  if (!sigma || !out) return NSR_ERR_INVALID_ARG;
  return nsr::sigma_noise(nsr_stream(stream), sigma, sigma_stride, noise, std_, P, out);
}

NSR_TEST_API int nsr_test_gamma_points(float* rgb4, int64_t P, void* stream) {
  if (!rgb4) return NSR_ERR_INVALID_ARG;
  return nsr::gamma_points(nsr_stream(stream), rgb4, P);
}
