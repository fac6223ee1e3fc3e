// Test hooks of the unit layer over the two kernels of the gradient with respect to the rays (tests/test_gpu_ray_grad_units.py;
// reference: tests/ray_grads_ref.py): the launchers nsr::encode_bwd and nsr::ray_grad of csrc/nsr_train_work.h, defined in
// nsr_train_gemm.hip.  Like the other hook files the wrappers marshal arguments and do no arithmetic; there is no kernel here.
#include "nsr_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

// src: HOST array of n_src DEVICE pointers; the band table is nsr_posenc_freqs' for (deg, embed)
NSR_TEST_API int nsr_test_encode_bwd(const float* const* src, int n_src, int64_t ld_src, const float* enc, int64_t ld_enc, int64_t P,
                                     int deg, int n_groups, unsigned embed, float* g_x, void* stream) {
  if (!src || !enc || !g_x) return NSR_ERR_INVALID_ARG;
  for (int j = 0; j < n_src && j < nsr::kMaxD; ++j)
    if (!src[j]) return NSR_ERR_INVALID_ARG;
  NsrBands bands;
  NSR_TRY(nsr_bands(deg, embed, bands));
  return nsr::encode_bwd(nsr_stream(stream), src, n_src, ld_src, enc, ld_enc, P, deg, n_groups, embed, &bands, g_x);
}

NSR_TEST_API int nsr_test_ray_grad(const float* g_x, const float* z, int64_t R, int N, const float* g_dir, int64_t ld_dir,
                                   const float* dir_enc, int64_t ld_enc, int deg_dir, unsigned embed, float* g_rays, int stride,
                                   int acc, void* stream) {
  if (!g_x || !z || !g_rays) return NSR_ERR_INVALID_ARG;
  NsrBands bands;
  NSR_TRY(nsr_bands(deg_dir, embed, bands));
  return nsr::ray_grad(nsr_stream(stream), g_x, z, R, N, g_dir, ld_dir, dir_enc, ld_enc, deg_dir, embed, &bands, g_rays, stride, acc);
}
