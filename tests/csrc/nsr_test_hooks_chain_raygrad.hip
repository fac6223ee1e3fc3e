// Test hooks of the unit layer over the chain path's ray gradient (tests/test_gpu_chain_ray_grad_units.py; reference:
// tests/chain_ray_grads_ref.py): the launchers nsr::raygrad_f16_pack and nsr::raygrad_f16 of csrc/nsr_train_work.h, defined in
// nsr_train_raygrad_f16.hip.  Like the other hook files the wrappers marshal arguments and do no arithmetic; there is no kernel here.
#include "nsr_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

// floats of one network's packed weight columns
NSR_TEST_API int64_t nsr_test_chain_raygrad_image_floats(void) { return nsr::kRayGradImageFloats; }

// w_coarse / w_fine: HOST arrays of 24 DEVICE pointers (state_dict order; tensors 0, 8 and 18 are read)
NSR_TEST_API int nsr_test_chain_raygrad_pack(const float* const* w_coarse, float* img_coarse, const float* const* w_fine,
                                             float* img_fine, void* stream) {
  return nsr::raygrad_f16_pack(nsr_stream(stream), w_coarse, img_coarse, w_fine, img_fine);
}

NSR_TEST_API int nsr_test_chain_raygrad(const float* img, const void* dpan, const float* pscale, const float* rays, int ray_stride,
                                        const float* z, int64_t R, int N, int stop_grad, float* g_x, float* g_dv, float* g_rays,
                                        int acc, void* stream) {
  return nsr::raygrad_f16(nsr_stream(stream), img, static_cast<const char*>(dpan), pscale, rays, ray_stride, z, R, N, stop_grad, g_x,
                          g_dv, g_rays, acc);
}
