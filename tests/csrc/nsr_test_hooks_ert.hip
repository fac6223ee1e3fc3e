// Test hook (tests/test_gpu_early_stop.py), linked into ab/libnsr_testhooks.so like nsr_test_hooks_render.hip: the split-fp16
// render + composite launch with early ray termination (the f16x3 route of nsr_render_rays_composited_ert) and BOTH device
// counters of the kernel: `cut`, the windows a terminated group did not run (the public entry point's `windows_cut`), and
// `skipped`, the windows ended after the density head by the empty-window skip, which the public entry points never pass.
// `tau` is the kernel's threshold -ln(eps) itself (0 = option off).  The wrapper marshals arguments and does no arithmetic.
#include <stddef.h>
#include "nsr_mlp_units.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

NSR_TEST_API int nsr_test_f16x3_render_composite_ert(const void* packed, const float* rays, int ray_stride, const float* z, int64_t R,
                                                     int N, int white_bkgd, float tau, float* comp_rgb, float* depth, float* opacity,
                                                     float* weights, unsigned* skipped, unsigned* cut, void* stream) {
  if (!packed || !rays || !z || R <= 0 || (N != 64 && N != 128) || !(tau >= 0.0f)) return NSR_ERR_INVALID_ARG;
  NsrCompOut co{comp_rgb, depth, opacity, weights, white_bkgd};
  co.skipped = skipped;
  co.ert_tau = tau;
  co.cut = cut;
  return nsr_f16x3_render_composite(packed, rays, ray_stride, z, R, N, nullptr, &co, nsr_blob_tail(packed, NSR_F16X3), stream);
}
