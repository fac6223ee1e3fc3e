// Test hook (tests/test_gpu_testtime.py), linked into ab/libnsr_testhooks.so like nsr_test_hooks_render.hip, whose wrapper it
// repeats for the sample counts that one refuses: the split-fp16 render + composite launch at 64 / 128 / 192 / 256 samples with
// `skipped`, the device word the kernel adds 1 to for every window (4 rays x 32 samples) it ends after the density head.  The
// counter exists only here: libnsr.so always passes null.  The wrapper marshals arguments and does no arithmetic.
#include <stddef.h>
#include "nsr_mlp_units.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

NSR_TEST_API int nsr_test_f16x3_render_composite_wide(const void* packed, const float* rays, int ray_stride, const float* z, int64_t R,
                                                      int N, int white_bkgd, float* raw, float* comp_rgb, float* depth, float* opacity,
                                                      float* weights, unsigned* skipped, void* stream) {
  if (!packed || !rays || !z || R <= 0 || (N != 64 && N != 128 && N != 192 && N != 256)) return NSR_ERR_INVALID_ARG;
  NsrCompOut co{comp_rgb, depth, opacity, weights, white_bkgd};
  co.skipped = skipped;
  return nsr_f16x3_render_composite(packed, rays, ray_stride, z, R, N, raw, &co, nsr_blob_tail(packed, NSR_F16X3), stream);
}
