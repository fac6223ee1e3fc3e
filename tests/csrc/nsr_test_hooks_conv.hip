// Test hooks of the convolution unit layer (tests/test_gpu_conv_units.py, tests/test_conv_units_cpu.py): the kernel choice of
// gemm_f16x3 as a value, and the explicit im2col of nsr_refine_conv.h on its own.  Like nsr_test_hooks.hip the wrappers marshal
// arguments and do no arithmetic; the convolution kernels themselves are reached through nsr_test_gemm_f16x3 there.
#include "nsr_refine_conv.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

// nsr::GemmF16Route of the launch gemm_f16x3 would make, or the negative status it would return.  Host arithmetic only: the
// pointers are tested for null and alignment and never followed, no device is needed.
NSR_TEST_API int nsr_test_gemm_f16x3_route(const nsr::GemmF16Args* a) {
  if (!a) return NSR_ERR_INVALID_ARG;
  return nsr::gemm_f16x3_route(*a);
}

// col (n_img * Ho * Wo, kp) = im2col of src, launched as nsr_refine.hip::conv launches it (one thread per row and column quad).
// nchw != 0: src is (n_img, cin, Hs, Ws) and ld is unused; else NHWC rows of ld floats, channels [0, cin) of each.
NSR_TEST_API int nsr_test_im2col(const float* src, int nchw, int64_t ld, int cin, int n_img, int Hs, int Ws, int stride, int up, int Ho,
                                 int Wo, int kp, float* col, void* stream) {
  if (!src || !col || cin <= 0 || n_img <= 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0 || stride <= 0 || kp < 9 * cin || (kp % 4))
    return NSR_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(col) & 15) || (!nchw && (cin % 4) == 0 && ((ld % 4) || (reinterpret_cast<uintptr_t>(src) & 15))))
    return NSR_ERR_INVALID_ARG;
  const int64_t total = (int64_t)n_img * Ho * Wo * (kp / 4);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (nchw) hipLaunchKernelGGL(im2col_kernel<true>, grid, block, 0, nsr_stream(stream), src, (int64_t)0, cin, n_img, Hs, Ws, stride, up, Ho, Wo, kp, col);
  else hipLaunchKernelGGL(im2col_kernel<false>, grid, block, 0, nsr_stream(stream), src, ld, cin, n_img, Hs, Ws, stride, up, Ho, Wo, kp, col);
  if (hipGetLastError() != hipSuccess) return NSR_ERR_LAUNCH;
  return NSR_OK;
}
