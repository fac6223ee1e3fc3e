// Test hooks of the in-kernel positional encodings (tests/test_gpu_encoding.py, reference: tests/encoding_ref.py):
//   nsr_test_sincos               csrc/nsr_common.h's nsr_sincos, one call per element -- the only kernel of this file;
//   nsr_test_encode_arch          the launcher nsr::encode_arch of csrc/nsr_train_work.h (the layer-by-layer training path);
//   nsr_test_f16x3_train_forward  the TRAIN forward of csrc/nsr_train_chain.h with its panels.
// Like nsr_test_hooks_chain.hip the two wrappers marshal arguments and do no arithmetic.
#include <stdint.h>
#include "nsr_train_chain.h"
#include "nsr_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

namespace {

__global__ void __launch_bounds__(256) sincos_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ sn,
                                                     float* __restrict__ cs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) nsr_sincos(x[i], sn[i], cs[i]);
}

}  // namespace

NSR_TEST_API int nsr_test_sincos(const float* x, int64_t n, float* sn, float* cs, void* stream) {
  if (!x || !sn || !cs || n < 0 || n > ((int64_t)1 << 31)) return NSR_ERR_INVALID_ARG;
  if (n == 0) return NSR_OK;
  hipLaunchKernelGGL(sincos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nsr_stream(stream), x, n, sn, cs);
  if (hipGetLastError() != hipSuccess) return NSR_ERR_LAUNCH;
  return NSR_OK;
}

// dst: HOST array of n_dst device pointers, each (P, ld) floats and 16-byte aligned; z may be null under view_dir
NSR_TEST_API int nsr_test_encode_arch(const float* rays, int ray_stride, const float* z, int64_t P, int N, int deg, int view_dir,
                                      float* const* dst, int n_dst, int64_t ld, int n_groups, void* stream) {
  if (!rays || !dst || (!z && !view_dir) || !nsr_ray_stride_ok(ray_stride)) return NSR_ERR_INVALID_ARG;
  if (P <= 0 || N <= 0 || deg < 0 || deg > 16 || n_dst < 1 || n_dst > nsr::kMaxD || n_groups < 1) return NSR_ERR_INVALID_ARG;
  if (ld < 4 * (int64_t)n_groups || (ld % 4) != 0) return NSR_ERR_INVALID_ARG;
  for (int j = 0; j < n_dst; ++j)
    if (!dst[j] || (reinterpret_cast<uintptr_t>(dst[j]) & 15)) return NSR_ERR_INVALID_ARG;
  return nsr::encode_arch(nsr_stream(stream), rays, ray_stride, z, P, N, deg, view_dir, dst, n_dst, ld, n_groups);
}

// packed: the network's f16x3 blob; raw (R N, 4); pan: nsr_test_train_panel_bytes(R N) bytes; sgn: nsr_test_train_sign_words(R N)
// dwords; status: null or four device words laid out like a blob's tail (word 0 the sticky flags, word 1 the colour-head options)
NSR_TEST_API int nsr_test_f16x3_train_forward(const void* packed, const float* rays, int ray_stride, const float* z, int64_t R, int N,
                                              float* raw, void* pan, unsigned* sgn, unsigned* status, void* stream) {
  if (!packed || !rays || !z || !raw || !pan || !sgn || R <= 0 || N <= 0 || !nsr_ray_stride_ok(ray_stride)) return NSR_ERR_INVALID_ARG;
  return nsr_f16x3_train_forward(packed, rays, ray_stride, z, R, N, raw, pan, sgn, status, stream);
}
