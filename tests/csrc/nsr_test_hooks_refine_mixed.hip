// Test hooks of the unit layer under the refinement network's split-fp16 training precision
// (tests/test_gpu_refine_mixed_units.py, reference: tests/refine_mixed_ref.py): the four launchers of
// csrc/nsr_refine_train_work.h that site_forward / site_backward call at NSR_F16X3.  One entry per launcher; the wrappers
// marshal arguments, refuse null pointers, the misalignments the kernels' 16-byte accesses cannot take and the shapes the
// launchers are not built for, and do no arithmetic; there is no kernel here.
#include "nsr_refine_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

namespace {
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
}  // namespace

// packed: pack_conv_kernel's f16x3 layout ([hi (np x 9 cin)] [lo] halves, np bias floats)
NSR_TEST_API int nsr_test_refine_conv_f16x3(const float* src, int64_t lds, int cin, int n_img, int Hs, int Ws, int stride, int up,
                                            const float* packed, int np, int cout, int act, float* dst, int64_t ld, void* stream) {
  if (!src || !packed || !dst || cin < 32 || (cin % 32) || lds < cin || (lds & 3) || n_img < 1 || Hs < 1 || Ws < 1 ||
      (stride != 1 && stride != 2) || np < 32 || (np % 32) || cout < 1 || cout > np || ld < cout)
    return NSR_ERR_INVALID_ARG;
  if (!al16(src) || !al16(packed) || !al4(dst)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_conv_f16x3(nsr_stream(stream), src, lds, cin, n_img, Hs, Ws, stride, up, packed, np, cout, act, dst, ld);
}

NSR_TEST_API int nsr_test_refine_flip_pack(const float* w, int cin, int cout, int np, void* dst, void* stream) {
  if (!w || !dst || cin < 1 || cout < 1 || np < cout || !al4(w) || !al4(dst)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_flip_pack(nsr_stream(stream), w, cin, cout, np, static_cast<unsigned short*>(dst));
}

NSR_TEST_API int nsr_test_refine_dgrad_f16x3(const float* dz, int np, const void* packed, int cin, int n_img, int H, int W,
                                             const unsigned* max_bits, float* dst, int64_t ld, void* stream) {
  if (!dz || !packed || !max_bits || !dst || np < 32 || cin < 128 || n_img < 1 || H < 1 || W < 1 || ld < cin) return NSR_ERR_INVALID_ARG;
  if (!al16(dz) || !al16(packed) || !al4(max_bits) || !al4(dst)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_dgrad_f16x3(nsr_stream(stream), dz, np, static_cast<const unsigned short*>(packed), cin, n_img, H, W, max_bits,
                                 dst, ld);
}

NSR_TEST_API int nsr_test_refine_fold2x2(const float* src, int C, int n_img, int Hs, int Ws, float* dst, int64_t ld, void* stream) {
  if (!src || !dst || C < 4 || (C & 3) || n_img < 1 || Hs < 1 || Ws < 1 || ld < C || (ld & 3) || !al16(src) || !al16(dst))
    return NSR_ERR_INVALID_ARG;
  return nsr::refine_fold2x2(nsr_stream(stream), src, C, n_img, Hs, Ws, dst, ld);
}

// dZ writers with the range word (the existing hooks of these launchers pass none)
NSR_TEST_API int nsr_test_refine_bn_bwd_range(const float* z, const float* da, int64_t ldda, const float* stat, const float* gamma,
                                              const float* beta, const float* m, int64_t rows, int C, float* dz, unsigned* max_bits,
                                              void* stream) {
  if (!z || !da || !stat || !gamma || !beta || !m || !dz || !max_bits || rows < 1 || C < 4 || (C & 3) || ldda < C || (ldda & 3))
    return NSR_ERR_INVALID_ARG;
  if (!al16(z) || !al16(da) || !al16(dz) || !al4(stat) || !al4(gamma) || !al4(beta) || !al4(m) || !al4(max_bits)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_bn_bwd(nsr_stream(stream), z, da, ldda, stat, gamma, beta, m, rows, C, dz, max_bits);
}

NSR_TEST_API int nsr_test_refine_tanh_bwd_range(const float* y, const float* g_out, int64_t px_per_img, int64_t rows, float* dz,
                                                unsigned* max_bits, void* stream) {
  if (!y || !g_out || !dz || !max_bits || px_per_img < 1 || rows < 1 || (rows % px_per_img) != 0 || !al4(y) || !al4(g_out) || !al4(dz) ||
      !al4(max_bits))
    return NSR_ERR_INVALID_ARG;
  return nsr::refine_tanh_bwd(nsr_stream(stream), y, g_out, px_per_img, rows, dz, max_bits);
}
