// Test hook of the unit layer under the refinement network's implicit split-fp16 weight gradient
// (tests/test_gpu_refine_wgrad_units.py, reference: tests/refine_wgrad_ref.py): the launcher of csrc/nsr_refine_wgrad_f16.hip
// -- kernel and slice-order reduce -- alone on caller-supplied dZ, input, range word and geometry.  The wrappers marshal
// arguments, refuse null pointers, the misalignments the kernel's 16-byte accesses cannot take and the shapes the launcher is
// not built for, and do no arithmetic; there is no kernel here.
#include "nsr_refine_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

namespace {
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
}  // namespace

// slice_len: 0 = the product's own (a function of the shape), otherwise pixels per slice (a multiple of 32): small cases that
// span several slices.  part: part_floats floats of scratch for the slices' partial tiles.
NSR_TEST_API int nsr_test_refine_wgrad_f16x3(const float* dz, int np, int cout, const float* src, int64_t ld, int cin, int n_img, int Hs,
                                             int Ws, int stride, int up, const unsigned* max_bits, float* part, int64_t part_floats,
                                             int acc, float* g, int64_t slice_len, void* stream) {
  if (!dz || !src || !max_bits || !part || !g || np < 32 || (np % 32) || cout < 1 || cout > np || cin < 128 || (cin % 128) || ld < cin ||
      (ld & 3) || n_img < 1 || Hs < 1 || Ws < 1 || (stride != 1 && stride != 2) || part_floats < (int64_t)cout * 9 * cin || slice_len < 0 ||
      (slice_len % 32))
    return NSR_ERR_INVALID_ARG;
  if (!al16(dz) || !al16(src) || !al4(max_bits) || !al4(part) || !al4(g)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_wgrad_f16x3(nsr_stream(stream), dz, np, cout, src, ld, cin, n_img, Hs, Ws, stride, up ? 1 : 0, max_bits, part,
                                 part_floats, acc ? 1 : 0, g, slice_len);
}

NSR_TEST_API int64_t nsr_test_refine_wgrad_slice_len(int cin, int cout, int64_t K) {
  if (cin < 128 || (cin % 128) || cout < 1 || K < 1) return -1;
  return nsr::refine_wgrad_slice_len(cin, cout, K);
}
