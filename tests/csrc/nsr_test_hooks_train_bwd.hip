// Test hook of the unit layer under the layer-by-layer training pair's split-fp16 backward (tests/test_gpu_train_bwd_f16_units.py,
// reference: tests/train_bwd_ref.py): the launchers of csrc/nsr_train_bwd_f16.hip alone on caller-supplied matrices -- the
// transposed split copy, the range word, the input gradient and the weight gradient.  The wrappers marshal arguments, refuse
// null pointers, the misalignments the kernels' 16-byte accesses cannot take and the shapes the launchers are not built for,
// and do no arithmetic; there is no kernel here.
#include "nsr_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

namespace {
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
}  // namespace

// halves: 2 * rows * cols halves (hi, then lo): the transposed split copy of w (rows x cols, row stride ldw)
NSR_TEST_API int nsr_test_split_f16_t(const float* w, int rows, int cols, int ldw, unsigned short* halves, void* stream) {
  if (!w || !halves || rows < 1 || cols < 1 || ldw < cols || !al16(halves)) return NSR_ERR_INVALID_ARG;
  return nsr::split_f16_t(nsr_stream(stream), w, rows, cols, ldw, halves, halves + (int64_t)rows * cols);
}

NSR_TEST_API int nsr_test_absmax_bits(const float* src, int64_t ld, int64_t P, int col0, int cols, unsigned* word, void* stream) {
  if (!src || !word || P < 1 || cols < 1 || col0 < 0 || ld < col0 + cols || !al4(word)) return NSR_ERR_INVALID_ARG;
  return nsr::absmax_bits(nsr_stream(stream), src, ld, P, col0, cols, word);
}

// wt: rows [0, N) of a transposed split copy, K halves per row used, row stride ldwt; its lo halves lo_off halves behind
NSR_TEST_API int nsr_test_dgrad_f16x3(const float* dy, int64_t lddy, int K, const unsigned short* wt, int64_t lo_off, int ldwt,
                                      const float* mask, int64_t ldm, float* dx, int64_t lddx, int64_t P, int N, float* col_tiles,
                                      unsigned* out_max, void* stream) {
  if (!dy || !wt || !dx || P < 1 || K < 32 || N < 32 || lddy < K || ldwt < K || lddx < N || (mask && ldm < N) || lo_off < 1)
    return NSR_ERR_INVALID_ARG;
  if (!al16(dy) || !al16(wt) || !al16(wt + lo_off) || !al4(dx) || !al4(mask) || !al4(col_tiles) || !al4(out_max)) return NSR_ERR_INVALID_ARG;
  return nsr::dgrad_f16x3(nsr_stream(stream), dy, lddy, K, wt, wt + lo_off, ldwt, mask, ldm, dx, lddx, P, N, col_tiles, out_max);
}

NSR_TEST_API int64_t nsr_test_bwd_f16_slice_len(int64_t P, int splits) {
  if (P < 1 || splits < 1) return -1;
  return nsr::bwd_f16_slice_len(P, splits);
}
NSR_TEST_API int nsr_test_n_splits(int64_t P) { return nsr::n_splits(P); }

NSR_TEST_API int nsr_test_wgrad_f16x3(const float* dy, int64_t lddy, int M, const float* x, int64_t ldx, int N, int64_t P,
                                      const unsigned* max_bits, float* partial, int splits, int64_t stride, void* stream) {
  if (!dy || !x || !max_bits || !partial || P < 1 || M < 32 || N < 32 || lddy < M || ldx < N || splits < 1 || stride < (int64_t)M * N)
    return NSR_ERR_INVALID_ARG;
  if (!al16(dy) || !al16(x) || !al4(max_bits) || !al4(partial)) return NSR_ERR_INVALID_ARG;
  return nsr::wgrad_f16x3(nsr_stream(stream), dy, lddy, M, x, ldx, N, P, max_bits, partial, splits, stride);
}
