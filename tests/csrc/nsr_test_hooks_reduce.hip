// Test hooks of the unit layer over the gradient reduction and placement kernels of the training step
// (tests/test_gpu_train_reduce_units.py, test_gpu_train_finish_jobs.py, test_gpu_chain_weight_grads.py; reference:
// tests/train_reduce_ref.py): the launchers of csrc/nsr_train_work.h that nsr_train_gemm.hip (layer-by-layer path) and
// nsr_train_wgrad.hip (chain path) define, and chain_weight_grads as a whole.  One entry per launcher.  Like
// nsr_test_hooks_heads.hip the wrappers marshal arguments and do no arithmetic; there is no kernel here.
#include "nsr_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

NSR_TEST_API int nsr_test_place(float* dst, int dst_ld, int r0, int c0, const float* src, int src_ld, int rows, int cols, int col0,
                                int transpose, void* stream) {
  if (!dst || !src) return NSR_ERR_INVALID_ARG;
  return nsr::place(nsr_stream(stream), dst, dst_ld, r0, c0, src, src_ld, rows, cols, col0, transpose);
}

NSR_TEST_API int nsr_test_scatter_heads(const float* d4, int64_t P, float* drgb, float* gsig, int64_t ldg, void* stream) {
  if (!d4 || !drgb || !gsig) return NSR_ERR_INVALID_ARG;
  return nsr::scatter_heads(nsr_stream(stream), d4, P, drgb, gsig, ldg);
}

NSR_TEST_API int nsr_test_colsum(const float* src, int64_t ld, int64_t P, int col0, int cols, float* dst, int accumulate,
                                 float* scratch, void* stream) {
  if (!src || !dst || !scratch) return NSR_ERR_INVALID_ARG;
  return nsr::colsum(nsr_stream(stream), src, ld, P, col0, cols, dst, accumulate, scratch);
}

// col_tiles: n_tiles * N floats, then the launcher's scratch of 64 * N doubles
NSR_TEST_API int nsr_test_tile_sums(float* col_tiles, int64_t n_tiles, int N, int n_bias, float* bias_grad, int acc, void* stream) {
  if (!col_tiles || !bias_grad) return NSR_ERR_INVALID_ARG;
  return nsr::tile_sums(nsr_stream(stream), col_tiles, n_tiles, N, n_bias, bias_grad, acc);
}

NSR_TEST_API int nsr_test_reduce_place(float* dst, int dst_ld, int dc0, int rows, int cols, const float* partial, int splits, int p_ld,
                                       int pr0, int pc0, int accumulate, float scale, int64_t stride, void* stream) {
  if (!dst || !partial) return NSR_ERR_INVALID_ARG;
  return nsr::reduce_place(nsr_stream(stream), dst, dst_ld, dc0, rows, cols, partial, splits, p_ld, pr0, pc0, accumulate, scale, stride);
}

NSR_TEST_API int nsr_test_panel_wsums(int R, int NW, const void* panel, int64_t P, const float* w, int w_stride, float* partial,
                                      int* slices, void* stream) {
  if (!panel || !w || !partial || !slices) return NSR_ERR_INVALID_ARG;
  return nsr::panel_wsums(nsr_stream(stream), R, NW, static_cast<const char*>(panel), P, w, w_stride, partial, slices);
}

NSR_TEST_API int nsr_test_finish_jobs(const nsr::FinishJob* jobs, int n, void* stream) {
  return nsr::finish_jobs(nsr_stream(stream), jobs, n);
}

// the Work fields chain_weight_grads reads (csrc/nsr_train_work.h) and its two scratch areas: slots = kChainSlots x n_splits(P) x
// 256 x 256 floats, row_part = kChainRowSlots x n_splits(P) x 256 floats; g: the 24 gradient tensors
NSR_TEST_API int nsr_test_chain_weight_grads(void* dpan, void* zpan, unsigned* gmax, float* pscale, float* d4, float* bias_part,
                                             float* slots, float* row_part, int64_t P, int64_t n_rays, float* const* g, int acc,
                                             void* stream) {
  if (!dpan || !zpan || !gmax || !pscale || !d4 || !bias_part || !slots || !row_part || !g) return NSR_ERR_INVALID_ARG;
  for (int t = 0; t < 24; ++t)
    if (!g[t]) return NSR_ERR_INVALID_ARG;
  nsr::Work k{};
  k.dpan = static_cast<char*>(dpan);
  k.kept.zpan = static_cast<char*>(zpan);
  k.gmax = gmax;
  k.pscale = pscale;
  k.d4 = d4;
  k.bias_part = bias_part;
  k.slots = slots;
  k.row_part = row_part;
  return nsr::chain_weight_grads(nsr_stream(stream), k, P, n_rays, g, acc);
}

// the sizes of the two scratch areas above, in floats: out[0] = slots, out[1] = row_part
NSR_TEST_API int nsr_test_chain_weight_grads_scratch(int64_t P, int64_t* out) {
  if (!out) return NSR_ERR_INVALID_ARG;
  const int64_t sp = nsr::n_splits(P);
  out[0] = (int64_t)nsr::kChainSlots * sp * 256 * 256;
  out[1] = (int64_t)nsr::kChainRowSlots * sp * 256;
  return NSR_OK;
}
