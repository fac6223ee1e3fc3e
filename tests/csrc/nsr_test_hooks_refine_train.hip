// Test hooks of the unit layer under the refinement network's train-mode pair (tests/test_gpu_refine_units.py, reference:
// tests/refine_units_ref.py): the launchers of csrc/nsr_refine_train_work.h, the ones site_forward / site_backward call.  One
// entry per launcher.  Like nsr_test_hooks_heads.hip the wrappers marshal arguments, refuse null pointers and the
// misalignments the kernels' float4 accesses cannot take, and do no arithmetic; there is no kernel here.
#include "nsr_refine_train_work.h"

#define NSR_TEST_API extern "C" __attribute__((visibility("default")))

namespace {
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
}  // namespace

// mode 0: x; mode 1: x, stat; mode 2: x, da, stat, gamma, beta.  *nparts_out = the partition count the launcher chose
NSR_TEST_API int nsr_test_refine_col_reduce(int mode, const float* x, int64_t ldx, const float* da, int64_t ldda, const float* stat,
                                            const float* gamma, const float* beta, int64_t rows, int C, float* part, int* nparts_out,
                                            void* stream) {
  if (mode < 0 || mode > 2 || !x || !part || !nparts_out || rows < 1 || C < 1 || ldx < C) return NSR_ERR_INVALID_ARG;
  if (mode >= 1 && !stat) return NSR_ERR_INVALID_ARG;
  if (mode == 2 && (!da || !gamma || !beta || ldda < C)) return NSR_ERR_INVALID_ARG;
  if (!al4(x) || !al4(part) || (da && !al4(da)) || (stat && !al4(stat)) || (gamma && !al4(gamma)) || (beta && !al4(beta)))
    return NSR_ERR_INVALID_ARG;
  nsr::ReduceArgs a{};
  a.x = x; a.ldx = ldx; a.da = da; a.ldda = ldda; a.stat = stat; a.gamma = gamma; a.beta = beta; a.rows = rows; a.C = C; a.part = part;
  const int np = nsr::refine_col_reduce(nsr_stream(stream), mode, a);
  if (np < 0) return np;
  *nparts_out = np;
  return NSR_OK;
}

NSR_TEST_API int nsr_test_refine_reduce_parts(int64_t rows) { return nsr::refine_reduce_parts(rows); }

// run_mean may be null
NSR_TEST_API int nsr_test_refine_fin_mean(const float* part, int nparts, int C, int64_t rows, float momentum, float* stat,
                                          float* run_mean, void* stream) {
  if (!part || !stat || nparts < 1 || C < 1 || rows < 1 || !al4(part) || !al4(stat) || !al4(run_mean)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_fin_mean(nsr_stream(stream), part, nparts, C, rows, momentum, stat, run_mean);
}

// run_var may be null
NSR_TEST_API int nsr_test_refine_fin_var(const float* part, int nparts, int C, int64_t rows, float momentum, float eps, float* stat,
                                         float* run_var, void* stream) {
  if (!part || !stat || nparts < 1 || C < 1 || rows < 1 || !al4(part) || !al4(stat) || !al4(run_var)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_fin_var(nsr_stream(stream), part, nparts, C, rows, momentum, eps, stat, run_var);
}

NSR_TEST_API int nsr_test_refine_fin_bn_bwd(const float* part, int nparts, int C, int64_t rows, int acc, float* g_gamma, float* g_beta,
                                            float* m, void* stream) {
  if (!part || !g_gamma || !g_beta || !m || nparts < 1 || C < 1 || rows < 1) return NSR_ERR_INVALID_ARG;
  if (!al4(part) || !al4(g_gamma) || !al4(g_beta) || !al4(m)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_fin_bn_bwd(nsr_stream(stream), part, nparts, C, rows, acc, g_gamma, g_beta, m);
}

NSR_TEST_API int nsr_test_refine_fin_bias(const float* part, int nparts, int C, int n_valid, int acc, float* g_bias, void* stream) {
  if (!part || !g_bias || nparts < 1 || C < 1 || n_valid < 0 || n_valid > C || !al4(part) || !al4(g_bias)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_fin_bias(nsr_stream(stream), part, nparts, C, n_valid, acc, g_bias);
}

// float4 accesses: every pointer on 16 bytes, C and ld multiples of 4
NSR_TEST_API int nsr_test_refine_bn_relu(const float* z, const float* stat, const float* gamma, const float* beta, int64_t rows, int C,
                                         float* dst, int64_t ld, void* stream) {
  if (!z || !stat || !gamma || !beta || !dst || rows < 1 || C < 4 || (C & 3) || ld < C || (ld & 3)) return NSR_ERR_INVALID_ARG;
  if (!al16(z) || !al16(stat) || !al16(gamma) || !al16(beta) || !al16(dst)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_bn_relu(nsr_stream(stream), z, stat, gamma, beta, rows, C, dst, ld);
}

NSR_TEST_API int nsr_test_refine_bn_bwd(const float* z, const float* da, int64_t ldda, const float* stat, const float* gamma,
                                        const float* beta, const float* m, int64_t rows, int C, float* dz, void* stream) {
  if (!z || !da || !stat || !gamma || !beta || !m || !dz || rows < 1 || C < 4 || (C & 3) || ldda < C || (ldda & 3)) return NSR_ERR_INVALID_ARG;
  if (!al16(z) || !al16(da) || !al16(dz) || !al4(stat) || !al4(gamma) || !al4(beta) || !al4(m)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_bn_bwd(nsr_stream(stream), z, da, ldda, stat, gamma, beta, m, rows, C, dz);
}

NSR_TEST_API int nsr_test_refine_relu_bwd(const float* a, const float* da, int64_t n, float* dz, void* stream) {
  if (!a || !da || !dz || n < 1 || !al4(a) || !al4(da) || !al4(dz)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_relu_bwd(nsr_stream(stream), a, da, n, dz);
}

NSR_TEST_API int nsr_test_refine_tanh_bwd(const float* y, const float* g_out, int64_t px_per_img, int64_t rows, float* dz, void* stream) {
  if (!y || !g_out || !dz || px_per_img < 1 || rows < 1 || (rows % px_per_img) != 0 || !al4(y) || !al4(g_out) || !al4(dz))
    return NSR_ERR_INVALID_ARG;
  return nsr::refine_tanh_bwd(nsr_stream(stream), y, g_out, px_per_img, rows, dz);
}

NSR_TEST_API int nsr_test_refine_max_idx(const float* src, int C, int R, int64_t px_per_img, int B, float* dst, int64_t ld,
                                         unsigned char* win, void* stream) {
  if (!src || !dst || !win || C < 1 || R < 1 || R > 255 || px_per_img < 1 || B < 1 || ld < C || !al4(src) || !al4(dst))
    return NSR_ERR_INVALID_ARG;
  return nsr::refine_max_idx(nsr_stream(stream), src, C, R, px_per_img, B, dst, ld, win);
}

NSR_TEST_API int nsr_test_refine_route(const float* g_max, int64_t ld, const unsigned char* win, int C, int R, int64_t px_per_img, int B,
                                       float* g_fc, void* stream) {
  if (!g_max || !win || !g_fc || C < 1 || R < 1 || R > 255 || px_per_img < 1 || B < 1 || ld < C || !al4(g_max) || !al4(g_fc))
    return NSR_ERR_INVALID_ARG;
  return nsr::refine_route(nsr_stream(stream), g_max, ld, win, C, R, px_per_img, B, g_fc);
}

// float4 accesses: dcol and dst on 16 bytes, kp, cin and ld multiples of 4
NSR_TEST_API int nsr_test_refine_col2im(const float* dcol, int kp, int cin, int n_img, int Hs, int Ws, int stride, int up, int Ho, int Wo,
                                        int acc, float* dst, int64_t ld, void* stream) {
  if (!dcol || !dst || cin < 4 || (cin & 3) || kp < 9 * cin || (kp & 3) || n_img < 1 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 ||
      (stride != 1 && stride != 2) || ld < cin || (ld & 3))
    return NSR_ERR_INVALID_ARG;
  if (!al16(dcol) || !al16(dst)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_col2im(nsr_stream(stream), dcol, kp, cin, n_img, Hs, Ws, stride, up, Ho, Wo, acc, dst, ld);
}

NSR_TEST_API int nsr_test_refine_wgrad_reduce(const float* part, int splits, int64_t split_stride, int kp, int cin, int cout, int acc,
                                              float* g, void* stream) {
  if (!part || !g || splits < 1 || cin < 1 || cout < 1 || kp < 9 * cin || split_stride < (int64_t)cout * kp || !al4(part) || !al4(g))
    return NSR_ERR_INVALID_ARG;
  return nsr::refine_wgrad_reduce(nsr_stream(stream), part, splits, split_stride, kp, cin, cout, acc, g);
}

NSR_TEST_API int nsr_test_refine_fwd_reduce(const float* part, int splits, int64_t split_stride, int np, int cout, const float* bias,
                                            int act, int64_t M, float* dst, int64_t ld, void* stream) {
  if (!part || !bias || !dst || splits < 1 || cout < 1 || np < cout || M < 1 || split_stride < M * np || ld < cout || !al4(part) ||
      !al4(bias) || !al4(dst))
    return NSR_ERR_INVALID_ARG;
  return nsr::refine_fwd_reduce(nsr_stream(stream), part, splits, split_stride, np, cout, bias, act, M, dst, ld);
}

NSR_TEST_API int nsr_test_refine_nhwc3_to_nchw(const float* src, int64_t px_per_img, int B, float* dst, void* stream) {
  if (!src || !dst || px_per_img < 1 || B < 1 || !al4(src) || !al4(dst)) return NSR_ERR_INVALID_ARG;
  return nsr::refine_nhwc3_to_nchw(nsr_stream(stream), src, px_per_img, B, dst);
}
