// Host launchers of the small kernels of the refinement network's train-mode pair (internal; defined in nsr_refine_train.hip
// next to the kernels, which stay in its anonymous namespace).  site_forward, site_backward and the max / route call sites go
// through these, and so does the unit layer (tests/csrc/nsr_test_hooks_refine_train.hip, tests/test_gpu_refine_units.py): a
// test runs the grid sizing and the partition count the product runs.  Every launcher returns NSR_OK or NSR_ERR_LAUNCH
// (refine_col_reduce: the partition count, or a negative status); none validates its arguments.
#pragma once
#include "nsr_common.h"

namespace nsr {

constexpr int kRefineMaxParts = 256;   // row partitions of a per-channel reduction

// Per-channel sums over the rows of a (rows x C) matrix, partition `blockIdx.y` of `nparts`: part[(v * nparts + p) * C + c].
//   MODE 0: sum of x                      (x: ld = ldx)
//   MODE 1: sum of (x - mean[c])^2
//   MODE 2: v = 0: sum of dy, v = 1: sum of dy * xhat, dy = dA * [bn_act(x) > 0]   (BatchNorm backward)
struct ReduceArgs {
  const float* x; int64_t ldx;
  const float* da; int64_t ldda;
  const float* stat;                 // mean[C], rstd[C]
  const float *gamma, *beta;
  int64_t rows; int C, nparts;
  float* part;
};
// partitions of 64 rows, at most kRefineMaxParts of them (then ceil(rows / kRefineMaxParts) rows each)
static inline int refine_reduce_parts(int64_t rows) {
  const int64_t want = (rows + 63) / 64;
  return (int)(want > kRefineMaxParts ? kRefineMaxParts : want);
}
// sets a.nparts = refine_reduce_parts(a.rows), launches mode 0 / 1 / 2 and returns the partition count (negative: a status)
NSR_INTERNAL int refine_col_reduce(hipStream_t st, int mode, ReduceArgs a);
// the partitions in order, in double -> stat[c] = mean; run_mean (may be null) moves towards it
NSR_INTERNAL int refine_fin_mean(hipStream_t st, const float* part, int nparts, int C, int64_t rows, float momentum, float* stat,
                                 float* run_mean);
// ... -> stat[C + c] = rstd from the biased variance; run_var (may be null) moves towards the unbiased one
NSR_INTERNAL int refine_fin_var(hipStream_t st, const float* part, int nparts, int C, int64_t rows, float momentum, float eps,
                                float* stat, float* run_var);
// sums of mode 2 -> d gamma, d beta (added to what is there if `acc`), m[c] = sum dy / n, m[C + c] = sum dy xhat / n
NSR_INTERNAL int refine_fin_bn_bwd(hipStream_t st, const float* part, int nparts, int C, int64_t rows, int acc, float* g_gamma,
                                   float* g_beta, float* m);
// column sums (mode 0) -> elements [0, n_valid) of the bias gradient
NSR_INTERNAL int refine_fin_bias(hipStream_t st, const float* part, int nparts, int C, int n_valid, int acc, float* g_bias);

// dst[r][c] = relu(gamma (z - mean) rstd + beta); z dense (rows x C), dst with row stride ld; C % 4 == 0
NSR_INTERNAL int refine_bn_relu(hipStream_t st, const float* z, const float* stat, const float* gamma, const float* beta, int64_t rows,
                                int C, float* dst, int64_t ld);
// dZ = gamma rstd (dy - m[c] - xhat m[C + c]), dy = dA [bn_act(z) > 0]; z, dz dense, dA with row stride ldda; C % 4 == 0
NSR_INTERNAL int refine_bn_bwd(hipStream_t st, const float* z, const float* da, int64_t ldda, const float* stat, const float* gamma,
                               const float* beta, const float* m, int64_t rows, int C, float* dz, unsigned* max_bits = nullptr);
// dz[i] = a[i] > 0 ? da[i] : 0 over n elements
NSR_INTERNAL int refine_relu_bwd(hipStream_t st, const float* a, const float* da, int64_t n, float* dz, unsigned* max_bits = nullptr);
// dz (rows x 32): columns 0..2 = g_out (NCHW, px_per_img pixels per image) (1 - y^2), y (rows x 3); columns 3..31 zero
NSR_INTERNAL int refine_tanh_bwd(hipStream_t st, const float* y, const float* g_out, int64_t px_per_img, int64_t rows, float* dz,
                                 unsigned* max_bits = nullptr);
// `max_bits` of the three above (null: off): the RANGE WORD of the split-fp16 input gradient.  The kernel raises *max_bits to the
// float bits of the largest |dz| it wrote (sign cleared; integer atomicMax on the bit pattern, one per wave: the result does not
// depend on the order, and a NaN or an infinity ends above every finite value).  The caller zeroes the word first.

// dst[(b, px)][c] = max over r of src[(b R + r, px)][c] (row stride ld), win = the first r that reaches it (NaN wins)
NSR_INTERNAL int refine_max_idx(hipStream_t st, const float* src, int C, int R, int64_t px_per_img, int B, float* dst, int64_t ld,
                                unsigned char* win);
// g_fc[(b R + r, px)][c] = (win == r) ? g_max[(b, px)][c] : 0; every element of g_fc is written
NSR_INTERNAL int refine_route(hipStream_t st, const float* g_max, int64_t ld, const unsigned char* win, int C, int R,
                              int64_t px_per_img, int B, float* g_fc);

// gather-form col2im of a 3x3 / pad 1 convolution (optionally behind a nearest x2 upsample): dst[(img, sy, sx)][c] (row stride
// ld) = or += the entries of dcol (n_img Ho Wo, kp) that im2col copied from that pixel; cin % 4 == 0
NSR_INTERNAL int refine_col2im(hipStream_t st, const float* dcol, int kp, int cin, int n_img, int Hs, int Ws, int stride, int up,
                               int Ho, int Wo, int acc, float* dst, int64_t ld);
// split-K partials (splits, >= cout rows x kp, tap-major) in order -> g[n][c][tap] (Cout, Cin, 3, 3), = or +=
NSR_INTERNAL int refine_wgrad_reduce(hipStream_t st, const float* part, int splits, int64_t split_stride, int kp, int cin, int cout,
                                     int acc, float* g);
// forward split-K partials (splits, M x np) in order in double, + bias, activation (GemmAct) -> dst[m][n], n < cout
NSR_INTERNAL int refine_fwd_reduce(hipStream_t st, const float* part, int splits, int64_t split_stride, int np, int cout,
                                   const float* bias, int act, int64_t M, float* dst, int64_t ld);
// ---- NSR_F16X3 (nsr_refine_dgrad_f16.hip): the split-fp16 MFMA with implicit gather, forward and input gradient
// Forward convolution of one site: 3x3 / pad 1 (stride 1 or 2, optionally behind a nearest x2 upsample) gathered from the fp32
// NHWC activation src (row stride lds, channels [0, cin), cin % 32 == 0), weights `packed` = pack_conv_kernel's f16x3 layout of
// the RAW weight ([hi (np x 9 cin)] [lo] halves, then np bias floats) -> dst[m][n] = act(sum 2^-6 + bias), n < cout, row stride
// ld.  One gemm_f16x3 call on its fp32-A route; NSR_ERR_UNSUPPORTED where the shape would take another one.
NSR_INTERNAL int refine_conv_f16x3(hipStream_t st, const float* src, int64_t lds, int cin, int n_img, int Hs, int Ws, int stride,
                                   int up, const float* packed, int np, int cout, int act, float* dst, int64_t ld);
// dst = [hi (cin x 9 np)] [lo] halves of B'[c][((2 - ky) * 3 + (2 - kx)) np + n] = 2^6 w[n][c][ky][kx] (w: (cout, cin, 3, 3));
// columns n >= cout zero
NSR_INTERNAL int refine_flip_pack(hipStream_t st, const float* w, int cin, int cout, int np, unsigned short* dst);
// Input gradient of a stride-1 convolution as an implicit 3x3 / pad 1 convolution of dz (n_img H W rows x np, dense) with
// refine_flip_pack's operand: dst[(img, y, x)][c] (row stride ld, c < cin) is STORED.  *max_bits = float bits of max |dz| (the
// range word above).  cin % 128 == 0 and np % 32 == 0, NSR_ERR_UNSUPPORTED otherwise.
NSR_INTERNAL int refine_dgrad_f16x3(hipStream_t st, const float* dz, int np, const unsigned short* packed, int cin, int n_img, int H,
                                    int W, const unsigned* max_bits, float* dst, int64_t ld);
// the nearest x2 upsample backwards: dst[(img, sy, sx)][c] (row stride ld) = the 2 x 2 block of src (n_img, 2 Hs, 2 Ws, C dense)
// summed in a fixed order; C % 4 == 0
NSR_INTERNAL int refine_fold2x2(hipStream_t st, const float* src, int C, int n_img, int Hs, int Ws, float* dst, int64_t ld);
// ---- weight_grad = NSR_F16X3 (nsr_refine_wgrad_f16.hip): the weight gradient on the split-fp16 MFMA without the col matrix
// Pixels per slice of a site's weight-gradient product: a function of the shape alone (cin, cout, K = output pixels of the call)
NSR_INTERNAL int64_t refine_wgrad_slice_len(int cin, int cout, int64_t K);
// g[n][c][ky][kx] (cout, cin, 3, 3) = or += (`acc`) sum over the output pixels of dz[(img, y, x)][n] (rows x np, dense)
// src[(img, s y + ky - 1, s x + kx - 1)][c] -- src NHWC (n_img, Hs, Ws) with row stride ld, read through the nearest x2
// upsample if `up`, zero padding.  *max_bits = float bits of max |dz| (the range word above).  Partials of the slices go to
// `part` (part_floats floats; as many slices per pass as fit) and are added in slice order by refine_wgrad_reduce.
// slice_len: 0 = refine_wgrad_slice_len (the product path), otherwise a multiple of 32 (the unit tests: small cases that span
// several slices).  cin % 128 == 0, np % 32 == 0, cout <= np, stride 1 or 2: NSR_ERR_UNSUPPORTED otherwise.
NSR_INTERNAL int refine_wgrad_f16x3(hipStream_t st, const float* dz, int np, int cout, const float* src, int64_t ld, int cin, int n_img,
                                    int Hs, int Ws, int stride, int up, const unsigned* max_bits, float* part, int64_t part_floats,
                                    int acc, float* g, int64_t slice_len = 0);
// (B px_per_img, 3) NHWC -> (B, 3, px_per_img)
NSR_INTERNAL int refine_nhwc3_to_nchw(hipStream_t st, const float* src, int64_t px_per_img, int B, float* dst);

}  // namespace nsr
