// Layer-by-layer GEMM path of the training step (precisions NSR_FP32 and NSR_F16X3_GEMM; nsr_train.hip calls it).
//
// The MLP runs layer by layer on one fp32-MFMA GEMM kernel (nsr_gemm.hip; nsr_gemm_f16.hip for the split-fp16 forward
// products) whose epilogue fuses bias / ReLU / sigmoid / the ReLU mask of the backward pass.  The kernel takes either memory
// orientation of each operand, so all three products of a linear layer (forward, input gradient, weight gradient) read
// the row-major (P, C) activations and the nn.Linear weights as they lie: nothing is transposed and nothing is stored
// twice.  The weight gradient is a split-K GEMM over the sample points with a deterministic second-pass reduction (no
// atomics: results are run-to-run identical).  Layers are padded to MFMA-friendly shapes once per step (63 -> 64 input
// channels, the skip concat as [pe64 | h4], the density head stacked under xyz_encoding_final as one 288-row layer, the
// colour head as 32 rows); the gradients are scattered back to the nn.Linear shapes by the reduction kernel.
#include "nsr_gemm.h"
#include "nsr_train_work.h"

using namespace nsr;

namespace {

// dst[(r0 + i) * ld + c0 + j] = src[i][col0 + j]  (or the transpose: dst[(r0 + j) * ld + c0 + i])
__global__ void place_kernel(float* __restrict__ dst, int dst_ld, int r0, int c0, const float* __restrict__ src,
                             int src_ld, int rows, int cols, int col0, int transpose) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * cols) return;
  const int i = idx / cols, j = idx % cols;
  const float v = src[(int64_t)i * src_ld + col0 + j];
  if (transpose) dst[(int64_t)(r0 + j) * dst_ld + c0 + i] = v;
  else dst[(int64_t)(r0 + i) * dst_ld + c0 + j] = v;
}

// E1 + cast_rays for the training layout: one thread per sample point.
//   x5 (P, 320) columns 0..63  = [pe63, 0]
//   gs (P, 288) columns 257..287 = [0 0 0, de27, 0]
__global__ void __launch_bounds__(256) encode_train_kernel(const float* __restrict__ rays, int stride,
                                                           const float* __restrict__ z, int64_t P, int N,
                                                           float* __restrict__ x5, float* __restrict__ gs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const NsrRay q = nsr_load_ray(rays, p / N, stride);
  const float zk = z[p];
  float pe[64];
#pragma unroll
  for (int c = 0; c < 3; ++c) pe[c] = __fadd_rn(q.o[c], __fmul_rn(zk, q.d[c]));   // cast_rays, models/utils.py:5-14
#pragma unroll
  for (int f = 0; f < 10; ++f)
#pragma unroll
    for (int c = 0; c < 3; ++c) nsr_sincos(ldexpf(pe[c], f), pe[3 + 6 * f + c], pe[3 + 6 * f + 3 + c]);
  pe[63] = 0.0f;
  float4* row = reinterpret_cast<float4*>(x5 + p * kX5);
#pragma unroll
  for (int i = 0; i < 16; ++i) row[i] = make_float4(pe[4 * i], pe[4 * i + 1], pe[4 * i + 2], pe[4 * i + 3]);
  float de[31];   // columns 257..287
  de[0] = de[1] = de[2] = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) de[3 + c] = q.v[c];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int c = 0; c < 3; ++c) nsr_sincos(ldexpf(q.v[c], f), de[6 + 6 * f + c], de[6 + 6 * f + 3 + c]);
  de[30] = 0.0f;
#pragma unroll
  for (int c = 0; c < 31; ++c) gs[p * kGs + 257 + c] = de[c];
}
// bias gradients.  Two deterministic passes each (double accumulation, then one finishing block):
//   colsum_few:  sums of <= 4 columns of a row-major buffer over all P rows (colour-head and density-head biases,
//                whose pre-activation gradients come from the compositing backward, not from a GEMM)
//   tilesum:     sums over the per-row-tile column sums a dgrad GEMM's epilogue left behind (every other bias)
constexpr int kSumBlocks = 256;
__global__ void __launch_bounds__(256) colsum_few_kernel(const float* __restrict__ src, int64_t ld, int64_t P, int col0,
                                                         int cols, double* __restrict__ partial) {
  __shared__ double red[4][256];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < P; r += (int64_t)kSumBlocks * 256)
    for (int c = 0; c < cols; ++c) s[c] += (double)src[r * ld + col0 + c];
  for (int c = 0; c < 4; ++c) red[c][threadIdx.x] = s[c];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int c = 0; c < 4; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + o];
    __syncthreads();
  }
  if ((int)threadIdx.x < cols) partial[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}
// block (x: 64-column group, y: slice of the row tiles): 64 columns x 4 row phases
__global__ void __launch_bounds__(256) tilesum_partial_kernel(const float* __restrict__ tiles, int64_t n_tiles, int ld,
                                                              int cols, double* __restrict__ partial) {
  __shared__ double red[4][64];
  const int cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl, phase = threadIdx.x >> 6;
  const int64_t per = (n_tiles + gridDim.y - 1) / gridDim.y;
  const int64_t lo = per * blockIdx.y, hi = (lo + per < n_tiles) ? lo + per : n_tiles;
  double s = 0.0;
  if (c < cols)
    for (int64_t t = lo + phase; t < hi; t += 4) s += (double)tiles[t * ld + c];
  red[phase][cl] = s;
  __syncthreads();
  if (phase == 0 && c < cols) partial[(int64_t)blockIdx.y * ld + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}
// dst[c] (+)= sum_j partial[j * ld + c]: one wavefront per column (4 columns per block), so the n partials of a
// column are loaded in parallel and combined by shuffles in a fixed order
__global__ void __launch_bounds__(256) sum_finish_kernel(const double* __restrict__ partial, int n, int ld, int cols,
                                                         float* __restrict__ dst, int accumulate) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= cols) return;   // wave-uniform
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += partial[(int64_t)j * ld + c];
  s = wave_sum_d(s);
  if (lane == 0) dst[c] = (accumulate ? dst[c] : 0.0f) + (float)s;
}

// second pass of the split-K weight gradient + scatter into the nn.Linear shape:
// dst[i * dst_ld + dc0 + j] (+)= sum_z partial[z * stride + (pr0 + i) * p_ld + pc0 + j]
__global__ void __launch_bounds__(256) reduce_place_kernel(float* __restrict__ dst, int dst_ld, int dc0, int rows, int cols,
                                                           const float* __restrict__ partial, int splits, int64_t stride,
                                                           int p_ld, int pr0, int pc0, int accumulate, float scale) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * cols) return;
  const int i = idx / cols, j = idx % cols;
  const float* src = partial + (int64_t)(pr0 + i) * p_ld + pc0 + j;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;   // four independent chains: the loads of a round are all in flight
  int zc = 0;
  for (; zc + 4 <= splits; zc += 4) {
    s0 += (double)src[(zc + 0) * stride];
    s1 += (double)src[(zc + 1) * stride];
    s2 += (double)src[(zc + 2) * stride];
    s3 += (double)src[(zc + 3) * stride];
  }
  for (; zc < splits; ++zc) s0 += (double)src[zc * stride];
  const double s = (s0 + s1) + (s2 + s3);
  float* d = dst + (int64_t)i * dst_ld + dc0 + j;
  *d = (accumulate ? *d : 0.0f) + (float)(s * (double)scale);   // scale: a power of two (pre-scaled operands)
}
}  // namespace

// ---- host wrappers over the kernels above, shared with nsr_train_arch.hip (declared in nsr_train_work.h)
int nsr::place(hipStream_t st, float* dst, int dst_ld, int r0, int c0, const float* src, int src_ld, int rows, int cols,
               int col0, int transpose) {
  const int n = rows * cols;
  hipLaunchKernelGGL(place_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dst, dst_ld, r0, c0, src, src_ld, rows, cols,
                     col0, transpose);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

// y (P, N) = act(x (P, K) w (N, K)^T + b); hi / lo (the weights' split-fp16 halves, row stride ldh) select the split-fp16 product
int nsr::lin_fwd_at(hipStream_t st, const float* x, int64_t ldx, int K, const float* w, int ldw, const float* b, int act,
                    float* y, int64_t ldy, int64_t P, int N, int n_valid, const unsigned short* hi, const unsigned short* lo,
                    int ldh) {
  GemmArgs g{};
  g.A = x; g.lda = ldx; g.B = w; g.ldb = ldw; g.C = y; g.ldc = ldy; g.bias = b;
  g.M = P; g.N = N; g.K = K; g.n_valid = n_valid; g.act = act; g.splits = 1;
  if (!hi) return gemm(g, st);
  GemmF16Args a{};
  a.g = g;
  a.g.acc_scale = kSplitInvScale;
  a.Bh = hi;
  a.Bl = lo;
  a.ldbh = ldh;
  return gemm_f16x3(a, st);
}
namespace {
// the default network: `split` (entry e of the pack's split block) selects the split-fp16 product
int lin_fwd(hipStream_t st, const float* x, int64_t ldx, int K, const float* w, int ldw, const float* b, int act,
            float* y, int64_t ldy, int64_t P, int N, int n_valid, const unsigned short* split = nullptr, int e = 0) {
  const unsigned short* hi = split ? split + split_offset(e) : nullptr;
  return lin_fwd_at(st, x, ldx, K, w, ldw, b, act, y, ldy, P, N, n_valid, hi, hi ? hi + (int64_t)kSplitRows[e] * kSplitK[e] : nullptr,
                    kSplitK[e]);
}
}  // namespace
// dx (P, N) = (dy (P, K) w[:, 0 : N]) * [mask > 0], w (K, ldw) in the nn.Linear layout (mask may be null);
// bias_grad (N) (+)= column sums of dx = the bias gradient of the layer that produced the masked activation
// n_bias (0: N): how many of the N columns the bias has (a padded layer's trailing columns are exact zeros)
int nsr::lin_dgrad(hipStream_t st, const Work& k, const float* dy, int64_t lddy, int K, const float* w, int ldw,
                   const float* mask, int64_t ldm, float* dx, int64_t lddx, int64_t P, int N, float* bias_grad, int acc,
                   int n_bias) {
  GemmArgs g{};
  g.A = dy; g.lda = lddy; g.B = w; g.ldb = ldw; g.b_kmajor = 1; g.C = dx; g.ldc = lddx;
  g.mask = mask; g.ldm = ldm; g.M = P; g.N = N; g.K = K; g.n_valid = N; g.act = kActNone; g.splits = 1;
  g.col_sums = bias_grad ? k.col_tiles : nullptr;
  const int rc = gemm(g, st);
  if (rc != NSR_OK || !bias_grad) return rc;
  double* part = reinterpret_cast<double*>(k.col_tiles + ((P + 127) / 128) * N);   // behind the tile sums
  const int slices = 64;
  hipLaunchKernelGGL(tilesum_partial_kernel, dim3((N + 63) / 64, slices), dim3(256), 0, st, k.col_tiles, (P + 127) / 128, N,
                     N, part);
  NSR_CHECK_LAUNCH();
  const int nb = n_bias > 0 ? n_bias : N;
  hipLaunchKernelGGL(sum_finish_kernel, dim3((nb + 3) / 4), dim3(256), 0, st, part, slices, N, nb, bias_grad, acc);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
// partial[z] (M x N) = sum over the z-th slice of the points of dy[p][0..M) x[p][0..N)^T
// (slice z at partial + z * stride)
int nsr::lin_wgrad(hipStream_t st, const float* dy, int64_t lddy, int M, const float* x, int64_t ldx, int N, int64_t P,
                   float* partial, int splits, int64_t stride) {
  GemmArgs g{};
  g.A = dy; g.lda = lddy; g.a_kmajor = 1; g.B = x; g.ldb = ldx; g.b_kmajor = 1; g.C = partial; g.ldc = N;
  g.M = M; g.N = N; g.K = P; g.n_valid = N; g.act = kActNone; g.splits = splits; g.split_stride = stride;
  return gemm(g, st);
}
int nsr::reduce_place(hipStream_t st, float* dst, int dst_ld, int dc0, int rows, int cols, const float* partial, int splits,
                      int p_ld, int pr0, int pc0, int accumulate, float scale, int64_t stride) {
  const int n = rows * cols;
  hipLaunchKernelGGL(reduce_place_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dst, dst_ld, dc0, rows, cols, partial,
                     splits, stride, p_ld, pr0, pc0, accumulate, scale);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
// `scratch`: >= kSumBlocks * 4 doubles (the split-K partial buffer is free between two weight gradients)
int nsr::colsum(hipStream_t st, const float* src, int64_t ld, int64_t P, int col0, int cols, float* dst, int accumulate,
                float* scratch) {
  if (cols > 4) return NSR_ERR_INVALID_ARG;
  double* part = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(colsum_few_kernel, dim3(kSumBlocks), dim3(256), 0, st, src, ld, P, col0, cols, part);
  NSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_finish_kernel, dim3((cols + 3) / 4), dim3(256), 0, st, part, kSumBlocks, 4, cols, dst, accumulate);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

int nsr::prepare_weights(hipStream_t st, const float* const* w, const WeightPack& q, int precision) {
  // zero the whole pack first (padding rows / columns), it is one contiguous block starting at w1p
  if (hipMemsetAsync(q.w1p, 0, (size_t)((q.brgbp + align64(64)) - q.w1p) * sizeof(float), st) != hipSuccess)
    return NSR_ERR_LAUNCH;
  NSR_TRY(place(st, q.w1p, 64, 0, 0, w[0], 63, 256, 63, 0, 0));
  NSR_TRY(place(st, q.w5p, 320, 0, 0, w[8], 319, 256, 63, 0, 0));
  NSR_TRY(place(st, q.w5p, 320, 0, 64, w[8], 319, 256, 256, 63, 0));
  NSR_TRY(place(st, q.w9p, 256, 0, 0, w[kFinalW], 256, 256, 256, 0, 0));
  NSR_TRY(place(st, q.w9p, 256, 256, 0, w[kSigmaW], 256, 1, 256, 0, 0));
  NSR_TRY(place(st, q.wdirp, 288, 0, 0, w[kDirW], 283, 128, 256, 0, 0));
  NSR_TRY(place(st, q.wdirp, 288, 0, kDeCol, w[kDirW], 283, 128, 27, 256, 0));
  NSR_TRY(place(st, q.wrgbp, 128, 0, 0, w[kRgbW], 128, 3, 128, 0, 0));
  NSR_TRY(place(st, q.b9p, 320, 0, 0, w[kFinalB], 256, 1, 256, 0, 0));
  NSR_TRY(place(st, q.b9p, 320, 0, 256, w[kSigmaB], 1, 1, 1, 0, 0));
  NSR_TRY(place(st, q.brgbp, 64, 0, 0, w[kRgbB], 3, 1, 3, 0, 0));
  if (precision == NSR_F16X3) {
    const float* src[12] = {q.w1p, w[2], w[4], w[6], q.w5p, w[10], w[12], w[14], q.w9p, q.w9p + 256 * 256, q.wdirp, q.wrgbp};
    for (int e = 0; e < 12; ++e) {
      const int64_t n = (int64_t)kSplitRows[e] * kSplitK[e];
      NSR_TRY(split_f16(src[e], n, q.split + split_offset(e), q.split + split_offset(e) + n, st));
    }
  }
  return NSR_OK;
}
int nsr::net_forward(hipStream_t st, const float* rays, int ray_stride, const float* z, int N, const float* const* w,
                     const WeightPack& q, const Kept& s, int64_t P, int precision, int color_none) {
  hipLaunchKernelGGL(encode_train_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, rays, ray_stride, z, P, N, s.x5, s.gs);
  NSR_CHECK_LAUNCH();
  const unsigned short* sp = precision == NSR_F16X3 ? q.split : nullptr;
  NSR_TRY(lin_fwd(st, s.x5, kX5, kPe, q.w1p, 64, w[1], kActRelu, s.h[1], kW, P, kW, kW, sp, 0));
  NSR_TRY(lin_fwd(st, s.h[1], kW, kW, w[2], 256, w[3], kActRelu, s.h[2], kW, P, kW, kW, sp, 1));
  NSR_TRY(lin_fwd(st, s.h[2], kW, kW, w[4], 256, w[5], kActRelu, s.h[3], kW, P, kW, kW, sp, 2));
  NSR_TRY(lin_fwd(st, s.h[3], kW, kW, w[6], 256, w[7], kActRelu, s.x5 + kPe, kX5, P, kW, kW, sp, 3));
  NSR_TRY(lin_fwd(st, s.x5, kX5, kX5, q.w5p, 320, w[9], kActRelu, s.h[5], kW, P, kW, kW, sp, 4));
  NSR_TRY(lin_fwd(st, s.h[5], kW, kW, w[10], 256, w[11], kActRelu, s.h[6], kW, P, kW, kW, sp, 5));
  NSR_TRY(lin_fwd(st, s.h[6], kW, kW, w[12], 256, w[13], kActRelu, s.h[7], kW, P, kW, kW, sp, 6));
  NSR_TRY(lin_fwd(st, s.h[7], kW, kW, w[14], 256, w[15], kActRelu, s.h[8], kW, P, kW, kW, sp, 7));
  // xyz_encoding_final stacked over the density head: [g | sigma] into columns 0..256 of the dir layer's input
  // (two launches: the 256 wide columns on the 8-wave tile, the density row on the narrow one, instead of a second
  // 256-wide column tile that would be 7/8 padding)
  NSR_TRY(lin_fwd(st, s.h[8], kW, kW, q.w9p, 256, q.b9p, kActNone, s.gs, kGs, P, kW, kW, sp, 8));
  NSR_TRY(lin_fwd(st, s.h[8], kW, kW, q.w9p + 256 * 256, 256, q.b9p + 256, kActNone, s.gs + kSigmaCol, kGs, P, 32, 1, sp, 9));
  NSR_TRY(lin_fwd(st, s.gs, kGs, kGs, q.wdirp, 288, w[kDirB], kActRelu, s.cc, kDirOut, P, kDirOut, kDirOut, sp, 10));
  NSR_TRY(lin_fwd(st, s.cc, kDirOut, kDirOut, q.wrgbp, 128, q.brgbp, color_none ? kActNone : kActSigmoid, s.rgb, 4, P, kRgbPad, 3, sp, 11));
  return NSR_OK;
}

int nsr::net_backward(hipStream_t st, const float* const* w, const WeightPack& q, const Work& k, int64_t P, float* const* g,
                      int acc, int stop_grad) {
  const Kept& s = k.kept;
  const int sp = n_splits(P);
  float* part = k.partial;
  // rgb head
  NSR_TRY(lin_wgrad(st, k.drgb, kRgbPad, kRgbPad, s.cc, kDirOut, kDirOut, P, part, sp));
  NSR_TRY(reduce_place(st, g[kRgbW], 128, 0, 3, 128, part, sp, kDirOut, 0, 0, acc));
  NSR_TRY(colsum(st, k.drgb, kRgbPad, P, 0, 3, g[kRgbB], acc, part));
  NSR_TRY(lin_dgrad(st, k, k.drgb, kRgbPad, kRgbPad, q.wrgbp, 128, s.cc, kDirOut, k.g0, kDirOut, P, kDirOut, g[kDirB], acc));
  // dir_encoding
  NSR_TRY(lin_wgrad(st, k.g0, kDirOut, kDirOut, s.gs, kGs, kGs, P, part, sp));
  NSR_TRY(reduce_place(st, g[kDirW], 283, 0, 128, 256, part, sp, kGs, 0, 0, acc));
  NSR_TRY(reduce_place(st, g[kDirW], 283, 256, 128, 27, part, sp, kGs, 0, kDeCol, acc));
  // d g (its column sums are xyz_encoding_final's bias gradient); column 256 keeps d sigma
  if (stop_grad) {   // --stop_grad (models/networks.py:218-219): dir_encoding's input is detached, d g = 0
    if (hipMemset2DAsync(k.g1, (size_t)kGs * sizeof(float), 0, (size_t)kW * sizeof(float), (size_t)P, st) != hipSuccess) return NSR_ERR_LAUNCH;
    if (!acc && hipMemsetAsync(g[kFinalB], 0, (size_t)kW * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
  } else {
    NSR_TRY(lin_dgrad(st, k, k.g0, kDirOut, kDirOut, q.wdirp, 288, nullptr, 0, k.g1, kGs, P, kW, g[kFinalB], acc));
  }
  // xyz_encoding_final + sigma (288-row layer over h8)
  NSR_TRY(lin_wgrad(st, k.g1, kGs, kW, s.h[8], kW, kW, P, part, sp));                 // rows 0..255: xyz_encoding_final
  NSR_TRY(reduce_place(st, g[kFinalW], 256, 0, 256, 256, part, sp, kW, 0, 0, acc));
  NSR_TRY(lin_wgrad(st, k.g1 + kSigmaCol, kGs, 32, s.h[8], kW, kW, P, part, sp));     // row 256 (+ 31 zero rows): sigma
  NSR_TRY(reduce_place(st, g[kSigmaW], 256, 0, 1, 256, part, sp, kW, 0, 0, acc));
  NSR_TRY(colsum(st, k.g1, kGs, P, 256, 1, g[kSigmaB], acc, part));
  NSR_TRY(lin_dgrad(st, k, k.g1, kGs, kGs, q.w9p, 256, s.h[8], kW, k.g0, kW, P, kW, g[15], acc));   // + bias of layer 8
  // xyz_encoding_8 .. 1; the gradient of layer L's pre-activation alternates between the two buffers
  const float* dy = k.g0;
  float* nx = k.g1;
  for (int L = 8; L >= 1; --L) {
    const float* xin = (L == 1 || L == 5) ? s.x5 : s.h[L - 1];
    const int64_t ldx = (L == 1 || L == 5) ? kX5 : kW;
    const int kin = (L == 1) ? kPe : (L == 5 ? kX5 : kW);
    NSR_TRY(lin_wgrad(st, dy, kW, kW, xin, ldx, kin, P, part, sp));
    float* gw = g[2 * (L - 1)];
    if (L == 1) NSR_TRY(reduce_place(st, gw, 63, 0, 256, 63, part, sp, kPe, 0, 0, acc));
    else if (L == 5) {
      NSR_TRY(reduce_place(st, gw, 319, 0, 256, 63, part, sp, kX5, 0, 0, acc));
      NSR_TRY(reduce_place(st, gw, 319, 63, 256, 256, part, sp, kX5, 0, kPe, acc));
    } else NSR_TRY(reduce_place(st, gw, 256, 0, 256, 256, part, sp, kW, 0, 0, acc));
    if (L == 1) break;
    // input of layer L is the output of layer L - 1 (relu'd): h4 sits in x5[:, 64:]
    const float* mask = (L - 1 == 4) ? s.x5 + kPe : s.h[L - 1];
    const int64_t ldm = (L - 1 == 4) ? kX5 : kW;
    // weights in the nn.Linear layout (out, in) ARE the K-major B operand of the input gradient
    const float* wl = (L == 5) ? q.w5p + kPe : w[2 * (L - 1)];
    const int ldw = (L == 5) ? kX5 : kW;
    NSR_TRY(lin_dgrad(st, k, dy, kW, kW, wl, ldw, mask, ldm, nx, kW, P, kW, g[2 * (L - 2) + 1], acc));   // + bias of layer L - 1
    const float* t0 = dy; dy = nx; nx = const_cast<float*>(t0);
  }
  return NSR_OK;
}
