// The layer-by-layer network of the training step (precisions NSR_FP32, NSR_F16X3_GEMM and NSR_F16X3_GEMM_BWD; the drivers of
// nsr_train.hip call it), for ANY architecture the reference's flags describe (include/nsr_train.h, nsr_arch: --D --W --skips --deg_pos --deg_dir
// --no_dir).  The default 8 x 256 network is the descriptor {8, 256, skips {4}, 10, 4, 0}: there is no second implementation.
//
// The MLP runs layer by layer on one fp32-MFMA GEMM kernel (nsr_gemm.hip; nsr_gemm_f16.hip for the split-fp16 forward
// products) whose epilogue fuses bias / ReLU / sigmoid / the ReLU mask of the backward pass.  The kernel takes either memory
// orientation of each operand, so all three products of a linear layer (forward, input gradient, weight gradient) read
// the row-major (P, C) activations and the nn.Linear weights as they lie: nothing is transposed and nothing is stored
// twice.  The weight gradient is a split-K GEMM over the sample points with a deterministic second-pass reduction (no
// atomics: results are run-to-run identical).  Under NSR_F16X3_GEMM_BWD the input and weight gradients run on the split-fp16 MFMA
// instead (nsr_train_bwd_f16.hip: the same contracts, the same order of products; the input gradients read transposed split
// copies of the weights, Pack::ht, the one thing that precision stores twice).
//
// Everything is a function of the descriptor at run time (Shape, nsr_train_work.h: the layout of a pass is described there):
// the padded shapes, the kept state, the padded weight copies and their split-fp16 halves (Pack), the drivers over the D trunk
// layers (net_forward / net_backward).  Layers are padded to multiples of 32 once per call; the gradients are scattered back
// to the nn.Linear shapes by the reduction kernel.  Backward: the density head is stacked under xyz_encoding_final as one
// (Wp + 32)-row layer, so the gradient of the trunk's last activation is one product over [d final | d sigma 0 .. 0]; the
// colour head is 32 rows.
#include "nsr_gemm.h"
#include "nsr_train_work.h"

using namespace nsr;

namespace {

inline int r32(int n) { return (n + 31) & ~31; }

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

// E1 + cast_rays with run-time degree: one thread per (sample point, 4 columns) writes dst[p][4 g .. 4 g + 4) of
//   [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...  | zeros up to 4 n_groups]      (x: the point o + z d, or the view direction)
// with nsr_sincos on the ldexpf frequencies.
// The row is computed once and written to every destination (one x buffer per skip layer; all with row stride ld).
struct EncodeDst {
  float* p[kMaxD];
  int n;
};
__global__ void __launch_bounds__(256) encode_arch_kernel(const float* __restrict__ rays, int stride, const float* __restrict__ z,
                                                          int64_t P, int N, int deg, int view_dir, EncodeDst dst, int64_t ld,
                                                          int n_groups, unsigned embed, NsrBands bands) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = idx / n_groups;
  const int g = (int)(idx % n_groups);
  if (p >= P) return;
  const NsrRay q = nsr_load_ray(rays, p / N, stride);
  float x[3];
  if (view_dir) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = q.v[c];
  } else {
    const float zk = z[p];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = __fadd_rn(q.o[c], __fmul_rn(zk, q.d[c]));   // cast_rays, models/utils.py:5-14
  }
  const int first = nsr_embed_first(embed), n_valid = first + 6 * deg;
  float out[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * g + e;
    float v = 0.0f;
    if (c < first) {
      v = c == 0 ? x[0] : (c == 1 ? x[1] : x[2]);
    } else if (c < n_valid) {
      const int f = (c - first) / 6, r = (c - first) % 6, comp = r % 3;
      const float xc = comp == 0 ? x[0] : (comp == 1 ? x[1] : x[2]);
      float sn, cs;
      nsr_sincos(nsr_band_arg(xc, f, bands, embed), sn, cs);
      v = r < 3 ? sn : cs;
    }
    out[e] = v;
  }
  for (int j = 0; j < dst.n; ++j)
    *reinterpret_cast<float4*>(dst.p[j] + p * ld + 4 * g) = make_float4(out[0], out[1], out[2], out[3]);
}

// the compositing backward's compact rows d4[p] = (d rgb_pre 0..2, d sigma) into the layouts the two heads' products read:
// drgb (P, 32) = [d rgb_pre | 0], gsig[p * ldg + 0 .. 32) = [d sigma | 0].  One thread per (point, float4).
__global__ void __launch_bounds__(256) scatter_heads_kernel(const float4* __restrict__ d4, int64_t P, float* __restrict__ drgb,
                                                            float* __restrict__ gsig, int64_t ldg) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = idx >> 3;
  const int j = (int)(idx & 7);
  if (p >= P) return;
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
  if (j == 0) {
    const float4 v = d4[p];
    a = make_float4(v.x, v.y, v.z, 0.0f);
    b.x = v.w;
  }
  reinterpret_cast<float4*>(drgb + p * 32)[j] = a;
  reinterpret_cast<float4*>(gsig + p * ldg)[j] = b;
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

// ---- the gradient with respect to the rays (nsr_train_arch_backward_r) ---------------------------------------------------
// Backward of encode_arch_kernel's row (the same column map): g_x[p][0..3) = d(loss) / d(x) of sample point p from the
// gradients of its encoded columns, summed over the n sources (layer 0 and every skip layer, in that order):
//   identity column c (none under NO_XYZ): g;   band f, sin column: f cos(f x) g;   cos column: -f sin(f x) g
// with sin / cos the values the forward kept in `enc` (row stride ld_enc).  `lanes` (8, 16 or 32, >= n_groups) lanes share a
// point, one float4 of columns each; their three partial sums meet in a fixed xor-shuffle order (double arithmetic).
struct EncodeSrc {
  const float* p[kMaxD];
  int n;
};
__global__ void __launch_bounds__(256) encode_bwd_kernel(EncodeSrc src, int64_t ld_src, const float* __restrict__ enc, int64_t ld_enc,
                                                         int64_t P, int deg, int n_groups, int lanes, unsigned embed, NsrBands bands,
                                                         float* __restrict__ g_x) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = idx / lanes;
  const int g = (int)(idx % lanes);
  const int first = nsr_embed_first(embed), n_valid = first + 6 * deg;
  double a[3] = {0.0, 0.0, 0.0};
  if (p < P && g < n_groups) {
    double gs[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < src.n; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(src.p[j] + p * ld_src + 4 * g);
      gs[0] += (double)v.x; gs[1] += (double)v.y; gs[2] += (double)v.z; gs[3] += (double)v.w;
    }
    const float* row = enc + p * ld_enc;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * g + e;
      if (c >= n_valid) continue;
      double t;
      int comp;
      if (c < first) {
        comp = c;
        t = gs[e];
      } else {
        const int f = (c - first) / 6, r = (c - first) % 6;
        comp = r % 3;
        const double band = (embed & NSR_EMBED_LINEAR_FREQS) ? (double)bands.f[f] : (double)ldexpf(1.0f, f);
        // the partner column of the same band and component: cos for a sin column, sin for a cos column
        t = r < 3 ? band * (double)row[c + 3] * gs[e] : -(band * (double)row[c - 3] * gs[e]);
      }
      a[0] += comp == 0 ? t : 0.0;
      a[1] += comp == 1 ? t : 0.0;
      a[2] += comp == 2 ? t : 0.0;
    }
  }
  // every lane of the wave takes part (lanes divides 64: the `lanes` lanes of a point lie in one wave)
  for (int o = lanes >> 1; o > 0; o >>= 1) {
    a[0] += __shfl_xor(a[0], o, 64);
    a[1] += __shfl_xor(a[1], o, 64);
    a[2] += __shfl_xor(a[2], o, 64);
  }
  if (p < P && g < 3) g_x[p * 3 + g] = (float)(g == 0 ? a[0] : (g == 1 ? a[1] : a[2]));
}

// One wavefront per ray, like the compositor: the ray's row of d(loss) / d(rays) from its N sample points x = o + z d,
//   g_o = sum_k g_x[k],  g_d = sum_k z[k] g_x[k]     (z does not depend on o or d: include/nsr_train.h)
// and, with g_dir (N rows of the gradients of the encoded view direction's columns, row stride ld_dir), the direction
// encoding's backward applied ONCE to their column sums -- every point of a ray holds the same encoded direction, dir_enc is
// the row of the ray's first point.  It joins g_d at stride 8 (the encoded direction is d) and goes to columns 8:11 at stride 11.
// Columns 6:8 (near, far) get zeros.  acc: the row is added to (the fine pass after the coarse one).  Double sums, lanes
// combined by wave_sum_d: a fixed order.
__global__ void __launch_bounds__(256) ray_grad_kernel(const float* __restrict__ g_x, const float* __restrict__ z, int64_t R, int N,
                                                       const float* __restrict__ g_dir, int64_t ld_dir,
                                                       const float* __restrict__ dir_enc, int64_t ld_enc, int deg_dir, unsigned embed,
                                                       NsrBands bands, float* __restrict__ g_rays, int stride, int acc) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= R) return;   // wave-uniform
  const int64_t base = r * N;
  double so[3] = {0.0, 0.0, 0.0}, sd[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0};
  for (int k = lane; k < N; k += 64) {
    const double zk = (double)z[base + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = (double)g_x[(base + k) * 3 + c];
      so[c] += v;
      sd[c] += zk * v;
    }
  }
  if (g_dir) {
    const int first = nsr_embed_first(embed), n_valid = first + 6 * deg_dir;
    const float* row = dir_enc + base * ld_enc;
    for (int c = lane; c < n_valid; c += 64) {
      double s = 0.0;
      for (int k = 0; k < N; ++k) s += (double)g_dir[(base + k) * ld_dir + c];
      double t;
      int comp;
      if (c < first) {
        comp = c;
        t = s;
      } else {
        const int f = (c - first) / 6, q = (c - first) % 6;
        comp = q % 3;
        const double band = (embed & NSR_EMBED_LINEAR_FREQS) ? (double)bands.f[f] : (double)ldexpf(1.0f, f);
        t = q < 3 ? band * (double)row[c + 3] * s : -(band * (double)row[c - 3] * s);
      }
      dv[0] += comp == 0 ? t : 0.0;
      dv[1] += comp == 1 ? t : 0.0;
      dv[2] += comp == 2 ? t : 0.0;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    so[c] = wave_sum_d(so[c]);
    sd[c] = wave_sum_d(sd[c]);
    dv[c] = wave_sum_d(dv[c]);
  }
  // lane j writes column j of the row
  if (lane >= stride) return;
  float v = 0.0f;
  if (lane < 3) v = (float)so[lane];
  else if (lane < 6) v = (float)(stride == 8 ? sd[lane - 3] + dv[lane - 3] : sd[lane - 3]);
  else if (lane >= 8) v = (float)dv[lane - 8];
  float* dst = g_rays + r * stride + lane;
  *dst = (acc && (lane < 6 || lane >= 8)) ? __fadd_rn(*dst, v) : v;
}
}  // namespace

// ---- host wrappers over the kernels above (nsr_train_work.h; the unit tests launch them one by one): the deterministic
// reductions and placements behind a linear layer's products
int nsr::place(hipStream_t st, float* dst, int dst_ld, int r0, int c0, const float* src, int src_ld, int rows, int cols,
               int col0, int transpose) {
  const int n = rows * cols;
  hipLaunchKernelGGL(place_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dst, dst_ld, r0, c0, src, src_ld, rows, cols,
                     col0, transpose);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int nsr::scatter_heads(hipStream_t st, const float* d4, int64_t P, float* drgb, float* gsig, int64_t ldg) {
  hipLaunchKernelGGL(scatter_heads_kernel, dim3((unsigned)((P * 8 + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(d4), P, drgb, gsig, ldg);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int nsr::tile_sums(hipStream_t st, float* col_tiles, int64_t n_tiles, int N, int n_bias, float* bias_grad, int acc) {
  double* part = reinterpret_cast<double*>(col_tiles + n_tiles * N);   // behind the tile sums
  const int slices = 64;
  hipLaunchKernelGGL(tilesum_partial_kernel, dim3((N + 63) / 64, slices), dim3(256), 0, st, col_tiles, n_tiles, N, N, part);
  NSR_CHECK_LAUNCH();
  const int nb = n_bias > 0 ? n_bias : N;
  hipLaunchKernelGGL(sum_finish_kernel, dim3((nb + 3) / 4), dim3(256), 0, st, part, slices, N, nb, bias_grad, acc);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int nsr::reduce_place(hipStream_t st, float* dst, int dst_ld, int dc0, int rows, int cols, const float* partial, int splits,
                      int p_ld, int pr0, int pc0, int accumulate, float scale, int64_t stride) {
  const int n = rows * cols;
  hipLaunchKernelGGL(reduce_place_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dst, dst_ld, dc0, rows, cols, partial,
                     splits, stride, p_ld, pr0, pc0, accumulate, scale);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
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

// g_x (P, 3) from the gradients of the encoded columns of n_src sources (each (P, ld_src), the first 4 n_groups columns read)
// and the encoded rows the forward kept
int nsr::encode_bwd(hipStream_t st, const float* const* src, int n_src, int64_t ld_src, const float* enc, int64_t ld_enc, int64_t P,
                    int deg, int n_groups, unsigned embed, const NsrBands* bands, float* g_x) {
  if (n_src < 1 || n_src > kMaxD || n_groups < 1 || n_groups > 32 || (ld_src & 3) != 0) return NSR_ERR_INVALID_ARG;
  if (nsr_embed_first(embed) + 6 * deg > 4 * n_groups || ((embed & NSR_EMBED_LINEAR_FREQS) && !bands)) return NSR_ERR_INVALID_ARG;
  EncodeSrc s{};
  for (int j = 0; j < n_src; ++j) s.p[j] = src[j];
  s.n = n_src;
  const int lanes = n_groups <= 8 ? 8 : (n_groups <= 16 ? 16 : 32);
  const int64_t n = P * lanes;
  if (n == 0) return NSR_OK;
  hipLaunchKernelGGL(encode_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s, ld_src, enc, ld_enc, P, deg, n_groups,
                     lanes, embed, bands ? *bands : NsrBands{}, g_x);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
// the R rows of g_rays (R, stride) from g_x (R N, 3), z (R N) and (g_dir non-null) the direction columns' gradients
int nsr::ray_grad(hipStream_t st, const float* g_x, const float* z, int64_t R, int N, const float* g_dir, int64_t ld_dir,
                  const float* dir_enc, int64_t ld_enc, int deg_dir, unsigned embed, const NsrBands* bands, float* g_rays,
                  int stride, int acc) {
  if (!nsr_ray_stride_ok(stride) || N < 1 || (g_dir && !dir_enc) || ((embed & NSR_EMBED_LINEAR_FREQS) && g_dir && !bands))
    return NSR_ERR_INVALID_ARG;
  if (R == 0) return NSR_OK;
  hipLaunchKernelGGL(ray_grad_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, g_x, z, R, N, g_dir, ld_dir, dir_enc, ld_enc,
                     deg_dir, embed, bands ? *bands : NsrBands{}, g_rays, stride, acc);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

namespace {

// ---- one linear layer's three products
// y (P, N) = act(x (P, K) w (N, K)^T + b); hi / lo (the weights' split-fp16 halves, row stride ldh) select the split-fp16 product
int lin_fwd_at(hipStream_t st, const float* x, int64_t ldx, int K, const float* w, int ldw, const float* b, int act,
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
// dx (P, N) = (dy (P, K) w[:, 0 : N]) * [mask > 0], w (K, ldw) in the nn.Linear layout (mask may be null);
// bias_grad (N) (+)= column sums of dx = the bias gradient of the layer that produced the masked activation
// n_bias (0: N): how many of the N columns the bias has (a padded layer's trailing columns are exact zeros)
// t.hi non-null (a pack prepared for NSR_F16X3_GEMM_BWD): the product on the split-fp16 MFMA from the transposed halves of the
// same columns (nsr_train_bwd_f16.hip), which also raises *out_max (may be null) to the float bits of the largest |dx|
struct WT {   // rows [0, N) of a transposed split copy: hi halves, the lo halves lo_off behind them, row stride ld halves
  const unsigned short* hi;
  int64_t lo_off;
  int ld;
};
int lin_dgrad(hipStream_t st, float* col_tiles, const float* dy, int64_t lddy, int K, const float* w, int ldw,
              const float* mask, int64_t ldm, float* dx, int64_t lddx, int64_t P, int N, float* bias_grad, int acc,
              int n_bias, WT t = WT{nullptr, 0, 0}, unsigned* out_max = nullptr) {
  if (t.hi) {
    NSR_TRY(dgrad_f16x3(st, dy, lddy, K, t.hi, t.hi + t.lo_off, t.ld, mask, ldm, dx, lddx, P, N, bias_grad ? col_tiles : nullptr,
                        out_max));
    return bias_grad ? tile_sums(st, col_tiles, (P + 127) / 128, N, n_bias, bias_grad, acc) : NSR_OK;
  }
  GemmArgs g{};
  g.A = dy; g.lda = lddy; g.B = w; g.ldb = ldw; g.b_kmajor = 1; g.C = dx; g.ldc = lddx;
  g.mask = mask; g.ldm = ldm; g.M = P; g.N = N; g.K = K; g.n_valid = N; g.act = kActNone; g.splits = 1;
  g.col_sums = bias_grad ? col_tiles : nullptr;
  const int rc = gemm(g, st);
  if (rc != NSR_OK || !bias_grad) return rc;
  return tile_sums(st, col_tiles, (P + 127) / 128, N, n_bias, bias_grad, acc);
}
// partial[z] (M x N) = sum over the z-th slice of the points of dy[p][0..M) x[p][0..N)^T
// (slice z at partial + z * stride)
int lin_wgrad(hipStream_t st, const float* dy, int64_t lddy, int M, const float* x, int64_t ldx, int N, int64_t P,
              float* partial, int splits, int64_t stride, const unsigned* max_bits = nullptr) {
  // max_bits non-null (NSR_F16X3_GEMM_BWD): on the split-fp16 MFMA, dy scaled by one power of two from the matrix's range word
  if (max_bits) return wgrad_f16x3(st, dy, lddy, M, x, ldx, N, P, max_bits, partial, splits, stride);
  GemmArgs g{};
  g.A = dy; g.lda = lddy; g.a_kmajor = 1; g.B = x; g.ldb = ldx; g.b_kmajor = 1; g.C = partial; g.ldc = N;
  g.M = M; g.N = N; g.K = P; g.n_valid = N; g.act = kActNone; g.splits = splits; g.split_stride = stride;
  return gemm(g, st);
}

// ---- the network
struct Mat { float* p; int64_t ld; };
Mat out_of(const Shape& S, const Kept& s, int l) {
  if (s.h[l]) return {s.h[l], S.Wp};
  return {s.x[S.x_of[l + 1]] + S.Kx, S.Xs};
}
Mat in_of(const Shape& S, const Kept& s, int l) {
  if (l == 0) return {s.x[0], S.ldx};
  if (S.skip(l)) return {s.x[S.x_of[l]], S.Xs};
  return out_of(S, s, l - 1);
}

struct Lin {   // a trunk layer's forward operand: weights with row stride ldw (the padded copy, or the caller's tensor), bias
  const float* w;
  int ldw;
  const float* b;
};
Lin trunk_lin(const Shape& S, const Pack& q, const float* const* w, int l) {
  return {q.wl[l] ? q.wl[l] : w[2 * l], q.wl[l] ? S.kin(l) : S.W, q.bl[l] ? q.bl[l] : w[2 * l + 1]};
}

// one forward layer: x (P, K) -> y (P, N); split: on entry e of the pack's split-fp16 halves
int fwd(hipStream_t st, const Pack& q, bool split, int e, const float* x, int64_t ldx, int K, const float* w, int ldw, const float* b, int act,
        float* y, int64_t ldy, int64_t P, int N, int n_valid) {
  const unsigned short* hi = split ? q.hi[e] : nullptr;
  return lin_fwd_at(st, x, ldx, K, w, ldw, b, act, y, ldy, P, N, n_valid, hi, hi ? hi + (int64_t)N * K : nullptr, K);
}

}  // namespace

int nsr::make_shape(const nsr_arch* a, Shape& S, unsigned embed) {
  if (!a) return NSR_ERR_INVALID_ARG;
  if (a->D < 1 || a->W < 2 || (a->W & 1) || a->deg_pos < 0 || a->deg_dir < 0 || (a->no_dir != 0 && a->no_dir != 1))
    return NSR_ERR_INVALID_ARG;
  if ((a->skips & 1u) || (a->D < 32 && (a->skips >> a->D) != 0u)) return NSR_ERR_INVALID_ARG;
  if (a->D > NSR_ARCH_MAX_D || a->W > NSR_ARCH_MAX_W || a->deg_pos > NSR_ARCH_MAX_DEG || a->deg_dir > NSR_ARCH_MAX_DEG)
    return NSR_ERR_UNSUPPORTED;
  S.arch = *a;
  S.D = a->D; S.W = a->W; S.H = a->W / 2; S.skips = a->skips; S.no_dir = a->no_dir;
  NSR_TRY(nsr_embed_check_net(embed, a->deg_pos, a->deg_dir, a->no_dir));
  S.embed = embed;
  NSR_TRY(nsr_bands(a->deg_pos, embed, S.bands_pos));
  NSR_TRY(nsr_bands(a->deg_dir, embed, S.bands_dir));
  S.in_xyz = nsr_embed_cols(a->deg_pos, embed); S.in_dir = nsr_embed_cols(a->deg_dir, embed);
  S.Kx = r32(S.in_xyz); S.Wp = r32(S.W); S.Hp = r32(S.H); S.Dp = a->no_dir ? 0 : r32(S.in_dir);
  S.Ci = S.Wp + S.Dp; S.Xs = S.Kx + S.Wp;
  int ns = 0;
  for (int l = 0; l < S.D; ++l) {
    S.x_of[l] = -1;
    if (S.skip(l)) S.x_of[l] = ns++;
  }
  S.x_of[0] = 0;
  S.n_x = ns > 0 ? ns : 1;
  S.ldx = ns > 0 ? S.Xs : S.Kx;
  int kin_max = S.Kx > S.Wp ? S.Kx : S.Wp;
  if (ns > 0) kin_max = S.Xs;
  int64_t m = (int64_t)S.Wp * kin_max;
  if ((int64_t)S.Hp * S.Ci > m) m = (int64_t)S.Hp * S.Ci;
  if (32 * (int64_t)S.Wp > m) m = 32 * (int64_t)S.Wp;
  S.part_stride = align64(m);
  return NSR_OK;
}
int64_t nsr::tensor_numel_of(const Shape& S, int t) {
  if (t < 0 || t >= S.n_tensors()) return 0;
  if (t < 2 * S.D) return (t & 1) ? S.W : (int64_t)S.W * S.fan_in(t / 2);
  switch (t - 2 * S.D) {
    case 0: return (int64_t)S.W * S.W;
    case 1: return S.W;
    case 2: return (int64_t)S.H * S.dir_in();
    case 3: return S.H;
    case 4: return S.W;
    case 5: return 1;
    case 6: return 3 * (int64_t)S.H;
    default: return 3;
  }
}

void nsr::carve_net_kept(Carver& a, const Shape& S, int64_t P, Kept& q) {
  for (int j = 0; j < S.n_x; ++j) q.x[j] = a.take(P * S.ldx);
  for (int l = 0; l < S.D; ++l) q.h[l] = (l + 1 < S.D && S.skip(l + 1)) ? nullptr : a.take(P * S.Wp);
  q.ci = a.take(P * S.Ci);   q.cc = a.take(P * S.Hp);
}
Pack nsr::carve_pack(Carver& a, const Shape& S, bool split) {
  Pack q{};
  const int64_t off0 = a.off;
  q.first = a.take(0);
  for (int l = 0; l < S.D; ++l) {
    const bool pad = l == 0 || S.skip(l) || S.W != S.Wp;
    q.wl[l] = a.take((int64_t)S.Wp * S.kin(l), pad);
    q.bl[l] = a.take(S.Wp, S.W != S.Wp);
  }
  q.w9 = a.take((int64_t)(S.Wp + 32) * S.Wp);   q.b9 = a.take(S.Wp + 32);
  q.wdir = a.take((int64_t)S.Hp * S.Ci);        q.bdir = a.take(S.Hp, S.H != S.Hp);
  q.wrgb = a.take(32 * (int64_t)S.Hp);          q.brgb = a.take(32);
  q.floats = a.off - off0;
  if (split) {
    for (int l = 0; l < S.D; ++l) q.hi[l] = reinterpret_cast<unsigned short*>(a.take((int64_t)S.Wp * S.kin(l)));
    q.hi[kFinalE] = reinterpret_cast<unsigned short*>(a.take((int64_t)S.Wp * S.Wp));
    q.hi[kSigmaE] = reinterpret_cast<unsigned short*>(a.take(32 * (int64_t)S.Wp));
    q.hi[kDirE] = reinterpret_cast<unsigned short*>(a.take((int64_t)S.Hp * S.Ci));
    q.hi[kRgbE] = reinterpret_cast<unsigned short*>(a.take(32 * (int64_t)S.Hp));
  }
  return q;
}
int nsr::prepare_weights(hipStream_t st, const Shape& S, const float* const* w, const Pack& q, bool split) {
  if (hipMemsetAsync(q.first, 0, (size_t)q.floats * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
  for (int l = 0; l < S.D; ++l) {
    if (q.wl[l]) {
      const int fi = S.fan_in(l), kin = S.kin(l);
      if (S.skip(l)) {
        NSR_TRY(place(st, q.wl[l], kin, 0, 0, w[2 * l], fi, S.W, S.in_xyz, 0, 0));
        NSR_TRY(place(st, q.wl[l], kin, 0, S.Kx, w[2 * l], fi, S.W, S.W, S.in_xyz, 0));
      } else {
        NSR_TRY(place(st, q.wl[l], kin, 0, 0, w[2 * l], fi, S.W, fi, 0, 0));
      }
    }
    if (q.bl[l]) NSR_TRY(place(st, q.bl[l], S.Wp, 0, 0, w[2 * l + 1], S.W, 1, S.W, 0, 0));
  }
  const int F = S.final_w();
  NSR_TRY(place(st, q.w9, S.Wp, 0, 0, w[F], S.W, S.W, S.W, 0, 0));
  NSR_TRY(place(st, q.w9, S.Wp, S.Wp, 0, w[S.sigma_w()], S.W, 1, S.W, 0, 0));
  NSR_TRY(place(st, q.b9, S.Wp + 32, 0, 0, w[F + 1], S.W, 1, S.W, 0, 0));
  NSR_TRY(place(st, q.b9, S.Wp + 32, 0, S.Wp, w[S.sigma_w() + 1], 1, 1, 1, 0, 0));
  NSR_TRY(place(st, q.wdir, S.Ci, 0, 0, w[S.dir_w()], S.dir_in(), S.H, S.W, 0, 0));
  if (!S.no_dir) NSR_TRY(place(st, q.wdir, S.Ci, 0, S.Wp, w[S.dir_w()], S.dir_in(), S.H, S.in_dir, S.W, 0));
  if (q.bdir) NSR_TRY(place(st, q.bdir, S.Hp, 0, 0, w[S.dir_w() + 1], S.H, 1, S.H, 0, 0));
  NSR_TRY(place(st, q.wrgb, S.Hp, 0, 0, w[S.rgb_w()], S.H, 3, S.H, 0, 0));
  NSR_TRY(place(st, q.brgb, 32, 0, 0, w[S.rgb_w() + 1], 3, 1, 3, 0, 0));
  if (split) {
    for (int l = 0; l < S.D; ++l) {
      const int64_t n = (int64_t)S.Wp * S.kin(l);
      NSR_TRY(split_f16(trunk_lin(S, q, w, l).w, n, q.hi[l], q.hi[l] + n, st));
    }
    const int64_t nf = (int64_t)S.Wp * S.Wp, ns = 32 * (int64_t)S.Wp, nd = (int64_t)S.Hp * S.Ci, nr = 32 * (int64_t)S.Hp;
    NSR_TRY(split_f16(q.w9, nf, q.hi[kFinalE], q.hi[kFinalE] + nf, st));
    NSR_TRY(split_f16(q.w9 + nf, ns, q.hi[kSigmaE], q.hi[kSigmaE] + ns, st));
    NSR_TRY(split_f16(q.wdir, nd, q.hi[kDirE], q.hi[kDirE] + nd, st));
    NSR_TRY(split_f16(q.wrgb, nr, q.hi[kRgbE], q.hi[kRgbE] + nr, st));
  }
  return NSR_OK;
}
// the transposed split halves of the matrices the input gradients multiply by (Pack::ht; hi then lo)
void nsr::carve_pack_t(Carver& a, const Shape& S, Pack& q) {
  for (int l = 0; l < S.D; ++l) q.ht[l] = reinterpret_cast<unsigned short*>(a.take((int64_t)S.Wp * S.kin(l)));
  q.ht[kFinalE] = reinterpret_cast<unsigned short*>(a.take((int64_t)(S.Wp + 32) * S.Wp));
  q.ht[kSigmaE] = nullptr;
  q.ht[kDirE] = reinterpret_cast<unsigned short*>(a.take((int64_t)S.Hp * S.Ci));
  q.ht[kRgbE] = reinterpret_cast<unsigned short*>(a.take(32 * (int64_t)S.Hp));
}
int nsr::prepare_weights_t(hipStream_t st, const Shape& S, const float* const* w, const Pack& q) {
  if (!q.ht[0]) return NSR_ERR_INVALID_ARG;
  for (int l = 0; l < S.D; ++l) {
    const Lin a = trunk_lin(S, q, w, l);
    NSR_TRY(split_f16_t(st, a.w, S.Wp, S.kin(l), a.ldw, q.ht[l], q.ht[l] + (int64_t)S.Wp * S.kin(l)));
  }
  const int ldg = S.Wp + 32;
  NSR_TRY(split_f16_t(st, q.w9, ldg, S.Wp, S.Wp, q.ht[kFinalE], q.ht[kFinalE] + (int64_t)ldg * S.Wp));
  NSR_TRY(split_f16_t(st, q.wdir, S.Hp, S.Ci, S.Ci, q.ht[kDirE], q.ht[kDirE] + (int64_t)S.Hp * S.Ci));
  NSR_TRY(split_f16_t(st, q.wrgb, 32, S.Hp, S.Hp, q.ht[kRgbE], q.ht[kRgbE] + 32 * (int64_t)S.Hp));
  return NSR_OK;
}

// one encoded row per sample point, columns [0, 4 n_groups), into each of the n_dst destinations (row stride ld floats)
int nsr::encode_arch(hipStream_t st, const float* rays, int ray_stride, const float* z, int64_t P, int N, int deg, int view_dir,
                     float* const* dst_rows, int n_dst, int64_t ld, int n_groups, unsigned embed, const NsrBands* bands) {
  if ((embed & NSR_EMBED_LINEAR_FREQS) && !bands) return NSR_ERR_INVALID_ARG;
  EncodeDst dst{};
  for (int j = 0; j < n_dst; ++j) dst.p[j] = dst_rows[j];
  dst.n = n_dst;
  const int64_t n = P * n_groups;
  hipLaunchKernelGGL(encode_arch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rays, ray_stride, z, P, N, deg,
                     view_dir, dst, ld, n_groups, embed, bands ? *bands : NsrBands{});
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

// E1 + cast_rays of the P = rays x N sample points, then the network with everything kept for the backward pass
int nsr::net_forward(hipStream_t st, const Shape& S, const float* rays, int ray_stride, const float* z, int N, const float* const* w,
                const Pack& q, const Kept& s, int64_t P, bool split, int color_none) {
  NSR_TRY(encode_arch(st, rays, ray_stride, z, P, N, S.arch.deg_pos, 0, s.x, S.n_x, (int64_t)S.ldx, S.Kx / 4, S.embed, &S.bands_pos));
  if (!S.no_dir) {
    float* const dir_rows = s.ci + S.Wp;
    NSR_TRY(encode_arch(st, rays, ray_stride, z, P, N, S.arch.deg_dir, 1, &dir_rows, 1, (int64_t)S.Ci, S.Dp / 4, S.embed, &S.bands_dir));
  }
  for (int l = 0; l < S.D; ++l) {
    const Mat x = in_of(S, s, l), y = out_of(S, s, l);
    const Lin a = trunk_lin(S, q, w, l);
    NSR_TRY(fwd(st, q, split, l, x.p, x.ld, S.kin(l), a.w, a.ldw, a.b, kActRelu, y.p, y.ld, P, S.Wp, S.Wp));
  }
  const Mat hD = out_of(S, s, S.D - 1);
  // xyz_encoding_final into the colour branch's input, the density head (stacked under it in w9) into column 3 of rgb
  NSR_TRY(fwd(st, q, split, kFinalE, hD.p, hD.ld, S.Wp, q.w9, S.Wp, q.b9, kActNone, s.ci, S.Ci, P, S.Wp, S.Wp));
  NSR_TRY(fwd(st, q, split, kSigmaE, hD.p, hD.ld, S.Wp, q.w9 + (int64_t)S.Wp * S.Wp, S.Wp, q.b9 + S.Wp, kActNone, s.rgb + 3, 4, P, 32, 1));
  NSR_TRY(fwd(st, q, split, kDirE, s.ci, S.Ci, S.Ci, q.wdir, S.Ci, q.bdir ? q.bdir : w[S.dir_w() + 1], kActRelu, s.cc, S.Hp, P, S.Hp, S.Hp));
  NSR_TRY(fwd(st, q, split, kRgbE, s.cc, S.Hp, S.Hp, q.wrgb, S.Hp, q.brgb, color_none ? kActNone : kActSigmoid, s.rgb, 4, P, 32, 3));
  return NSR_OK;
}

// backward of the network from k.d4 (composite_bwd's rows); g: its 2 D + 8 gradient tensors
// rg (null: none): also this pass's rows of d(loss) / d(rays) -- the input gradients of layer 0, of every skip layer's pe
// columns and of dir_encoding's direction columns (k.gpe, k.gdir), then encode_bwd and ray_grad
int nsr::net_backward(hipStream_t st, const Shape& S, const float* const* w, const Pack& q, const Work& k, int64_t P,
                      float* const* g, int acc, int stop_grad, const RayGrad* rg) {
  const Kept& s = k.kept;
  const int sp = n_splits(P);
  const int64_t ps = S.part_stride;
  float* part = k.partial;
  const int ldg = S.Wp + 32;
  // NSR_F16X3_GEMM_BWD: every product below on the split-fp16 MFMA.  Range word i holds the float bits of the largest magnitude
  // of one gradient matrix: 0 = d rgb_pre, 1 = d sigma (both from d4), 2 = the colour head's input gradient, 3 = dir_encoding's,
  // 4 = the stacked final + sigma layer's, 5 .. = the trunk layers' top down -- raised by the product that writes the matrix,
  // read by the weight gradient that contracts it over the points
  const bool f16 = q.ht[0] != nullptr;
  auto word = [&](int i) -> unsigned* { return f16 ? k.range + i : nullptr; };
  auto wt = [&](int e, int K, int64_t n, int row0) -> WT {   // rows row0 .. of entry e, a (rows x K) transposed copy of n halves
    return f16 ? WT{q.ht[e] + (int64_t)row0 * K, n, K} : WT{nullptr, 0, 0};
  };
  if (f16) {
    if (hipMemsetAsync(k.range, 0, kRangeWords * sizeof(unsigned), st) != hipSuccess) return NSR_ERR_LAUNCH;
    NSR_TRY(absmax_bits(st, k.d4, 4, P, 0, 3, word(0)));
    NSR_TRY(absmax_bits(st, k.d4, 4, P, 3, 1, word(1)));
  }
  const int64_t n_rgb = 32 * (int64_t)S.Hp, n_dir = (int64_t)S.Hp * S.Ci, n_w9 = (int64_t)ldg * S.Wp;
  NSR_TRY(scatter_heads(st, k.d4, P, k.drgb, k.g1 + S.Wp, ldg));
  // rgb head
  NSR_TRY(lin_wgrad(st, k.drgb, 32, 32, s.cc, S.Hp, S.Hp, P, part, sp, ps, word(0)));
  NSR_TRY(reduce_place(st, g[S.rgb_w()], S.H, 0, 3, S.H, part, sp, S.Hp, 0, 0, acc, 1.0f, ps));
  NSR_TRY(colsum(st, k.drgb, 32, P, 0, 3, g[S.rgb_w() + 1], acc, part));
  NSR_TRY(lin_dgrad(st, k.col_tiles, k.drgb, 32, 32, q.wrgb, S.Hp, s.cc, S.Hp, k.g0, S.Hp, P, S.Hp, g[S.dir_w() + 1], acc, S.H,
                    wt(kRgbE, 32, n_rgb, 0), word(2)));
  // dir_encoding: its input is [final | dir pe]
  NSR_TRY(lin_wgrad(st, k.g0, S.Hp, S.Hp, s.ci, S.Ci, S.Ci, P, part, sp, ps, word(2)));
  NSR_TRY(reduce_place(st, g[S.dir_w()], S.dir_in(), 0, S.H, S.W, part, sp, S.Ci, 0, 0, acc, 1.0f, ps));
  if (!S.no_dir) NSR_TRY(reduce_place(st, g[S.dir_w()], S.dir_in(), S.W, S.H, S.in_dir, part, sp, S.Ci, 0, S.Wp, acc, 1.0f, ps));
  const int F = S.final_w();
  if (stop_grad) {   // --stop_grad (models/networks.py:218-219): dir_encoding's input is detached, d final = 0
    if (hipMemset2DAsync(k.g1, (size_t)ldg * sizeof(float), 0, (size_t)S.Wp * sizeof(float), (size_t)P, st) != hipSuccess) return NSR_ERR_LAUNCH;
    if (!acc && hipMemsetAsync(g[F + 1], 0, (size_t)S.W * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
  } else {
    NSR_TRY(lin_dgrad(st, k.col_tiles, k.g0, S.Hp, S.Hp, q.wdir, S.Ci, nullptr, 0, k.g1, ldg, P, S.Wp, g[F + 1], acc, S.W,
                      wt(kDirE, S.Hp, n_dir, 0), word(3)));
  }
  // --stop_grad detaches dir_encoding's whole input, the encoded direction included
  const bool dir_term = rg && !S.no_dir && !stop_grad;
  if (dir_term) NSR_TRY(lin_dgrad(st, k.col_tiles, k.g0, S.Hp, S.Hp, q.wdir + S.Wp, S.Ci, nullptr, 0, k.gdir, S.Dp, P, S.Dp, nullptr, 0, 0,
                                  wt(kDirE, S.Hp, n_dir, S.Wp)));
  // xyz_encoding_final + sigma: the (Wp + 32)-row layer over the trunk's last activation
  const Mat hD = out_of(S, s, S.D - 1);
  NSR_TRY(lin_wgrad(st, k.g1, ldg, S.Wp, hD.p, hD.ld, S.Wp, P, part, sp, ps, word(3)));
  NSR_TRY(reduce_place(st, g[F], S.W, 0, S.W, S.W, part, sp, S.Wp, 0, 0, acc, 1.0f, ps));
  NSR_TRY(lin_wgrad(st, k.g1 + S.Wp, ldg, 32, hD.p, hD.ld, S.Wp, P, part, sp, ps, word(1)));
  NSR_TRY(reduce_place(st, g[S.sigma_w()], S.W, 0, 1, S.W, part, sp, S.Wp, 0, 0, acc, 1.0f, ps));
  NSR_TRY(colsum(st, k.g1, ldg, P, S.Wp, 1, g[S.sigma_w() + 1], acc, part));
  NSR_TRY(lin_dgrad(st, k.col_tiles, k.g1, ldg, ldg, q.w9, S.Wp, hD.p, hD.ld, k.g0, S.Wp, P, S.Wp, g[2 * (S.D - 1) + 1], acc, S.W,
                    wt(kFinalE, ldg, n_w9, 0), word(4)));
  // trunk, top down; the gradient of a layer's pre-activation alternates between the two buffers
  const float* dy = k.g0;
  float* nx = k.g1;
  int dyw = 4;   // the range word of dy
  for (int l = S.D - 1; l >= 0; --l) {
    const Mat x = in_of(S, s, l);
    const int kin = S.kin(l), fi = S.fan_in(l);
    NSR_TRY(lin_wgrad(st, dy, S.Wp, S.Wp, x.p, x.ld, kin, P, part, sp, ps, word(dyw)));
    float* gw = g[2 * l];
    if (S.skip(l)) {   // [pe | h] columns of the padded product -> the nn.Linear columns
      NSR_TRY(reduce_place(st, gw, fi, 0, S.W, S.in_xyz, part, sp, kin, 0, 0, acc, 1.0f, ps));
      NSR_TRY(reduce_place(st, gw, fi, S.in_xyz, S.W, S.W, part, sp, kin, 0, S.Kx, acc, 1.0f, ps));
    } else {
      NSR_TRY(reduce_place(st, gw, fi, 0, S.W, fi, part, sp, kin, 0, 0, acc, 1.0f, ps));
    }
    if (rg && (l == 0 || S.skip(l))) {   // the layer reads the encoded position: the gradient of its pe columns
      const Lin a = trunk_lin(S, q, w, l);
      NSR_TRY(lin_dgrad(st, k.col_tiles, dy, S.Wp, S.Wp, a.w, a.ldw, nullptr, 0, k.gpe + (int64_t)(l == 0 ? 0 : 1 + S.x_of[l]) * P * S.Kx, S.Kx, P, S.Kx,
                        nullptr, 0, 0, wt(l, S.Wp, (int64_t)S.Wp * kin, 0)));
    }
    if (l == 0) break;
    // the layer's input h is the ReLU output of layer l - 1: its mask, and that layer's bias gradient
    const Mat m = out_of(S, s, l - 1);
    const Lin a = trunk_lin(S, q, w, l);
    NSR_TRY(lin_dgrad(st, k.col_tiles, dy, S.Wp, S.Wp, a.w + (S.skip(l) ? S.Kx : 0), a.ldw, m.p, m.ld, nx, S.Wp, P, S.Wp, g[2 * (l - 1) + 1],
                      acc, S.W, wt(l, S.Wp, (int64_t)S.Wp * kin, S.skip(l) ? S.Kx : 0), word(dyw + 1)));
    ++dyw;
    const float* t0 = dy; dy = nx; nx = const_cast<float*>(t0);
  }
  if (!rg) return NSR_OK;
  const float* src[kMaxD];
  const int n_src = S.n_pe();   // layer 0 first, then the skip layers upwards
  for (int j = 0; j < n_src; ++j) src[j] = k.gpe + (int64_t)j * P * S.Kx;
  NSR_TRY(encode_bwd(st, src, n_src, S.Kx, s.x[0], S.ldx, P, S.arch.deg_pos, S.Kx / 4, S.embed, &S.bands_pos, k.gx));
  return ray_grad(st, k.gx, rg->z, rg->rays, rg->N, dir_term ? k.gdir : nullptr, S.Dp, s.ci + S.Wp, S.Ci, S.arch.deg_dir, S.embed,
                  &S.bands_dir, rg->rows, rg->stride, rg->acc);
}

// a trunk layer without a padded copy is the GEMMs' operand where the caller holds it: 16-byte aligned (include/nsr_train.h)
int nsr::check_alignment(const Shape& S, const float* const* w) {
  for (int l = 1; l < S.D; ++l)
    if (!S.skip(l) && S.W == S.Wp && (reinterpret_cast<uintptr_t>(w[2 * l]) & 15) != 0) return NSR_ERR_INVALID_ARG;
  return NSR_OK;
}

