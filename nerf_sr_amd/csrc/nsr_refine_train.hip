// Train-mode forward / backward pair of the refinement network (include/nsr_refine.h, "training"; reference:
// models/networks.py:735-990 in .train(), models/refine_model.py:84-175).  fp32, NHWC, one launch sequence per layer.
//
// Forward, per convolution: the raw weight re-laid tap-major (pack_conv_kernel without a fold) -> im2col over chunks of
// images -> gemm(), split-K in chains of 32 whose partials a reduce kernel adds in double -> the pre-activation Z (bias
// included) -> per-channel batch mean, then the centred sum of squares in
// a second pass -> running statistics (momentum; unbiased variance) -> normalise + affine + ReLU into the destination
// slice of the concatenated decoder buffers.  The encoder runs twice with the same weights (synthesised patches, then
// the B R reference patches), each call on its own batch statistics; the max over R keeps a uint8 winner index.
//
// Backward, per convolution in reverse: BatchNorm backward (two per-channel reductions, then dZ) -> weight gradient as a
// split-K gemm() with both operands K-major (k = output pixel; the im2col of the saved input is recomputed per chunk) and
// a fixed-order reduce of the partials -> dcol = dZ W as a gemm() with W K-major -> gather-form col2im (every input
// pixel sums its taps, through the x2 upsample those of its four upsampled pixels; no atomics).  The F_max gradients
// are routed to the winning reference, skip-connection gradients are accumulated in place in the gradient of the
// concatenated buffers, the encoder's second call adds into the gradients of its first.
//
// NSR_F16X3 (opt-in; nsr_refine_train_forward_p / _backward_p): the forward convolutions of layers 1 .. 18 are one
// gemm_f16x3 call per site that gathers the window from the saved fp32 input (no im2col, no split-K, no chunks), the input
// gradients of the stride-1 sites an implicit convolution of dZ with the flipped weight (nsr_refine_dgrad_f16.hip; behind an
// upsample at the upsampled extent, then a 2 x 2 fold).  Everything else, the weight gradients included, is as above, and the
// saved state is the same: a backward of either precision runs on the saved state of a forward of either.
//
// weight_grad = NSR_F16X3 (opt-in, independent of the precision; nsr_refine_train_backward_w): the weight gradient of every
// site but layer 0 is one implicit split-fp16 product over the whole site (nsr_refine_wgrad_f16.hip: no im2col, no chunks,
// pixel slices that are a function of the shape, added in order); the kernels that write dZ then raise the range word at
// every such site.  With NSR_FP32 nothing is launched differently.
//
// Every reduction has a fixed order (no float atomics): two identical calls give identical bits.  The 17 convolution
// biases in front of a BatchNorm are cancelled by the mean subtraction: their gradients are DEFINED as exact zeros.
//
// Zero padding the GEMM needs (K % 32 == 0): the rows of the im2col matrix past a chunk's last output pixel are zeroed,
// dZ carries 32 zeroed rows behind its last one, D.conv9's dZ is 32 columns wide (3 real) and the re-laid weight has
// pad32(Cout) rows, the padding ones zero.
#include "nsr_refine_conv.h"
#include "nsr_refine_train_work.h"

using namespace nsr;

namespace {

constexpr int kNL = NSR_REFINE_N_LAYERS;
constexpr int kNSites = 26;              // 7 (encoder, synthesised) + 7 (encoder, references) + 12 (decoder)
constexpr int kKpMax = 13824;            // 9 x 1536: D.conv3
constexpr int kCMax = 512;
constexpr int kMaxParts = kRefineMaxParts;   // row partitions of a per-channel reduction
constexpr int kMaxSplits = 64;
constexpr int kFwdKChunk = 32;          // forward: K summed by the MFMA in chains of 32 (one K tile), the chains added in double
constexpr int64_t kPartFloats = (int64_t)8 * kCMax * kKpMax;   // split-K partials of one weight gradient
constexpr uint64_t kMagic = 0x31545246525343ull;               // "CSRFRT1"
constexpr int64_t kHeaderFloats = 64;
struct Header {
  uint64_t magic, floats;
  int B, R, H, W, img_chunk, precision;   // precision: of the forward that wrote it (informative: a backward of either runs on it)
};
static_assert(sizeof(Header) <= kHeaderFloats * 4 && sizeof(Header) % 4 == 0, "header");

inline int64_t align64(int64_t n) { return (n + 63) & ~(int64_t)63; }
constexpr const Layer& layer(int l) { return kLayersV[0][l]; }
inline int kp_of(int l) { return pad32(9 * layer(l).cin); }
inline int np_of(int l) { return pad32(layer(l).cout); }
// positions of a layer's tensors: in the 106 (weight, bias, [gamma, beta, running_mean, running_var]), in the 72
// parameters (weight, bias, [gamma, beta]) and in the 34 running statistics (mean, var)
inline int t_of(int l) { return l == 0 ? 0 : 2 + 6 * (l - 1); }
inline int p_of(int l) { return l == 0 ? 0 : 2 + 4 * (l - 1); }
inline int r_of(int l) { return 2 * (l - 1); }

#define NSR_TRY(expr)              \
  do {                             \
    const int rc_ = (expr);        \
    if (rc_ != NSR_OK) return rc_; \
  } while (0)

// an NHWC activation (or its gradient): channels [ch0, ch0 + C) of a buffer with row stride ld
struct Act {
  float* p;
  int64_t ld;
  int ch0;
};
inline float* at(const Act& t) { return t.p + t.ch0; }

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------

// BatchNorm2d (train) + ReLU on one value; the backward recomputes the ReLU mask with the same expression
__device__ __forceinline__ float bn_act(float z, float mean, float rstd, float g, float b) {
  return nsr_relu_nan(__fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(z, mean), rstd), g), b));
}

// Per-channel sums over the rows of a (rows x C) matrix (ReduceArgs and its three modes: nsr_refine_train_work.h)
template <int MODE>
__global__ void __launch_bounds__(256) col_reduce_kernel(ReduceArgs a) {
  __shared__ float sh[2][4][64];
  const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6, c = blockIdx.x * 64 + cl, p = blockIdx.y;
  const int64_t rpp = (a.rows + a.nparts - 1) / a.nparts;
  const int64_t r0 = p * rpp, r1 = (r0 + rpp < a.rows) ? r0 + rpp : a.rows;
  float s0 = 0.0f, s1 = 0.0f;
  if (c < a.C) {
    float mean = 0.0f, rstd = 0.0f, g = 0.0f, b = 0.0f;
    if (MODE >= 1) mean = a.stat[c];
    if (MODE == 2) { rstd = a.stat[a.C + c]; g = a.gamma[c]; b = a.beta[c]; }
    for (int64_t r = r0 + rl; r < r1; r += 4) {
      const float x = a.x[r * a.ldx + c];
      if (MODE == 0) s0 += x;
      if (MODE == 1) { const float d = x - mean; s0 += d * d; }
      if (MODE == 2) {
        const float dy = bn_act(x, mean, rstd, g, b) > 0.0f ? a.da[r * a.ldda + c] : 0.0f;
        s0 += dy;
        s1 += dy * ((x - mean) * rstd);
      }
    }
  }
  sh[0][rl][cl] = s0;
  sh[1][rl][cl] = s1;
  __syncthreads();
  if (rl == 0 && c < a.C) {
    a.part[(int64_t)p * a.C + c] = ((sh[0][0][cl] + sh[0][1][cl]) + sh[0][2][cl]) + sh[0][3][cl];
    if (MODE == 2) a.part[((int64_t)a.nparts + p) * a.C + c] = ((sh[1][0][cl] + sh[1][1][cl]) + sh[1][2][cl]) + sh[1][3][cl];
  }
}

__device__ __forceinline__ double part_sum(const float* part, int nparts, int C, int c) {
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += (double)part[(int64_t)p * C + c];
  return s;
}
// the partitions in order -> mean[c]; running_mean (may be null) moves towards it
__global__ void fin_mean_kernel(const float* __restrict__ part, int nparts, int C, int64_t rows, float momentum,
                                float* __restrict__ stat, float* __restrict__ run_mean) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float mean = (float)(part_sum(part, nparts, C, c) / (double)rows);
  stat[c] = mean;
  if (run_mean) run_mean[c] = __fadd_rn(__fmul_rn(1.0f - momentum, run_mean[c]), __fmul_rn(momentum, mean));
}
// ... -> rstd[c] from the BIASED variance; running_var (may be null) moves towards the UNBIASED one
__global__ void fin_var_kernel(const float* __restrict__ part, int nparts, int C, int64_t rows, float momentum, float eps,
                               float* __restrict__ stat, float* __restrict__ run_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double ss = part_sum(part, nparts, C, c);
  const float var = (float)(ss / (double)rows);
  stat[C + c] = __fdiv_rn(1.0f, sqrtf(__fadd_rn(var, eps)));
  if (run_var) {
    const float unbiased = (float)(ss / (double)(rows - 1));
    run_var[c] = __fadd_rn(__fmul_rn(1.0f - momentum, run_var[c]), __fmul_rn(momentum, unbiased));
  }
}
// sums of MODE 2 -> d gamma = sum dy xhat, d beta = sum dy (added to what is there if `acc`); m[c] = sum dy / n,
// m[C + c] = sum dy xhat / n for bn_bwd_kernel
__global__ void fin_bn_bwd_kernel(const float* __restrict__ part, int nparts, int C, int64_t rows, int acc,
                                  float* __restrict__ g_gamma, float* __restrict__ g_beta, float* __restrict__ m) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double s1 = part_sum(part, nparts, C, c), s2 = part_sum(part + (int64_t)nparts * C, nparts, C, c);
  g_beta[c] = (acc ? g_beta[c] : 0.0f) + (float)s1;
  g_gamma[c] = (acc ? g_gamma[c] : 0.0f) + (float)s2;
  m[c] = (float)(s1 / (double)rows);
  m[C + c] = (float)(s2 / (double)rows);
}
// column sums of dZ -> bias gradient
__global__ void fin_bias_kernel(const float* __restrict__ part, int nparts, int C, int n_valid, int acc, float* __restrict__ g_bias) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_valid) return;
  g_bias[c] = (acc ? g_bias[c] : 0.0f) + (float)part_sum(part, nparts, C, c);
}

// dst[r][ch0 + c] = relu(gamma (z - mean) rstd + beta); one thread per channel quad
__global__ void __launch_bounds__(256) bn_relu_kernel(const float* __restrict__ z, const float* __restrict__ stat,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, int64_t rows,
                                                      int C, float* __restrict__ dst, int64_t ld) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * (C / 4)) return;
  const int c = (int)(idx % (C / 4)) * 4;
  const int64_t r = idx / (C / 4);
  const float4 v = *reinterpret_cast<const float4*>(z + r * C + c);
  const float4 mu = *reinterpret_cast<const float4*>(stat + c), rs = *reinterpret_cast<const float4*>(stat + C + c);
  const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c);
  *reinterpret_cast<float4*>(dst + r * ld + c) = make_float4(bn_act(v.x, mu.x, rs.x, g.x, b.x), bn_act(v.y, mu.y, rs.y, g.y, b.y),
                                                             bn_act(v.z, mu.z, rs.z, g.z, b.z), bn_act(v.w, mu.w, rs.w, g.w, b.w));
}

// The range word of the split-fp16 input gradient (nsr_refine_train_work.h): *max_bits = max(*max_bits, float bits of the
// wave's largest |v|).  Every lane of the wave calls it (lanes without an element pass 0).  An integer maximum of bit patterns
// does not depend on the order; the plain read in front only spares the atomics that could not raise the word.
__device__ __forceinline__ void raise_max_bits(unsigned* max_bits, unsigned bits) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)bits, o, 64);
    bits = bits > t ? bits : t;
  }
  if ((threadIdx.x & 63) == 0 && bits > __hip_atomic_load(max_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(max_bits, bits);
}
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// dZ = gamma rstd (dy - sum dy / n - xhat sum(dy xhat) / n), dy = dA [a > 0]
__global__ void __launch_bounds__(256) bn_bwd_kernel(const float* __restrict__ z, const float* __restrict__ da, int64_t ldda,
                                                     const float* __restrict__ stat, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ m, int64_t rows, int C,
                                                     float* __restrict__ dz, unsigned* __restrict__ max_bits) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned mb = 0u;
  if (idx < rows * (C / 4)) {
    const int c = (int)(idx % (C / 4)) * 4;
    const int64_t r = idx / (C / 4);
    const float4 v4 = *reinterpret_cast<const float4*>(z + r * C + c), d4 = *reinterpret_cast<const float4*>(da + r * ldda + c);
    const float v[4] = {v4.x, v4.y, v4.z, v4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float mean = stat[c + e], rstd = stat[C + c + e], g = gamma[c + e];
      const float dy = bn_act(v[e], mean, rstd, g, beta[c + e]) > 0.0f ? d[e] : 0.0f;
      const float xhat = (v[e] - mean) * rstd;
      o[e] = (g * rstd) * ((dy - m[c + e]) - xhat * m[C + c + e]);
    }
    *reinterpret_cast<float4*>(dz + r * C + c) = make_float4(o[0], o[1], o[2], o[3]);
    mb = umax(umax(abs_bits(o[0]), abs_bits(o[1])), umax(abs_bits(o[2]), abs_bits(o[3])));
  }
  if (max_bits) raise_max_bits(max_bits, mb);      // outside the branch: every lane of the wave takes part in the shuffles
}

// E.conv1 (ReLU only): dZ = dA [a > 0]
__global__ void __launch_bounds__(256) relu_bwd_kernel(const float* __restrict__ a, const float* __restrict__ da, int64_t n,
                                                       float* __restrict__ dz, unsigned* __restrict__ max_bits) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float v = 0.0f;
  if (idx < n) dz[idx] = v = a[idx] > 0.0f ? da[idx] : 0.0f;
  if (max_bits) raise_max_bits(max_bits, abs_bits(v));
}

// D.conv9 (tanh): dZ[(b, px)][c] = g_out[b][c][px] (1 - y^2) for c < 3, 0 for the 29 padding columns
__global__ void __launch_bounds__(256) tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ g_out, int64_t px_per_img,
                                                       int64_t rows, float* __restrict__ dz, unsigned* __restrict__ max_bits) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float v = 0.0f;
  if (idx < rows * 32) {
    const int c = (int)(idx & 31);
    const int64_t r = idx >> 5;
    if (c < 3) {
      const float t = y[r * 3 + c];
      v = g_out[((r / px_per_img) * 3 + c) * px_per_img + r % px_per_img] * (1.0f - t * t);
    }
    dz[idx] = v;
  }
  if (max_bits) raise_max_bits(max_bits, abs_bits(v));
}

// dst[(b, px)][c] = max_r src[(b R + r, px)][c], idx = the FIRST r that reaches it (torch.max; NaN wins as in torch)
__global__ void __launch_bounds__(256) max_idx_kernel(const float* __restrict__ src, int C, int R, int64_t px_per_img, int64_t n,
                                                      float* __restrict__ dst, int64_t ld, unsigned char* __restrict__ win) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over B * px * C
  if (idx >= n) return;
  const int c = (int)(idx % C);
  const int64_t bp = idx / C, b = bp / px_per_img, px = bp % px_per_img;
  float m = src[((b * R) * px_per_img + px) * C + c];
  int w = 0;
  for (int r = 1; r < R; ++r) {
    const float t = src[((b * R + r) * px_per_img + px) * C + c];
    if (!(m != m) && (t != t || t > m)) { m = t; w = r; }
  }
  dst[bp * ld + c] = m;
  win[idx] = (unsigned char)w;
}
// the gradient of the maximum goes to its winner: g_fc[(b R + r, px)][c] = (win == r) ? g_max[(b, px)][c] : 0
__global__ void __launch_bounds__(256) route_kernel(const float* __restrict__ g_max, int64_t ld, const unsigned char* __restrict__ win,
                                                    int C, int R, int64_t px_per_img, int64_t n, float* __restrict__ g_fc) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over B * px * C
  if (idx >= n) return;
  const int c = (int)(idx % C);
  const int64_t bp = idx / C, b = bp / px_per_img, px = bp % px_per_img;
  const float g = g_max[bp * ld + c];
  const int w = win[idx];
  for (int r = 0; r < R; ++r) g_fc[((b * R + r) * px_per_img + px) * C + c] = (r == w) ? g : 0.0f;
}

// Gather-form col2im of a 3x3 / pad 1 convolution: source pixel (img, sy, sx), channel quad c sums the entries of
// dcol (n_img Ho Wo, kp) that im2col_kernel copied from it -- <= 9 taps, <= 36 through the nearest x2 upsample --
// in a fixed order, and stores (or adds, `acc`) the sum at dst[(img, sy, sx)][c].
__global__ void __launch_bounds__(256) col2im_kernel(const float* __restrict__ dcol, int kp, int cin, int n_img, int Hs, int Ws,
                                                     int stride, int up, int Ho, int Wo, int acc, float* __restrict__ dst, int64_t ld) {
  const int q = cin / 4;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n_img * Hs * Ws * q) return;
  const int c = (int)(idx % q) * 4;
  const int64_t px = idx / q;
  const int sx = (int)(px % Ws), sy = (int)((px / Ws) % Hs), img = (int)(px / ((int64_t)Ws * Hs));
  const int rep = up ? 2 : 1;
  float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int dy = 0; dy < rep; ++dy)
    for (int dx = 0; dx < rep; ++dx) {
      const int iy = up ? 2 * sy + dy : sy, ix = up ? 2 * sx + dx : sx;   // pixel of the image the convolution saw
      for (int ky = 0; ky < 3; ++ky) {
        const int ty = iy + 1 - ky;                                       // = oy * stride
        if (ty < 0 || (ty % stride) != 0 || ty / stride >= Ho) continue;
        for (int kx = 0; kx < 3; ++kx) {
          const int tx = ix + 1 - kx;
          if (tx < 0 || (tx % stride) != 0 || tx / stride >= Wo) continue;
          const int64_t m = ((int64_t)img * Ho + ty / stride) * Wo + tx / stride;
          const float4 t = *reinterpret_cast<const float4*>(dcol + m * kp + (ky * 3 + kx) * cin + c);
          s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
      }
    }
  float4* d = reinterpret_cast<float4*>(dst + px * ld + c);
  if (acc) {
    const float4 o = *d;
    s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
  }
  *d = s;
}

// split-K partials (splits, M rows x kp, tap-major) in order -> g[n][c][tap] (the reference's (Cout, Cin, 3, 3))
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ part, int splits, int64_t split_stride, int kp,
                                                           int cin, int cout, int acc, float* __restrict__ g) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (n * cin + c) * 9 + tap
  if (idx >= (int64_t)cout * cin * 9) return;
  const int tap = (int)(idx % 9), c = (int)((idx / 9) % cin), n = (int)(idx / (9 * (int64_t)cin));
  const float* p = part + (int64_t)n * kp + tap * cin + c;
  float s = acc ? g[idx] : 0.0f;
  for (int z = 0; z < splits; ++z) s += p[z * split_stride];
  g[idx] = s;
}

// forward split-K partials (splits, M x np) added in order in double, + bias, activation -> dst[m][n] (n < cout)
__global__ void __launch_bounds__(256) fwd_reduce_kernel(const float* __restrict__ part, int splits, int64_t split_stride, int np,
                                                         int cout, const float* __restrict__ bias, int act, int64_t M,
                                                         float* __restrict__ dst, int64_t ld) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * cout) return;
  const int n = (int)(idx % cout);
  const int64_t m = idx / cout;
  const float* p = part + m * np + n;
  double s = 0.0;
  for (int z = 0; z < splits; ++z) s += (double)p[z * split_stride];
  float v = (float)(s + (double)bias[n]);
  if (act == kActRelu) v = nsr_relu_nan(v);
  else if (act == kActTanh) v = tanhf(v);
  dst[m * ld + n] = v;
}

// (B H W, 3) NHWC -> (B, 3, H, W)
__global__ void nhwc3_to_nchw_kernel(const float* __restrict__ src, int64_t px_per_img, int64_t n, float* __restrict__ dst) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int64_t px = idx % px_per_img, c = (idx / px_per_img) % 3, b = idx / (3 * px_per_img);
  dst[idx] = src[(b * px_per_img + px) * 3 + c];
}
__global__ void header_kernel(Header h, unsigned* __restrict__ dst) {
  const unsigned* src = reinterpret_cast<const unsigned*>(&h);
  const int i = threadIdx.x;
  if (i < (int)(sizeof(Header) / 4)) dst[i] = src[i];
}

inline dim3 blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// launchers (nsr_refine_train_work.h): the only places the kernels above are launched from
// ---------------------------------------------------------------------------------------------------------------
namespace nsr {

int refine_col_reduce(hipStream_t st, int mode, ReduceArgs a) {
  a.nparts = refine_reduce_parts(a.rows);
  const dim3 grid((unsigned)((a.C + 63) / 64), (unsigned)a.nparts);
  if (mode == 0) hipLaunchKernelGGL(col_reduce_kernel<0>, grid, dim3(256), 0, st, a);
  else if (mode == 1) hipLaunchKernelGGL(col_reduce_kernel<1>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(col_reduce_kernel<2>, grid, dim3(256), 0, st, a);
  NSR_CHECK_LAUNCH();
  return a.nparts;
}
int refine_fin_mean(hipStream_t st, const float* part, int nparts, int C, int64_t rows, float momentum, float* stat, float* run_mean) {
  hipLaunchKernelGGL(fin_mean_kernel, dim3((C + 255) / 256), dim3(256), 0, st, part, nparts, C, rows, momentum, stat, run_mean);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_fin_var(hipStream_t st, const float* part, int nparts, int C, int64_t rows, float momentum, float eps, float* stat,
                   float* run_var) {
  hipLaunchKernelGGL(fin_var_kernel, dim3((C + 255) / 256), dim3(256), 0, st, part, nparts, C, rows, momentum, eps, stat, run_var);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_fin_bn_bwd(hipStream_t st, const float* part, int nparts, int C, int64_t rows, int acc, float* g_gamma, float* g_beta,
                      float* m) {
  hipLaunchKernelGGL(fin_bn_bwd_kernel, dim3((C + 255) / 256), dim3(256), 0, st, part, nparts, C, rows, acc, g_gamma, g_beta, m);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_fin_bias(hipStream_t st, const float* part, int nparts, int C, int n_valid, int acc, float* g_bias) {
  hipLaunchKernelGGL(fin_bias_kernel, dim3((C + 255) / 256), dim3(256), 0, st, part, nparts, C, n_valid, acc, g_bias);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_bn_relu(hipStream_t st, const float* z, const float* stat, const float* gamma, const float* beta, int64_t rows, int C,
                   float* dst, int64_t ld) {
  hipLaunchKernelGGL(bn_relu_kernel, blocks(rows * (C / 4)), dim3(256), 0, st, z, stat, gamma, beta, rows, C, dst, ld);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_bn_bwd(hipStream_t st, const float* z, const float* da, int64_t ldda, const float* stat, const float* gamma,
                  const float* beta, const float* m, int64_t rows, int C, float* dz, unsigned* max_bits) {
  hipLaunchKernelGGL(bn_bwd_kernel, blocks(rows * (C / 4)), dim3(256), 0, st, z, da, ldda, stat, gamma, beta, m, rows, C, dz, max_bits);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_relu_bwd(hipStream_t st, const float* a, const float* da, int64_t n, float* dz, unsigned* max_bits) {
  hipLaunchKernelGGL(relu_bwd_kernel, blocks(n), dim3(256), 0, st, a, da, n, dz, max_bits);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_tanh_bwd(hipStream_t st, const float* y, const float* g_out, int64_t px_per_img, int64_t rows, float* dz, unsigned* max_bits) {
  hipLaunchKernelGGL(tanh_bwd_kernel, blocks(rows * 32), dim3(256), 0, st, y, g_out, px_per_img, rows, dz, max_bits);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_max_idx(hipStream_t st, const float* src, int C, int R, int64_t px_per_img, int B, float* dst, int64_t ld,
                   unsigned char* win) {
  const int64_t n = (int64_t)B * px_per_img * C;
  hipLaunchKernelGGL(max_idx_kernel, blocks(n), dim3(256), 0, st, src, C, R, px_per_img, n, dst, ld, win);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_route(hipStream_t st, const float* g_max, int64_t ld, const unsigned char* win, int C, int R, int64_t px_per_img, int B,
                 float* g_fc) {
  const int64_t n = (int64_t)B * px_per_img * C;
  hipLaunchKernelGGL(route_kernel, blocks(n), dim3(256), 0, st, g_max, ld, win, C, R, px_per_img, n, g_fc);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_col2im(hipStream_t st, const float* dcol, int kp, int cin, int n_img, int Hs, int Ws, int stride, int up, int Ho, int Wo,
                  int acc, float* dst, int64_t ld) {
  const int64_t n = (int64_t)n_img * Hs * Ws * (cin / 4);
  hipLaunchKernelGGL(col2im_kernel, blocks(n), dim3(256), 0, st, dcol, kp, cin, n_img, Hs, Ws, stride, up, Ho, Wo, acc, dst, ld);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_wgrad_reduce(hipStream_t st, const float* part, int splits, int64_t split_stride, int kp, int cin, int cout, int acc,
                        float* g) {
  hipLaunchKernelGGL(wgrad_reduce_kernel, blocks((int64_t)cout * cin * 9), dim3(256), 0, st, part, splits, split_stride, kp, cin, cout,
                     acc, g);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_fwd_reduce(hipStream_t st, const float* part, int splits, int64_t split_stride, int np, int cout, const float* bias, int act,
                      int64_t M, float* dst, int64_t ld) {
  hipLaunchKernelGGL(fwd_reduce_kernel, blocks(M * cout), dim3(256), 0, st, part, splits, split_stride, np, cout, bias, act, M, dst, ld);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
int refine_nhwc3_to_nchw(hipStream_t st, const float* src, int64_t px_per_img, int B, float* dst) {
  const int64_t n = (int64_t)B * 3 * px_per_img;
  hipLaunchKernelGGL(nhwc3_to_nchw_kernel, blocks(n), dim3(256), 0, st, src, px_per_img, n, dst);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

}  // namespace nsr

namespace {

// ---------------------------------------------------------------------------------------------------------------
// layouts
// ---------------------------------------------------------------------------------------------------------------

// Saved state.  Floats per patch set (P = H W pixels, R references), without the 64-float header and the per-layer
// statistics (26 x 1024 floats per call):
//   encoder, per image (1 + R of them): input 3 P | A1 128 P | Z2, A2 2 x 128 P | Z3, A3, Z4, A4 4 x 64 P |
//                                       Z5, A5, Z6, A6 4 x 32 P | Z7, A7 2 x 8 P                     = 787 P
//     (the synthesised call's A2, A4, A6, A7 live in the concatenated decoder inputs below: 232 P less for that image)
//   decoder: cat1 16 P | cat3 96 P | cat5 192 P | cat7 384 P | Z of 11 layers 688 P | A of 8 plain layers 464 P | rgb 3 P
//   winner indices: 232 P bytes
// = (787 R + 2398) P floats + 232 P bytes: 143 MB for R = 8, P = 64 x 64; 4.6 GB for the reference's batch of 32.
struct Saved {
  float *x[2];                          // the two input tensors, NCHW (E.conv1's weight gradient reads them)
  float *a1[2], *a3[2], *a5[2];         // plain encoder activations of the two calls
  float *fc[4];                         // the reference call's features before the max
  float *cat1, *cat3, *cat5, *cat7;     // decoder inputs [x_up | F_synth | F_max]
  float *d[8];                          // plain decoder activations: D.conv1, 2, 3, 4, 5, 6, 7, 8
  float *rgb;                           // tanh output, NHWC
  float *Z[kNSites], *stat[kNSites];
  unsigned char* win[4];
};
struct Carver {
  float* base;
  int64_t off;
  float* take(int64_t n) {
    float* p = base ? base + off : nullptr;
    off += align64(n);
    return p;
  }
};
// site numbering: 0..6 encoder on the synthesised patches, 7..13 encoder on the references, 14..25 decoder (layers 7..18)
inline int site_layer(int s) { return s < 7 ? s : (s < 14 ? s - 7 : s - 7); }
inline int site_call(int s) { return s < 7 ? 0 : (s < 14 ? 1 : 2); }

int64_t carve_saved(int B, int R, int H, int W, Saved* out, float* base) {
  const int64_t px[4] = {(int64_t)H * W, (int64_t)H * W / 4, (int64_t)H * W / 16, (int64_t)H * W / 64};
  const int64_t n[3] = {B, (int64_t)B * R, B};
  const int lvl[kNL] = {0, 0, 1, 1, 2, 2, 3, 3, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0, 0};   // output level of a layer
  Carver a{base, kHeaderFloats};
  Saved tmp;
  Saved& k = out ? *out : tmp;
  for (int c = 0; c < 2; ++c) {
    k.x[c] = a.take(n[c] * px[0] * 3);
    k.a1[c] = a.take(n[c] * px[0] * 128);
    k.a3[c] = a.take(n[c] * px[1] * 256);
    k.a5[c] = a.take(n[c] * px[2] * 512);
  }
  const int fcw[4] = {128, 256, 512, 512};
  for (int i = 0; i < 4; ++i) k.fc[i] = a.take(n[1] * px[i] * fcw[i]);
  k.cat1 = a.take(B * px[3] * 1024);
  k.cat3 = a.take(B * px[2] * 1536);
  k.cat5 = a.take(B * px[1] * 768);
  k.cat7 = a.take(B * px[0] * 384);
  const int dl[8] = {7, 8, 10, 11, 13, 14, 16, 17};
  for (int i = 0; i < 8; ++i) k.d[i] = a.take(B * px[lvl[dl[i]]] * layer(dl[i]).cout);
  k.rgb = a.take(B * px[0] * 3);
  for (int s = 0; s < kNSites; ++s) {
    const int l = site_layer(s);
    k.Z[s] = layer(l).bn ? a.take(n[site_call(s)] * px[lvl[l]] * layer(l).cout) : nullptr;
    k.stat[s] = a.take(2 * kCMax);
  }
  for (int i = 0; i < 4; ++i) k.win[i] = reinterpret_cast<unsigned char*>(a.take((B * px[i] * fcw[i] + 3) / 4));
  return a.off;
}

struct Work {
  float *col, *dcol, *wr, *part, *red, *m;
  int64_t dcol_floats;
  float *gz, *ga, *gb;                       // dZ of the layer at hand, two ping-pong activation gradients
  float *gcat1, *gcat3, *gcat5, *gcat7;      // gradients of the concatenated decoder inputs
  float *gfc[4];                             // gradients of the reference call's features
};
int resolve_chunk(int B, int R, int H, int W, int img_chunk) {
  const int64_t n = (int64_t)B * R;
  int64_t c = img_chunk;
  if (c <= 0) c = ((int64_t)1 << 28) / ((int64_t)H * W * 3456);   // an im2col matrix of at most 1 GiB
  c = c < 1 ? 1 : c;
  return (int)(c > n ? n : c);
}
int64_t carve_work(int B, int R, int H, int W, int chunk, Work* out, float* base) {
  const int64_t px[4] = {(int64_t)H * W, (int64_t)H * W / 4, (int64_t)H * W / 16, (int64_t)H * W / 64};
  const int64_t nref = (int64_t)B * R;
  Carver a{base, 0};
  Work tmp;
  Work& k = out ? *out : tmp;
  // widest im2col row per full-resolution pixel: D.conv7 (9 x 384); 32 padding rows of the widest layer behind it
  const int64_t col = (int64_t)chunk * px[0] * 3456 + (int64_t)32 * kKpMax;
  k.col = a.take(col);
  k.dcol = a.take(col);
  k.dcol_floats = col;
  k.wr = a.take((int64_t)kCMax * kKpMax + kCMax);
  k.part = a.take(kPartFloats);
  k.red = a.take((int64_t)2 * kMaxParts * kCMax);
  k.m = a.take(2 * kCMax);
  const int64_t act = nref * px[0] * 128;
  k.gz = a.take(act + 32 * kCMax);
  k.ga = a.take(act);
  k.gb = a.take(act);
  k.gcat1 = a.take(B * px[3] * 1024);
  k.gcat3 = a.take(B * px[2] * 1536);
  k.gcat5 = a.take(B * px[1] * 768);
  k.gcat7 = a.take(B * px[0] * 384);
  const int fcw[4] = {128, 256, 512, 512};
  for (int i = 0; i < 4; ++i) k.gfc[i] = a.take(nref * px[i] * fcw[i]);
  return a.off;
}

// one convolution of one call: where it reads and writes, forward and backward
struct Site {
  int l, call, n_img, Hs, Ws;     // Hs x Ws: the source (before the optional upsample)
  Act src;                        // input activation (unused by layer 0: the NCHW input tensor)
  Act dst;                        // output activation
  float *Z, *stat;
  Act gdst;                       // gradient of the output activation
  Act gsrc; int gacc;             // gradient of the input activation: stored, or added to what is there
};

void encoder_sites(Site* s, int call, int n_img, int H, int W, const Saved& k, const Work& w, const Act (&f)[4], const Act (&g)[4]) {
  const Act a1{k.a1[call], 128, 0}, a3{k.a3[call], 256, 0}, a5{k.a5[call], 512, 0};
  const Act ga128{w.ga, 128, 0}, gb256{w.gb, 256, 0}, ga512{w.ga, 512, 0}, none{nullptr, 0, 0};
  const Site t[7] = {
      {0, call, n_img, H, W, none, a1, nullptr, nullptr, ga128, none, 0},
      {1, call, n_img, H, W, a1, f[0], nullptr, nullptr, g[0], ga128, 0},
      {2, call, n_img, H, W, f[0], a3, nullptr, nullptr, gb256, g[0], 1},
      {3, call, n_img, H / 2, W / 2, a3, f[1], nullptr, nullptr, g[1], gb256, 0},
      {4, call, n_img, H / 2, W / 2, f[1], a5, nullptr, nullptr, ga512, g[1], 1},
      {5, call, n_img, H / 4, W / 4, a5, f[2], nullptr, nullptr, g[2], ga512, 0},
      {6, call, n_img, H / 4, W / 4, f[2], f[3], nullptr, nullptr, g[3], g[2], 1},
  };
  for (int i = 0; i < 7; ++i) s[i] = t[i];
}

void build_sites(Site* s, int B, int R, int H, int W, const Saved& k, const Work& w) {
  const Act cat1{k.cat1, 1024, 0}, cat3{k.cat3, 1536, 0}, cat5{k.cat5, 768, 0}, cat7{k.cat7, 384, 0};
  const Act gcat1{w.gcat1, 1024, 0}, gcat3{w.gcat3, 1536, 0}, gcat5{w.gcat5, 768, 0}, gcat7{w.gcat7, 384, 0};
  auto slice = [](Act t, int ch0) { t.ch0 = ch0; return t; };
  const Act fs[4] = {slice(cat7, 128), slice(cat5, 256), slice(cat3, 512), cat1};
  const Act gs[4] = {slice(gcat7, 128), slice(gcat5, 256), slice(gcat3, 512), gcat1};
  const Act fr[4] = {{k.fc[0], 128, 0}, {k.fc[1], 256, 0}, {k.fc[2], 512, 0}, {k.fc[3], 512, 0}};
  const Act gr[4] = {{w.gfc[0], 128, 0}, {w.gfc[1], 256, 0}, {w.gfc[2], 512, 0}, {w.gfc[3], 512, 0}};
  encoder_sites(s, 0, B, H, W, k, w, fs, gs);
  encoder_sites(s + 7, 1, B * R, H, W, k, w, fr, gr);
  const int h3 = H / 8, w3 = W / 8;
  auto d = [&](int i) { const int dl[8] = {7, 8, 10, 11, 13, 14, 16, 17}; return Act{k.d[i], layer(dl[i]).cout, 0}; };
  auto ga = [&](int C) { return Act{w.ga, C, 0}; };
  auto gb = [&](int C) { return Act{w.gb, C, 0}; };
  const Act none{nullptr, 0, 0}, rgb{k.rgb, 3, 0};
  const Site t[12] = {
      {7, 2, B, h3, w3, cat1, d(0), nullptr, nullptr, gb(512), gcat1, 0},
      {8, 2, B, h3, w3, d(0), d(1), nullptr, nullptr, ga(512), gb(512), 0},
      {9, 2, B, h3, w3, d(1), cat3, nullptr, nullptr, gcat3, ga(512), 0},                       // upsample + conv2_up
      {10, 2, B, 2 * h3, 2 * w3, cat3, d(2), nullptr, nullptr, gb(512), gcat3, 0},
      {11, 2, B, 2 * h3, 2 * w3, d(2), d(3), nullptr, nullptr, ga(512), gb(512), 0},
      {12, 2, B, 2 * h3, 2 * w3, d(3), cat5, nullptr, nullptr, gcat5, ga(512), 0},              // upsample + conv4_up
      {13, 2, B, 4 * h3, 4 * w3, cat5, d(4), nullptr, nullptr, gb(256), gcat5, 0},
      {14, 2, B, 4 * h3, 4 * w3, d(4), d(5), nullptr, nullptr, ga(256), gb(256), 0},
      {15, 2, B, 4 * h3, 4 * w3, d(5), cat7, nullptr, nullptr, gcat7, ga(256), 0},              // upsample + conv6_up
      {16, 2, B, H, W, cat7, d(6), nullptr, nullptr, gb(128), gcat7, 0},
      {17, 2, B, H, W, d(6), d(7), nullptr, nullptr, ga(128), gb(128), 0},
      {18, 2, B, H, W, d(7), rgb, nullptr, nullptr, none, ga(128), 0},
  };
  for (int i = 0; i < 12; ++i) s[14 + i] = t[i];
  for (int i = 0; i < kNSites; ++i) {
    s[i].Z = k.Z[i];
    s[i].stat = k.stat[i];
  }
}

struct Geo {
  int Ho, Wo, kp, np;
  int64_t rows_img;
};
Geo geo(const Site& s) {
  const Layer& L = layer(s.l);
  const int Hin = L.up ? 2 * s.Hs : s.Hs, Win = L.up ? 2 * s.Ws : s.Ws;
  Geo g;
  g.Ho = (Hin - 1) / L.stride + 1;
  g.Wo = (Win - 1) / L.stride + 1;
  g.kp = kp_of(s.l);
  g.np = np_of(s.l);
  g.rows_img = (int64_t)g.Ho * g.Wo;
  return g;
}

// f16x3: the same matrix x 2^6 as (hi, lo) fp16 halves (pack_conv_kernel), the operand of gemm_f16x3
int relayout(hipStream_t st, const Site& s, const float* const* t, float* wr, int f16x3 = 0) {
  const Layer& L = layer(s.l);
  const int kp = kp_of(s.l), np = np_of(s.l);
  const int64_t n = (int64_t)np * kp + np;
  hipLaunchKernelGGL(pack_conv_kernel, blocks(n), dim3(256), 0, st, t[t_of(s.l)], t[t_of(s.l) + 1], (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, L.cin, L.cout, kp, np, f16x3, wr);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
// the im2col matrix of images [i0, i0 + nc) of the site's input
int im2col(hipStream_t st, const Site& s, const Geo& g, const float* x_nchw, int i0, int nc, float* col) {
  const Layer& L = layer(s.l);
  const int64_t total = (int64_t)nc * g.rows_img * (g.kp / 4);
  if (s.l == 0)
    hipLaunchKernelGGL(im2col_kernel<true>, blocks(total), dim3(256), 0, st, x_nchw + (int64_t)i0 * 3 * s.Hs * s.Ws, (int64_t)0, L.cin, nc,
                       s.Hs, s.Ws, L.stride, L.up, g.Ho, g.Wo, g.kp, col);
  else
    hipLaunchKernelGGL(im2col_kernel<false>, blocks(total), dim3(256), 0, st, at(s.src) + (int64_t)i0 * s.Hs * s.Ws * s.src.ld, s.src.ld,
                       L.cin, nc, s.Hs, s.Ws, L.stride, L.up, g.Ho, g.Wo, g.kp, col);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
#define NSR_REDUCE(np_, ...)          \
  do {                                \
    np_ = refine_col_reduce(__VA_ARGS__); \
    if (np_ < 0) return np_;          \
  } while (0)

// the range word of a site's split-fp16 input gradient (nsr_refine_train_work.h): the first of the kCMax floats behind the
// re-laid weight, which hold the bias in the forward and nothing the backward reads
inline unsigned* range_word(const Work& w) { return reinterpret_cast<unsigned*>(w.wr + (int64_t)kCMax * kKpMax); }

int site_forward(hipStream_t st, const Site& s, const float* const* t, float* const* running, float momentum, const float* x_nchw,
                 int chunk, const Work& w, int prec) {
  const Layer& L = layer(s.l);
  const Geo g = geo(s);
  // NSR_F16X3, layers 1 .. 18 (cin % 32 == 0): ONE split-fp16 GEMM per site that gathers the 3 x 3 window from the saved fp32
  // input while it stages it -- no im2col, no split-K, no chunks.  Layer 0 (K = 32) stays on the fp32 route.
  const bool f16 = prec == NSR_F16X3 && s.l != 0;
  NSR_TRY(relayout(st, s, t, w.wr, f16 ? 1 : 0));
  if (f16)
    NSR_TRY(refine_conv_f16x3(st, at(s.src), s.src.ld, L.cin, s.n_img, s.Hs, s.Ws, L.stride, L.up, w.wr, g.np, L.cout,
                              L.bn ? (int)kActNone : L.act, L.bn ? s.Z : at(s.dst), L.bn ? (int64_t)L.cout : s.dst.ld));
  for (int i0 = 0; i0 < s.n_img && !f16; i0 += chunk) {
    const int nc = s.n_img - i0 < chunk ? s.n_img - i0 : chunk;
    NSR_TRY(im2col(st, s, g, x_nchw, i0, nc, w.col));
    // K in chains of kFwdKChunk: in ONE chain the fp32 MFMA adds a K of up to 13,824 with 2.5 - 4 x the rounding error of
    // the reference's blocked fp32 convolution, which moves ReLU decisions the reference's fp32 run shares with fp64 (and
    // with them whole gradients by 1e-3).  The partials go to the backward's dcol buffer (free here), as many rows per
    // pass as fit, and are added in double, then bias and activation.
    const int64_t M = (int64_t)nc * g.rows_img;
    const int splits = g.kp / kFwdKChunk > 1 ? g.kp / kFwdKChunk : 1;
    const int64_t ld = L.bn ? (int64_t)L.cout : s.dst.ld;
    float* dst = (L.bn ? s.Z : at(s.dst)) + (int64_t)i0 * g.rows_img * ld;
    int64_t pass = w.dcol_floats / ((int64_t)splits * g.np);      // rows whose partials fit
    pass = pass > M ? M : pass;
    for (int64_t m0 = 0; m0 < M; m0 += pass) {
      const int64_t mb = M - m0 < pass ? M - m0 : pass;
      GemmArgs a{};
      a.A = w.col + m0 * g.kp; a.lda = g.kp; a.B = w.wr; a.ldb = g.kp; a.C = w.dcol; a.ldc = g.np;
      a.M = mb; a.N = g.np; a.K = g.kp; a.n_valid = L.cout; a.act = kActNone; a.splits = splits; a.split_stride = mb * g.np;
      NSR_TRY(gemm(a, st));
      NSR_TRY(refine_fwd_reduce(st, w.dcol, splits, a.split_stride, g.np, L.cout, w.wr + (int64_t)g.np * g.kp,
                                L.bn ? (int)kActNone : L.act, mb, dst + m0 * ld, ld));
    }
  }
  if (!L.bn) return NSR_OK;
  // batch statistics over the WHOLE call: mean, then the centred sum of squares
  const int64_t rows = (int64_t)s.n_img * g.rows_img;
  const int C = L.cout;
  float* rm = running ? running[r_of(s.l)] : nullptr;
  float* rv = running ? running[r_of(s.l) + 1] : nullptr;
  ReduceArgs r{};
  r.x = s.Z; r.ldx = C; r.stat = s.stat; r.rows = rows; r.C = C; r.part = w.red;
  int np;
  NSR_REDUCE(np, st, 0, r);
  NSR_TRY(refine_fin_mean(st, w.red, np, C, rows, momentum, s.stat, rm));
  NSR_REDUCE(np, st, 1, r);
  NSR_TRY(refine_fin_var(st, w.red, np, C, rows, momentum, kBnEps, s.stat, rv));
  const float* gamma = t[t_of(s.l) + 2];
  const float* beta = t[t_of(s.l) + 3];
  return refine_bn_relu(st, s.Z, s.stat, gamma, beta, rows, C, at(s.dst), s.dst.ld);
}

// `acc`: this site adds to the parameter gradients (the encoder's second call)
int site_backward(hipStream_t st, const Site& s, const float* const* t, float* const* grads, const float* g_out, const float* x_nchw,
                  int chunk, const Work& w, int acc, int prec, int wgrad) {
  const Layer& L = layer(s.l);
  const Geo g = geo(s);
  const int64_t rows = (int64_t)s.n_img * g.rows_img;
  const int C = L.cout, ldz = g.np;       // dZ is dense: Cout columns, 32 for D.conv9
  const int p = p_of(s.l);
  int np;
  // NSR_F16X3: the input gradient of a stride-1 site is an implicit convolution of dZ on the split-fp16 MFMA; the kernel that
  // writes dZ leaves its largest magnitude in the range word.  Stride-2 sites (the accumulating ones) keep dcol + col2im.
  const bool implicit = prec == NSR_F16X3 && s.l != 0 && L.stride == 1;
  // weight_grad = NSR_F16X3: the weight gradient of every site but layer 0 (K = 27) is one implicit split-fp16 product over
  // the whole site (nsr_refine_wgrad_f16.hip), scaled by the same range word
  const bool wg16 = wgrad == NSR_F16X3 && s.l != 0;
  unsigned* const mbits = (implicit || wg16) ? range_word(w) : nullptr;
  if (implicit && s.gacc) return NSR_ERR_UNSUPPORTED;
  if (mbits && hipMemsetAsync(mbits, 0, sizeof(unsigned), st) != hipSuccess) return NSR_ERR_LAUNCH;
  // ---- dZ and the gradients of the per-channel parameters
  if (L.bn) {
    const float *gamma = t[t_of(s.l) + 2], *beta = t[t_of(s.l) + 3];
    ReduceArgs r{};
    r.x = s.Z; r.ldx = C; r.da = at(s.gdst); r.ldda = s.gdst.ld; r.stat = s.stat; r.gamma = gamma; r.beta = beta;
    r.rows = rows; r.C = C; r.part = w.red;
    NSR_REDUCE(np, st, 2, r);
    NSR_TRY(refine_fin_bn_bwd(st, w.red, np, C, rows, acc, grads[p + 2], grads[p + 3], w.m));
    NSR_TRY(refine_bn_bwd(st, s.Z, at(s.gdst), s.gdst.ld, s.stat, gamma, beta, w.m, rows, C, w.gz, mbits));
    // the bias in front of a BatchNorm is cancelled by the mean subtraction: its gradient is exactly zero
    if (!acc && hipMemsetAsync(grads[p + 1], 0, (size_t)C * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
  } else {
    if (L.act == kActTanh) NSR_TRY(refine_tanh_bwd(st, s.dst.p, g_out, g.rows_img, rows, w.gz, mbits));
    else NSR_TRY(refine_relu_bwd(st, s.dst.p, s.gdst.p, rows * C, w.gz));
    ReduceArgs r{};
    r.x = w.gz; r.ldx = ldz; r.rows = rows; r.C = ldz; r.part = w.red;
    NSR_REDUCE(np, st, 0, r);
    NSR_TRY(refine_fin_bias(st, w.red, np, ldz, C, acc, grads[p + 1]));
  }
  // 32 zeroed rows behind dZ: the K padding of the last chunk's weight-gradient product
  if (hipMemsetAsync(w.gz + rows * ldz, 0, (size_t)32 * ldz * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
  // in front of the re-layout below: the bias it writes behind the widest layer's weight lands on the range word
  if (wg16)
    NSR_TRY(refine_wgrad_f16x3(st, w.gz, ldz, C, at(s.src), s.src.ld, L.cin, s.n_img, s.Hs, s.Ws, L.stride, L.up, mbits, w.part,
                               kPartFloats, acc, grads[p]));
  if (implicit) NSR_TRY(refine_flip_pack(st, t[t_of(s.l)], L.cin, C, g.np, reinterpret_cast<unsigned short*>(w.wr)));
  else if (s.l != 0) NSR_TRY(relayout(st, s, t, w.wr));
  const int Mw = C < 4 ? 4 : C;           // rows of the weight-gradient product (a K-major operand needs >= 4)
  for (int i0 = 0; i0 < s.n_img && !(wg16 && implicit); i0 += chunk) {
    const int nc = s.n_img - i0 < chunk ? s.n_img - i0 : chunk;
    const int64_t M = (int64_t)nc * g.rows_img, Kp = (M + 31) & ~(int64_t)31;
    const float* dz = w.gz + (int64_t)i0 * g.rows_img * ldz;
    if (!wg16) {
      // ---- weight gradient: dW[n][k] = sum over the output pixels p of dZ[p][n] col[p][k]
      NSR_TRY(im2col(st, s, g, x_nchw, i0, nc, w.col));
      if (Kp > M && hipMemsetAsync(w.col + M * g.kp, 0, (size_t)(Kp - M) * g.kp * sizeof(float), st) != hipSuccess) return NSR_ERR_LAUNCH;
      int64_t splits = Kp / 256, cap = kPartFloats / ((int64_t)Mw * g.kp);
      splits = splits > cap ? cap : splits;
      splits = splits > kMaxSplits ? kMaxSplits : (splits < 1 ? 1 : splits);
      GemmArgs a{};
      a.A = dz; a.lda = ldz; a.a_kmajor = 1; a.B = w.col; a.ldb = g.kp; a.b_kmajor = 1;
      a.C = w.part; a.ldc = g.kp; a.M = Mw; a.N = g.kp; a.K = Kp; a.n_valid = g.kp; a.act = kActNone;
      a.splits = (int)splits; a.split_stride = (int64_t)Mw * g.kp;
      NSR_TRY(gemm(a, st));
      NSR_TRY(refine_wgrad_reduce(st, w.part, (int)splits, a.split_stride, g.kp, L.cin, C, (acc || i0 > 0) ? 1 : 0, grads[p]));
    }
    if (s.l == 0 || implicit) continue;   // no gradient with respect to the input images; implicit: below, whole site
    // ---- input gradient: dcol = dZ W, then every input pixel gathers its taps
    GemmArgs d{};
    d.A = dz; d.lda = ldz; d.B = w.wr; d.ldb = g.kp; d.b_kmajor = 1; d.C = w.dcol; d.ldc = g.kp;
    d.M = M; d.N = g.kp; d.K = g.np; d.n_valid = g.kp; d.act = kActNone; d.splits = 1;
    NSR_TRY(gemm(d, st));
    NSR_TRY(refine_col2im(st, w.dcol, g.kp, L.cin, nc, s.Hs, s.Ws, L.stride, L.up, g.Ho, g.Wo, s.gacc,
                          at(s.gsrc) + (int64_t)i0 * s.Hs * s.Ws * s.gsrc.ld, s.gsrc.ld));
  }
  if (!implicit) return NSR_OK;
  // ---- input gradient, NSR_F16X3: dX = dZ * flipped weight, stored straight into the gsrc slice
  const unsigned short* bw = reinterpret_cast<const unsigned short*>(w.wr);
  if (!L.up) return refine_dgrad_f16x3(st, w.gz, ldz, bw, L.cin, s.n_img, s.Hs, s.Ws, mbits, at(s.gsrc), s.gsrc.ld);
  // behind the x2 upsample: the same convolution at the upsampled extent into the dcol buffer (free here), as many images per
  // pass as fit, then every source pixel sums its 2 x 2 block.  A pass changes nothing per element: no dependence on img_chunk.
  const int64_t per_img = g.rows_img * L.cin;            // rows_img = 4 Hs Ws
  int64_t pass = w.dcol_floats / per_img;
  if (pass < 1) return NSR_ERR_WORKSPACE;
  pass = pass > s.n_img ? s.n_img : pass;
  for (int64_t i0 = 0; i0 < s.n_img; i0 += pass) {
    const int nc = (int)(s.n_img - i0 < pass ? s.n_img - i0 : pass);
    NSR_TRY(refine_dgrad_f16x3(st, w.gz + i0 * g.rows_img * ldz, ldz, bw, L.cin, nc, g.Ho, g.Wo, mbits, w.dcol, L.cin));
    NSR_TRY(refine_fold2x2(st, w.dcol, L.cin, nc, s.Hs, s.Ws, at(s.gsrc) + i0 * s.Hs * s.Ws * s.gsrc.ld, s.gsrc.ld));
  }
  return NSR_OK;
}

bool shape_ok(int B, int R, int H, int W) { return B >= 1 && R >= 1 && R <= 255 && H > 0 && W > 0 && (H % 8) == 0 && (W % 8) == 0; }
int check_shape(int B, int R, int H, int W) {
  if (B < 1 || R < 1 || R > 255 || H <= 0 || W <= 0) return NSR_ERR_INVALID_ARG;
  if ((H % 8) || (W % 8)) return NSR_ERR_UNSUPPORTED;
  if ((int64_t)B * H * W / 64 < 2) return NSR_ERR_INVALID_ARG;     // one value per channel: no batch variance
  return NSR_OK;
}

}  // namespace

extern "C" size_t nsr_refine_train_workspace_bytes(int B, int R, int H, int W, int img_chunk) {
  if (check_shape(B, R, H, W) != NSR_OK) return 0;
  return (size_t)carve_work(B, R, H, W, resolve_chunk(B, R, H, W, img_chunk), nullptr, nullptr) * sizeof(float);
}

extern "C" size_t nsr_refine_train_saved_bytes(int B, int R, int H, int W) {
  if (check_shape(B, R, H, W) != NSR_OK) return 0;
  return (size_t)carve_saved(B, R, H, W, nullptr, nullptr) * sizeof(float);
}

extern "C" int nsr_refine_train_forward_p(int precision, const float* const* tensors, float* const* running, float momentum,
                                          const float* x_synth, const float* x_candi, int B, int R, int H, int W, int img_chunk,
                                          float* out, void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes,
                                          void* stream) {
  if (precision != NSR_FP32 && precision != NSR_F16X3) return NSR_ERR_UNSUPPORTED;
  NSR_TRY(check_shape(B, R, H, W));
  if (!tensors || !x_synth || !x_candi || !out || !workspace || !saved || !(momentum >= 0.0f && momentum <= 1.0f)) return NSR_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0 || (reinterpret_cast<uintptr_t>(saved) & 255) != 0) return NSR_ERR_INVALID_ARG;
  for (int i = 0; i < NSR_REFINE_N_TENSORS; ++i)
    if (!tensors[i]) return NSR_ERR_INVALID_ARG;
  if (running)
    for (int i = 0; i < 2 * (kNL - 2); ++i)
      if (!running[i]) return NSR_ERR_INVALID_ARG;
  const int chunk = resolve_chunk(B, R, H, W, img_chunk);
  if (workspace_bytes < (size_t)carve_work(B, R, H, W, chunk, nullptr, nullptr) * sizeof(float)) return NSR_ERR_WORKSPACE;
  const int64_t total = carve_saved(B, R, H, W, nullptr, nullptr);
  if (saved_bytes < (size_t)total * sizeof(float)) return NSR_ERR_WORKSPACE;
  hipStream_t st = nsr_stream(stream);
  Work w;
  Saved k;
  carve_work(B, R, H, W, chunk, &w, static_cast<float*>(workspace));
  carve_saved(B, R, H, W, &k, static_cast<float*>(saved));
  Site s[kNSites];
  build_sites(s, B, R, H, W, k, w);
  const Header h{kMagic, (uint64_t)total, B, R, H, W, chunk, precision};
  hipLaunchKernelGGL(header_kernel, dim3(1), dim3(64), 0, st, h, reinterpret_cast<unsigned*>(saved));
  NSR_CHECK_LAUNCH();
  // encoder on the synthesised patches, encoder on the references, the max over the references, decoder: the running
  // statistics of the encoder are updated twice, in this order
  const int64_t px0 = (int64_t)H * W;
  if (hipMemcpyAsync(k.x[0], x_synth, (size_t)B * 3 * px0 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(k.x[1], x_candi, (size_t)B * R * 3 * px0 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return NSR_ERR_LAUNCH;
  for (int i = 0; i < 7; ++i) NSR_TRY(site_forward(st, s[i], tensors, running, momentum, k.x[0], chunk, w, precision));
  for (int i = 7; i < 14; ++i) NSR_TRY(site_forward(st, s[i], tensors, running, momentum, k.x[1], chunk, w, precision));
  const int64_t px[4] = {px0, px0 / 4, px0 / 16, px0 / 64};
  const int fcw[4] = {128, 256, 512, 512};
  const Act mx[4] = {{k.cat7, 384, 256}, {k.cat5, 768, 512}, {k.cat3, 1536, 1024}, {k.cat1, 1024, 512}};
  for (int i = 0; i < 4; ++i) NSR_TRY(refine_max_idx(st, k.fc[i], fcw[i], R, px[i], B, at(mx[i]), mx[i].ld, k.win[i]));
  for (int i = 14; i < kNSites; ++i) NSR_TRY(site_forward(st, s[i], tensors, running, momentum, nullptr, chunk, w, precision));
  return refine_nhwc3_to_nchw(st, k.rgb, px0, B, out);
}

extern "C" int nsr_refine_train_forward(const float* const* tensors, float* const* running, float momentum, const float* x_synth,
                                        const float* x_candi, int B, int R, int H, int W, int img_chunk, float* out, void* workspace,
                                        size_t workspace_bytes, void* saved, size_t saved_bytes, void* stream) {
  return nsr_refine_train_forward_p(NSR_FP32, tensors, running, momentum, x_synth, x_candi, B, R, H, W, img_chunk, out, workspace,
                                    workspace_bytes, saved, saved_bytes, stream);
}

extern "C" int nsr_refine_train_backward_w(int precision, int weight_grad, const float* const* tensors, const float* g_out,
                                           float* const* grads, void* workspace, size_t workspace_bytes, const void* saved,
                                           size_t saved_bytes, void* stream) {
  if (weight_grad != NSR_FP32 && weight_grad != NSR_F16X3) return NSR_ERR_UNSUPPORTED;
  if (precision != NSR_FP32 && precision != NSR_F16X3) return NSR_ERR_UNSUPPORTED;
  if (!tensors || !g_out || !grads || !workspace || !saved) return NSR_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0 || (reinterpret_cast<uintptr_t>(saved) & 255) != 0) return NSR_ERR_INVALID_ARG;
  for (int i = 0; i < NSR_REFINE_N_TENSORS; ++i)
    if (!tensors[i]) return NSR_ERR_INVALID_ARG;
  for (int i = 0; i < NSR_REFINE_N_PARAMS; ++i)
    if (!grads[i]) return NSR_ERR_INVALID_ARG;
  if (saved_bytes < (size_t)kHeaderFloats * sizeof(float)) return NSR_ERR_WORKSPACE;
  // the run's shape, read back from the header the forward call wrote (waits for the stream)
  hipStream_t st = nsr_stream(stream);
  Header h{};
  if (hipMemcpyAsync(&h, saved, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return NSR_ERR_LAUNCH;
  if (h.magic != kMagic) return NSR_ERR_INVALID_ARG;
  if (h.floats > saved_bytes / sizeof(float)) return NSR_ERR_WORKSPACE;
  if (check_shape(h.B, h.R, h.H, h.W) != NSR_OK || h.img_chunk < 1 || h.img_chunk != resolve_chunk(h.B, h.R, h.H, h.W, h.img_chunk) ||
      (uint64_t)carve_saved(h.B, h.R, h.H, h.W, nullptr, nullptr) != h.floats)
    return NSR_ERR_INVALID_ARG;
  const int B = h.B, R = h.R, H = h.H, W = h.W, chunk = h.img_chunk;
  if (workspace_bytes < (size_t)carve_work(B, R, H, W, chunk, nullptr, nullptr) * sizeof(float)) return NSR_ERR_WORKSPACE;
  Work w;
  Saved k;
  carve_work(B, R, H, W, chunk, &w, static_cast<float*>(workspace));
  carve_saved(B, R, H, W, &k, const_cast<float*>(static_cast<const float*>(saved)));   // read only
  Site s[kNSites];
  build_sites(s, B, R, H, W, k, w);
  // decoder, then the encoder's call on the synthesised patches (its features' gradients sit in the gradients of the
  // concatenated buffers), then the call on the references (gradients routed to the winners) ADDING to the same gradients
  for (int i = kNSites - 1; i >= 14; --i)
    NSR_TRY(site_backward(st, s[i], tensors, grads, g_out, nullptr, chunk, w, 0, precision, weight_grad));
  for (int i = 6; i >= 0; --i) NSR_TRY(site_backward(st, s[i], tensors, grads, nullptr, k.x[0], chunk, w, 0, precision, weight_grad));
  const int64_t px0 = (int64_t)H * W;
  const int64_t px[4] = {px0, px0 / 4, px0 / 16, px0 / 64};
  const int fcw[4] = {128, 256, 512, 512};
  const Act gmx[4] = {{w.gcat7, 384, 256}, {w.gcat5, 768, 512}, {w.gcat3, 1536, 1024}, {w.gcat1, 1024, 512}};
  for (int i = 0; i < 4; ++i) NSR_TRY(refine_route(st, at(gmx[i]), gmx[i].ld, k.win[i], fcw[i], R, px[i], B, w.gfc[i]));
  for (int i = 13; i >= 7; --i) NSR_TRY(site_backward(st, s[i], tensors, grads, nullptr, k.x[1], chunk, w, 1, precision, weight_grad));
  return NSR_OK;
}

extern "C" int nsr_refine_train_backward_p(int precision, const float* const* tensors, const float* g_out, float* const* grads,
                                           void* workspace, size_t workspace_bytes, const void* saved, size_t saved_bytes,
                                           void* stream) {
  return nsr_refine_train_backward_w(precision, NSR_FP32, tensors, g_out, grads, workspace, workspace_bytes, saved, saved_bytes, stream);
}

extern "C" int nsr_refine_train_backward(const float* const* tensors, const float* g_out, float* const* grads, void* workspace,
                                         size_t workspace_bytes, const void* saved, size_t saved_bytes, void* stream) {
  return nsr_refine_train_backward_p(NSR_FP32, tensors, g_out, grads, workspace, workspace_bytes, saved, saved_bytes, stream);
}
