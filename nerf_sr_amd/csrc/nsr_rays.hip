// Ray-side stages of the path: sub-pixel ray generation (R1-R4), positional
// encoding as a stand-alone op (E1), stratified sampling (S1), the s^2 mean (A1)
// and the HR un-flatten (A2).  All HBM-bound elementwise kernels: one thread per
// output element / ray, coalesced stores, fp32 arithmetic in the reference's
// operation order (compiled with -ffp-contract=off).
#include <math.h>
#include "nsr_common.h"
#include "nsr_raygen.h"
#include "nsr_embed.h"
#include "../../include/nsr_data.h"

// ---------------------------------------------------------------------------
// R1-R4  (reference: models/utils.py:98-196, data/llff_downX_dataset.py:473-490)
// ---------------------------------------------------------------------------
struct GenRaysArgs {
  float c2w[12];
  NsrRayCam cam;
};

// rays of the LR pixels [lr0, lr0 + n_rays / s^2): output row r holds ray  lr0 * s^2 + r  of the frame
__global__ void __launch_bounds__(256) gen_rays_kernel(GenRaysArgs a, float* __restrict__ rays, int64_t lr0,
                                                       int64_t n_rays) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const int s = a.cam.s, s2 = s * s, w_lr = a.cam.W / s;
  const int64_t lr = lr0 + r / s2;
  const int sub = (int)(r % s2);
  const int py = (int)(lr / w_lr) * s + sub / s;   // HR row  (h s1)
  const int px = (int)(lr % w_lr) * s + sub % s;   // HR col  (w s2)
  float4 q0, q1;
  nsr_raygen_pixel(a.cam, a.c2w, px, py, q0, q1);   // nsr_raygen.h: shared with the batch kernel of nsr_data.hip
  float4* out = reinterpret_cast<float4*>(rays + r * 8);
  out[0] = q0;
  out[1] = q1;
}

extern "C" int nsr_gen_rays(const float* c2w, int H, int W, double focal, int s, int ndc, float near_, float far_,
                            float* rays_dev, void* stream) {
  if (H <= 0 || W <= 0 || s <= 0) return NSR_ERR_INVALID_ARG;
  return nsr_gen_rays_range(c2w, H, W, focal, s, ndc, near_, far_, 0, (int64_t)(H / s) * (W / s), rays_dev, stream);
}

extern "C" int nsr_gen_rays_range(const float* c2w, int H, int W, double focal, int s, int ndc, float near_, float far_,
                                  int64_t lr_lo, int64_t lr_hi, float* rays_dev, void* stream) {
  return nsr_gen_rays_opt(c2w, H, W, focal, s, ndc, near_, far_, 0u, lr_lo, lr_hi, rays_dev, stream);
}

// ... plus the direction options of the datasets (include/nsr_data.h): bit 0 no pixel centres, bit 1 unified direction
extern "C" int nsr_gen_rays_opt(const float* c2w, int H, int W, double focal, int s, int ndc, float near_, float far_,
                                unsigned options, int64_t lr_lo, int64_t lr_hi, float* rays_dev, void* stream) {
  GenRaysArgs a;
  if (!c2w || !nsr_ray_cam(a.cam, H, W, focal, s, ndc, near_, far_, options)) return NSR_ERR_INVALID_ARG;
  if (lr_lo < 0 || lr_hi < lr_lo || lr_hi > (int64_t)(H / s) * (W / s)) return NSR_ERR_INVALID_ARG;
  if (lr_hi == lr_lo) return NSR_OK;   // empty shard: nothing to write (the pointer may be null)
  if (!rays_dev || (reinterpret_cast<uintptr_t>(rays_dev) & 15) != 0) return NSR_ERR_INVALID_ARG;
  for (int i = 0; i < 12; ++i) a.c2w[i] = c2w[i];
  const int64_t n = (lr_hi - lr_lo) * s * s;
  const int threads = 256;
  const int64_t blocks = (n + threads - 1) / threads;
  hipLaunchKernelGGL(gen_rays_kernel, dim3((unsigned)blocks), dim3(threads), 0, nsr_stream(stream), a, rays_dev, lr_lo, n);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

// ---------------------------------------------------------------------------
// E1  (reference: models/embedding.py:44-62)
// ---------------------------------------------------------------------------
// the option word's column map (include/nsr.h): the identity columns unless NO_XYZ, then per band sin of the 3-vector, cos of it
__global__ void __launch_bounds__(256) posenc_kernel(const float* __restrict__ x, int64_t n, int deg, unsigned embed,
                                                     NsrBands bands, float* __restrict__ out) {
  const int first = nsr_embed_first(embed);
  const int C = first + 6 * deg;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * C) return;
  const int64_t row = idx / C;
  const int col = (int)(idx - row * C);
  float v;
  if (col < first) {
    v = x[row * 3 + col];
  } else {
    const int f = (col - first) / 6, c = (col - first) % 6;
    const float arg = nsr_band_arg(x[row * 3 + (c % 3)], f, bands, embed);   // log-scale: 2^f * x, exact
    v = (c < 3) ? sinf(arg) : cosf(arg);
  }
  out[idx] = v;
}

extern "C" int nsr_posenc_freqs(int deg, unsigned embed, float* freqs) {
  if (deg < 0 || deg > kEmbedMaxDeg || (embed & ~kEmbedBits) != 0u || (deg > 0 && !freqs)) return NSR_ERR_INVALID_ARG;
  if (!(embed & NSR_EMBED_LINEAR_FREQS) || deg == 1) {
    for (int k = 0; k < deg; ++k) freqs[k] = ldexpf(1.0f, k);
    return NSR_OK;
  }
  // torch.linspace(1, 2^(deg-1), deg), fp32, ATen's symmetric form; the upper half with ONE rounding (nsr_linspace01)
  const float end = ldexpf(1.0f, deg - 1);
  const float step = (end - 1.0f) / (float)(deg - 1);
  for (int i = 0; i < deg; ++i)
    freqs[i] = (i < deg / 2) ? 1.0f + step * (float)i : fmaf(-step, (float)(deg - 1 - i), end);
  return NSR_OK;
}

extern "C" int nsr_posenc_e(const float* x, int64_t n, int deg, unsigned embed, float* out, void* stream) {
  if (n < 0 || deg < 0 || deg > kEmbedMaxDeg || (embed & ~kEmbedBits) != 0u) return NSR_ERR_INVALID_ARG;
  const int C = nsr_embed_cols(deg, embed);
  if (n == 0 || C == 0) return NSR_OK;
  if (!x || !out) return NSR_ERR_INVALID_ARG;
  NsrBands bands;
  if (nsr_bands(deg, embed, bands) != NSR_OK) return NSR_ERR_INVALID_ARG;
  const int64_t total = n * C;
  const int threads = 256;
  hipLaunchKernelGGL(posenc_kernel, dim3((unsigned)((total + threads - 1) / threads)), dim3(threads), 0,
                     nsr_stream(stream), x, n, deg, embed, bands, out);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_posenc(const float* x, int64_t n, int deg, float* out, void* stream) {
  return nsr_posenc_e(x, n, deg, 0u, out, stream);
}

// ---------------------------------------------------------------------------
// S1  (reference: models/utils.py:5-44)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sample_kernel(const float* __restrict__ rays, int stride, int64_t R, int N, int lindisp,
                                                     const float* __restrict__ u, float* __restrict__ z,
                                                     float* __restrict__ pts) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= R * N) return;
  const int64_t r = idx / N;
  const int k = (int)(idx - r * N);
  const NsrRay q = nsr_load_ray(rays, r, stride);
  const float near_ = q.near_, far_ = q.far_;
  float zk = nsr_coarse_z(near_, far_, nsr_linspace01(k, N), lindisp);
  if (u != nullptr) {
    // per-bin jitter: lower + u * (upper - lower)   (utils.py:37-41)
    const float zl = (k > 0) ? nsr_coarse_z(near_, far_, nsr_linspace01(k - 1, N), lindisp) : zk;
    const float zr = (k < N - 1) ? nsr_coarse_z(near_, far_, nsr_linspace01(k + 1, N), lindisp) : zk;
    const float lower = (k > 0) ? __fmul_rn(0.5f, __fadd_rn(zl, zk)) : zk;
    const float upper = (k < N - 1) ? __fmul_rn(0.5f, __fadd_rn(zk, zr)) : zk;
    zk = __fadd_rn(lower, __fmul_rn(u[idx], __fsub_rn(upper, lower)));
  }
  z[idx] = zk;
  if (pts != nullptr) {
    pts[idx * 3 + 0] = __fadd_rn(q.o[0], __fmul_rn(zk, q.d[0]));
    pts[idx * 3 + 1] = __fadd_rn(q.o[1], __fmul_rn(zk, q.d[1]));
    pts[idx * 3 + 2] = __fadd_rn(q.o[2], __fmul_rn(zk, q.d[2]));
  }
}

extern "C" int nsr_sample_along_rays(const float* rays, int ray_stride, int64_t R, int n_samples, int lindisp,
                                     const float* u, float* z, float* pts, void* stream) {
  if (R < 0 || n_samples <= 0 || !nsr_ray_stride_ok(ray_stride)) return NSR_ERR_INVALID_ARG;
  if (R == 0) return NSR_OK;
  if (!rays || !z || (ray_stride == 8 && (reinterpret_cast<uintptr_t>(rays) & 15) != 0)) return NSR_ERR_INVALID_ARG;
  const int64_t total = R * n_samples;
  const int threads = 256;
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((total + threads - 1) / threads)), dim3(threads), 0,
                     nsr_stream(stream), rays, ray_stride, R, n_samples, lindisp, u, z, pts);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

// ---------------------------------------------------------------------------
// A1  (reference: models/nerf_downX_model.py:337-348)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sr_mean_kernel(const float* __restrict__ hr, int64_t n_lr, int s2, int c,
                                                      float* __restrict__ lr) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_lr * c) return;
  const int64_t p = idx / c;
  const int ch = (int)(idx - p * c);
  float acc = 0.0f;
  for (int k = 0; k < s2; ++k) acc = __fadd_rn(acc, hr[(p * s2 + k) * c + ch]);
  lr[idx] = __fdiv_rn(acc, (float)s2);
}

extern "C" int nsr_sr_mean(const float* hr, int64_t n_lr, int s2, int c, float* lr, void* stream) {
  if (n_lr < 0 || s2 <= 0 || c <= 0) return NSR_ERR_INVALID_ARG;
  if (n_lr == 0) return NSR_OK;
  if (!hr || !lr) return NSR_ERR_INVALID_ARG;
  const int64_t total = n_lr * c;
  const int threads = 256;
  hipLaunchKernelGGL(sr_mean_kernel, dim3((unsigned)((total + threads - 1) / threads)), dim3(threads), 0,
                     nsr_stream(stream), hr, n_lr, s2, c, lr);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

// ---------------------------------------------------------------------------
// A2  (reference: models/nerf_downX_model.py:410-416)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) unflatten_kernel(const float* __restrict__ x, int H, int W, int s, int c,
                                                        float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over the OUTPUT (H, W, c)
  const int64_t total = (int64_t)H * W * c;
  if (idx >= total) return;
  const int ch = (int)(idx % c);
  const int64_t pix = idx / c;
  const int px = (int)(pix % W), py = (int)(pix / W);
  const int w_lr = W / s;
  const int64_t src = ((int64_t)(py / s) * w_lr + px / s) * (s * s) + (py % s) * s + (px % s);
  out[idx] = x[src * c + ch];
}

extern "C" int nsr_unflatten(const float* x, int H, int W, int s, int c, float* out, void* stream) {
  if (!x || !out || H <= 0 || W <= 0 || s <= 0 || c <= 0 || H % s != 0 || W % s != 0) return NSR_ERR_INVALID_ARG;
  const int64_t total = (int64_t)H * W * c;
  const int threads = 256;
  hipLaunchKernelGGL(unflatten_kernel, dim3((unsigned)((total + threads - 1) / threads)), dim3(threads), 0,
                     nsr_stream(stream), x, H, W, s, c, out);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
