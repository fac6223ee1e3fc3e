// Training / validation ray batches (include/nsr_data.h): the rows idx[0..B) of the reference datasets' all_rays / all_rgbs /
// all_rgbs_ori buffers, produced from the poses and the 8-bit images in one launch.  One thread per (batch row, sub-pixel):
// it generates that sub-pixel's ray (nsr_raygen.h, the body of gen_rays_kernel) and converts that HR pixel's target; the
// thread of sub-pixel 0 also writes the row's LR target.  Launch-latency bound at training batch sizes (512 LR pixels at
// s = 2: 2,048 threads, 96 KB written); the reads are 12 floats of a pose and 3-4 bytes per pixel.
// Compiled with -ffp-contract=off: separate fp32 operations, like the tensor expressions of the datasets.
#include <math.h>
#include "nsr_common.h"
#include "nsr_raygen.h"
#include "../../include/nsr_data.h"

namespace {

struct RaysetArgs {
  NsrRayCam cam;
  const float* poses;
  const uint8_t* hr;
  const uint8_t* lr;
  int64_t n_rows;      // n_views * w * h
  int x0, y0, w, h;
  int C, lr_mode, layout, patch_w;
};

// ToTensor (+ blend onto white for RGBA) of one pixel: the expressions of image_to_targets_kernel /
// image_to_targets_rgba_kernel (nsr_image.hip)
__device__ __forceinline__ void pixel_target(const uint8_t* __restrict__ p, int C, float v[3]) {
  if (C == 4) {
    const float a = __fdiv_rn((float)p[3], 255.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fadd_rn(__fmul_rn(__fdiv_rn((float)p[c], 255.0f), a), __fsub_rn(1.0f, a));
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn((float)p[c], 255.0f);
  }
}

__global__ void __launch_bounds__(256) rayset_batch_kernel(RaysetArgs a, const int64_t* __restrict__ idx, int64_t n_threads,
                                                           float* __restrict__ rays, float* __restrict__ rgbs,
                                                           float* __restrict__ rgbs_ori, unsigned* status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_threads) return;
  const int s = a.cam.s, s2 = s * s;
  const int64_t b = t / s2;
  const int sub = (int)(t - b * s2);
  const int dy = sub / s, dx = sub - dy * s;
  // output row of this sub-pixel: batch order, or the patch raster (h1 s1) (w1 s2)
  int64_t orow = t;
  if (a.layout == 1) {
    const int64_t h1 = b / a.patch_w, w1 = b - h1 * a.patch_w;
    orow = (h1 * s + dy) * ((int64_t)a.patch_w * s) + w1 * s + dx;
  }
  const int64_t i = idx[b];
  float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
  float hr_t[3] = {0.f, 0.f, 0.f}, lr_t[3] = {0.f, 0.f, 0.f};
  if (i >= 0 && i < a.n_rows) {      // an index outside the set never forms an address
    const int64_t per_view = (int64_t)a.w * a.h;
    const int64_t view = i / per_view;
    const int rem = (int)(i - view * per_view);
    const int ly = a.y0 + rem / a.w, lx = a.x0 + rem % a.w;     // LR pixel of the frame
    const int py = ly * s + dy, px = lx * s + dx;               // HR pixel
    const int H = a.cam.H, W = a.cam.W;
    if (rays) nsr_raygen_pixel(a.cam, a.poses + view * 12, px, py, q0, q1);
    const uint8_t* hr_view = a.hr + view * H * W * a.C;
    if (rgbs_ori) pixel_target(hr_view + ((int64_t)py * W + px) * a.C, a.C, hr_t);
    if (rgbs && sub == 0) {
      if (a.lr_mode == 0) {
        pixel_target(a.lr + ((view * (H / s) + ly) * (W / s) + lx) * a.C, a.C, lr_t);
      } else {
        // F.avg_pool2d of the ToTensor image: channel sums in dy*s+dx order, one division; RGBA is blended afterwards
        float m[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < s2; ++k) {
          const uint8_t* p = hr_view + ((int64_t)(ly * s + k / s) * W + (lx * s + k % s)) * a.C;
          for (int c = 0; c < a.C; ++c) m[c] = __fadd_rn(m[c], __fdiv_rn((float)p[c], 255.0f));
        }
        for (int c = 0; c < a.C; ++c) m[c] = __fdiv_rn(m[c], (float)s2);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          lr_t[c] = (a.C == 4) ? __fadd_rn(__fmul_rn(m[c], m[3]), __fsub_rn(1.0f, m[3])) : m[c];
      }
    }
  } else if (sub == 0 && status) {
    atomicOr(status, NSR_FLAG_INPUT_RANGE);
  }
  if (rays) {
    float4* out = reinterpret_cast<float4*>(rays + orow * 8);
    out[0] = q0;
    out[1] = q1;
  }
  if (rgbs_ori) {
    rgbs_ori[orow * 3 + 0] = hr_t[0]; rgbs_ori[orow * 3 + 1] = hr_t[1]; rgbs_ori[orow * 3 + 2] = hr_t[2];
  }
  if (rgbs && sub == 0) {
    rgbs[b * 3 + 0] = lr_t[0]; rgbs[b * 3 + 1] = lr_t[1]; rgbs[b * 3 + 2] = lr_t[2];
  }
}

}  // namespace

extern "C" int nsr_rayset_batch(const struct nsr_rayset* d, const int64_t* idx_dev, int64_t B, int layout, float* rays,
                                float* rgbs, float* rgbs_ori, unsigned* status, void* stream) {
  if (!d || B < 0) return NSR_ERR_INVALID_ARG;
  RaysetArgs a;
  if (!nsr_ray_cam(a.cam, d->H, d->W, d->focal, d->s, d->ndc, d->near_, d->far_, d->options)) return NSR_ERR_INVALID_ARG;
  if (!d->poses || !d->hr || d->n_views <= 0) return NSR_ERR_INVALID_ARG;
  if (d->C != 3 && d->C != 4) return NSR_ERR_INVALID_ARG;
  if (d->lr_mode != NSR_LR_FROM_IMAGES && d->lr_mode != NSR_LR_MEAN_OF_HR) return NSR_ERR_INVALID_ARG;
  if (d->lr_mode == NSR_LR_FROM_IMAGES && !d->lr) return NSR_ERR_INVALID_ARG;
  if (d->x0 < 0 || d->y0 < 0 || d->w <= 0 || d->h <= 0 || d->x0 > d->W / d->s - d->w || d->y0 > d->H / d->s - d->h)
    return NSR_ERR_INVALID_ARG;      // window outside the LR frame
  if (layout != 0 && layout != 1) return NSR_ERR_INVALID_ARG;
  if (layout == 1 && (d->patch_w <= 0 || B % d->patch_w != 0)) return NSR_ERR_INVALID_ARG;
  if (B == 0) return NSR_OK;
  if (!idx_dev || (reinterpret_cast<uintptr_t>(rays) & 15) != 0) return NSR_ERR_INVALID_ARG;
  if (!rays && !rgbs && !rgbs_ori) return NSR_OK;
  const int64_t n = B * d->s * d->s;
  const int threads = 256;
  const int64_t blocks = (n + threads - 1) / threads;
  if (blocks > 0x7fffffff) return NSR_ERR_INVALID_ARG;
  a.poses = d->poses; a.hr = d->hr; a.lr = d->lr;
  a.n_rows = (int64_t)d->n_views * d->w * d->h;
  a.x0 = d->x0; a.y0 = d->y0; a.w = d->w; a.h = d->h;
  a.C = d->C; a.lr_mode = d->lr_mode; a.layout = layout; a.patch_w = d->patch_w;
  hipLaunchKernelGGL(rayset_batch_kernel, dim3((unsigned)blocks), dim3(threads), 0, nsr_stream(stream), a, idx_dev, n, rays,
                     rgbs, rgbs_ori, status);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
