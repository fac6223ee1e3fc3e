// Refinement-stage patch batches (include/nsr_refine_data.h): sr / gt patches warped on the fly from the 8-bit images with
// Pillow's perspective + bilinear arithmetic in double, reference patches cropped from the 8-bit reference image.
//
// Thread mapping of patch_batch_kernel.  A sample is 1 + R jobs: job 0 is the warp job (the sr and the gt patch share their
// source coordinates, so one thread computes them once and interpolates both images), jobs 1..R are the R reference crops.  A
// workgroup of 256 threads owns 256 consecutive pixels (row-major in the patch) of ONE job of ONE sample, so the sample, the job,
// the coefficient row and the box are workgroup-uniform (scalar loads, SGPRs), adjacent threads take adjacent x of a patch row
// and every store instruction of a wave writes consecutive floats of one channel plane.  The first R + 1 threads turn the
// sample's position words into positions (each validates x, y and one reference position), the verdict is combined with
// __syncthreads_and and the positions travel through LDS; an invalid sample forms no address and its rows are zeros.
// Compiled with -ffp-contract=off; the double / fp32 arithmetic is spelled with the *_rn intrinsics all the same.
#include <math.h>
#include "nsr_common.h"
#include "../../include/nsr_refine_data.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxR = NSR_REFINE_MAX_REF_PATCHES;

struct PatchArgs {
  const uint8_t* gt;
  const uint8_t* sr;
  const uint8_t* ref;
  const double* coeffs;
  const int32_t* bboxs;
  int n_img, n_aug, H, W, P, R, off, with_gt, mode;
};

// ToTensor + Normalize(0.5, 0.5) of one byte: three fp32 operations
__device__ __forceinline__ float byte_to_target(int v) {
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.0f), 0.5f), 0.5f);
}

// Source coordinates of destination pixel (x, y) under coefficient row a[0..8): false = outside the image (the pixel is 0).
// On success x0 / x1 / y0 / y1 are the clamped neighbour indices and dx, dy the fractions.
__device__ __forceinline__ bool warp_coords(const double* __restrict__ a, int x, int y, int W, int H, int& x0, int& x1, int& y0,
                                            int& y1, double& dx, double& dy) {
  const double xin = __dadd_rn((double)x, 0.5), yin = __dadd_rn((double)y, 0.5);
  const double den = __dadd_rn(__dadd_rn(__dmul_rn(a[6], xin), __dmul_rn(a[7], yin)), 1.0);
  double xs = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[0], xin), __dmul_rn(a[1], yin)), a[2]), den);
  double ys = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[3], xin), __dmul_rn(a[4], yin)), a[5]), den);
  if (!(xs >= 0.0 && xs < (double)W && ys >= 0.0 && ys < (double)H)) return false;      // NaN / inf: outside
  xs = __dsub_rn(xs, 0.5);
  ys = __dsub_rn(ys, 0.5);
  const double fx = floor(xs), fy = floor(ys);       // in [-1, W - 1], [-1, H - 1]
  dx = __dsub_rn(xs, fx);
  dy = __dsub_rn(ys, fy);
  const int ix = (int)fx, iy = (int)fy;
  x0 = max(ix, 0);                  // ix <= W - 1
  x1 = min(ix + 1, W - 1);          // ix + 1 >= 0
  y0 = max(iy, 0);
  y1 = min(iy + 1, H - 1);
  return true;
}

// One channel of the bilinear blend: the differences are integer differences of bytes (exact), the rest double
__device__ __forceinline__ int bilinear_byte(int p00, int p01, int p10, int p11, double dx, double dy) {
  const double v1 = __dadd_rn((double)p00, __dmul_rn((double)(p01 - p00), dx));
  const double v2 = __dadd_rn((double)p10, __dmul_rn((double)(p11 - p10), dx));
  const double v = __dadd_rn(v1, __dmul_rn(__dsub_rn(v2, v1), dy));
  return (int)v & 255;              // (UINT8) of a value in [0, 255]: truncation
}

__device__ __forceinline__ void warp_pixel(const uint8_t* __restrict__ img, int W, int x0, int x1, int y0, int y1, double dx, double dy,
                                           int out[3]) {
  const uint8_t* r0 = img + (int64_t)y0 * W * 3;
  const uint8_t* r1 = img + (int64_t)y1 * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = bilinear_byte(r0[x0 * 3 + c], r0[x1 * 3 + c], r1[x0 * 3 + c], r1[x1 * 3 + c], dx, dy);
}

// lo + word % (hi - lo); false for an empty range or a negative word.  The modulo is not uniform: values below 2^31 % (hi - lo)
// are favoured by at most (hi - lo) / 2^31 -- under 3e-7 for any image below 640 pixels a side.
__device__ __forceinline__ bool map_word(int word, int lo, int hi, int& v) {
  if (word < 0 || hi <= lo) return false;
  v = lo + word % (hi - lo);
  return true;
}
__device__ __forceinline__ bool in_range(int v, int lo, int hi) { return v >= lo && v < hi; }

__global__ void __launch_bounds__(kThreads) patch_batch_kernel(PatchArgs a, const int32_t* __restrict__ aug_idx,
                                                               const int32_t* __restrict__ words, int from_draws, int chunks,
                                                               float* __restrict__ sr_patch, float* __restrict__ gt_patch,
                                                               float* __restrict__ ref_patches, int32_t* __restrict__ starts_out,
                                                               unsigned* status) {
  __shared__ int s_pos[2 + 2 * kMaxR + 1];
  const int tid = threadIdx.x;
  const int P = a.P, R = a.R, n_words = 2 + 2 * R + 1;
  // workgroup-uniform decode: (sample, job, chunk of 256 pixels)
  const int64_t blk = blockIdx.x;
  const int64_t b = blk / ((int64_t)(R + 1) * chunks);
  const int rem = (int)(blk - b * (R + 1) * chunks);
  const int job = rem / chunks, chunk = rem - job * chunks;
  const int aug = aug_idx[b];
  const bool val = a.mode == NSR_PATCHES_VAL;

  // ---- the row's box; everything below stays inside the image only if the box does
  int ok = val ? (aug >= 0 && aug < a.n_img) : (aug >= 0 && aug < a.n_aug);
  int wl = 0, hl = 0, wh = a.W, hh = a.H;
  if (ok && !val) {
    const int32_t* bx = a.bboxs + (int64_t)aug * 4;
    wl = bx[0]; hl = bx[1]; wh = bx[2]; hh = bx[3];
    ok = wl >= 0 && hl >= 0 && wh <= a.W && hh <= a.H && wl <= wh && hl <= hh;
  }
  // ---- positions: thread t <= R validates (or draws) x, y and its own word pair; t == R owns gt_slot
  if (tid <= R) {
    const int32_t* w = words + b * n_words;
    int x = 0, y = 0;
    if (ok) {
      if (from_draws) ok = map_word(w[0], wl, wh - P, x) && map_word(w[1], hl, hh - P, y);
      else { x = w[0]; y = w[1]; ok = in_range(x, wl, wh - P) && in_range(y, hl, hh - P); }
    }
    if (tid == 0) { s_pos[0] = x; s_pos[1] = y; }
    if (tid < R) {
      int rx = 0, ry = 0;
      if (ok) {
        const int off = val ? P : a.off, cut = val ? P : 0;
        const int rxl = max(wl, x - off), rxh = min(wh - P, x + off) - cut;
        const int ryl = max(hl, y - off), ryh = min(hh - P, y + off) - cut;
        if (from_draws) ok = map_word(w[2 + 2 * tid], rxl, rxh, rx) && map_word(w[3 + 2 * tid], ryl, ryh, ry);
        else { rx = w[2 + 2 * tid]; ry = w[3 + 2 * tid]; ok = in_range(rx, rxl, rxh) && in_range(ry, ryl, ryh); }
      }
      s_pos[2 + 2 * tid] = rx; s_pos[3 + 2 * tid] = ry;
    } else {
      int slot = -1;
      if (ok && a.with_gt) {
        if (from_draws) ok = map_word(w[n_words - 1], 0, R, slot);
        else { slot = w[n_words - 1]; ok = in_range(slot, 0, R); }
      }
      s_pos[n_words - 1] = slot;
    }
  }
  ok = __syncthreads_and(ok);
  if (job == 0 && chunk == 0) {
    if (starts_out && tid < n_words) starts_out[b * n_words + tid] = ok ? s_pos[tid] : 0;
    if (!ok && tid == 0 && status) atomicOr(status, NSR_FLAG_INPUT_RANGE);
  }

  const int pix = chunk * kThreads + tid;
  if (pix >= P * P) return;
  const int py = pix / P, px = pix - py * P;
  const int64_t plane = (int64_t)P * P;
  if (job == 0) {
    // ---- sr + gt: one set of source coordinates, two images
    float s[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f};
    int slot = -1;
    if (ok) {
      int vs[3] = {0, 0, 0}, vg[3] = {0, 0, 0};
      const int x = s_pos[0] + px, y = s_pos[1] + py;
      const int64_t img_off = val ? (int64_t)aug * a.H * a.W * 3 : 0;
      if (val) {       // identity: the source bytes themselves
        const int64_t o = img_off + ((int64_t)y * a.W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { vs[c] = a.sr[o + c]; vg[c] = a.gt[o + c]; }
      } else {
        double co[8];
        const double* cr = a.coeffs + (int64_t)aug * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) co[k] = cr[k];
        int x0, x1, y0, y1;
        double dx, dy;
        if (warp_coords(co, x, y, a.W, a.H, x0, x1, y0, y1, dx, dy)) {
          warp_pixel(a.sr, a.W, x0, x1, y0, y1, dx, dy, vs);
          warp_pixel(a.gt, a.W, x0, x1, y0, y1, dx, dy, vg);
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) { s[c] = byte_to_target(vs[c]); g[c] = byte_to_target(vg[c]); }
      slot = s_pos[n_words - 1];
    }
    const int64_t o = b * 3 * plane + pix;
#pragma unroll
    for (int c = 0; c < 3; ++c) { sr_patch[o + c * plane] = s[c]; gt_patch[o + c * plane] = g[c]; }
    if (slot >= 0) {       // with_gt_patch: this sample's gt patch fills reference slot `slot` (the crop job of that slot stands back)
      const int64_t ro = (b * R + slot) * 3 * plane + pix;
#pragma unroll
      for (int c = 0; c < 3; ++c) ref_patches[ro + c * plane] = g[c];
    }
  } else {
    // ---- reference crop k
    const int k = job - 1;
    if (ok && s_pos[n_words - 1] == k) return;
    float r[3] = {0.f, 0.f, 0.f};
    if (ok) {
      const int x = s_pos[2 + 2 * k] + px, y = s_pos[3 + 2 * k] + py;
      const uint8_t* p = a.ref + ((int64_t)y * a.W + x) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] = byte_to_target(p[c]);
    }
    const int64_t ro = (b * R + k) * 3 * plane + pix;
#pragma unroll
    for (int c = 0; c < 3; ++c) ref_patches[ro + c * plane] = r[c];
  }
}

// One workgroup per coefficient row: every thread scans destination pixels t, t + 256, ..., keeps the min / max of x and y where
// the warped ground-truth pixel has a non-zero channel; wave shuffles, then LDS, then thread 0 writes the box.  Integer min / max:
// the result is the same whatever the order.
__global__ void __launch_bounds__(kThreads) aug_bbox_kernel(PatchArgs a, int32_t* __restrict__ out) {
  __shared__ int s_red[4][kThreads / NSR_WAVE];
  const int row = blockIdx.x, tid = threadIdx.x;
  double co[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) co[k] = a.coeffs[(int64_t)row * 8 + k];
  int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
  const int n = a.H * a.W;
  for (int i = tid; i < n; i += kThreads) {
    const int y = i / a.W, x = i - y * a.W;
    int x0, x1, y0, y1, v[3];
    double dx, dy;
    if (!warp_coords(co, x, y, a.W, a.H, x0, x1, y0, y1, dx, dy)) continue;
    warp_pixel(a.gt, a.W, x0, x1, y0, y1, dx, dy, v);
    if ((v[0] | v[1] | v[2]) != 0) {
      xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    xmin = min(xmin, __shfl_xor(xmin, o, 64)); ymin = min(ymin, __shfl_xor(ymin, o, 64));
    xmax = max(xmax, __shfl_xor(xmax, o, 64)); ymax = max(ymax, __shfl_xor(ymax, o, 64));
  }
  if ((tid & (NSR_WAVE - 1)) == 0) {
    const int w = tid / NSR_WAVE;
    s_red[0][w] = xmin; s_red[1][w] = ymin; s_red[2][w] = xmax; s_red[3][w] = ymax;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kThreads / NSR_WAVE; ++w) {
      xmin = min(xmin, s_red[0][w]); ymin = min(ymin, s_red[1][w]); xmax = max(xmax, s_red[2][w]); ymax = max(ymax, s_red[3][w]);
    }
    const bool any = xmax >= 0;
    out[row * 4 + 0] = any ? xmin : 0; out[row * 4 + 1] = any ? ymin : 0;
    out[row * 4 + 2] = any ? xmax + 1 : 0; out[row * 4 + 3] = any ? ymax + 1 : 0;
  }
}

__global__ void __launch_bounds__(kThreads) warp_image_kernel(PatchArgs a, int row, int source, float* __restrict__ out) {
  const int i = blockIdx.x * kThreads + threadIdx.x, n = a.H * a.W;
  if (i >= n) return;
  const int y = i / a.W, x = i - y * a.W;
  double co[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) co[k] = a.coeffs[(int64_t)row * 8 + k];
  int x0, x1, y0, y1, v[3] = {0, 0, 0};
  double dx, dy;
  if (warp_coords(co, x, y, a.W, a.H, x0, x1, y0, y1, dx, dy)) warp_pixel(source ? a.sr : a.gt, a.W, x0, x1, y0, y1, dx, dy, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(int64_t)c * n + i] = byte_to_target(v[c]);
}

// descriptor checks shared by the three entry points
bool desc_args(const struct nsr_refine_patchset* d, PatchArgs& a) {
  if (!d || !d->gt || !d->sr || !d->ref) return false;
  if (d->H <= 0 || d->W <= 0 || (int64_t)d->H * d->W > (1 << 28) || d->n_img <= 0) return false;
  if (d->patch_len <= 0 || d->patch_len > d->H || d->patch_len > d->W) return false;
  if (d->num_ref_patches <= 0 || d->num_ref_patches > kMaxR) return false;
  if (d->mode == NSR_PATCHES_TRAIN) {
    if (!d->coeffs || !d->bboxs || d->n_aug <= 0 || d->n_img != 1 || d->ref_offset <= 0 || d->ref_offset > (1 << 28))
      return false;
    if ((reinterpret_cast<uintptr_t>(d->coeffs) & 7) != 0 || (reinterpret_cast<uintptr_t>(d->bboxs) & 3) != 0) return false;
  } else if (d->mode == NSR_PATCHES_VAL) {
    if (d->with_gt_patch) return false;
  } else {
    return false;
  }
  a.gt = d->gt; a.sr = d->sr; a.ref = d->ref; a.coeffs = d->coeffs; a.bboxs = d->bboxs;
  a.n_img = d->n_img; a.n_aug = d->n_aug; a.H = d->H; a.W = d->W; a.P = d->patch_len; a.R = d->num_ref_patches;
  a.off = d->ref_offset; a.with_gt = d->with_gt_patch != 0; a.mode = d->mode;
  return true;
}

}  // namespace

extern "C" int nsr_refine_patch_batch(const struct nsr_refine_patchset* d, const int32_t* aug_idx, const int32_t* starts,
                                      const int32_t* draws, int64_t B, float* sr_patch, float* gt_patch, float* ref_patches,
                                      int32_t* starts_out, unsigned* status, void* stream) {
  PatchArgs a;
  if (B < 0 || !desc_args(d, a)) return NSR_ERR_INVALID_ARG;
  if (B == 0) return NSR_OK;
  if (!aug_idx || !sr_patch || !gt_patch || !ref_patches) return NSR_ERR_INVALID_ARG;
  if ((starts != nullptr) == (draws != nullptr)) return NSR_ERR_INVALID_ARG;      // exactly one of the two
  if (draws && !starts_out) return NSR_ERR_INVALID_ARG;
  for (const void* p : {(const void*)aug_idx, (const void*)starts, (const void*)draws, (const void*)sr_patch, (const void*)gt_patch,
                        (const void*)ref_patches, (const void*)starts_out, (const void*)status})
    if ((reinterpret_cast<uintptr_t>(p) & 3) != 0) return NSR_ERR_INVALID_ARG;
  const int chunks = (a.P * a.P + kThreads - 1) / kThreads;
  const int64_t blocks = B * (a.R + 1) * chunks;
  if (blocks > 0x7fffffff) return NSR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(patch_batch_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, nsr_stream(stream), a, aug_idx,
                     starts ? starts : draws, draws ? 1 : 0, chunks, sr_patch, gt_patch, ref_patches, starts_out, status);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_refine_aug_bbox(const struct nsr_refine_patchset* d, int32_t* bboxs_out, void* stream) {
  PatchArgs a;
  if (!d || !d->coeffs) return NSR_ERR_INVALID_ARG;
  struct nsr_refine_patchset t = *d;
  t.bboxs = bboxs_out;                 // not read: only its presence and alignment are checked
  if (!bboxs_out || !desc_args(&t, a) || d->mode != NSR_PATCHES_TRAIN) return NSR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(aug_bbox_kernel, dim3((unsigned)a.n_aug), dim3(kThreads), 0, nsr_stream(stream), a, bboxs_out);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}

extern "C" int nsr_refine_warp_image(const struct nsr_refine_patchset* d, int row, int source, float* out, void* stream) {
  PatchArgs a;
  if (!desc_args(d, a) || d->mode != NSR_PATCHES_TRAIN) return NSR_ERR_INVALID_ARG;
  if (row < 0 || row >= a.n_aug || (source != 0 && source != 1) || !out || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
    return NSR_ERR_INVALID_ARG;
  const int blocks = (a.H * a.W + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(warp_image_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, nsr_stream(stream), a, row, source, out);
  NSR_CHECK_LAUNCH();
  return NSR_OK;
}
