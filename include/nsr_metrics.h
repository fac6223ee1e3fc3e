/* nsr_metrics.h — C ABI of the evaluation metrics: SSIM and PSNR of rendered / refined frames against ground truth.
 *
 * Replaces models/criterions.py:190-284 (`SSIM.__call__`: reflect pad, five-way cat, depthwise conv2d, a dozen
 * elementwise passes) and :27-36 (`PSNR.forward`, with `value[valid_mask]`) with one launch plus a small fixed-order
 * reduction each.  Products, window sums and the sums over an image are DOUBLE: the reference's fp32 `E[x^2] - mu^2`
 * loses up to 3e-5 of an SSIM on a flat-background frame; these entry points agree with the reference evaluated in
 * fp64.  No float atomics: a frame gives the same bits alone, at any batch size and in any slot of the batch.
 *
 * Same conventions as nsr.h (device pointers, caller-owned workspace, enqueue on the caller's stream, int status,
 * nothing allocated, no host synchronisation).  A workspace is scratch: its contents on entry do not matter and are
 * unspecified on return (one buffer may serve calls of any shapes, one at a time per stream); its size depends on the size
 * function's arguments only.
 */
#ifndef NSR_METRICS_H_
#define NSR_METRICS_H_

#include "nsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* memory order of the two images of nsr_ssim */
#define NSR_LAYOUT_BCHW 0 /* (B, C, H, W): the refinement side's frames */
#define NSR_LAYOUT_BHWC 1 /* (B, H, W, C): the NeRF side's frames */

/* Bytes of workspace nsr_ssim needs: one double per (image, channel, 32 x 32 output tile).  0 for sizes that are not
 * positive. */
size_t nsr_ssim_workspace_bytes(int B, int C, int H, int W);

/* SSIM of `output` against `target`, fp32, B images of C channels and H x W pixels in `layout` order.
 * `window`: DEVICE table (kh, kw) fp32, row-major -- the reference's `_kernel` (an fp32 outer product, :234; any
 * table works: Gaussian, uniform, non-square).  kh and kw odd; the images are reflect-padded by (kh-1)/2 rows and
 * (kw-1)/2 columns, which must be < H and < W (torch's own reflect condition).  c1, c2: (k1 L)^2, (k2 L)^2.
 * ssim (B) double: the mean of the (a1 a2) / (b1 b2) map over (C, H, W) of each image.
 * ssim_map: null, or (B, C, H, W) fp32 (always this order) that receives the map itself.
 * NSR_ERR_UNSUPPORTED: a window whose staged tiles exceed 64 KB of LDS (about 59 x 59 taps). */
int nsr_ssim(const float* output, const float* target, int B, int C, int H, int W, int layout, const float* window, int kh,
             int kw, double c1, double c2, double* ssim, float* ssim_map, void* workspace, size_t workspace_bytes,
             void* stream);

/* Gradient of nsr_ssim with respect to its two images: one launch, no workspace, nothing per pixel in device memory.
 * Same images, sizes, `layout`, window and constants as the forward call (the forward's outputs are not needed: every
 * window sum is recomputed, in double).  Upstream gradients, fp32, either may be null (= 0) but not both:
 *   g_ssim (B): of the per-image values; g_map (B, C, H, W), always this order: of the map.
 * An output pixel q then weighs G_q = g_ssim[b] / (C H W) + g_map[b, c, q].
 * grad_output / grad_target: fp32 in `layout` order, either may be null (not computed) but not both; every element of a
 * requested gradient is overwritten, so the buffers may be uninitialised.  The bits of one gradient do not depend on
 * whether the other is requested.  Products and sums are double, only the final store rounds to fp32: the result agrees
 * with fp64 autograd of the reference's `SSIM.__call__` to 2^-24 of the gradient's largest magnitude.  No atomics: an
 * image's gradient has the same bits alone, at any batch size, in any slot of the batch and in both layouts.
 * A workgroup owns a 16 x 32 (rows x columns) tile of input pixels and keeps in LDS
 *   8 (kh + 8) kw + 2 * 4 (16 + 2 (kh - 1)) (32 + 2 (kw - 1)) + 4 * 8 (16 + kh - 1) (32 + kw - 1) bytes
 * (window as double between four zero rows above and below; x and y over the tile +- 2 pad; four double coefficient maps
 * over the tile +- pad): 51 592 bytes for the 11 x 11 window.  NSR_ERR_UNSUPPORTED: a window for which this exceeds 64 KB
 * (13 x 13 is the largest square one).
 * B == 0 is a no-op. */
int nsr_ssim_backward(const float* output, const float* target, int B, int C, int H, int W, int layout,
                      const float* window, int kh, int kw, double c1, double c2, const float* g_ssim, const float* g_map,
                      float* grad_output, float* grad_target, void* stream);

/* Bytes of workspace nsr_psnr needs: two doubles per 4096-element block of every segment. */
size_t nsr_psnr_workspace_bytes(int n_seg, int64_t n);

/* Mean squared error and PSNR = -10 log10(mse) of n_seg segments of n fp32 elements each (a, b: (n_seg, n)).
 * mask: null, or uint8 validity flags, one per `mask_group` consecutive elements ((n_seg, n / mask_group);
 * mask_group 1: an element mask, mask_group C: a row mask over (rows, C) data; n % mask_group == 0) -- the reference's
 * `value[valid_mask]`.  Differences are formed and summed in double in a fixed order that does not depend on n_seg.
 * mse, psnr (n_seg) double, either may be null; an empty selection gives NaN (torch.mean of nothing). */
int nsr_psnr(const float* a, const float* b, int n_seg, int64_t n, const uint8_t* mask, int mask_group, double* mse,
             double* psnr, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSR_METRICS_H_ */
