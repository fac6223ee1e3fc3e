/* nsr_losses.h — C ABI of the image-space regularisers: total variation, image-gradient L1, (bilateral) Laplacian.
 *
 * Replaces models/criterions.py:56-69 (`TVLoss`), :71-101 (`GradientLoss`), :103-115 (`LaplacianLoss`) and :118-137
 * (`BilateralLaplacianLoss`): each a chain of slices, pads, elementwise passes and reductions, mirrored once more by
 * autograd.  Here every loss is one tile launch plus a fixed-order finishing launch, and its gradient is one launch in gather
 * form.  Inputs are fp32 and are widened to double; differences, the bilateral `exp`, products and sums are DOUBLE, in the
 * reference's operand order, so the values agree with the reference's classes evaluated on `.double()` inputs.  No atomics:
 * identical calls give identical bits.
 *
 * Same conventions as nsr.h (device pointers, caller-owned workspace, enqueue on the caller's stream, int status, nothing
 * allocated, no host synchronisation, every argument checked before anything is enqueued).  A workspace is scratch: its contents
 * on entry do not matter and are unspecified on return (one buffer may serve calls of any kinds and shapes, one at a time per
 * stream).
 *
 * A workgroup owns a 32 x 32 tile of one image plane and stages it with its halo once in LDS, as fp32:
 *   forward   TV, gradient: 33 x 33 per image (one element right and down);  Laplacian: 34 x 34 (one element all round);
 *   backward  TV, gradient: 34 x 34 per image;  Laplacian: 36 x 36 (two elements all round: the stencil centred one pixel
 *             away reads one pixel further) plus four 34 x 34 double maps, one per direction, of sign(w t) w of every stencil
 *             centred in the tile +- 1: 5 184 + 36 992 = 42 176 bytes, whatever the guide's channel count (the guide is read
 *             from device memory once per stencil, not staged).
 * Planes are addressed by strides, so (H, W, C) (planes = channels, stride 1), (B, C, H, W) and (N, H, W) share one core.
 */
#ifndef NSR_LOSSES_H_
#define NSR_LOSSES_H_

#include "nsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `kind` of nsr_loss_workspace_bytes */
#define NSR_LOSS_TV 0
#define NSR_LOSS_GRADIENT 1
#define NSR_LOSS_LAPLACIAN 2           /* plain or bilateral: the guide changes nothing about the workspace */

/* Bytes of workspace the forward entry point of `kind` needs for n_img images of C planes of H x W: one double per
 * (plane, 32 x 32 tile, partial sum) -- two sums for TV and gradient, four for the Laplacian.  TV: n_img = 1, C = channels;
 * gradient: n_img = B; Laplacian: n_img = N and C is ignored (pass the guide's channel count or 1).  0 for an unknown kind
 * and for sizes the entry point refuses. */
size_t nsr_loss_workspace_bytes(int kind, int64_t n_img, int C, int H, int W);

/* TVLoss of x (H, W, C):  sum (x[i+1] - x[i])^2 / ((H-1) W C)  +  sum (x[:, j+1] - x[:, j])^2 / (H (W-1) C).
 * loss: one DEVICE double.  H < 2 or W < 2 (the reference divides 0 by 0): NSR_ERR_INVALID_ARG. */
int nsr_tv_loss(const float* x, int H, int W, int C, double* loss, void* workspace, size_t workspace_bytes, void* stream);

/* Gradient of nsr_tv_loss.  g: one DEVICE fp32, the upstream d/d loss, read by the kernel.  grad_x (H, W, C) fp32: every
 * element is overwritten.  Per element up to four contributions, summed and scaled in double; only the store rounds. */
int nsr_tv_loss_backward(const float* x, int H, int W, int C, const float* g, float* grad_x, void* stream);

/* GradientLoss of a against b, both (B, C, H, W):  dx[h, w] = x[h, w+1] - x[h, w], 0 in the last column; dy the same along
 * rows, 0 in the last row;  loss = (mean |dx_a - dx_b| + mean |dy_a - dy_b|) / 2, both means over all B C H W elements.
 * H or W of 1 is legal. */
int nsr_gradient_loss(const float* a, const float* b, int B, int C, int H, int W, double* loss, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Gradient of nsr_gradient_loss.  grad_a / grad_b (B, C, H, W) fp32: either may be null (not computed) but not both; the
 * bits of one do not depend on whether the other is requested.  |.| differentiates to sign with sign(0) = 0. */
int nsr_gradient_loss_backward(const float* a, const float* b, int B, int C, int H, int W, const float* g, float* grad_a,
                               float* grad_b, void* stream);

/* LaplacianLoss of d (N, H, W): the second differences t = d[p - e] + d[p + e] - 2 d[p] along e = column, row, main diagonal
 * and anti-diagonal, each averaged in absolute value over its own index set (N H (W-2), N (H-2) W, N (H-2) (W-2) twice); the
 * four means are summed and divided by 4.
 * guide: null, or (N, H, W, C) fp32 -- BilateralLaplacianLoss: every t is multiplied by
 *   w = exp(-sum_c |guide[p - e] + guide[p + e] - 2 guide[p]| / gamma)
 * before the absolute value.  C is read only with a guide; gamma is used only with one but must always be positive (pass 1
 * without a guide).
 * H < 3, W < 3, gamma <= 0, or a guide with C <= 0: NSR_ERR_INVALID_ARG. */
int nsr_laplacian_loss(const float* d, const float* guide, int N, int H, int W, int C, double gamma, double* loss,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Gradient of nsr_laplacian_loss with respect to d (the guide gets none: in the reference it is the target image).
 * grad_d (N, H, W) fp32, every element overwritten: up to twelve contributions per element (the centre of each of four
 * stencils with coefficient -2, the two ends of each with +1). */
int nsr_laplacian_loss_backward(const float* d, const float* guide, int N, int H, int W, int C, double gamma, const float* g,
                                float* grad_d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSR_LOSSES_H_ */
