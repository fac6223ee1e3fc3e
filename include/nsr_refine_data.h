/* nsr_refine_data.h -- C ABI of the refinement stage's training / validation patch batches (the `train` and `val` splits of
 * data/llff_refine_dataset.py:113-146, 214-254).
 *
 * The reference warps the ground-truth and the synthesised image `aug_num` times with a random perspective on the host, keeps
 * all 2 * aug_num results as fp32 tensors and slices 1 + 1 + num_ref_patches patches per sample out of them.  Here the two
 * images stay 8-bit on the device next to a table of perspective coefficients and a table of bounding boxes, and
 * nsr_refine_patch_batch produces a batch in ONE launch: a pixel of an sr / gt patch is the source image warped on the fly
 * with Pillow's 8-bit `Image.transform(size, PERSPECTIVE, coeffs, BILINEAR)` arithmetic (what `TF.perspective` runs on a PIL
 * image), a reference patch is a plain crop.  No warped image is ever stored.
 *
 * The warp rule, every operation a separate IEEE double operation (no contraction):
 *   xin = x + 0.5, yin = y + 0.5
 *   xs = (a0*xin + a1*yin + a2) / (a6*xin + a7*yin + 1),  ys = (a3*xin + a4*yin + a5) / (a6*xin + a7*yin + 1)
 *   the pixel is 0 unless 0 <= xs < W and 0 <= ys < H (a non-finite xs / ys counts as outside)
 *   xs -= 0.5, ys -= 0.5;  x0 = floor(xs), y0 = floor(ys);  dx = xs - x0, dy = ys - y0;  neighbour indices clamped to the image
 *   v1 = p00 + (p01 - p00) * dx,  v2 = p10 + (p11 - p10) * dx,  v = v1 + (v2 - v1) * dy,  byte = (uint8_t)v  (truncation)
 * and the byte becomes the fp32 value (byte / 255 - 0.5) / 0.5 (ToTensor, Normalize(0.5, 0.5)), three fp32 operations.
 *
 * Same conventions as nsr.h (device pointers, caller-owned memory, enqueue on the caller's stream, int status).
 */
#ifndef NSR_REFINE_DATA_H_
#define NSR_REFINE_DATA_H_

#include "nsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSR_PATCHES_TRAIN 0 /* aug_idx selects a coefficient row and its box; the one image pair is warped */
#define NSR_PATCHES_VAL 1   /* aug_idx selects the view; identity coefficients, the box is the whole image, and the reference
                               window is the reference's own: [max(0, x - P), min(W - P, x + P) - P), likewise in y
                               (get_start_pos subtracts patch_len once more, llff_refine_dataset.py:197-200, 247-252) */

#define NSR_REFINE_MAX_REF_PATCHES 64

/* A patch set: a plain HOST struct holding DEVICE pointers. */
struct nsr_refine_patchset {
  const uint8_t* gt;      /* device, (n_img, H, W, 3): ground-truth images */
  const uint8_t* sr;      /* device, (n_img, H, W, 3): synthesised images */
  const uint8_t* ref;     /* device, (H, W, 3): the reference image; `train`: the ground-truth image itself */
  const double* coeffs;   /* device, (n_aug, 8): perspective coefficients destination -> source; row 0 is the identity
                             1,0,0, 0,1,0, 0,0.  NSR_PATCHES_VAL: unused, may be NULL */
  const int32_t* bboxs;   /* device, (n_aug, 4): x0, y0, x1, y1 of each row (nsr_refine_aug_bbox).  NSR_PATCHES_VAL: unused */
  int n_img;              /* NSR_PATCHES_TRAIN: 1 */
  int n_aug;
  int H, W;
  int patch_len;          /* P <= min(H, W) */
  int num_ref_patches;    /* R in [1, NSR_REFINE_MAX_REF_PATCHES] */
  int ref_offset;         /* half width of the window the reference patches are drawn from (NSR_PATCHES_TRAIN) */
  int with_gt_patch;      /* != 0: reference slot `gt_slot` of every sample holds the sample's gt_patch (NSR_PATCHES_TRAIN only) */
  int mode;               /* NSR_PATCHES_* */
};

/* One launch: B samples.
 *   aug_idx     device int32 (B): the augmentation (NSR_PATCHES_TRAIN, in [0, n_aug)) or the view (NSR_PATCHES_VAL, in [0, n_img))
 *   starts      device int32 (B, 2 + 2R + 1): x, y, (ref_x, ref_y) x R, gt_slot -- explicit positions, or NULL
 *   draws       device int32 (B, 2 + 2R + 1): raw non-negative random words in the same layout, or NULL; the kernel maps each
 *               word to lo + word % (hi - lo) with the reference's ranges, in the reference's order:
 *                 x in [wl, wh - P), y in [hl, hh - P)                          (wl, hl, wh, hh: the box of the row)
 *                 ref_x in [max(wl, x - off), min(wh - P, x + off)), ref_y likewise   (NSR_PATCHES_VAL: see above)
 *               gt_slot in [0, R) (with_gt_patch; otherwise the word is unused and the position is written as -1)
 *               Exactly one of starts / draws is given.
 *   sr_patch, gt_patch   (B, 3, P, P) fp32;  ref_patches (B, R, 3, P, P) fp32
 *   starts_out  device int32 (B, 2 + 2R + 1): the positions used; required with draws, optional (may be NULL) with starts
 *   status      device word or NULL.  A sample whose aug_idx, box or any position is outside its range (with draws: an empty
 *               range or a negative word) never forms an address: its rows are written as zeros and NSR_FLAG_INPUT_RANGE is
 *               OR-ed into *status.  gt_slot is checked only with with_gt_patch.
 * B == 0 returns NSR_OK whatever the other pointers are. */
int nsr_refine_patch_batch(const struct nsr_refine_patchset* desc, const int32_t* aug_idx, const int32_t* starts,
                           const int32_t* draws, int64_t B, float* sr_patch, float* gt_patch, float* ref_patches,
                           int32_t* starts_out, unsigned* status, void* stream);

/* Setup, one launch for all rows: bboxs_out (n_aug, 4) int32 = x0, y0, x1 + 1, y1 + 1 of the destination pixels whose warped
 * ground-truth pixel (image 0) has a non-zero channel; 0, 0, 0, 0 where there is none.  One workgroup per row reduces with integer
 * min / max in a fixed order: the result does not depend on the launch.  desc->bboxs is not read.  NSR_PATCHES_TRAIN only. */
int nsr_refine_aug_bbox(const struct nsr_refine_patchset* desc, int32_t* bboxs_out, void* stream);

/* The whole warped and normalised image of one row, (3, H, W) fp32: what the reference keeps as gt_pspc_imgs[a] (source 0) or
 * sr_pspc_imgs[a] (source 1).  For inspection and tests; batches never need it.  NSR_PATCHES_TRAIN only. */
int nsr_refine_warp_image(const struct nsr_refine_patchset* desc, int a, int source, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSR_REFINE_DATA_H_ */
