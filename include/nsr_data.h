/* nsr_data.h -- C ABI of the training / validation ray batches (the part of
 * data/llff_downX_dataset.py and data/blender_downX_dataset.py that is on the training path).
 *
 * The reference datasets materialise, for every view, the fp32 ray tensor (h*w, s*s, 8), the LR targets (h*w, 3) and
 * the HR targets (h*w, s*s, 3), concatenate them over the views (`all_rays`, `all_rgbs`, `all_rgbs_ori`) and index
 * the three buffers with a batch of row numbers.  Here the scene stays what it is on disk -- one 3x4 pose per view and
 * the 8-bit images -- and nsr_rayset_batch produces the rows of a batch from it in ONE launch: the ray of a row is
 * generated (the arithmetic of nsr_gen_rays, bit for bit), its targets are converted from the bytes (the arithmetic
 * of nsr_image_to_targets / nsr_image_to_targets_rgba, bit for bit).
 *
 * Same conventions as nsr.h (device pointers, caller-owned memory, enqueue on the caller's stream, int status).
 */
#ifndef NSR_DATA_H_
#define NSR_DATA_H_

#include "nsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* option word of the ray directions (models/utils.py get_ray_directions, data/llff_downX_dataset.py:270-276) */
#define NSR_RAYS_NO_PIXEL_CENTERS 1u /* --use_pixel_centers false: the pixel offset is 0 instead of 0.5 */
#define NSR_RAYS_UNIFIED_DIR 2u      /* --unified_dir: all s*s sub-pixels of an LR pixel share the camera-space direction
                                        get_ray_directions(H // s, W // s, focal // s) of that LR pixel (the focal is
                                        floor-divided, as there); the NDC projection keeps the HR H, W, focal */

#define NSR_LR_FROM_IMAGES 0 /* rgbs rows are read from `lr`  (--ds_method lanc) */
#define NSR_LR_MEAN_OF_HR 1  /* rgbs rows are the mean of the s*s HR pixels (--ds_method avg: F.avg_pool2d of the
                                ToTensor image; summed sequentially over dy*s+dx, one division -- nsr_sr_mean's order.  C = 4:
                                the four channels are averaged, then blended onto white, as the Blender dataset does) */

/* A scene: a plain HOST struct holding DEVICE pointers. */
struct nsr_rayset {
  const float* poses;  /* device, (n_views, 12) fp32: row-major 3x4 camera-to-world matrices */
  int n_views;
  int H, W, s;         /* HR image size and the downscale factor; H % s == 0, W % s == 0 */
  double focal;        /* HR focal length */
  int ndc;             /* != 0: NDC rays (near / far become 0 / 1) */
  float near_, far_;
  unsigned options;    /* NSR_RAYS_* */
  int x0, y0, w, h;    /* window in LR pixels; the whole frame is 0, 0, W/s, H/s (the Blender `train_crop` centre crop is a
                          smaller one).  Row numbers count inside the window. */
  const uint8_t* hr;   /* device, (n_views, H, W, C) */
  const uint8_t* lr;   /* device, (n_views, H/s, W/s, C), or NULL with lr_mode NSR_LR_MEAN_OF_HR */
  int C;               /* 3 (RGB) or 4 (RGBA: targets are blended onto white, rgb * a + (1 - a)) */
  int lr_mode;         /* NSR_LR_* */
  int patch_w;         /* layout 1 only: w1, the patch width in LR pixels */
};

/* One launch: the rows idx[0..B) of the reference's `all_rays` / `all_rgbs` / `all_rgbs_ori`.
 *   idx_dev   device int64 (B): view * (w*h) + row * w + col, row / col inside the window
 *             (data/llff_downX_dataset.py:362; with the crop data/blender_downX_dataset.py:122-160)
 *   layout    0: rays (B, s*s, 8), rgbs_ori (B, s*s, 3), sub-pixel index dy*s+dx
 *             1: the B = h1 * w1 pixels (w1 = desc->patch_w) as a patch raster '(h1 s1) (w1 s2) c'
 *                (data/llff_downX_dataset.py:435): rays (h1*s, w1*s, 8), rgbs_ori (h1*s, w1*s, 3)
 *   rgbs      (B, 3) in batch order under both layouts
 *   any of rays / rgbs / rgbs_ori may be NULL (not produced); rays must be 16-byte aligned
 *   status    device word or NULL.  An index outside [0, n_views*w*h) never forms an address: its rows are written
 *             as zeros and NSR_FLAG_INPUT_RANGE is OR-ed into *status.
 * B == 0 returns NSR_OK whatever the output pointers are. */
int nsr_rayset_batch(const struct nsr_rayset* desc, const int64_t* idx_dev, int64_t B, int layout, float* rays, float* rgbs,
                     float* rgbs_ori, unsigned* status, void* stream);

/* nsr_gen_rays_range with the option word (test and validation views).  options == 0: nsr_gen_rays_range itself. */
int nsr_gen_rays_opt(const float* c2w, int H, int W, double focal, int s, int ndc, float near_, float far_, unsigned options,
                     int64_t lr_lo, int64_t lr_hi, float* rays_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSR_DATA_H_ */
