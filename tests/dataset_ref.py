"""Numpy restatement of the rules ``nerf_sr_amd.data.RaySet`` implements on the device: which row of the reference
datasets' ``all_rays`` / ``all_rgbs`` / ``all_rgbs_ori`` an index names, the LR-pixel window (Blender ``train_crop``), the
``reg_patch`` raster layout and the validation sample.  Rays come from ``oracle.nerf_oracle`` (read only), 8-bit resizes
from ``oracle.image_oracle``.  tests/test_dataset_cpu.py pins this file to the fixture the reference's own classes wrote
(tests/golden/dataset.npz); tests/test_gpu_dataset.py uses it where the fixture has no recorded sample."""
import numpy as np
import torch

from oracle import image_oracle as io_oracle
from oracle import nerf_oracle as oc


def regroup(x, H, W, s):
    """'(h s1) (w s2) c -> (h w) (s1 s2) c'"""
    c = x.shape[-1]
    return x.reshape(H // s, s, W // s, s, c).transpose(0, 2, 1, 3, 4).reshape((H // s) * (W // s), s * s, c)


def hr_rays(pose, H, W, focal, s, ndc, near, far, use_pixel_centers=True, unified_dir=False):
    """(H*W, 8) fp32: get_ray_directions (with the two options) -> get_rays -> get_ndc_rays, near / far columns."""
    if unified_dir:      # data/llff_downX_dataset.py:274-276: LR grid, floor-divided focal, repeated over the sub-pixels
        d = oc.ray_directions(H // s, W // s, focal // s, use_pixel_centers)
        d = d.repeat_interleave(s, 0).repeat_interleave(s, 1)
    else:
        d = oc.ray_directions(H, W, focal, use_pixel_centers)
    o, d = oc.rays_from_pose(d, torch.FloatTensor(np.asarray(pose)))
    if ndc:
        o, d = oc.ndc_rays(H, W, focal, 1.0, o, d)
        near, far = 0, 1
    rays = torch.cat([o, d, near * torch.ones_like(o[:, :1]), far * torch.ones_like(o[:, :1])], 1)
    return rays.numpy()


def view_rays(pose, H, W, focal, s, ndc, near, far, **options):
    return regroup(hr_rays(pose, H, W, focal, s, ndc, near, far, **options), H, W, s)


def to_float(img_u8):
    """ToTensor, and for RGBA the datasets' blend onto white."""
    f = img_u8.astype(np.float32) / np.float32(255.0)
    return f[..., :3] * f[..., 3:4] + (np.float32(1.0) - f[..., 3:4]) if img_u8.shape[-1] == 4 else f


def avg_pool(f, s):
    """F.avg_pool2d(img, s) of a float (H, W, C) image: channel sums in dy*s+dx order, one division."""
    H, W, C = f.shape
    g = regroup(f, H, W, s)
    acc = np.zeros((g.shape[0], C), np.float32)
    for k in range(s * s):
        acc = acc + g[:, k]
    return acc / np.float32(s * s)


def resize(img_u8, wh):
    return (io_oracle.resize_lanczos_rgba_u8 if img_u8.shape[-1] == 4 else io_oracle.resize_lanczos_u8)(img_u8, wh)


def view_targets(px_u8, W, H, s, ds_method="lanc"):
    """(rgbs (h*w, 3), rgbs_ori (h*w, s*s, 3), hr u8, lr u8 or None) of one scene image."""
    hr = resize(px_u8, (W, H))
    ori = regroup(to_float(hr), H, W, s)
    if ds_method == "lanc":
        lr = resize(hr, (W // s, H // s))
        return to_float(lr).reshape(-1, 3), ori, hr, lr
    f = avg_pool(hr.astype(np.float32) / np.float32(255.0), s)          # all C channels are pooled, RGBA blended afterwards
    rgbs = f[:, :3] * f[:, 3:4] + (np.float32(1.0) - f[:, 3:4]) if hr.shape[-1] == 4 else f
    return rgbs, ori, hr, None


def crop_window(W, H, s, frac):
    """LR-pixel window (x0, y0, w, h) of the Blender ``train_crop`` centre crop (blender_downX_dataset.py:124-130), or a
    ValueError where the reference's separately computed HR and LR crops would not cover the same pixels."""
    w_lr, h_lr = W // s, H // s
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    dh, dw = int(h_lr // 2 * frac), int(w_lr // 2 * frac)
    x0, y0 = w_lr // 2 - dw, h_lr // 2 - dh
    if (W // 2 - dW, H // 2 - dH, 2 * dW, 2 * dH) != (x0 * s, y0 * s, 2 * dw * s, 2 * dh * s) or dw == 0 or dh == 0:
        raise ValueError("HR and LR centre crops disagree")
    return x0, y0, 2 * dw, 2 * dh


class RefSet:
    """The concatenated buffers of a scene, with the window applied per view."""

    def __init__(self, poses, px_list, W, H, s, focal, ndc, near, far, ds_method="lanc", window=None, **options):
        self.W, self.H, self.s = W, H, s
        w_lr, h_lr = W // s, H // s
        self.window = (0, 0, w_lr, h_lr) if window is None else window
        x0, y0, w, h = self.window
        keep = (np.arange(y0, y0 + h)[:, None] * w_lr + np.arange(x0, x0 + w)[None, :]).reshape(-1)
        rays, rgbs, ori = [], [], []
        for pose, px in zip(poses, px_list):
            rays.append(view_rays(pose, H, W, focal, s, ndc, near, far, **options)[keep])
            a, b, _, _ = view_targets(px, W, H, s, ds_method)
            rgbs.append(a[keep])
            ori.append(b[keep])
        self.rays, self.rgbs, self.rgbs_ori = np.concatenate(rays), np.concatenate(rgbs), np.concatenate(ori)

    def index(self, view, row, col):
        _, _, w, h = self.window
        return view * w * h + row * w + col

    def patch(self, view, row, col, length):
        """reg_patch sample (llff_downX_dataset.py:428-436): rows of the patch, rays as the raster (h1 s1) (w1 s2) c."""
        s = self.s
        idx = np.array([self.index(view, row + i, col + j) for i in range(length) for j in range(length)])
        r = self.rays[idx].reshape(length, length, s, s, 8).transpose(0, 2, 1, 3, 4).reshape(length * s, length * s, 8)
        return idx, r, self.rgbs[idx]


def validation_sample(pose, px_u8, W, H, s, focal, ndc, near, far, ds_method="lanc", **options):
    """The `val` sample: LLFF (RGB) pools the HR image whatever ds_method is (llff_downX_dataset.py:499-509); Blender
    (RGBA) follows ds_method and adds the alpha > 0 masks (blender_downX_dataset.py:184-223)."""
    rays_ori = hr_rays(pose, H, W, focal, s, ndc, near, far, **options)
    rgba = px_u8.shape[-1] == 4
    rgbs, ori, hr, lr = view_targets(px_u8, W, H, s, ds_method if rgba else "avg")
    out = {"rays": regroup(rays_ori, H, W, s), "rays_ori": rays_ori, "c2w": np.asarray(pose, np.float32), "rgbs": rgbs, "rgbs_ori": ori}
    if rgba:
        out["valid_mask_ori"] = (hr[..., 3] > 0).reshape(-1)
        if lr is not None:
            out["valid_mask"] = (lr[..., 3] > 0).reshape(-1)
        else:
            out["valid_mask"] = avg_pool(hr.astype(np.float32) / np.float32(255.0), s)[:, 3] > 0
    return out

