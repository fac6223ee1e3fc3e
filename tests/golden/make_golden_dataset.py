#!/usr/bin/env python3
"""Golden vectors of the reference datasets' training / validation buffers (data/llff_downX_dataset.py,
data/blender_downX_dataset.py): what ``nerf_sr_amd.data.RaySet`` has to reproduce.

Runs ONLY in the development container.  The reference's OWN dataset classes are instantiated (through the import shim of
``make_golden.py`` and the ``ToTensor`` stand-in of ``make_golden_warp.py``) on two tiny synthetic scenes written to a
temporary directory; the fixture stores data only: the scene files' bytes, and the tensors the classes built from them.

  * LLFF scene: 5 views, 32 x 24 PNGs -> HR 16 x 12, a COLMAP reconstruction written with ``tests/colmap_writer.py``.
    ``all_rays / all_rgbs / all_rgbs_ori`` of the `train` split for the defaults at s = 2 and s = 4, ``--unified_dir``,
    ``--use_pixel_centers false``, ``--spheric_poses``, ``--ds_method avg --include_var``; three ``reg_patch`` samples
    (``--reg_patch_len 2``) with the (image, row, col) their random draw decoded to; the `val` sample.
  * Blender scene: 3 RGBA views, 32 x 32 PNGs -> HR 16 x 16, s = 2: `train`, `train_crop` (``--precrop_frac 0.5``), one `val`
    sample with its masks.
  * the two test-pose generators (``create_spiral_poses`` / ``create_spheric_poses``) at n = 8.

    python tests/golden/make_golden_dataset.py            # rewrites tests/golden/dataset.npz
"""
import io as _io
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
from make_golden_warp import ToTensor, look_at_colmap  # noqa: E402
import colmap_writer  # noqa: E402


def llff_opt(root, **kw):
    o = dict(dataset_root=root, img_wh=(16, 12), spheric_poses=False, val_num=1, sisr_path=None, use_subset=False, subset_num=20,
             unified_dir=False, use_pixel_centers=True, downscale=2, reg_patch_len=2, include_var=False, with_ref=False,
             no_ref_loss=True, ds_method="lanc", all_ref=False, patch_len=4)
    o.update(kw)
    return SimpleNamespace(**o)


def blender_opt(root, **kw):
    o = dict(dataset_root=root, img_wh=(16, 16), use_pixel_centers=True, downscale=2, ds_method="lanc", rand_dir=False,
             precrop_frac=0.5)
    o.update(kw)
    return SimpleNamespace(**o)


def png_bytes(arr, mode):
    buf = _io.BytesIO()
    Image.fromarray(arr, mode).save(buf, format="PNG")
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def main():
    mg.install_shim()
    import torchvision.transforms as T
    T.ToTensor = ToTensor
    torch.set_grad_enabled(False)
    from data.llff_downX_dataset import LLFFDownXDataset, create_spiral_poses, create_spheric_poses
    from data.blender_downX_dataset import BlenderDownXDataset

    rng = np.random.default_rng(41)
    out = {}

    # ------------------------------------------------------------------ LLFF scene
    root = tempfile.mkdtemp(prefix="nsr_ds_llff_")
    os.makedirs(os.path.join(root, "images"))
    n_img, W0, H0 = 5, 32, 24
    names = [f"img_{i:02d}.png" for i in range(n_img)]
    yy, xx = np.mgrid[0:H0, 0:W0]
    for i, n in enumerate(names):
        smooth = np.stack([127 + 100 * np.sin(xx / 3.0 + i), 127 + 100 * np.cos(yy / 2.5 - i), (xx * 8 + yy * 3 + 40 * i) % 256], -1)
        px = np.clip(smooth + rng.integers(-6, 7, (H0, W0, 3)), 0, 255).astype(np.uint8)
        b = png_bytes(px, "RGB")
        with open(os.path.join(root, "images", n), "wb") as f:
            f.write(b.tobytes())
        out[f"llff_png_{i}"] = b
        out[f"llff_px_{i}"] = px
    pts = rng.normal(0, 0.6, (48, 3)) + np.array([0.0, 0.0, 4.0])
    centres = [np.array([0.3 * (i - 2), 0.08 * ((i * 3) % 5 - 2), -0.15 * (i % 3)]) for i in range(n_img)]
    c2ws = np.stack([look_at_colmap(c, np.array([0.0, 0.0, 4.0])) for c in centres])
    tracks = [[1, 2, 3, 4, 5] for _ in range(len(pts))]
    focal0 = 2.1 * W0
    colmap_writer.write_reconstruction(os.path.join(root, "sparse", "0"), W0, H0, focal0, names, c2ws, pts, tracks)
    out.update(llff_names=np.array(names), llff_c2ws=c2ws, llff_points=pts, llff_src_wh=np.array([W0, H0]), llff_src_focal=np.float64(focal0))

    def record(prefix, ds, same_targets_as=None):
        out[f"{prefix}_rays"] = mg.np32(ds.all_rays)
        if same_targets_as is not None:      # the direction options leave the targets alone: checked here, stored once
            assert np.array_equal(mg.np32(ds.all_rgbs), out[f"{same_targets_as}_rgbs"])
            assert np.array_equal(mg.np32(ds.all_rgbs_ori), out[f"{same_targets_as}_rgbs_ori"])
            return
        out[f"{prefix}_rgbs"] = mg.np32(ds.all_rgbs)
        out[f"{prefix}_rgbs_ori"] = mg.np32(ds.all_rgbs_ori)

    base = LLFFDownXDataset(llff_opt(root), "train")
    out.update(llff_poses=np.asarray(base.poses, np.float64), llff_focal=np.float64(base.focal), llff_bounds=np.asarray(base.bounds, np.float64))
    record("llff_s2", base)
    record("llff_s4", LLFFDownXDataset(llff_opt(root, downscale=4), "train"))
    record("llff_unified", LLFFDownXDataset(llff_opt(root, unified_dir=True), "train"), same_targets_as="llff_s2")
    record("llff_nocentre", LLFFDownXDataset(llff_opt(root, use_pixel_centers=False), "train"), same_targets_as="llff_s2")
    record("llff_spheric", LLFFDownXDataset(llff_opt(root, spheric_poses=True), "train"), same_targets_as="llff_s2")
    record("llff_avgvar", LLFFDownXDataset(llff_opt(root, ds_method="avg", include_var=True), "train"))

    patch = LLFFDownXDataset(llff_opt(root), "reg_patch")
    w_lr = 16 // 2
    per_row = w_lr - 2 + 1
    for k, seed in enumerate((3, 17, 40)):
        torch.manual_seed(seed)
        sample = patch[0]
        torch.manual_seed(seed)
        i_patch = torch.randint(high=patch.n_patches, size=(1,))[0].item()
        i_img, i_patch = i_patch // patch.n_img_patches, i_patch % patch.n_img_patches
        out[f"llff_patch{k}_loc"] = np.array([i_img, i_patch // per_row, i_patch % per_row], np.int64)
        out[f"llff_patch{k}_rays"] = mg.np32(sample["patch_rays"])
        out[f"llff_patch{k}_rgbs"] = mg.np32(sample["patch_rgbs"])

    val = LLFFDownXDataset(llff_opt(root), "val")
    sample = val[0]
    out["llff_val_idx"] = np.int64(val.val_idx)
    for k in ("rays", "rays_ori", "c2w", "rgbs", "rgbs_ori"):
        out[f"llff_val_{k}"] = mg.np32(sample[k])

    # ------------------------------------------------------------------ test-pose generators
    radii = np.percentile(np.abs(base.poses[..., 3]), 90, axis=0)
    out.update(path_radii=radii, path_focus=np.float64(3.5), path_spiral=create_spiral_poses(radii, 3.5, 8),
               path_radius=np.float64(1.1 * base.bounds.min()), path_spheric=create_spheric_poses(1.1 * base.bounds.min(), 8))

    # ------------------------------------------------------------------ Blender scene
    broot = tempfile.mkdtemp(prefix="nsr_ds_blender_")
    yy, xx = np.mgrid[0:32, 0:32]
    for split, n_fr in (("train", 3), ("val", 1)):
        os.makedirs(os.path.join(broot, split))
        frames = []
        for i in range(n_fr):
            alpha = np.clip((13.0 - np.hypot(xx - 15.0 - i, yy - 16.0 + i)) * 60.0, 0, 255)
            px = np.stack([127 + 110 * np.sin(xx / 4.0 + i), 127 + 110 * np.cos(yy / 3.0), (xx * 5 + yy * 7 + 30 * i) % 256, alpha], -1)
            px[..., :3] = np.clip(px[..., :3] + rng.integers(-6, 7, (32, 32, 3)), 0, 255)
            px = px.astype(np.uint8)
            b = png_bytes(px, "RGBA")
            with open(os.path.join(broot, split, f"r_{i}.png"), "wb") as f:
                f.write(b.tobytes())
            out[f"blender_{split}_png_{i}"] = b
            out[f"blender_{split}_px_{i}"] = px
            th = 0.7 * i + (0.3 if split == "val" else 0.0)
            c2w = np.eye(4)
            c2w[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]) @ \
                np.array([[1, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
            c2w[:3, 3] = c2w[:3, :3] @ np.array([0.0, 0.0, 4.0])
            frames.append({"file_path": f"./{split}/r_{i}", "transform_matrix": c2w.tolist()})
        meta = json.dumps({"camera_angle_x": 0.6911112070083618, "frames": frames})
        with open(os.path.join(broot, f"transforms_{split}.json"), "w") as f:
            f.write(meta)
        out[f"blender_{split}_json"] = np.frombuffer(meta.encode(), dtype=np.uint8)
    btrain = BlenderDownXDataset(blender_opt(broot), "train")
    out.update(blender_focal=np.float64(btrain.focal), blender_poses=np.asarray(btrain.poses, np.float64))
    record("blender_train", btrain)
    record("blender_crop", BlenderDownXDataset(blender_opt(broot), "train_crop"))
    sample = BlenderDownXDataset(blender_opt(broot), "val")[0]
    for k in ("rays", "rays_ori", "c2w", "rgbs", "rgbs_ori", "valid_mask", "valid_mask_ori"):
        out[f"blender_val_{k}"] = mg.np32(sample[k])

    path = os.path.join(HERE, "dataset.npz")
    np.savez_compressed(path, **out)
    print("dataset fixture ->", path, f"{os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
