#!/usr/bin/env python3
"""Train on a scene held as poses + 8-bit images (needs an MI355X): ``nerf_sr_amd.data.RaySet`` produces every batch on the
device -- the loop of the reference's train.py (shuffled epochs of ``set_input`` -> ``optimize_parameters``, the optional
``--reg_patch`` regulariser, ``validate`` on the held-out view) without its option parser, visualiser and savers.

Default: a synthetic scene.  The "teacher" field of nerf_sr_amd.weights is rendered from a few poses, the frames are
quantised to 8 bit like image files are, and the last one is held out for validation.

    python examples/train_scene.py [--iters 300] [--batch 512] [--reg-patch 8]
    python examples/train_scene.py --llff DIR --wh 504 378           # an LLFF scene (images/, sparse/0/*.bin)
    python examples/train_scene.py --blender DIR --wh 400 400        # a Blender scene (transforms_*.json)
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_sr_amd import cameras, ops, train  # noqa: E402
from nerf_sr_amd.data import RaySet  # noqa: E402
from nerf_sr_amd.model import NeRFDownXModel, default_options  # noqa: E402
from nerf_sr_amd.weights import make_state_dict  # noqa: E402


def synthetic_scene(wh, s, n_views):
    """Teacher frames as uint8 images + their poses; the last view is the validation view."""
    W, H = wh
    teacher_c = ops.VanillaMLP(precision="f16x3").load_state_dict(make_state_dict(99))
    teacher_f = ops.VanillaMLP(precision="f16x3").load_state_dict(make_state_dict(100))
    poses, images = [], []
    for k in range(n_views):
        pose = cameras.spiral_pose((k + 0.5) / n_views)
        rays = ops.subpixel_rays(pose, wh, cameras.llff_focal(W), s, True)
        hr = ops.unflatten_reshape(ops.forward_rays(teacher_c, teacher_f, rays.view(-1, 8), 64, 64, False)["fine_comp_rgbs"].clone(), wh, s)
        poses.append(pose)
        images.append((hr.clamp(0, 1) * 255).round().to(torch.uint8))            # what an image file would hold
    kw = dict(focal=cameras.llff_focal(W), ds_method="avg")
    return RaySet(poses[:-1], images[:-1], wh, s, True, **kw), RaySet(poses[-1:], images[-1:], wh, s, True, **kw), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batch", type=int, default=512, help="LR pixels per step (x s^2 sub-rays)")
    ap.add_argument("--wh", type=int, nargs=2, default=(504, 378))
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--views", type=int, default=4, help="synthetic scene: number of views (the last is held out)")
    ap.add_argument("--reg-patch", type=int, default=0, help="regulariser patch length in LR pixels (0: off), every 10th iteration")
    ap.add_argument("--llff", default="", help="LLFF scene directory")
    ap.add_argument("--blender", default="", help="Blender scene directory")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    wh, s = tuple(a.wh), a.downscale
    if a.llff:
        train_set, val_set, white = RaySet.from_llff(a.llff, wh, s, "train"), RaySet.from_llff(a.llff, wh, s, "val"), False
    elif a.blender:
        train_set, val_set, white = RaySet.from_blender(a.blender, wh, s, "train"), RaySet.from_blender(a.blender, wh, s, "val"), True
    else:
        train_set, val_set, white = synthetic_scene(wh, s, a.views)
    print(f"{train_set.n_views} training views, {len(train_set)} LR pixels, {train_set.resident_bytes() / 2**20:.1f} MiB on the device "
          f"(fp32 buffers: {len(train_set) * (s * s * 44 + 12) / 2**20:.1f} MiB)")
    student = train.Trainer(make_state_dict(7, field="plain"), make_state_dict(8, field="plain"), white_bkgd=white, downscale=s,
                            randomized=True, noise_std=0.0 if white else 1.0, lr=5e-4, ray_chunk=s * s * a.batch)
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    patch_gen = torch.Generator().manual_seed(a.seed)
    it, t0 = 0, time.time()
    while it < a.iters:
        for b in train_set.epoch(a.batch, gen):
            student.set_input(b["rays"], b["rgbs"])
            losses = student.optimize_parameters()
            if a.reg_patch and it % 10 == 0:
                student.regularize_patch(train_set.random_patch(a.reg_patch, patch_gen)["patch_rays"], a.reg_patch)
            if it % 50 == 0 or it == a.iters - 1:
                lc, lf = losses.tolist()
                print(f"iter {it:4d}  coarse mse {lc:.5f}  fine mse {lf:.5f}  ({(it + 1) / (time.time() - t0):.1f} it/s)")
            it += 1
            if it >= a.iters:
                break
    if train_set.status():
        raise RuntimeError("a batch index left the set")
    opt = default_options(img_wh=wh, downscale=s, white_bkgd=white, precision="f16x3")
    sd_c, sd_f = ({k: v.cpu().numpy() for k, v in sd.items()} for sd in student.state_dicts())
    model = NeRFDownXModel(opt).load_networks(sd_c, sd_f).eval()
    for name, value in model.validate([val_set.view(0)]).items():
        print(f"{name:22s} {value:9.4f}" + (" dB" if "psnr" in name else ""))


if __name__ == "__main__":
    main()
