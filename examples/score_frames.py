#!/usr/bin/env python3
"""How many dB, what SSIM: score one synthetic field against another with NeRFDownXModel.validate (needs an MI355X).  The
"teacher" field rendered by the inference path is the ground truth of three views (LR means as ``rgbs``, the rendered rays as
``rgbs_ori``); the "student" is a model with other weights, validated over those views -- the reference's
``model.validate(dataset)`` without its datasets and savers.

    python examples/score_frames.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_sr_amd import cameras, ops  # noqa: E402
from nerf_sr_amd.model import NeRFDownXModel, default_options  # noqa: E402
from nerf_sr_amd.weights import make_state_dict  # noqa: E402


def main():
    W, H, s = 504, 378, 2
    opt = default_options(img_wh=(W, H), downscale=s, precision="f16x3")
    teacher = NeRFDownXModel(opt).load_networks(make_state_dict(99), make_state_dict(100)).eval()
    views = []
    for t in (0.1, 0.5, 0.9):
        rays = ops.subpixel_rays(cameras.spiral_pose(t), (W, H), cameras.llff_focal(W), s, True)          # (N_lr, 4, 8)
        hr = teacher.forward_rays(rays.view(-1, 8))["fine_comp_rgbs"].clone()
        views.append({"rays": rays, "rgbs": ops.sr_mean(hr, rays.shape[0], s * s), "rgbs_ori": hr})
    student = NeRFDownXModel(opt).load_networks(make_state_dict(99), make_state_dict(101)).eval()
    for name, value in student.validate(views).items():
        print(f"{name:22s} {value:9.4f}" + (" dB" if "psnr" in name else ""))
    same = teacher.validate(views)
    print(f"teacher against itself: fine SSIM {same['loss_fine_ssim_ori']:.6f}, fine PSNR {same['loss_fine_psnr_ori']:.1f} dB")


if __name__ == "__main__":
    main()
