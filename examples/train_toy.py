#!/usr/bin/env python3
"""A few hundred training iterations of the HIP path on a synthetic scene (needs an MI355X): the "teacher" is the
synthetic field of nerf_sr_amd.weights rendered by the inference path, the "student" starts from a different seed and
is trained with Trainer.optimize_parameters on random LR-pixel batches of the teacher's frames -- the loop structure of
the reference's train.py (set_input -> optimize_parameters) without its datasets / options / visualiser.

    python examples/train_toy.py [--iters 300] [--batch 512]
    python examples/train_toy.py --arch 6,192,1+3      # a non-default network (--D --W --skips): the layer-by-layer pair
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_sr_amd import cameras, ops, train  # noqa: E402
from nerf_sr_amd.weights import make_state_dict, make_state_dict_arch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batch", type=int, default=512, help="LR pixels per step (x4 sub-rays)")
    ap.add_argument("--arch", default="", help="D,W,skips of a non-default network, skips joined by '+' ('6,192,1+3'; '4,128,' = none)")
    ap.add_argument("--no-xyz", action="store_true", help="the embedding's --no_xyz (the layer-by-layer pair, on the default network without --arch)")
    ap.add_argument("--no-logscale", action="store_true", help="the embedding's --no_logscale (likewise)")
    ap.add_argument("--precision", default="f16x3_gemm", choices=train.ARCH_PRECISIONS,
                    help="the student's arithmetic with --arch / --no-xyz / --no-logscale (the layer-by-layer pair): 'f16x3_gemm_bwd' "
                         "runs the gradient products on the split-fp16 MFMA as well")
    a = ap.parse_args()
    W, H, s = 504, 378, 2
    if a.arch or a.no_xyz or a.no_logscale:
        return main_arch(a, W, H, s)
    teacher_c = ops.VanillaMLP(precision="f16x3").load_state_dict(make_state_dict(99))
    teacher_f = ops.VanillaMLP(precision="f16x3").load_state_dict(make_state_dict(100))
    frames = []
    for t in (0.1, 0.5, 0.9):                                    # three training views
        rays = ops.subpixel_rays(cameras.spiral_pose(t), (W, H), cameras.llff_focal(W), s, True)          # (N_lr, 4, 8)
        out = ops.forward_rays(teacher_c, teacher_f, rays.view(-1, 8), 64, 64, False)
        frames.append((rays, ops.sr_mean(out["fine_comp_rgbs"].clone(), rays.shape[0], s * s)))
    student = train.Trainer(make_state_dict(7, field="plain"), make_state_dict(8, field="plain"), randomized=True, noise_std=1.0,
                            lr=5e-4, ray_chunk=4 * a.batch)
    t0 = time.time()
    for it in range(a.iters):
        rays, target = frames[it % len(frames)]
        sel = torch.randint(0, rays.shape[0], (a.batch,), device="cuda")
        student.set_input(rays[sel], target[sel])
        losses = student.optimize_parameters()
        if it % 50 == 0 or it == a.iters - 1:
            lc, lf = losses.tolist()
            print(f"iter {it:4d}  coarse mse {lc:.5f}  fine mse {lf:.5f}  ({(it + 1) / (time.time() - t0):.1f} it/s)")


def main_arch(a, W, H, s):
    """The same loop for ``--arch D,W,skips``: teacher and student are networks of that architecture; the teacher's frames are
    its deterministic train-mode forward, the student trains through ``Trainer(..., arch=)``."""
    arch = {}            # the embedding options alone: the default network as a descriptor
    if a.arch:
        D, Wd, skips = a.arch.split(",")
        arch = {"D": int(D), "W": int(Wd), "skips": tuple(int(x) for x in skips.split("+") if x)}
    embed = (1 if a.no_xyz else 0) | (2 if a.no_logscale else 0)      # weights.embed_of of an options object
    sd = lambda seed: make_state_dict_arch(seed, no_xyz=a.no_xyz, **arch)
    teacher = [{k: torch.from_numpy(v).cuda() for k, v in sd(seed).items()} for seed in (99, 100)]
    frames = []
    for t in (0.1, 0.5, 0.9):
        rays = ops.subpixel_rays(cameras.spiral_pose(t), (W, H), cameras.llff_focal(W), s, True)
        with torch.no_grad():
            out = train.forward_rays_train(teacher[0], teacher[1], rays.view(-1, 8), None, precision="f16x3_gemm", arch=arch,
                                           ray_chunk=16384, embed=embed)
        frames.append((rays, out["fine_comp_rgbs"].view(rays.shape[0], s * s, 3).mean(1)))
    student = train.Trainer(sd(7), sd(8), randomized=True, noise_std=1.0,
                            lr=5e-4, ray_chunk=4 * a.batch, precision=a.precision, arch=arch, embed=embed)
    t0 = time.time()
    for it in range(a.iters):
        rays, target = frames[it % len(frames)]
        sel = torch.randint(0, rays.shape[0], (a.batch,), device="cuda")
        student.set_input(rays[sel], target[sel])
        losses = student.optimize_parameters()
        if it % 50 == 0 or it == a.iters - 1:
            lc, lf = losses.tolist()
            print(f"iter {it:4d}  coarse mse {lc:.5f}  fine mse {lf:.5f}  ({(it + 1) / (time.time() - t0):.1f} it/s)")


if __name__ == "__main__":
    main()
