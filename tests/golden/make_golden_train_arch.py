#!/usr/bin/env python3
"""Golden vectors of ONE TRAINING ITERATION of the reference on NON-DEFAULT architectures (``--D --W --skips --deg_pos
--deg_dir --no_dir``, models/networks.py:124-128, models/nerf_model.py:53-57): the two networks of ``arch.npz`` and one
``--no_dir`` network.

Runs ONLY in the development container (imports the reference through the shim of ``make_golden.py``).  Same protocol and
the same digests as ``make_golden_train.py`` (whose ``RecordDraws`` / ``sample_idx`` are imported): ``set_input`` /
``optimize_parameters`` of ``NeRFDownXModel`` on 24 LR pixels at s = 2, the recorded draws, the forward outputs, the losses,
(norm, sum, 512-element subsample) of every gradient tensor and of the coarse weights after the Adam step.  Data only;
weights are not stored: ``nerf_sr_amd.weights.make_state_dict_arch(21 / 22, **arch)`` (22 / 23 for ``odd_dense``).

    python tests/golden/make_golden_train_arch.py      # rewrites tests/golden/train_arch.npz
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shim + helpers; also puts the repo on sys.path)
from make_golden_train import RecordDraws, sample_idx  # noqa: E402

from nerf_sr_amd.weights import make_state_dict_arch  # noqa: E402
from nerf_sr_amd import cameras  # noqa: E402

SEED_C, SEED_F = 21, 22
# name -> (architecture, NDC rays (LLFF) or Blender, white background, (near, far), noise_std, torch seed, weight seeds)
ODD = {"D": 6, "W": 192, "skips": (1, 3), "deg_pos": 10, "deg_dir": 4, "no_dir": False}
CASES = {
    "small": ({"D": 4, "W": 128, "skips": (2,), "deg_pos": 6, "deg_dir": 2, "no_dir": False}, True, False, (0.0, 1.0), 1.0, 31, (SEED_C, SEED_F)),
    "odd": (ODD, False, True, (2.0, 6.0), 0.0, 32, (SEED_C, SEED_F)),
    "nodir": ({"D": 4, "W": 128, "skips": (2,), "deg_pos": 6, "deg_dir": 2, "no_dir": True}, False, True, (2.0, 6.0), 0.0, 33, (SEED_C, SEED_F)),
    # the coarse network of `odd` (seed 21) is empty wherever a Blender camera looks (raw density <= 0: zero opacity, and a
    # gradient that is exactly zero in the reference): the same architecture and rays with weights whose coarse field has
    # density, so that the two-skip backward of the coarse pass counts too
    "odd_dense": (ODD, False, True, (2.0, 6.0), 0.0, 32, (22, 23)),
}
S, N_LR = 2, 24


def build_train_model(arch, white_bkgd, noise_std, dataset_mode, seeds):
    from options.train_options import TrainOptions
    from models import create_model
    tmp = tempfile.mkdtemp(prefix="nsr_golden_train_arch_")
    argv = ["x", "--name", "golden", "--checkpoints_dir", tmp, "--dataset_root", tmp,
            "--model", "nerf_downX", "--dataset_mode", dataset_mode, "--img_wh", "16", "12",
            "--downscale", str(S), "--N_coarse", "64", "--N_importance", "64",
            "--D", str(arch["D"]), "--W", str(arch["W"]), "--skips", *[str(s) for s in arch["skips"]],
            "--deg_pos", str(arch["deg_pos"]), "--deg_dir", str(arch["deg_dir"])]
    if arch["no_dir"]:
        argv.append("--no_dir")
    if white_bkgd:
        argv.append("--white_bkgd")
    old, sys.argv = sys.argv, argv
    try:
        opt = TrainOptions().parse(None)
    finally:
        sys.argv = old
    opt.white_bkgd = white_bkgd
    opt.noise_std = noise_std
    opt.randomized = True
    model = create_model(opt)
    for net, seed in ((model.netCoarse, seeds[0]), (model.netFine, seeds[1])):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict_arch(seed, **arch).items()})
    model.train()
    return model, opt


def one_case(tag, arch, ndc, white, near_far, noise_std, seed, seeds):
    torch.manual_seed(seed)
    model, opt = build_train_model(arch, white, noise_std, "llff_downX" if ndc else "blender_downX", seeds)
    import models.utils as ru
    import einops
    s = S
    H, W = 12 * s // 2, 16 * s // 2
    focal = cameras.llff_focal(W) if ndc else cameras.blender_focal(W)
    c2w = torch.from_numpy(cameras.spiral_pose(0.7) if ndc else cameras.spheric_pose(35.0, -25.0, 4.0)).float()
    dirs = ru.get_ray_directions(H, W, focal)
    o, d = ru.get_rays(dirs, c2w)
    if ndc:
        o, d = ru.get_ndc_rays(H, W, focal, 1.0, o, d)
    near = near_far[0] * torch.ones_like(o[:, :1])
    far = near_far[1] * torch.ones_like(o[:, :1])
    rays = torch.cat([o, d, near, far], 1).view(H, W, 8)
    rays = einops.rearrange(rays, "(h s1) (w s2) c -> (h w) (s1 s2) c", s1=s, s2=s)
    sel = torch.randperm(rays.shape[0])[:N_LR]
    rays = rays[sel].contiguous()                                  # (n_lr, s^2, 8): a batch of LR pixels
    target = torch.rand(N_LR, 3)
    w0_c = {k: v.detach().clone() for k, v in model.netCoarse.state_dict().items()}
    model.set_input({"rays": rays.clone(), "rgbs": target.clone()})
    with RecordDraws() as rec:
        model.optimize_parameters()
    kinds = [t for t, _ in rec.draws]
    want = ["rand_like"] + (["randn_like"] if noise_std > 0 else []) + ["rand"] + (["randn_like"] if noise_std > 0 else [])
    assert kinds == want, kinds
    p = tag + "."
    out = {p + "rays": mg.np32(rays.view(-1, 8)), p + "target_lr": mg.np32(target), p + "s2": s * s, p + "white_bkgd": white,
           p + "randomized": True, p + "noise_std": noise_std, p + "lr": opt.lr, p + "beta1": opt.beta1,
           p + "lambda_coarse": opt.lambda_coarse_mse, p + "lambda_fine": opt.lambda_fine_mse,
           p + "D": arch["D"], p + "W": arch["W"], p + "skips": np.array(arch["skips"], np.int64), p + "deg_pos": arch["deg_pos"],
           p + "deg_dir": arch["deg_dir"], p + "no_dir": arch["no_dir"], p + "seed_coarse": seeds[0], p + "seed_fine": seeds[1]}
    it = iter(rec.draws)
    out[p + "u_coarse"] = mg.np32(next(it)[1])
    if noise_std > 0:
        out[p + "noise_coarse"] = mg.np32(next(it)[1])
    out[p + "u_fine"] = mg.np32(next(it)[1])
    if noise_std > 0:
        out[p + "noise_fine"] = mg.np32(next(it)[1])
    out[p + "lr_coarse"] = mg.np32(model.out_coarse_comp_rgbs)
    out[p + "lr_fine"] = mg.np32(model.out_fine_comp_rgbs)
    out[p + "hr_coarse"] = mg.np32(model.out_coarse_comp_rgbs_ori)
    out[p + "hr_fine"] = mg.np32(model.out_fine_comp_rgbs_ori)
    out[p + "fine_weights"] = mg.np32(model.out_fine_weights)
    out[p + "loss_coarse_mse"] = float(model.loss_coarse_mse)
    out[p + "loss_fine_mse"] = float(model.loss_fine_mse)
    out[p + "loss_tot"] = float(model.loss_tot)
    for net, name in ((model.netCoarse, "coarse"), (model.netFine, "fine")):
        mod = net.module if hasattr(net, "module") else net
        for k, prm in mod.named_parameters():
            g = prm.grad.detach() if prm.grad is not None else torch.zeros_like(prm)
            out[f"{p}gnorm_{name}.{k}"] = float(g.double().norm())
            out[f"{p}gsum_{name}.{k}"] = float(g.double().sum())
            out[f"{p}grad_{name}.{k}"] = mg.np32(g).reshape(-1)[sample_idx(g.numel())]
    for k, v in model.netCoarse.state_dict().items():
        out[f"{p}dw_norm_coarse.{k}"] = float((v.detach() - w0_c[k]).double().norm())
        out[f"{p}w1_coarse.{k}"] = mg.np32(v).reshape(-1)[sample_idx(v.numel())]
    print(tag, "loss", out[p + "loss_tot"])
    return out


def main():
    mg.install_shim()
    torch.set_grad_enabled(True)
    out = {"seed_coarse": SEED_C, "seed_fine": SEED_F}
    for tag, (arch, ndc, white, near_far, noise_std, seed, seeds) in CASES.items():
        out.update(one_case(tag, arch, ndc, white, near_far, noise_std, seed, seeds))
    path = os.path.join(HERE, "train_arch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
