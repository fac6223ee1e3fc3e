#!/usr/bin/env python3
"""Golden vectors of the reference's autograd-only training iterations (the losses the fused step does not compute).

Runs ONLY in the development container (needs the reference).  Reuses make_golden_train.py's shim and helpers (that file is
not changed) and records, as data only:
  train_patch_tv.npz   one ``regularize_patch`` call (--reg_patch --reg_patch_len 4 --downscale 2: an 8 x 8 HR patch, 64 rays
                       in raster order, randomized, noise_std 1, LLFF pose): the draws, both TV losses, a digest of every
                       gradient tensor, the weights after the reference's Adam step (both networks, digests)
  train_llff_clip.npz  one ``optimize_parameters`` with --grad_clip_val low enough that clip_grad_norm_ scales the gradients:
                       the draws, the pre-clip total norm, the clipped gradients' digests and the weights after the step

    python tests/golden/make_golden_train_autograd.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_train as mgt  # noqa: E402  (shim + helpers of the training fixtures)

mg = mgt.mg
from nerf_sr_amd import cameras  # noqa: E402


def _hr_rays(model, s):
    """The rays of make_golden_train.one_case's small LLFF grid, HR raster order (H, W, 8)."""
    import models.utils as ru
    H, W = 12 * s // 2, 16 * s // 2
    focal = cameras.llff_focal(W)
    c2w = torch.from_numpy(cameras.spiral_pose(0.7)).float()
    o, d = ru.get_rays(ru.get_ray_directions(H, W, focal), c2w)
    o, d = ru.get_ndc_rays(H, W, focal, 1.0, o, d)
    return torch.cat([o, d, torch.zeros_like(o[:, :1]), torch.ones_like(o[:, :1])], 1).view(H, W, 8)


def _digests(out, model, w0):
    for net, name in ((model.netCoarse, "coarse"), (model.netFine, "fine")):
        mod = net.module if hasattr(net, "module") else net
        for k, p in mod.named_parameters():
            g = p.grad.detach() if p.grad is not None else torch.zeros_like(p)
            out[f"gnorm_{name}.{k}"] = float(g.double().norm())
            out[f"grad_{name}.{k}"] = mg.np32(g).reshape(-1)[mgt.sample_idx(g.numel())]
        for k, v in mod.state_dict().items():
            out[f"w1_{name}.{k}"] = mg.np32(v).reshape(-1)[mgt.sample_idx(v.numel())]
            out[f"w0_{name}.{k}"] = mg.np32(w0[name][k]).reshape(-1)[mgt.sample_idx(v.numel())]


def _draw_dict(draws, noisy):
    kinds = [t for t, _ in draws]
    want = ["rand_like"] + (["randn_like"] if noisy else []) + ["rand"] + (["randn_like"] if noisy else [])
    assert kinds == want, kinds
    it = iter(draws)
    d = {"u_coarse": mg.np32(next(it)[1])}
    if noisy:
        d["noise_coarse"] = mg.np32(next(it)[1])
    d["u_fine"] = mg.np32(next(it)[1])
    if noisy:
        d["noise_fine"] = mg.np32(next(it)[1])
    return d


def patch_case():
    torch.manual_seed(21)
    model, opt = mgt.build_train_model(False, 99, 100, 2, True, 1.0, "llff_downX", ("--reg_patch", "--reg_patch_len", "4"))
    rays = _hr_rays(model, 2)[2:10, 4:12].reshape(-1, 8).contiguous()          # 8 x 8 HR patch, raster order
    w0 = {n: {k: v.detach().clone() for k, v in m.state_dict().items()} for n, m in (("coarse", model.netCoarse), ("fine", model.netFine))}
    with mgt.RecordDraws() as rec:
        model.regularize_patch({"patch_rays": rays[None].clone()})
    out = {"rays": mg.np32(rays), "patch_len": 4, "s2": 4, "white_bkgd": False, "noise_std": 1.0, "seed_coarse": 99,
           "seed_fine": 100, "lr": opt.lr, "beta1": opt.beta1, "reg_lambda_tv": 1.0,
           "loss_coarse_tv": float(model.loss_coarse_patch), "loss_fine_tv": float(model.loss_fine_patch),
           **_draw_dict(rec.draws, True)}
    _digests(out, model, w0)
    path = os.path.join(HERE, "train_patch_tv.npz")
    np.savez_compressed(path, **out)
    print("patch_tv", out["loss_coarse_tv"], out["loss_fine_tv"], "->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


def clip_case(clip_val=0.02):
    torch.manual_seed(22)
    model, opt = mgt.build_train_model(False, 99, 100, 2, True, 1.0, "llff_downX", ("--grad_clip_val", str(clip_val)))
    import einops
    hr = _hr_rays(model, 2)
    rays = einops.rearrange(hr, "(h s1) (w s2) c -> (h w) (s1 s2) c", s1=2, s2=2)
    rays = rays[torch.randperm(rays.shape[0])[:24]].contiguous()
    target = torch.rand(24, 3)
    w0 = {n: {k: v.detach().clone() for k, v in m.state_dict().items()} for n, m in (("coarse", model.netCoarse), ("fine", model.netFine))}
    norms = []
    orig = torch.nn.utils.clip_grad_norm_

    def clip_and_record(params, max_norm, *a, **k):
        total = orig(params, max_norm, *a, **k)
        norms.append(float(total))
        return total
    torch.nn.utils.clip_grad_norm_ = clip_and_record
    model.set_input({"rays": rays.clone(), "rgbs": target.clone()})
    try:
        with mgt.RecordDraws() as rec:
            model.optimize_parameters()
    finally:
        torch.nn.utils.clip_grad_norm_ = orig
    assert len(norms) == 1 and norms[0] > clip_val, norms
    out = {"rays": mg.np32(rays.view(-1, 8)), "target_lr": mg.np32(target), "s2": 4, "white_bkgd": False, "randomized": True,
           "noise_std": 1.0, "seed_coarse": 99, "seed_fine": 100, "lr": opt.lr, "beta1": opt.beta1,
           "lambda_coarse": opt.lambda_coarse_mse, "lambda_fine": opt.lambda_fine_mse, "grad_clip_val": clip_val,
           "pre_clip_norm": norms[0], "loss_tot": float(model.loss_tot), **_draw_dict(rec.draws, True)}
    _digests(out, model, w0)
    path = os.path.join(HERE, "train_llff_clip.npz")
    np.savez_compressed(path, **out)
    print("llff_clip", out["pre_clip_norm"], "->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


def main():
    mg.install_shim()
    torch.set_grad_enabled(True)
    patch_case()
    clip_case()


if __name__ == "__main__":
    main()
