#!/usr/bin/env python3
"""Golden vectors of d(loss_tot)/d(rays) from the reference itself: ``optimize_parameters`` of ``NeRFDownXModel`` with
``data_rays.requires_grad_()`` on the ``small`` and ``odd_dense`` cases of ``train_arch.npz``.

Runs ONLY in the development container (imports the reference through the shim of ``make_golden.py``).  The iteration is the
one ``make_golden_train_arch.py`` runs -- the same seeds, model, pose, LR-pixel selection and target --, which this script
checks by asserting that it reproduced the rays and the recorded draws stored in ``train_arch.npz`` bit for bit.  Data only:
per case ``data_rays.grad[:, :6]`` (fp32; the origin and direction columns -- the reference also differentiates through near /
far, which the library does not).

    python tests/golden/make_golden_ray_grads.py      # rewrites tests/golden/ray_grads.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shim + helpers; also puts the repo on sys.path)
import make_golden_train_arch as ta  # noqa: E402
from make_golden_train import RecordDraws  # noqa: E402

from nerf_sr_amd import cameras  # noqa: E402

TAGS = ("small", "odd_dense")


def one_case(tag, stored):
    arch, ndc, white, near_far, noise_std, seed, seeds = ta.CASES[tag]
    torch.manual_seed(seed)
    model, _ = ta.build_train_model(arch, white, noise_std, "llff_downX" if ndc else "blender_downX", seeds)
    import models.utils as ru
    import einops
    s = ta.S
    H, W = 12 * s // 2, 16 * s // 2
    focal = cameras.llff_focal(W) if ndc else cameras.blender_focal(W)
    c2w = torch.from_numpy(cameras.spiral_pose(0.7) if ndc else cameras.spheric_pose(35.0, -25.0, 4.0)).float()
    o, d = ru.get_rays(ru.get_ray_directions(H, W, focal), c2w)
    if ndc:
        o, d = ru.get_ndc_rays(H, W, focal, 1.0, o, d)
    rays = torch.cat([o, d, near_far[0] * torch.ones_like(o[:, :1]), near_far[1] * torch.ones_like(o[:, :1])], 1).view(H, W, 8)
    rays = einops.rearrange(rays, "(h s1) (w s2) c -> (h w) (s1 s2) c", s1=s, s2=s)
    rays = rays[torch.randperm(rays.shape[0])[:ta.N_LR]].contiguous()
    target = torch.rand(ta.N_LR, 3)
    model.set_input({"rays": rays.clone(), "rgbs": target.clone()})
    model.data_rays.requires_grad_()
    # forward_rays reads near[0] / far[0] of data_rays through .numpy(), which torch refuses on a tensor that requires grad:
    # for this one call .numpy() detaches first (the value read is self.far, a constant of the variance losses, which are off)
    numpy_of = torch.Tensor.numpy
    torch.Tensor.numpy = lambda t, *a, **k: numpy_of(t.detach(), *a, **k)
    try:
        with RecordDraws() as rec:
            model.optimize_parameters()
    finally:
        torch.Tensor.numpy = numpy_of
    p = tag + "."
    assert np.array_equal(mg.np32(model.data_rays.detach()), stored[p + "rays"]), tag
    assert np.array_equal(mg.np32(target), stored[p + "target_lr"]), tag
    names = ["u_coarse"] + (["noise_coarse"] if noise_std > 0 else []) + ["u_fine"] + (["noise_fine"] if noise_std > 0 else [])
    assert len(rec.draws) == len(names), [t for t, _ in rec.draws]
    for name, (_, value) in zip(names, rec.draws):
        assert np.array_equal(mg.np32(value), stored[p + name]), (tag, name)
    assert abs(float(model.loss_tot) - float(stored[p + "loss_tot"])) == 0.0, tag
    g = mg.np32(model.data_rays.grad)
    assert g.shape == stored[p + "rays"].shape and np.isfinite(g).all()
    print(tag, "loss", float(model.loss_tot), "|g_o|", float(np.linalg.norm(g[:, :3])), "|g_d|", float(np.linalg.norm(g[:, 3:6])))
    return g[:, :6].copy()


def main():
    mg.install_shim()
    torch.set_grad_enabled(True)
    stored = np.load(os.path.join(HERE, "train_arch.npz"))
    out = {tag: one_case(tag, stored) for tag in TAGS}
    path = os.path.join(HERE, "ray_grads.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
