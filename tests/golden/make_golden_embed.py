#!/usr/bin/env python3
"""Golden vectors for the EMBEDDING options of the path (models/embedding.py:17-18 ``--no_xyz``, ``--no_logscale``): the
reference's own ``PositionalEncoding`` bands, network calls, ``forward`` and one ``optimize_parameters`` iteration.

Runs only where the reference tree is at hand (it is imported through the shim of ``make_golden.py``); follows
``make_golden_arch.py`` and ``make_golden_train_arch.py`` (same protocol, same digests) and writes data only:

  * ``embed.npz``: ``freq_bands`` under ``--no_logscale`` for deg = 1 .. 16; for the words NO_XYZ / LINEAR / both on the
    4 x 128 network of ``arch.npz`` over 64 rays of ``path_llff.npz``, and for both flags on the default 8 x 256 network over
    16 rays of ``path_blender.npz`` (white background): the state-dict shapes, the sample points and directions behind the
    first 256 encoded rows, ``mlp_in_256`` / ``mlp_out_256`` / ``mlp_sigma_only_64``, the eight ``forward()`` outputs, and
    ``gap_*`` = max |fp32 - fp64| of the reference's own render of the same case (the parity rule allows 2 x that gap).
  * ``train_embed.npz``: one iteration with both flags on the 4 x 128 network and one with ``--no_logscale`` on its
    ``--no_dir`` variant, draws recorded.

Weights are not stored: ``nerf_sr_amd.weights.make_state_dict_arch(seed, no_xyz=..., **arch)``.

    python tests/golden/make_golden_embed.py
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
NO_XYZ, LINEAR = 1, 2
SMALL = {"D": 4, "W": 128, "skips": (2,), "deg_pos": 6, "deg_dir": 2}
DEFAULT = {"D": 8, "W": 256, "skips": (4,), "deg_pos": 10, "deg_dir": 4}
# name -> (architecture, option word, rays fixture, white background, rays)
CASES = {
    "nx": (SMALL, NO_XYZ, "llff", False, 64),
    "lin": (SMALL, LINEAR, "llff", False, 64),
    "both": (SMALL, NO_XYZ | LINEAR, "llff", False, 64),
    "default_both": (DEFAULT, NO_XYZ | LINEAR, "blender", True, 16),
}
OUT_KEYS = ("coarse_comp_rgbs", "coarse_depth", "coarse_opacity", "coarse_weights",
            "fine_comp_rgbs", "fine_depth", "fine_opacity", "fine_weights")
# training: name -> (architecture, option word, NDC rays, white background, (near, far), noise_std, torch seed)
TRAIN_CASES = {
    "both": ({**SMALL, "no_dir": False}, NO_XYZ | LINEAR, True, False, (0.0, 1.0), 1.0, 41),
    "lin_nodir": ({**SMALL, "no_dir": True}, LINEAR, False, True, (2.0, 6.0), 0.0, 43),
}
S, N_LR = 2, 24


def arch_argv(arch, embed):
    argv = ["--D", str(arch["D"]), "--W", str(arch["W"]), "--skips", *[str(s) for s in arch["skips"]],
            "--deg_pos", str(arch["deg_pos"]), "--deg_dir", str(arch["deg_dir"])]
    return argv + (["--no_xyz"] if embed & NO_XYZ else []) + (["--no_logscale"] if embed & LINEAR else []) \
        + (["--no_dir"] if arch.get("no_dir") else [])


def build(options_cls, argv, arch, embed, white, train):
    from models import create_model
    old, sys.argv = sys.argv, argv
    try:
        opt = options_cls().parse(None)
    finally:
        sys.argv = old
    assert bool(opt.no_xyz) == bool(embed & NO_XYZ) and bool(opt.no_logscale) == bool(embed & LINEAR)
    opt.white_bkgd = white
    model = create_model(opt)
    for net, seed in ((model.netCoarse, SEED_C), (model.netFine, SEED_F)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict_arch(seed, no_xyz=bool(embed & NO_XYZ), **arch).items()})
    model.train() if train else model.eval()
    return model, opt


def build_eval(arch, embed, white):
    from options.test_options import TestOptions
    tmp = tempfile.mkdtemp(prefix="nsr_golden_embed_")
    argv = ["x", "--name", "golden", "--checkpoints_dir", tmp, "--dataset_root", tmp, "--model", "nerf_downX",
            "--dataset_mode", "llff_downX", "--img_wh", "32", "16", "--downscale", "2", "--N_coarse", "64", "--N_importance", "64"] \
        + arch_argv(arch, embed) + (["--white_bkgd"] if white else [])
    model, opt = build(TestOptions, argv, arch, embed, white, False)
    opt.noise_std = 0.0
    return model


def forward_outputs(model, rays):
    model.set_input({"rays": rays[None]})
    model.forward()
    return {k: getattr(model, f"out_{k}").detach() for k in OUT_KEYS}


def eval_case(case, arch, embed, tag, white, n_rays):
    import models.utils as ru
    g = np.load(os.path.join(HERE, f"path_{tag}.npz"))
    model = build_eval(arch, embed, white)
    rays = torch.from_numpy(g["rays"])[:n_rays].contiguous()
    out = {f"{case}_embed": embed, f"{case}_n_rays": n_rays, f"{case}_white_bkgd": white,
           f"{case}_rays": f"path_{tag}.npz"}
    for k, v in model.netCoarse.state_dict().items():
        out[f"{case}_shape.{k}"] = np.array(v.shape, np.int64)
    f32 = forward_outputs(model, rays)
    for k in OUT_KEYS:
        out[f"{case}_{k}"] = mg.np32(f32[k])
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    z_c, xyz_c = ru.sample_along_rays(o, d, near, far, 64, False, False)
    x = torch.cat([model.embeddings['pos'](xyz_c.view(-1, 3)), model.embeddings['dir'](d).repeat_interleave(64, dim=0)], -1)
    out[f"{case}_xyz_256"] = mg.np32(xyz_c.view(-1, 3)[:256])
    out[f"{case}_dir_256"] = mg.np32(d.repeat_interleave(64, dim=0)[:256])
    out[f"{case}_mlp_in_256"] = mg.np32(x[:256])
    y32, s32 = model.netCoarse(x[:256]), model.netCoarse(x[:64], sigma_only=True)
    out[f"{case}_mlp_out_256"] = mg.np32(y32)
    out[f"{case}_mlp_sigma_only_64"] = mg.np32(s32)
    # the reference's own fp32-vs-fp64 gap on this case: the same modules and functions in double (the bands stay the fp32
    # table, promoted)
    model.netCoarse.double()
    model.netFine.double()
    f64 = forward_outputs(model, rays.double())
    for k in OUT_KEYS:
        out[f"{case}_gap_{k}"] = float((f32[k].double() - f64[k]).abs().max())
    xd = torch.cat([model.embeddings['pos'](xyz_c.double().view(-1, 3)), model.embeddings['dir'](d.double()).repeat_interleave(64, dim=0)], -1)
    out[f"{case}_gap_mlp_in_256"] = float((x[:256].double() - xd[:256]).abs().max())
    out[f"{case}_gap_mlp_out_256"] = float((y32.double() - model.netCoarse(x[:256].double())).abs().max())
    out[f"{case}_gap_mlp_sigma_only_64"] = float((s32.double() - model.netCoarse(x[:64].double(), sigma_only=True)).abs().max())
    print(case, {k: out[f"{case}_gap_{k}"] for k in ("fine_comp_rgbs", "fine_weights", "mlp_out_256")})
    return out


def freq_bands():
    from models.embedding import PositionalEncoding
    from types import SimpleNamespace
    out = {}
    for deg in range(1, 17):
        pe = PositionalEncoding(3, deg, SimpleNamespace(no_xyz=False, no_logscale=True))
        out[f"freq_bands_{deg}"] = mg.np32(torch.as_tensor(pe.freq_bands))
    return out


def train_case(tag, arch, embed, ndc, white, near_far, noise_std, seed):
    """make_golden_train_arch.one_case with the embedding flags."""
    from options.train_options import TrainOptions
    import models.utils as ru
    import einops
    torch.manual_seed(seed)
    tmp = tempfile.mkdtemp(prefix="nsr_golden_train_embed_")
    argv = ["x", "--name", "golden", "--checkpoints_dir", tmp, "--dataset_root", tmp, "--model", "nerf_downX",
            "--dataset_mode", "llff_downX" if ndc else "blender_downX", "--img_wh", "16", "12", "--downscale", str(S),
            "--N_coarse", "64", "--N_importance", "64"] + arch_argv(arch, embed) + (["--white_bkgd"] if white else [])
    model, opt = build(TrainOptions, argv, arch, embed, white, True)
    opt.noise_std = noise_std
    opt.randomized = True
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
    rays = rays[sel].contiguous()
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
           p + "deg_dir": arch["deg_dir"], p + "no_dir": arch["no_dir"], p + "embed": embed,
           p + "seed_coarse": SEED_C, p + "seed_fine": SEED_F}
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
    torch.set_grad_enabled(False)
    out = {"seed_coarse": SEED_C, "seed_fine": SEED_F}
    out.update(freq_bands())
    for case, (arch, embed, tag, white, n_rays) in CASES.items():
        out.update(eval_case(case, arch, embed, tag, white, n_rays))
    path = os.path.join(HERE, "embed.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
    torch.set_grad_enabled(True)
    out = {"seed_coarse": SEED_C, "seed_fine": SEED_F}
    for tag, case in TRAIN_CASES.items():
        out.update(train_case(tag, *case))
    path = os.path.join(HERE, "train_embed.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
