"""Helpers of the non-default-architecture training tests (tests/test_train_arch_cpu.py, tests/test_gpu_train_arch.py):
the cases of ``tests/golden/train_arch.npz`` and the restatement of one training iteration for any encoding degrees.

``oracle.train_oracle.forward_train`` hard-codes the direction degree 4, so the restatement composes the oracle's stage
functions itself: ``oc.posenc(d, deg_dir)``, ``oc.sample_coarse``, ``oc.render_points(..., deg_pos=)``, ``oc.composite``,
``oc.resample_fine`` (coarse weights detached), ``oc.sr_mean``.  The network's depth, width and skips are read off the
tensors' shapes by ``oc.mlp_forward``; a ``--no_dir`` network is recognised by its narrow ``dir_encoding``."""
import os

import numpy as np
import torch

from nerf_sr_amd.weights import arch_spec, make_state_dict_arch
from oracle import nerf_oracle as oc

CASES = ("small", "odd", "nodir", "odd_dense")
HEAD = ("rgb.0.weight", "rgb.0.bias", "dir_encoding.0.weight", "dir_encoding.0.bias", "xyz_encoding_final.weight",
        "xyz_encoding_final.bias", "sigma.weight", "sigma.bias")
DEFAULT_ARCH = {"D": 8, "W": 256, "skips": (4,), "deg_pos": 10, "deg_dir": 4, "no_dir": False}


def load_case(golden_dir, tag):
    """One case of train_arch.npz as a dict keyed like the train_*.npz fixtures, plus "arch"."""
    z = np.load(os.path.join(golden_dir, "train_arch.npz"))
    g = {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + ".")}
    g["seed_coarse"], g["seed_fine"] = int(g["seed_coarse"]), int(g["seed_fine"])
    g["arch"] = {"D": int(g["D"]), "W": int(g["W"]), "skips": tuple(int(s) for s in g["skips"]), "deg_pos": int(g["deg_pos"]),
                 "deg_dir": int(g["deg_dir"]), "no_dir": bool(g["no_dir"])}
    return g


def state_dicts(g):
    return make_state_dict_arch(g["seed_coarse"], **g["arch"]), make_state_dict_arch(g["seed_fine"], **g["arch"])


def draws_of(g):
    return {k: g[k] for k in ("u_coarse", "noise_coarse", "u_fine", "noise_fine") if k in g}


def forward_train(sd_c, sd_f, rays, arch, n_coarse=64, n_importance=64, white_bkgd=False, u_coarse=None, noise_coarse=None,
                  u_fine=None, noise_fine=None, noise_std=0.0, gamma_correct=False, sigma_activation="relu",
                  color_activation="sigmoid", stop_grad=False):
    """Train-mode forward_rays (models/nerf_downX_model.py:280-313) for the encoding degrees of ``arch``."""
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    de = oc.posenc(rays[:, 8:11] if rays.shape[1] == 11 else d, arch["deg_dir"])
    kw = dict(gamma_correct=gamma_correct, color_activation=color_activation, stop_grad=stop_grad, deg_pos=arch["deg_pos"])
    z, xyz = oc.sample_coarse(o, d, near, far, n_coarse, False, u=u_coarse)
    rgb, sig = oc.render_points(sd_c, xyz, de, **kw)
    if noise_coarse is not None and noise_std > 0:
        sig = sig + noise_coarse * noise_std
    c_rgb, c_depth, c_op, c_w = oc.composite(rgb, sig, z, white_bkgd, sigma_activation)
    z2, xyz2 = oc.resample_fine(o, d, z, c_w.detach(), n_importance, u=u_fine)
    rgb2, sig2 = oc.render_points(sd_f, xyz2, de, **kw)
    if noise_fine is not None and noise_std > 0:
        sig2 = sig2 + noise_fine * noise_std
    f_rgb, f_depth, f_op, f_w = oc.composite(rgb2, sig2, z2, white_bkgd, sigma_activation)
    return {"coarse_comp_rgbs": c_rgb, "coarse_depth": c_depth, "coarse_opacity": c_op, "coarse_weights": c_w,
            "fine_comp_rgbs": f_rgb, "fine_depth": f_depth, "fine_opacity": f_op, "fine_weights": f_w}


def mse_loss_of(target_lr, s2, lambda_coarse=1.0, lambda_fine=1.0):
    """The reference's loss_tot (comp_low_res_output + calculate_losses): returns f(out) -> (total, loss_c, loss_f)."""
    def f(out):
        n_lr = target_lr.shape[0]
        mse = torch.nn.functional.mse_loss
        lc = mse(oc.sr_mean(out["coarse_comp_rgbs"], n_lr, s2), target_lr) * lambda_coarse
        lf = mse(oc.sr_mean(out["fine_comp_rgbs"], n_lr, s2), target_lr) * lambda_fine
        return lc + lf, lc, lf
    return f


def loss_and_grads(sd_c_np, sd_f_np, g, dtype=torch.float64, loss_fn=None, **flags):
    """The restatement of one iteration on fixture case ``g`` (its rays, draws, noise_std, white background): losses and the
    gradient of ``loss_fn(out)[0]`` (default: the reference's loss_tot) with respect to both networks' tensors."""
    sd_c = {k: v.clone().requires_grad_(True) for k, v in oc.to_torch_sd(sd_c_np, dtype).items()}
    sd_f = {k: v.clone().requires_grad_(True) for k, v in oc.to_torch_sd(sd_f_np, dtype).items()}
    cast = lambda t: torch.as_tensor(t).to(dtype)
    out = forward_train(sd_c, sd_f, cast(g["rays"]), g["arch"], 64, 64, bool(g["white_bkgd"]), noise_std=float(g["noise_std"]),
                        **{k: cast(v) for k, v in draws_of(g).items()}, **flags)
    if loss_fn is None:
        loss_fn = mse_loss_of(cast(g["target_lr"]), int(g["s2"]), float(g["lambda_coarse"]), float(g["lambda_fine"]))
    res = loss_fn(out)
    total = res[0] if isinstance(res, tuple) else res
    total.backward()
    grad_of = lambda v: v.grad.detach() if v.grad is not None else torch.zeros_like(v)
    info = {k: v.detach() for k, v in out.items()}
    info["loss_tot"] = float(total.detach())
    if isinstance(res, tuple):
        info["loss_coarse_mse"], info["loss_fine_mse"] = float(res[1].detach()), float(res[2].detach())
    return info, {k: grad_of(v) for k, v in sd_c.items()}, {k: grad_of(v) for k, v in sd_f.items()}


def assert_grads_close(got, want, spec, what, per_tensor=2e-3, head=5e-4, whole=2e-3):
    """The project's gradient bounds (tests/test_gpu_train.py): every tensor within ``per_tensor`` of its norm, the layers
    above the trunk within ``head``, the whole gradient within ``whole``.  No tensor is excluded."""
    num = den = 0.0
    worst = (0.0, None)
    for k in spec:
        a, b = got[k].detach().cpu().double(), want[k].double()
        err, nrm = float((a - b).norm()), float(b.norm())
        num, den = num + err ** 2, den + nrm ** 2
        if nrm > 0 and err / nrm > worst[0]:
            worst = (err / nrm, k)
        assert err <= per_tensor * nrm + 1e-9, (what, k, err / max(nrm, 1e-300))
        if head is not None and k in HEAD:
            assert err <= head * nrm + 1e-9, (what, k, err / max(nrm, 1e-300))
    if den == 0.0:      # the loss does not reach this network on these rays (an empty coarse field: zero opacity everywhere,
        #                  so the reference's own gradient is exactly zero, e.g. `odd` coarse): the result must be zero too
        assert num == 0.0, (what, num)
        print(f"{what}: reference gradient is exactly zero, and so is the result")
        return 0.0, worst
    rel = (num / den) ** 0.5
    print(f"{what}: whole gradient {rel:.2e}, worst tensor {worst[1]} {worst[0]:.2e}")
    assert rel < whole, (what, rel)
    return rel, worst


def spec_of(arch):
    return arch_spec(**arch)
