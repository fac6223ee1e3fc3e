"""The fp64 restatement of the path under the embedding options ``--no_xyz`` / ``--no_logscale`` (models/embedding.py:17-18),
for tests/test_embed_options_cpu.py and tests/test_gpu_embed_options.py.

``oracle.nerf_oracle.posenc`` has no options, and ``render_points`` / ``forward_rays`` call it, so this helper composes the
oracle's stage functions (``sample_coarse``, ``mlp_forward`` -- which reads every width off the tensors --, ``composite``,
``resample_fine``, ``sr_mean``) around its own ``posenc(x, deg, embed)``.  The bands under ``--no_logscale`` are the fp32
table ``torch.linspace(1, 2^(deg-1), deg)`` promoted to the dtype of ``x``, as in the reference, whose ``freq_bands`` is an
fp32 tensor whatever the input."""
import os

import numpy as np
import torch

from nerf_sr_amd.weights import arch_spec, make_state_dict_arch
from oracle import nerf_oracle as oc

NO_XYZ, LINEAR = 1, 2
SMALL = {"D": 4, "W": 128, "skips": (2,), "deg_pos": 6, "deg_dir": 2}
DEFAULT = {"D": 8, "W": 256, "skips": (4,), "deg_pos": 10, "deg_dir": 4}
# the cases of tests/golden/embed.npz: name -> (architecture, option word, rays fixture, white background)
CASES = {"nx": (SMALL, NO_XYZ, "llff", False), "lin": (SMALL, LINEAR, "llff", False),
         "both": (SMALL, NO_XYZ | LINEAR, "llff", False), "default_both": (DEFAULT, NO_XYZ | LINEAR, "blender", True)}
TRAIN_CASES = ("both", "lin_nodir")
OUT_KEYS = ("coarse_comp_rgbs", "coarse_depth", "coarse_opacity", "coarse_weights",
            "fine_comp_rgbs", "fine_depth", "fine_opacity", "fine_weights")


def options_of(embed):
    """The option attributes of a word, as keyword arguments of ``default_options`` / a ``SimpleNamespace``."""
    return {"no_xyz": bool(embed & NO_XYZ), "no_logscale": bool(embed & LINEAR)}


def freq_bands(deg, embed):
    if embed & LINEAR:
        return torch.linspace(1, 2 ** (deg - 1), deg)
    return 2 ** torch.linspace(0, deg - 1, deg)


def posenc(x, deg, embed=0):
    """models/embedding.py:44-62 with its two options: ``[x |] sin(f x), cos(f x)`` per band."""
    parts = [] if embed & NO_XYZ else [x]
    for f in freq_bands(deg, embed):
        parts.append(torch.sin(f * x))
        parts.append(torch.cos(f * x))
    return torch.cat(parts, -1)


def render_points(sd, xyz, dir_embedded, deg_pos, embed, **kw):
    """oc.render_points around ``posenc(.., embed)`` (gamma_correct is not needed here)."""
    R, N = xyz.shape[:2]
    x = torch.cat([posenc(xyz.reshape(-1, 3), deg_pos, embed), dir_embedded.repeat_interleave(N, dim=0)], -1)
    out = oc.mlp_forward(sd, x, **kw).view(R, N, -1)
    return out[..., :-1], out[..., -1]


def forward_rays(sd_c, sd_f, rays, arch, embed, n_coarse=64, n_importance=64, white_bkgd=False, u_coarse=None, noise_coarse=None,
                 u_fine=None, noise_fine=None, noise_std=0.0):
    """Eval-mode forward_rays (no draws) or the train-mode one (models/nerf_downX_model.py:280-313) under the word ``embed``."""
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    de = posenc(rays[:, 8:11] if rays.shape[1] == 11 else d, arch["deg_dir"], embed)
    z, xyz = oc.sample_coarse(o, d, near, far, n_coarse, False, u=u_coarse)
    rgb, sig = render_points(sd_c, xyz, de, arch["deg_pos"], embed)
    if noise_coarse is not None and noise_std > 0:
        sig = sig + noise_coarse * noise_std
    c = oc.composite(rgb, sig, z, white_bkgd)
    z2, xyz2 = oc.resample_fine(o, d, z, c[3].detach(), n_importance, u=u_fine)
    rgb2, sig2 = render_points(sd_f, xyz2, de, arch["deg_pos"], embed)
    if noise_fine is not None and noise_std > 0:
        sig2 = sig2 + noise_fine * noise_std
    f = oc.composite(rgb2, sig2, z2, white_bkgd)
    return dict(zip(OUT_KEYS, tuple(c) + tuple(f)))


def state_dicts(g, arch, embed):
    kw = dict(no_xyz=bool(embed & NO_XYZ), **arch)
    return make_state_dict_arch(int(g["seed_coarse"]), **kw), make_state_dict_arch(int(g["seed_fine"]), **kw)


def spec_of(arch, embed):
    return arch_spec(no_xyz=bool(embed & NO_XYZ), **arch)


def bound(g, case, key, borrowed):
    """A bound borrowed from the tests of the default encoding; under the linear bands, whose arguments carry the rounding of
    ``freq * x``, at least 2 x the reference's own fp32-vs-fp64 gap on the same case (recorded in the fixture): the parity
    rule of the README."""
    embed = int(g[f"{case}_embed"])
    return max(borrowed, 2.0 * float(g[f"{case}_gap_{key}"])) if embed & LINEAR else borrowed


# ---- training (tests/golden/train_embed.npz) ----------------------------------------------------------------------------
def load_train_case(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "train_embed.npz"))
    g = {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + ".")}
    g["seed_coarse"], g["seed_fine"], g["embed"] = int(g["seed_coarse"]), int(g["seed_fine"]), int(g["embed"])
    g["arch"] = {"D": int(g["D"]), "W": int(g["W"]), "skips": tuple(int(s) for s in g["skips"]), "deg_pos": int(g["deg_pos"]),
                 "deg_dir": int(g["deg_dir"]), "no_dir": bool(g["no_dir"])}
    return g


def draws_of(g):
    return {k: g[k] for k in ("u_coarse", "noise_coarse", "u_fine", "noise_fine") if k in g}


def loss_and_grads(sd_c_np, sd_f_np, g, dtype=torch.float64):
    """One iteration of the reference's loss_tot on training case ``g``: outputs, losses, both networks' gradients."""
    sd_c = {k: v.clone().requires_grad_(True) for k, v in oc.to_torch_sd(sd_c_np, dtype).items()}
    sd_f = {k: v.clone().requires_grad_(True) for k, v in oc.to_torch_sd(sd_f_np, dtype).items()}
    cast = lambda t: torch.as_tensor(t).to(dtype)
    out = forward_rays(sd_c, sd_f, cast(g["rays"]), g["arch"], g["embed"], 64, 64, bool(g["white_bkgd"]),
                       noise_std=float(g["noise_std"]), **{k: cast(v) for k, v in draws_of(g).items()})
    target, s2 = cast(g["target_lr"]), int(g["s2"])
    mse = torch.nn.functional.mse_loss
    lc = mse(oc.sr_mean(out["coarse_comp_rgbs"], target.shape[0], s2), target) * float(g["lambda_coarse"])
    lf = mse(oc.sr_mean(out["fine_comp_rgbs"], target.shape[0], s2), target) * float(g["lambda_fine"])
    (lc + lf).backward()
    grad_of = lambda v: v.grad.detach() if v.grad is not None else torch.zeros_like(v)
    info = {k: v.detach() for k, v in out.items()}
    info.update(loss_tot=float((lc + lf).detach()), loss_coarse_mse=float(lc.detach()), loss_fine_mse=float(lf.detach()))
    return info, {k: grad_of(v) for k, v in sd_c.items()}, {k: grad_of(v) for k, v in sd_f.items()}
