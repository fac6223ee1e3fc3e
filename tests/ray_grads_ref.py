"""Restatement of the two kernels behind the gradient with respect to the rays (csrc/nsr_train_gemm.hip: encode_bwd_kernel,
ray_grad_kernel; include/nsr_train.h, nsr_train_arch_backward_r) in numpy float64 -- the reference of
tests/test_ray_grads_cpu.py (against torch autograd) and tests/test_gpu_ray_grad_units.py (bit for bit, on exact inputs).

Column map of an encoded 3-vector (encode_arch_kernel): ``[x (3 columns; none under NO_XYZ) | sin(f_0 x) (3) cos(f_0 x) (3) |
sin(f_1 x) ...]``.  ``variant`` selects a deliberately WRONG form, for the test that the restatement tells them apart."""
import numpy as np
import torch

NO_XYZ, LINEAR_FREQS = 1, 2
VARIANTS = ("swap_sign", "no_f", "no_z", "dir_at_11")


def bands_of(deg: int, embed: int) -> np.ndarray:
    """nsr_posenc_freqs' table as fp32 values: 2^k, or torch.linspace(1, 2^(deg-1), deg) under LINEAR_FREQS."""
    if deg == 0:
        return np.zeros(0, np.float32)
    if not (embed & LINEAR_FREQS):
        return (2.0 ** np.arange(deg)).astype(np.float32)
    return torch.linspace(1.0, 2.0 ** (deg - 1), deg, dtype=torch.float32).numpy()


def n_cols(deg: int, embed: int) -> int:
    return (0 if embed & NO_XYZ else 3) + 6 * deg


def posenc_e(x: torch.Tensor, deg: int, embed: int) -> torch.Tensor:
    """The encoding with the option word, in torch (differentiable): oc.posenc when the word is 0."""
    parts = [] if embed & NO_XYZ else [x]
    for f in bands_of(deg, embed):
        parts += [torch.sin(float(f) * x), torch.cos(float(f) * x)]
    return torch.cat(parts, -1) if parts else x[..., :0]


def encode_bwd(g_cols, enc, deg: int, embed: int, variant=None) -> np.ndarray:
    """g_x (P, 3) from g_cols (n_src, P, >= C) -- the sources are summed in order -- and the kept encoded rows enc (P, >= C)."""
    g = np.asarray(g_cols, np.float64).sum(0)
    enc = np.asarray(enc, np.float64)
    first = 0 if embed & NO_XYZ else 3
    gx = np.zeros((g.shape[0], 3), np.float64)
    if first:
        gx += g[:, 0:3]
    for k, f in enumerate(bands_of(deg, embed).astype(np.float64)):
        c = first + 6 * k
        sn, cs = enc[:, c:c + 3], enc[:, c + 3:c + 6]
        g_sin, g_cos = g[:, c:c + 3], g[:, c + 3:c + 6]
        scale = 1.0 if variant == "no_f" else f
        gx += scale * (cs * g_sin + sn * g_cos) if variant == "swap_sign" else scale * (cs * g_sin - sn * g_cos)
    return gx


def ray_grad(g_x, z, g_dir, dir_enc, deg_dir: int, embed: int, stride: int, variant=None) -> np.ndarray:
    """(R, stride) rows from g_x (R, N, 3), z (R, N), g_dir (R, N, >= C) or None and the kept encoded direction dir_enc (R, >= C)."""
    g_x, z = np.asarray(g_x, np.float64), np.asarray(z, np.float64)
    R = g_x.shape[0]
    out = np.zeros((R, stride), np.float64)
    out[:, 0:3] = g_x.sum(1)
    out[:, 3:6] = g_x.sum(1) if variant == "no_z" else (z[:, :, None] * g_x).sum(1)
    if g_dir is not None:
        dv = encode_bwd(np.asarray(g_dir, np.float64).sum(1)[None], dir_enc, deg_dir, embed)
        if stride == 8:
            out[:, 3:6] += dv
        else:
            out[:, 8:11] = dv
            if variant == "dir_at_11":
                out[:, 3:6] += dv
    return out


def autograd_rows(rays, z, g_pe, g_dirpe, deg_pos: int, deg_dir: int, embed: int, encode=posenc_e) -> np.ndarray:
    """d / d(rays) of sum(g_pe * enc(o + z d)) + sum(g_dirpe * enc(v) repeated over the samples) by torch fp64 autograd."""
    from oracle import nerf_oracle as oc
    rays = torch.as_tensor(rays, dtype=torch.float64).clone().requires_grad_(True)
    z = torch.as_tensor(z, dtype=torch.float64)
    o, d = rays[:, 0:3], rays[:, 3:6]
    v = rays[:, 8:11] if rays.shape[1] == 11 else d
    x = oc.points_on_rays(o, d, z)
    loss = (torch.as_tensor(g_pe, dtype=torch.float64) * encode(x, deg_pos, embed)).sum()
    if g_dirpe is not None:
        loss = loss + (torch.as_tensor(g_dirpe, dtype=torch.float64) * encode(v, deg_dir, embed)[:, None, :]).sum()
    loss.backward()
    return rays.grad.numpy()
