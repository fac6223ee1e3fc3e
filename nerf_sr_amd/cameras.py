"""Synthetic camera poses for tests and benchmarks (numpy, host side).

No dataset can be loaded offline, so the configs of BASELINE.json are driven by
synthetic poses of the same *shape* as the reference's test trajectories:

* forward-facing "LLFF-like": a pose on the render spiral the reference builds
  with ``create_spiral_poses(radii, focus_depth)`` (``data/llff_downX_dataset.py:86-118``):
  camera centre ``(cos t, -sin t, -sin t/2) * radii`` looking at ``(0, 0, -focus)``.
* inward-facing "Blender-like": a pose on a sphere of radius 4 looking at the
  origin (``data/blender_downX_dataset.py`` uses the dataset's transforms; the
  360 trajectory of ``create_spheric_poses`` has the same geometry).

Both return ``c2w`` as a (3, 4) float32 matrix ``[x | y | z | centre]`` with the
camera looking down ``-z`` (OpenGL / NeRF convention used by ``get_rays``).
"""
from __future__ import annotations

import numpy as np


def _unit(v):
    return v / np.linalg.norm(v)


def look_at_pose(centre, target, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """c2w (3,4) for a camera at ``centre`` whose -z axis points at ``target``."""
    centre = np.asarray(centre, dtype=np.float64)
    z = _unit(centre - np.asarray(target, dtype=np.float64))   # camera +z points away from the target
    x = _unit(np.cross(np.asarray(up, dtype=np.float64), z))
    y = np.cross(z, x)
    return np.stack([x, y, z, centre], 1).astype(np.float32)


def spiral_pose(t: float, radii=(0.3, 0.3, 0.1), focus_depth: float = 3.5) -> np.ndarray:
    """One pose of the forward-facing render spiral at angle ``t`` (radians)."""
    centre = np.array([np.cos(t), -np.sin(t), -np.sin(0.5 * t)]) * np.asarray(radii, dtype=np.float64)
    return look_at_pose(centre, (0.0, 0.0, -focus_depth))


def spheric_pose(theta_deg: float, phi_deg: float = -30.0, radius: float = 4.0) -> np.ndarray:
    """Inward-facing pose on a sphere: azimuth ``theta``, elevation ``-phi``."""
    th, ph = np.deg2rad(theta_deg), np.deg2rad(phi_deg)
    centre = radius * np.array([np.cos(ph) * np.sin(th), -np.sin(ph), np.cos(ph) * np.cos(th)])
    return look_at_pose(centre, (0.0, 0.0, 0.0))


def llff_focal(width_px: int) -> float:
    """HR focal in pixels for a fern-like capture (COLMAP f ~ 3260.5 px at 4032 px wide)."""
    return 3260.5263 * width_px / 4032.0


def blender_focal(width_px: int, camera_angle_x: float = 0.6911112070083618) -> float:
    """``0.5*800/tan(0.5*angle) * W/800`` (``data/blender_downX_dataset.py:77-80``)."""
    return 0.5 * 800.0 / np.tan(0.5 * camera_angle_x) * width_px / 800.0


def rays_from_pose(c2w, H: int, W: int, focal: float, s: int, ndc: bool, near: float, far: float, rows=None):
    """The (H * W, 8) ray rows ``[o, d, near, far]`` of one pose in ``ops.all_rays``' row order, written in torch so that autograd
    differentiates them with respect to ``c2w`` (3, 4) -- pose refinement through ``train.forward_rays_train`` with rays that
    require grad.  The same chain as ``nsr_gen_rays`` (R1-R4): camera-space directions of the pixel CENTRES
    ``((i + 0.5 - W/2) / f, -(j + 0.5 - H/2) / f, -1)``, rotated by ``c2w[:, :3]`` and normalised, origin ``c2w[:, 3]``; with
    ``ndc`` the forward-facing NDC warp at near = 1 and bounds 0 / 1 (LLFF), else ``near`` / ``far`` as given (Blender); then the
    regroup in which LR pixel (h, w) owns its s x s HR sub-pixel rays: row ((h * W/s + w) * s + dy) * s + dx is HR pixel
    (h s + dy, w s + dx).  H, W, focal: of the HR image.  ``rows``: an index tensor selecting rows (None: all).  Any device;
    values in ``c2w``'s dtype.  In fp32 the rows lie within 2.4e-7 of the oracle's grid on the host and of ``nsr_gen_rays``' rows
    on a device (the two differ from each other by more under the NDC warp: see the comment below)."""
    import torch
    if c2w.shape != (3, 4):
        raise ValueError(f"c2w must be (3, 4), got {tuple(c2w.shape)}")
    if H % s or W % s:
        raise ValueError("H and W must be multiples of s")
    dev, dt = c2w.device, c2w.dtype
    r = torch.arange(H * W, device=dev) if rows is None else torch.as_tensor(rows, device=dev).long()
    w_lr = W // s
    lr, sub = r // (s * s), r % (s * s)
    py = (lr // w_lr) * s + sub // s
    px = (lr % w_lr) * s + sub % s
    gx, gy = px.to(dt) + 0.5, py.to(dt) + 0.5
    # Under the NDC warp one ulp in a direction becomes several in the row, so the fp32 arithmetic is pinned down where a
    # device would otherwise choose it.  The rotation runs in nsr_gen_rays' operation order (csrc/nsr_raygen.h), d_k =
    # fma(cz, R_k2, fma(cy, R_k1, cx R_k0)): the inner fma is evaluated in double (its product is exact there) and rounded
    # once, cz = -1 makes the outer one a subtraction -- a matrix product's summation order is the library's choice.  On a
    # device, fp32 quotients and the square root are taken in double and rounded once as well (correctly rounded: 53 >= 2 x 24
    # + 2), because a division by a host scalar is a multiplication by its reciprocal there.  The normalisation follows the
    # device's own reference: on the host torch.norm, which accumulates in double, as the reference's get_rays does; on a device
    # nsr_gen_rays' fp32 sum of squares in its order.
    wide = torch.float64
    pinned = dt == torch.float32 and dev.type != "cpu"
    div = (lambda p_, q_: (p_.to(wide) / q_.to(wide)).to(dt)) if pinned else (lambda p_, q_: p_ / q_)
    f = torch.tensor(focal, dtype=dt, device=dev)
    cx, cy = div(gx - W / 2, f), -div(gy - H / 2, f)
    d = torch.stack([(cy.to(wide) * c2w[k, 1].to(wide) + (cx * c2w[k, 0]).to(wide)).to(dt) - c2w[k, 2] for k in range(3)], -1)
    if dev.type == "cpu":
        nrm = torch.norm(d, dim=-1, keepdim=True)
    else:
        sq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
        nrm = torch.sqrt(sq.to(wide)).to(dt) if pinned else torch.sqrt(sq)
    d = div(d, nrm)
    o = c2w[:, 3].expand(d.shape)
    if ndc:       # get_ndc_rays at near = 1 (models/utils.py:155-196), then near / far := 0 / 1
        t = div(-(1.0 + o[..., 2]), d[..., 2])
        o = o + t[..., None] * d
        ox_oz, oy_oz = div(o[..., 0], o[..., 2]), div(o[..., 1], o[..., 2])
        ax, ay = -1.0 / (W / (2.0 * focal)), -1.0 / (H / (2.0 * focal))
        o2 = 1.0 + div(torch.full_like(o[..., 2], 2.0), o[..., 2])
        o, d = torch.stack([ax * ox_oz, ay * oy_oz, o2], -1), \
            torch.stack([ax * (div(d[..., 0], d[..., 2]) - ox_oz), ay * (div(d[..., 1], d[..., 2]) - oy_oz), 1 - o2], -1)
        near, far = 0.0, 1.0
    one = torch.ones_like(o[:, :1])
    return torch.cat([o, d, near * one, far * one], 1)
