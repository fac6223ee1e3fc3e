"""The gradient with respect to the rays, without a GPU: the restatement of its two kernels (tests/ray_grads_ref.py) against
torch fp64 autograd of the oracle's encoding and cast_rays, the restatement's power to tell wrong forms from the right one,
``cameras.rays_from_pose`` against the oracle's ray grid, and the new exports."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as oc
from tests import ray_grads_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_XYZ, LINEAR = rr.NO_XYZ, rr.LINEAR_FREQS


def _inputs(R, N, stride, deg_pos, deg_dir, embed, seed):
    rng = np.random.default_rng(seed)
    rays = rng.uniform(-1.0, 1.0, (R, stride))
    rays[:, 6], rays[:, 7] = 0.0, 1.0
    z = np.sort(rng.uniform(0.05, 1.5, (R, N)), axis=1)
    g_pe = rng.standard_normal((R, N, rr.n_cols(deg_pos, embed)))
    g_dir = rng.standard_normal((R, N, rr.n_cols(deg_dir, embed)))
    return rays, z, g_pe, g_dir


def _restated(rays, z, g_pe, g_dir, deg_pos, deg_dir, embed, variant=None):
    """The two kernels on what the forward would have kept: the encoded points and the encoded direction."""
    R, N = z.shape
    stride = rays.shape[1]
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    x = oc.points_on_rays(t(rays[:, 0:3]), t(rays[:, 3:6]), t(z)).reshape(-1, 3)
    v = t(rays[:, 8:11] if stride == 11 else rays[:, 3:6])
    enc, enc_dir = rr.posenc_e(x, deg_pos, embed).numpy(), rr.posenc_e(v, deg_dir, embed).numpy()
    # two sources (layer 0 and one skip layer) that sum to the gradient of the encoded columns
    half = 0.25 * g_pe.reshape(R * N, -1)
    g_x = rr.encode_bwd([half, 3.0 * half], enc, deg_pos, embed, variant if variant in ("swap_sign", "no_f") else None)
    return rr.ray_grad(g_x.reshape(R, N, 3), z, g_dir, enc_dir, deg_dir, embed, stride, variant)


# --no_xyz on a degree-0 encoding has no columns: the library refuses it (include/nsr_train.h), and it is no case here
@pytest.mark.parametrize("stride", (8, 11))
@pytest.mark.parametrize("deg,embed", [(d, e) for d in (0, 1, 6, 10) for e in (0, NO_XYZ, LINEAR, NO_XYZ | LINEAR)
                                       if not ((e & NO_XYZ) and d == 0)])
def test_restatement_is_autograd(deg, embed, stride):
    """Degrees 0, 1, 6, 10 (positions; the direction takes min(deg, 4)), both embed bits, 8- and 11-wide rays."""
    deg_dir = min(deg, 4)
    rays, z, g_pe, g_dir = _inputs(5, 7, stride, deg, deg_dir, embed, 10 * deg + embed + stride)
    want = rr.autograd_rows(rays, z, g_pe, g_dir, deg, deg_dir, embed)
    got = _restated(rays, z, g_pe, g_dir, deg, deg_dir, embed)
    assert got.shape == want.shape == (5, stride)
    assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    assert (got[:, 6:8] == 0.0).all() and (want[:, 6:8] == 0.0).all()
    if stride == 11 and rr.n_cols(deg_dir, embed) > 0:
        assert np.abs(want[:, 8:11]).max() > 0.0


def test_word_zero_is_the_oracles_encoding():
    x = torch.from_numpy(np.random.default_rng(0).uniform(-2, 2, (9, 3)))
    for deg in (0, 1, 6, 10):
        assert torch.equal(rr.posenc_e(x, deg, 0), oc.posenc(x, deg))
    want = rr.autograd_rows(*_inputs(3, 4, 8, 6, 4, 0, 1), 6, 4, 0, encode=lambda t, deg, embed: oc.posenc(t, deg))
    assert np.array_equal(want, rr.autograd_rows(*_inputs(3, 4, 8, 6, 4, 0, 1), 6, 4, 0))


@pytest.mark.parametrize("variant", rr.VARIANTS)
def test_restatement_tells_wrong_variants_apart(variant):
    stride = 11 if variant == "dir_at_11" else 8
    rays, z, g_pe, g_dir = _inputs(5, 7, stride, 6, 4, 0, 3)
    want = rr.autograd_rows(rays, z, g_pe, g_dir, 6, 4, 0)
    right = _restated(rays, z, g_pe, g_dir, 6, 4, 0)
    wrong = _restated(rays, z, g_pe, g_dir, 6, 4, 0, variant)
    scale = np.abs(want).max()
    assert np.abs(right - want).max() <= 1e-11 * scale
    assert np.abs(wrong - want).max() > 1e-3 * scale, variant


def test_band_table_is_the_librarys():
    import ctypes
    from nerf_sr_amd import _lib
    lib = _lib.load()
    for deg in (1, 2, 6, 10, 16):
        for embed in (0, LINEAR):
            f = (ctypes.c_float * 16)()
            assert lib.nsr_posenc_freqs(deg, embed, f) == 0
            assert np.array_equal(np.array(f[:deg], np.float32), rr.bands_of(deg, embed)), (deg, embed)


@pytest.mark.parametrize("ndc", (True, False))
def test_rays_from_pose_is_the_oracles_grid(golden_dir, ndc):
    """8 x 6 <- 4 x 3: every row within 2.4e-7 of oc.subpixel_ray_grid, in fp32; differentiable with respect to the pose."""
    from nerf_sr_amd import cameras
    rg = np.load(os.path.join(golden_dir, "raygrid.npz"))
    scene = "llff" if ndc else "blender"
    W, H, s = 8, 6, 2
    c2w = torch.from_numpy(rg[f"{scene}_c2w"].astype(np.float32)[:3, :4])
    focal = float(rg[f"{scene}_focal"]) * W / int(rg["W"])
    want = oc.subpixel_ray_grid(c2w, H, W, focal, s, ndc, 2.0, 6.0).reshape(-1, 8)
    got = cameras.rays_from_pose(c2w, H, W, focal, s, ndc, 2.0, 6.0)
    assert got.shape == (48, 8) and got.dtype == torch.float32
    assert float((got - want).abs().max()) <= 2.4e-7
    rows = torch.tensor([47, 0, 13, 13, 30])
    picked = cameras.rays_from_pose(c2w, H, W, focal, s, ndc, 2.0, 6.0, rows=rows)      # (a matrix product of another shape)
    assert picked.shape == (5, 8) and float((picked - want[rows]).abs().max()) <= 2.4e-7
    pose = c2w.double().requires_grad_(True)
    coef = torch.from_numpy(np.random.default_rng(2).standard_normal((48, 8)))
    (cameras.rays_from_pose(pose, H, W, focal, s, ndc, 2.0, 6.0) * coef).sum().backward()
    ref = c2w.double().requires_grad_(True)
    dirs = oc.ray_directions(H, W, focal).double()
    o, d = oc.rays_from_pose(dirs, ref)
    if ndc:
        o, d = oc.ndc_rays(H, W, focal, 1.0, o, d)
    od = torch.cat([o, d], 1).view(H, W, 6).view(H // s, s, W // s, s, 6).permute(0, 2, 1, 3, 4).reshape(-1, 6)
    (od * coef[:, :6]).sum().backward()
    # the oracle builds its pixel grid in fp32 (2^-24 relative per direction component), rays_from_pose in the pose's dtype
    assert float((pose.grad - ref.grad).abs().max()) <= 1e-6 * float(ref.grad.abs().max())
    assert not re.search(r"^\s*(import|from)\s+oracle", open(os.path.join(REPO, "nerf_sr_amd", "cameras.py")).read(), re.M)


def test_new_exports_are_declared_and_bound():
    from nerf_sr_amd import _lib
    header = open(os.path.join(REPO, "include", "nsr_train.h")).read()
    lib = _lib.load()
    for name in ("nsr_train_arch_backward_r", "nsr_train_arch_workspace_bytes_r"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.nsr_version() == 131
    assert "near / far needs the resampler's backward" in header
    # sizes: the `_r` workspace is the `_e` one plus the three matrices; 0 where the pair refuses
    arch = _lib.NsrArch(8, 256, 1 << 4, 10, 4, 0)
    import ctypes
    for prec in (_lib.NSR_FP32, _lib.NSR_F16X3_GEMM):
        e = lib.nsr_train_arch_workspace_bytes_e(ctypes.byref(arch), 0, prec, 32, 64, 64)
        r = lib.nsr_train_arch_workspace_bytes_r(ctypes.byref(arch), 0, prec, 32, 64, 64)
        P = 32 * 128
        assert e > 0 and r == e + 4 * (2 * P * 64 + P * 32 + P * 3)
    assert lib.nsr_train_arch_workspace_bytes_r(ctypes.byref(arch), 0, _lib.NSR_F16X3, 32, 64, 64) == 0
    assert lib.nsr_train_arch_workspace_bytes_r(ctypes.byref(arch), 4, _lib.NSR_FP32, 32, 64, 64) == 0
    assert lib.nsr_train_arch_backward_r(None, 0, None, None, None, None, None, None, 8, None, 0, None, 0, None) == -1
