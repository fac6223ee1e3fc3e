"""Pins tests/train_heads_ref.py without a device: (a) ref_composite_bwd against torch.autograd in float64 through a plain
restatement of the forward, (b) ref_lr_loss against autograd of the loss as the model states it, (c) an fp32 emulation of the
kernel's arithmetic stays inside error_bounds on the real-valued cases of tests/test_gpu_train_heads.py, (d) each deliberately
wrong reference of the teeth test leaves the bound on at least one element."""
import itertools

import numpy as np
import pytest
import torch

from tests import train_heads_ref as hr

RTOL = 1e-11


def forward_cumprod(pre, sigma, z, flags):
    """models/rendering.py's compositing, restated: -> comp (R, 3), depth (R,), opacity (R,), weights (R, N)"""
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], 1)
    dens = torch.log(1.0 + torch.exp(sigma - 1.0)) if flags & hr.SOFTPLUS else torch.relu(sigma)
    alpha = 1.0 - torch.exp(-delta * dens)
    shifted = torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], 1)
    w = alpha * torch.cumprod(shifted, 1)[:, :-1]
    head = hr.head_of(flags)
    rgb = pre if head == 2 else (torch.sigmoid(pre) if head == 0 else torch.sigmoid(pre) ** (1.0 / 2.2))
    comp = (w[:, :, None] * rgb).sum(1)
    if flags & hr.WHITE:
        comp = comp + 1.0 - w.sum(1, keepdim=True)
    return rgb, comp, (w * z).sum(1), w.sum(1), w


ALL_FLAGS = [f for f in range(16) if not ((f & hr.GAMMA) and (f & hr.COLOR_NONE))]      # every option word the step accepts
SUBSETS = [s for n in range(4) for s in itertools.combinations(("g_depth", "g_opacity", "g_weights"), n)]


@pytest.mark.parametrize("N", (2, 3, 65))
def test_ref_composite_bwd_equals_autograd(N):
    R = 5
    rng = np.random.default_rng(N)
    z = torch.from_numpy(2.0 + np.cumsum(rng.uniform(0.2, 1.8, (R, N)) * (4.0 / N), 1))
    sig_np = rng.uniform(-0.6, 1.5, (R, N))
    sig_np[:, -1] = rng.uniform(1e-11, 3e-11, R)                  # a live last sample under relu: delta = 1e10
    sig_np[0, -1] = -0.3
    g = dict(g_comp=rng.standard_normal((R, 3)), g_depth=rng.standard_normal(R), g_opacity=rng.standard_normal(R),
             g_weights=rng.standard_normal((R, N)))
    worst = 0.0
    for flags, names in itertools.product(ALL_FLAGS, SUBSETS):
        pre = torch.from_numpy(rng.standard_normal((R, N, 3))).requires_grad_()
        sigma = torch.from_numpy(sig_np).requires_grad_()
        rgb, comp, depth, opac, w = forward_cumprod(pre, sigma, z, flags)
        L = (comp * torch.from_numpy(g["g_comp"])).sum()
        if "g_depth" in names:
            L = L + (depth * torch.from_numpy(g["g_depth"])).sum()
        if "g_opacity" in names:
            L = L + (opac * torch.from_numpy(g["g_opacity"])).sum()
        if "g_weights" in names:
            L = L + (w * torch.from_numpy(g["g_weights"])).sum()
        L.backward()
        want = torch.cat([pre.grad, sigma.grad[:, :, None]], 2).numpy()
        up = {n: (g[n] if n in names else None) for n in ("g_depth", "g_opacity", "g_weights")}
        got, bias = hr.ref_composite_bwd(rgb.detach().numpy(), sig_np, z.numpy(), g["g_comp"], flags, **up)
        got = got.reshape(R, N, 4)
        scale = np.abs(want).max((1, 2), keepdims=True)
        assert (scale > 0).all()
        err = float((np.abs(got - want) / scale).max())
        worst = max(worst, err)
        assert err <= RTOL, (flags, names, err)
        assert np.allclose(bias, want.sum(1), rtol=0, atol=1e-9 * float(scale.max()))
    print(f"N {N}: largest |ref - autograd| / max|d4| per ray {worst:.2e}")


@pytest.mark.parametrize("s2,lam_var,lam_dvar", [(1, 0.0, 0.0), (4, 0.0, 0.0), (4, 0.3, 0.0), (9, 0.3, 0.2), (16, 0.0, 0.2), (9, 0.0, 0.0)])
def test_ref_lr_loss_equals_autograd(s2, lam_var, lam_dvar):
    n_lr, lam, far = 37, 0.7, 6.0
    rng = np.random.default_rng(s2)
    comp = torch.from_numpy(rng.uniform(0, 1, (n_lr, s2, 3))).requires_grad_()
    depth = torch.from_numpy(rng.uniform(2, 6, (n_lr, s2))).requires_grad_()
    target = torch.from_numpy(rng.uniform(0, 1, (n_lr, 3)))
    lr = comp.mean(1)
    L = lam * torch.nn.functional.mse_loss(lr, target)
    var_rgb = var_d = torch.zeros(())
    if s2 > 1:
        var_rgb, var_d = torch.var(comp, 1).sum(), torch.var(depth / far, 1).sum()
        L = L + lam_var * var_rgb + lam_dvar * var_d
    L.backward()
    var_rgb, var_d = var_rgb.detach(), var_d.detach()
    scale = 1.0 / (3.0 * n_lr)
    got_lr, g_comp, g_depth, sums = hr.ref_lr_loss(comp.detach().numpy(), target.numpy(), s2, scale, lam, lam_var, lam_dvar, far,
                                                   depth.detach().numpy())
    want_gc = comp.grad.numpy().reshape(-1, 3)
    assert np.abs(got_lr - lr.detach().numpy()).max() <= RTOL
    assert np.abs(g_comp - want_gc).max() <= RTOL * np.abs(want_gc).max()
    want_gd = depth.grad.numpy().reshape(-1) if depth.grad is not None else np.zeros(n_lr * s2)
    assert np.abs(g_depth - want_gd).max() <= RTOL * max(np.abs(want_gd).max(), 1e-300)
    assert sums.shape == (3, 1)
    mse = float(torch.nn.functional.mse_loss(lr, target).detach())
    assert abs(sums[0, 0] * scale - mse) <= RTOL * mse
    if lam_var:
        assert abs(sums[1, 0] - float(var_rgb)) <= RTOL * float(var_rgb)
    if lam_dvar:
        assert abs(sums[2, 0] - float(var_d)) <= RTOL * float(var_d)
    # the finish: the loss values the step reports
    carry, loss, (vl, vd) = hr.ref_loss_finish(sums.reshape(-1), 1, scale, lam, 1, np.zeros(6), lam_var, lam_dvar)
    assert loss == np.float32(lam * sums[0, 0] * scale) and carry[1] == sums[0, 0] and carry[0] == 0.0
    assert vl == np.float32(lam_var * sums[1, 0]) and vd == np.float32(lam_dvar * sums[2, 0])


def test_block_tree_and_finish_order_on_integers():
    """integer-valued partials: any order gives the same sum, so the tree and the strided per-thread sums must give the plain one"""
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257, 1000):
        sums = rng.integers(0, 1 << 20, (3, n)).astype(np.float64)
        carry0 = np.arange(6, dtype=np.float64) * 1e6
        carry, loss, _ = hr.ref_loss_finish(sums.reshape(-1), n, 0.25, 0.5, 0, carry0, 1.0, 1.0)
        assert carry[0] == carry0[0] + sums[0].sum() and carry[2] == carry0[2] + sums[1].sum() and carry[4] == carry0[4] + sums[2].sum()
        assert (carry[1::2] == carry0[1::2]).all() and loss == np.float32(0.5 * carry[0] * 0.25)


@pytest.mark.parametrize("N", hr.ALL_N)
def test_fp32_emulation_stays_within_the_bound(N):
    """(c): np.float32 operation by operation, libm exp rounded to fp32 -- a correct implementation reaches the bound's inside"""
    case = hr.composite_case(5, N)
    worst = {}
    for flags, names in hr.option_sets():
        up = hr.upstream(case, names)
        args = (case["rgb4"], case["sigma"], case["z"], case["g_comp"], flags)
        ref, _ = hr.ref_composite_bwd(*args, **up)
        bound, _ = hr.error_bounds(*args, **up)
        got = hr.emulate_composite_bwd(*args, **up).astype(np.float64)
        assert np.isfinite(ref).all() and np.isfinite(bound).all() and np.isfinite(got).all(), (flags, names)
        err = np.abs(got - ref)
        nz = bound > 0
        assert (err[~nz] == 0).all(), (flags, names)
        ratio = float((err[nz] / bound[nz]).max())
        worst[hr.flag_name(flags)] = max(worst.get(hr.flag_name(flags), 0.0), ratio)
        assert (err <= bound).all(), (flags, names, ratio)
    print(f"N {N:3d}: largest emulated err / bound per option: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("N", (65, 193))
def test_wrong_references_leave_the_bound(N):
    """(d): on the inputs of the GPU file's teeth test"""
    case = hr.composite_case(5, N)
    args = (case["rgb4"], case["sigma"], case["z"], case["g_comp"], hr.WHITE)
    up = hr.upstream(case, ("g_depth",))
    ref, _ = hr.ref_composite_bwd(*args, **up)
    bound, _ = hr.error_bounds(*args, **up)
    for what in hr.WRONG:
        bad, _ = hr.ref_composite_bwd(*args, **up, wrong=what)
        n = int((np.abs(bad - ref) > 2.0 * bound).sum())        # beyond the bound even from the far side of it
        print(f"N {N} {what}: {n} elements differ by more than twice the bound")
        assert n > 0, what


def test_bound_is_absolute_where_fp32_absorbs():
    """the delta sigma = 20 sample: f is 1e-10 in fp32 and 2.2e-9 in fp64; T of every later sample is off by a factor of 20 and
    still inside the bound, which at those samples is far above the result itself"""
    case = hr.composite_case(5, 65)
    args = (case["rgb4"], case["sigma"], case["z"], case["g_comp"], 0)
    ref, _ = hr.ref_composite_bwd(*args)
    bound, _ = hr.error_bounds(*args)
    got = hr.emulate_composite_bwd(*args).astype(np.float64)
    r, k = hr.RAY_OPAQUE_MID, 65 // 2 + 1
    sl = slice(r * 65 + k, r * 65 + (3 * 65) // 4)
    live = ref[sl, :3] != 0                                       # (sigma <= 0: w = 0 on both sides)
    rel = np.abs(got[sl, :3] - ref[sl, :3])[live] / np.abs(ref[sl, :3])[live]
    assert rel.max() > 0.5 and (np.abs(got[sl] - ref[sl]) <= bound[sl]).all()
