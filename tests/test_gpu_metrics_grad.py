"""The differentiable SSIM on the device (``nsr_ssim_backward`` behind ``metrics.SSIM`` under autograd, and
``RefineTrainer(refine_with_ssim=True)``) against fp64 autograd of tests/metrics_ref.py on the CPU, fed the same fp32 values
cast to double (tests/test_metrics_grad_cpu.py ties that oracle to the reference's own class).

Bound.  max |g - g64| <= 2^-23 max |g64| per gradient tensor.  Derived, not measured: the kernel's arithmetic is double and
its only rounding is the fp32 store, at most 2^-24 of an element's own magnitude; the bound leaves a factor of two.
Emulated on the CPU (the fp64 gradient rounded to fp32) the distance is 2.0e-8 ... 4.3e-8 of the maximum.  Everything the
fixed summation order promises is compared by bits."""
import os

import numpy as np
import pytest
import torch

from nerf_sr_amd.refine import make_refine_state_dict
from . import metrics_ref as ref
from .metrics_ref import ssim_options

pytestmark = pytest.mark.gpu
TAGS = ["tiny", "ragged", "gray", "box", "flat", "rows"]
BOUND = 2.0 ** -23


@pytest.fixture(scope="module")
def g(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return np.load(os.path.join(golden_dir, "metrics.npz"))


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def case(g, tag):
    """(x, y, SSIM options) on the CPU in fp32.  ``rows``: 8-bit levels, (1, 2, 7, 67) -- H = 7 < 2 pad + 1 gives rows 1..5 both
    reflected aliases at once, over three column tiles, the last one ragged."""
    if tag != "rows":
        return torch.from_numpy(g[f"x_{tag}"]), torch.from_numpy(g[f"y_{tag}"]), ssim_options(g, tag)
    gen = torch.Generator().manual_seed(31)
    x = torch.round(torch.rand(1, 2, 7, 67, generator=gen) * 255) / 255
    y = torch.round((x + 0.1 * torch.randn(1, 2, 7, 67, generator=gen)).clamp(0, 1) * 255) / 255
    return x.float(), y.float(), dict(data_range=(0.0, 1.0), kernel_size=(11, 11), sigma=(1.5, 1.5), gaussian=True)


def upstream(shape, tag):
    """Seeded fp32 weights: per image (B,), and per map element (B, C, H, W) at the scale of the mean's own 1 / (C H W)."""
    gen = torch.Generator().manual_seed(100 + TAGS.index(tag))
    B, C, H, W = shape
    return (torch.rand(B, generator=gen) + 0.5).float(), (torch.randn(shape, generator=gen) / (C * H * W)).float()


_ORACLE = {}


def oracle(g, tag, with_map):
    """fp64 autograd of metrics_ref.ssim_map on the CPU (computed once per case and kept), and the distance of the same
    composition in fp32 from it: the reference's own fp32-autograd error."""
    key = (tag, with_map)
    if key not in _ORACLE:
        x, y, kw = case(g, tag)
        v, gm = upstream(tuple(x.shape), tag)
        res = {}
        for dt in (torch.float64, torch.float32):
            xd, yd = x.to(dt).requires_grad_(True), y.to(dt).requires_grad_(True)
            m = ref.ssim_map(xd, yd, **kw)
            up = (m.mean((1, 2, 3)) * v.to(dt)).sum()
            if with_map:
                up = up + (m * gm.to(dt)).sum()
            res[dt] = torch.autograd.grad(up, (xd, yd))
        g64 = res[torch.float64]
        own = [float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(res[torch.float32], g64)]
        _ORACLE[key] = (g64, own)
    return _ORACLE[key]


def device_grads(x, y, kw, v, gm=None, layout="BCHW", wrt=(True, True), reduction="none"):
    """Gradients of sum(v * ssim) (+ sum(gm * map)) through metrics.SSIM; inputs given in BCHW and permuted for BHWC."""
    from nerf_sr_amd.metrics import SSIM
    to = (lambda t: t) if layout == "BCHW" else (lambda t: t.permute(0, 2, 3, 1).contiguous())
    xd, yd = to(x).cuda().requires_grad_(wrt[0]), to(y).cuda().requires_grad_(wrt[1])
    s = SSIM(**kw)
    if gm is None:
        vals = s(xd, yd, reduction=reduction, layout=layout)
        up = (vals * v.cuda()).sum() if reduction == "none" else vals
    else:
        vals, smap = s(xd, yd, reduction="none", layout=layout, return_map=True)
        up = (vals * v.cuda()).sum() + (smap * gm.cuda()).sum()
    up.backward()
    return xd.grad, yd.grad


@pytest.mark.parametrize("with_map", [False, True], ids=["values", "values+map"])
@pytest.mark.parametrize("tag", TAGS)
def test_gradients_vs_fp64_autograd(g, tag, with_map):
    x, y, kw = case(g, tag)
    v, gm = upstream(tuple(x.shape), tag)
    (gx64, gy64), own = oracle(g, tag, with_map)
    gx, gy = device_grads(x, y, kw, v, gm if with_map else None)
    assert gx.dtype == torch.float32 and gy.dtype == torch.float32 and tuple(gx.shape) == tuple(x.shape) == tuple(gy.shape)
    errs = [float((got.cpu().double() - want).abs().max() / want.abs().max()) for got, want in ((gx, gx64), (gy, gy64))]
    print(f"{tag}/{'values+map' if with_map else 'values'}: max |g - g64| / max |g64| = {errs[0]:.2e} (output) {errs[1]:.2e} (target), "
          f"bound {BOUND:.2e}; torch fp32 autograd of the same composition: {own[0]:.1e} {own[1]:.1e}")
    assert errs[0] <= BOUND and errs[1] <= BOUND, (tag, errs)


def test_gradient_invariances(g):
    x, y, kw = case(g, "ragged")
    v, gm = upstream(tuple(x.shape), "ragged")
    gx, gy = device_grads(x, y, kw, v, gm)
    # BHWC inputs give the permuted BCHW gradients
    hx, hy = device_grads(x, y, kw, v, gm, layout="BHWC")
    assert tuple(hx.shape) == (2, 45, 70, 3)
    assert bits(hx.permute(0, 3, 1, 2).contiguous()) == bits(gx) and bits(hy.permute(0, 3, 1, 2).contiguous()) == bits(gy)
    # only one gradient requested: the bits of the both-requested call, and nothing for the other input
    ox, none_y = device_grads(x, y, kw, v, gm, wrt=(True, False))
    none_x, oy = device_grads(x, y, kw, v, gm, wrt=(False, True))
    assert none_x is None and none_y is None and bits(ox) == bits(gx) and bits(oy) == bits(gy)
    # an image's gradient is the same alone, in each slot of a batch of three, and on a second call
    one = torch.ones(1)
    ax, ay = device_grads(x[:1], y[:1], kw, one)
    again = device_grads(x[:1], y[:1], kw, one)
    assert bits(again[0]) == bits(ax) and bits(again[1]) == bits(ay)
    fx, fy = torch.flip(x[1:], dims=(3,)), torch.flip(y[1:], dims=(2,))
    for slot in range(3):
        order = [1, 2]
        order.insert(slot, 0)
        bx, by = torch.cat([x, fx])[order].contiguous(), torch.cat([y, fy])[order].contiguous()
        sx, sy = device_grads(bx, by, kw, torch.ones(3))
        assert bits(sx[slot:slot + 1]) == bits(ax) and bits(sy[slot:slot + 1]) == bits(ay), slot
    # reduction='mean' is 'none' driven with an upstream of fp32 1 / B
    mx, my = device_grads(x, y, kw, None, reduction="mean")
    nx, ny = device_grads(x, y, kw, torch.full((2,), 0.5))
    assert bits(mx) == bits(nx) and bits(my) == bits(ny)
    # SSIM is stationary at output == target: the gradient with respect to x of ssim(x, x) is what rounding in double leaves of
    # terms of the size of the ragged gradients -- far below one fp32 spacing of them (1e-10 = 5e5 double spacings, for the
    # cancellation of 2 x V against x Z over 121 taps and the 1 / b2 <= 1 / c2 = 1.1e3 in both)
    from nerf_sr_amd.metrics import SSIM
    xs = x.cuda().requires_grad_(True)
    SSIM(**kw)(xs, xs, reduction="sum").backward()
    scale = float(device_grads(x, y, kw, torch.ones(2))[0].abs().max())
    print(f"ssim(x, x): max |grad| {float(xs.grad.abs().max()):.2e} against {scale:.2e} of ssim(x, y)")
    assert bool(torch.isfinite(xs.grad).all()) and float(xs.grad.abs().max()) <= 1e-10 * scale


def test_forward_is_unchanged_by_autograd(g):
    from nerf_sr_amd.metrics import SSIM
    x, y, kw = case(g, "ragged")
    s = SSIM(**kw)
    xc, yc = x.cuda(), y.cuda()
    vals, smap = s(xc, yc, reduction="none", return_map=True)
    assert vals.grad_fn is None and smap.grad_fn is None and not vals.requires_grad and s(xc, yc).grad_fn is None
    xg = xc.clone().requires_grad_(True)
    gvals, gsmap = s(xg, yc, reduction="none", return_map=True)
    assert gvals.grad_fn is not None and gsmap.grad_fn is not None
    assert bits(gvals) == bits(vals) and bits(gsmap) == bits(smap)
    for red in ("mean", "sum"):
        assert bits(s(xg, yc, reduction=red)) == bits(s(xc, yc, reduction=red))
    with torch.no_grad():
        assert s(xg, yc).grad_fn is None
    yg = yc.clone().requires_grad_(True)
    hw = lambda t: t.permute(0, 2, 3, 1).contiguous()
    assert bits(s(hw(xc), hw(yg), reduction="none", layout="BHWC")) == bits(vals)


# ------------------------------------------------------------------------------------------------------ trainer
def patch_batch():
    """B = 2, R = 2, 16 x 16: forward_train's smallest shape that the window's padding (5) admits."""
    gen = torch.Generator().manual_seed(9)
    gt = (torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1)
    sr = (gt + 0.2 * torch.randn(2, 3, 16, 16, generator=gen)).clamp(-1, 1)
    refs = (gt.unsqueeze(1) + 0.1 * torch.randn(2, 2, 3, 16, 16, generator=gen)).clamp(-1, 1)
    return {"sr_patch": sr, "ref_patches": refs, "gt_patch": gt}


def test_trainer_ssim_loss(g):
    from nerf_sr_amd import refine
    from nerf_sr_amd.metrics import SSIM
    sd, batch, lam = make_refine_state_dict(7), patch_batch(), 0.75
    tr = refine.RefineTrainer(sd, refine_with_l1=False, refine_with_ssim=True, lambda_refine_ssim=lam)
    tr.set_input(batch)
    tr.forward()
    tr.backward()
    score = SSIM(data_range=(-1, 1))(tr.pred.detach(), tr.data_gt_patch)
    assert bits(tr.loss_ssim) == bits(lam * (1 - score)) and bits(tr.loss_tot) == bits(tr.loss_ssim) and float(tr.loss_l1) == 0.0
    assert abs(float(score) - float(ref.ssim(tr.pred.detach().cpu().double(), batch["gt_patch"].double(), reduction="mean", data_range=(-1, 1)))) <= 1e-6
    # by hand: forward_train + metrics.SSIM + backward() on a second copy of the same state
    by = refine.RefineTrainer(sd)
    pred = refine.forward_train(by.params, by.running, tr.data_sr_patch, tr.data_ref_patches, by.momentum, by.img_chunk)
    assert bits(pred) == bits(tr.pred)
    (lam * (1 - SSIM(data_range=(-1, 1))(pred, tr.data_gt_patch))).backward()
    live = 0
    for k, p in tr.params.items():
        assert bits(p.grad) == bits(by.params[k].grad), k
        live += int(float(p.grad.abs().max()) > 0)
    assert live >= 50                                    # the 17 biases in front of a BatchNorm get exact zeros, the rest moves
    # with the defaults nothing changes: L1 alone, loss_ssim a constant zero outside the graph
    plain = refine.RefineTrainer(sd)
    plain.set_input(batch)
    plain.forward()
    plain.backward()
    assert float(plain.loss_ssim) == 0.0 and plain.loss_ssim.grad_fn is None and bits(plain.loss_tot) == bits(plain.loss_l1)
    # both: the sum
    both = refine.RefineTrainer(sd, refine_with_ssim=True)
    both.set_input(batch)
    both.forward()
    both.calculate_losses()
    assert bits(both.loss_tot) == bits(both.loss_mse + both.loss_l1 + both.loss_ssim) and bits(both.loss_l1) == bits(plain.loss_l1)


def test_ten_steps_on_the_ssim_loss_raise_the_ssim(g):
    from nerf_sr_amd import refine
    tr = refine.RefineTrainer(make_refine_state_dict(7), refine_with_l1=False, refine_with_ssim=True)
    tr.set_input(patch_batch())
    losses = [float(tr.optimize_parameters()) for _ in range(10)]
    tr.forward()
    tr.calculate_losses()
    first, last = 1.0 - losses[0], 1.0 - float(tr.loss_ssim.detach())
    print(f"SSIM of the batch: {first:.4f} -> {last:.4f} after ten steps (1 - SSIM per step: {[round(v, 4) for v in losses]})")
    assert all(np.isfinite(losses)) and last > first
