"""The image-space regularisers on the device (include/nsr_losses.h behind nerf_sr_amd/losses.py) against the reference's own
classes evaluated in fp64 (tests/golden/losses.npz) and, on larger shapes, against fp64 autograd of tests/losses_ref.py on the
CPU fed the same fp32 values (tests/test_losses_cpu.py ties that restatement to the reference's classes).

Bounds, derived and not measured.
  loss      |device double - loss64| <= 1e-10 |loss64|, and exactly 0 where loss64 is 0: the kernels evaluate the reference's
            expression in double, so the terms agree to a few double spacings, and a sum of at most 4e5 non-negative double
            terms in another order differs by at most n 2^-53 = 4.4e-11 of the sum.
  gradient  max |g - g64| <= 2^-23 max |g64| per tensor: double arithmetic and ONE rounding, the fp32 store, at most 2^-24 of
            an element's own magnitude (the bound and reasoning of tests/test_gpu_metrics_grad.py).  The fixtures' gradients
            are of 0.7 * loss with 0.7 in double while the device multiplies by fp32(0.7), which is 2^-25.7 off: together
            2^-24 + 2^-25.7 < 2^-23.  Where the fp64 gradient is exactly 0 (constant, ramp, quantised inputs,
            targets == inputs) the device gradient must be exactly 0: sign(0) = 0.
Everything the fixed summation order promises is compared by bits."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from nerf_sr_amd.weights import make_state_dict, STATE_DICT_SPEC
from . import losses_ref as ref

pytestmark = pytest.mark.gpu
LOSS_RTOL = 1e-10
GRAD_BOUND = 2.0 ** -23
UP32 = float(np.float32(0.7))
ZERO_CASES = ("const", "ramp", "quant", "half")     # the cases built to have exact zeros (a random case's fp64 gradient may hold a
#                                                   zero too, where rounding residues of unrelated terms happen to cancel)
HEAD = ("rgb.0.weight", "rgb.0.bias", "dir_encoding.0.weight", "dir_encoding.0.bias", "xyz_encoding_final.weight",
        "xyz_encoding_final.bias", "sigma.weight", "sigma.bias")


@pytest.fixture(scope="module")
def g(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return np.load(os.path.join(golden_dir, "losses.npz"))


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def _p(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def device_double(kind, *tensors, gamma=0.1):
    """The loss as the entry point writes it: one device double.  tensors: device fp32, contiguous."""
    lib = _lib.load()
    loss = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    if kind == "tv":
        (x,) = tensors
        H, W, C = x.shape
        ws = torch.empty(lib.nsr_loss_workspace_bytes(_lib.NSR_LOSS_TV, 1, C, H, W), dtype=torch.uint8, device="cuda")
        st = lib.nsr_tv_loss(_p(x), H, W, C, _p(loss), _p(ws), ws.numel(), _stream())
    elif kind == "gradient":
        a, b = tensors
        B, C, H, W = a.shape
        ws = torch.empty(lib.nsr_loss_workspace_bytes(_lib.NSR_LOSS_GRADIENT, B, C, H, W), dtype=torch.uint8, device="cuda")
        st = lib.nsr_gradient_loss(_p(a), _p(b), B, C, H, W, _p(loss), _p(ws), ws.numel(), _stream())
    else:
        d, guide = tensors
        N, H, W = d.shape
        C = 1 if guide is None else guide.shape[3]
        ws = torch.empty(lib.nsr_loss_workspace_bytes(_lib.NSR_LOSS_LAPLACIAN, N, C, H, W), dtype=torch.uint8, device="cuda")
        st = lib.nsr_laplacian_loss(_p(d), _p(guide), N, H, W, C, gamma, _p(loss), _p(ws), ws.numel(), _stream())
    assert st == 0, (kind, st)
    return loss


def fixture_cases(g):
    """(id, kind, fp32 inputs on the CPU, names of the differentiable ones, gamma)."""
    cases = []
    for tag in g["tv_tags"]:
        cases.append((f"tv_{tag}", "tv", {"x": g[f"tv_{tag}_x"]}, ["x"], None))
    for tag in g["gradient_tags"]:
        cases.append((f"gradient_{tag}", "gradient", {"a": g[f"gradient_{tag}_a"], "b": g[f"gradient_{tag}_b"]}, ["a", "b"], None))
    for tag in g["laplacian_tags"]:
        cases.append((f"laplacian_{tag}", "laplacian", {"d": g[f"laplacian_{tag}_d"]}, ["d"], None))
    for tag in g["bilateral_tags"]:
        cases.append((f"bilateral_{tag}", "laplacian", {"d": g[f"bilateral_{tag}_d"], "guide": g[f"bilateral_{tag}_guide"]}, ["d"],
                      float(g[f"bilateral_{tag}_gamma"])))
    return cases


def class_call(kind, inputs, gamma):
    """The public class over device tensors, in the order of the reference's call signature."""
    from nerf_sr_amd import losses
    if kind == "tv":
        return losses.TVLoss()(inputs["x"])
    if kind == "gradient":
        return losses.GradientLoss()(inputs["a"], inputs["b"])
    if "guide" in inputs:
        return losses.BilateralLaplacianLoss(gamma=gamma)(inputs["d"], inputs["guide"])
    return losses.LaplacianLoss()(inputs["d"])


def check_grad(got, want, what, exact_zeros):
    got, want = got.detach().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f"{what}: max |g - g64| = {err:.3e}, max |g64| = {scale:.3e}, ratio {err / scale if scale else 0.0:.2e} (bound {GRAD_BOUND:.2e})")
    assert err <= GRAD_BOUND * scale, (what, err, scale)
    if exact_zeros:
        assert not got[want == 0].any(), f"{what}: non-zero where the fp64 gradient is exactly 0"


def test_fixture_losses(g):
    for cid, kind, arrays, _, gamma in fixture_cases(g):
        dev = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
        if kind == "gradient" and dev["a"].ndim == 3:
            raw = (dev["a"].unsqueeze(0), dev["b"].unsqueeze(0))
        elif kind == "laplacian":
            raw = (dev["d"], dev.get("guide"))
        else:
            raw = tuple(dev.values())
        dbl = device_double(kind, *raw, gamma=gamma or 0.1)
        want = float(g[f"{cid}_loss64"])
        got = float(dbl)
        print(f"{cid}: device {got:.17g} loss64 {want:.17g} rel {abs(got - want) / want if want else 0.0:.2e} "
              f"(reference's own fp32: {abs(float(g[f'{cid}_loss32']) - want) / want if want else 0.0:.1e})")
        assert abs(got - want) <= LOSS_RTOL * abs(want), (cid, got, want)
        if want == 0:
            assert got == 0, cid
        out = class_call(kind, dev, gamma)
        assert out.dtype == torch.float32 and out.ndim == 0 and out.is_cuda and out.grad_fn is None
        assert bits(out) == bits(dbl[0].to(torch.float32)), cid


def test_fixture_gradients(g):
    for cid, kind, arrays, wrt, gamma in fixture_cases(g):
        dev = {k: torch.from_numpy(v).cuda().requires_grad_(k in wrt) for k, v in arrays.items()}
        out = class_call(kind, dev, gamma)
        assert out.grad_fn is not None
        (0.7 * out).backward()
        for n in wrt:
            want = g[f"{cid}_g{n}64"]
            if not np.abs(want).max():
                assert dev[n].grad.shape == want.shape and not bool(dev[n].grad.any()), cid
                continue
            check_grad(dev[n].grad, want, f"{cid} d/d{n}", exact_zeros=cid.split("_")[1] in ZERO_CASES)
        # the forward value is the same bits with and without grad
        assert bits(out) == bits(class_call(kind, {k: v.detach() for k, v in dev.items()}, gamma)), cid


def test_gradient_loss_singly_and_together(g):
    from nerf_sr_amd.losses import GradientLoss
    for tag in ("1x3x33x34", "half", "quant", "3d"):
        a, b = torch.from_numpy(g[f"gradient_{tag}_a"]).cuda(), torch.from_numpy(g[f"gradient_{tag}_b"]).cuda()
        res = {}
        for wrt in ((True, True), (True, False), (False, True)):
            x, y = a.clone().requires_grad_(wrt[0]), b.clone().requires_grad_(wrt[1])
            (0.7 * GradientLoss()(x, y)).backward()
            res[wrt] = (x.grad, y.grad)
        assert res[(True, False)][1] is None and res[(False, True)][0] is None
        assert bits(res[(True, False)][0]) == bits(res[(True, True)][0]) and bits(res[(False, True)][1]) == bits(res[(True, True)][1])
        assert tuple(res[(True, True)][0].shape) == tuple(a.shape)


# ------------------------------------------------------------------------------------------------------ larger shapes
_BIG = {}


def big_case(kind):
    """Seeded fp32 inputs and the fp64 oracle (loss, gradients of fp32(0.7) * loss) on the CPU, computed once and kept."""
    if kind not in _BIG:
        gen = torch.Generator().manual_seed({"gradient": 51, "bilateral": 52, "tv": 53}[kind])
        rnd = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).float()
        if kind == "gradient":                  # the refinement batch: 32 patches of 3 x 64 x 64
            inputs, wrt, fn = [rnd(32, 3, 64, 64), rnd(32, 3, 64, 64)], (0, 1), ref.gradient
        elif kind == "bilateral":
            inputs, wrt, fn = [rnd(16, 64, 64), rnd(16, 64, 64, 3) * 0.05], (0,), lambda d, gd: ref.laplacian(d, gd, 0.1)
        else:
            inputs, wrt, fn = [rnd(64, 64, 3)], (0,), ref.tv
        dbl = [t.double().requires_grad_(i in wrt) for i, t in enumerate(inputs)]
        loss = fn(*dbl)
        grads = torch.autograd.grad(UP32 * loss, [dbl[i] for i in wrt])
        _BIG[kind] = (inputs, float(loss.detach()), [gr.numpy() for gr in grads])
    return _BIG[kind]


@pytest.mark.parametrize("kind", ["gradient", "bilateral", "tv"])
def test_larger_shapes_vs_fp64_autograd(kind):
    """Several workgroups per plane and per reduction, tiles with neighbours on all sides."""
    from nerf_sr_amd import losses
    inputs, want_loss, want_grads = big_case(kind)
    dev = [t.cuda() for t in inputs]
    if kind == "gradient":
        dbl = device_double("gradient", *dev)
        leaves = [t.clone().requires_grad_(True) for t in dev]
        out = losses.GradientLoss()(*leaves)
    elif kind == "bilateral":
        dbl = device_double("laplacian", *dev, gamma=0.1)
        leaves = [dev[0].clone().requires_grad_(True)]
        out = losses.BilateralLaplacianLoss()(leaves[0], dev[1])
    else:
        dbl = device_double("tv", *dev)
        leaves = [dev[0].clone().requires_grad_(True)]
        out = losses.TVLoss()(leaves[0])
    print(f"{kind}: device {float(dbl):.17g} fp64 {want_loss:.17g} rel {abs(float(dbl) - want_loss) / want_loss:.2e}")
    assert abs(float(dbl) - want_loss) <= LOSS_RTOL * want_loss
    assert bits(out) == bits(dbl[0].to(torch.float32))
    (0.7 * out).backward()
    for i, (leaf, want) in enumerate(zip(leaves, want_grads)):
        check_grad(leaf.grad, want, f"{kind} input {i}", exact_zeros=False)


def test_reproducible_and_fully_overwritten():
    """Two identical calls give identical bits; gradient buffers pre-filled with NaN come back fully overwritten (ragged
    tiles: 33 x 35 and 70 x 45)."""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(61)
    rnd = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).float().cuda()
    up = torch.tensor([0.7], dtype=torch.float32, device="cuda")
    nan_like = lambda t: torch.full_like(t, float("nan"))
    x = rnd(33, 35, 3)
    a, b = rnd(2, 3, 70, 45), rnd(2, 3, 70, 45)
    d, guide = rnd(2, 33, 35), rnd(2, 33, 35, 3) * 0.05
    runs = []
    for _ in range(2):
        gx, ga, gb, gd, gdb = nan_like(x), nan_like(a), nan_like(b), nan_like(d), nan_like(d)
        vals = [device_double("tv", x), device_double("gradient", a, b), device_double("laplacian", d, None),
                device_double("laplacian", d, guide, gamma=0.1)]
        assert lib.nsr_tv_loss_backward(_p(x), 33, 35, 3, _p(up), _p(gx), _stream()) == 0
        assert lib.nsr_gradient_loss_backward(_p(a), _p(b), 2, 3, 70, 45, _p(up), _p(ga), _p(gb), _stream()) == 0
        assert lib.nsr_laplacian_loss_backward(_p(d), None, 2, 33, 35, 1, 1.0, _p(up), _p(gd), _stream()) == 0
        assert lib.nsr_laplacian_loss_backward(_p(d), _p(guide), 2, 33, 35, 3, 0.1, _p(up), _p(gdb), _stream()) == 0
        grads = [gx, ga, gb, gd, gdb]
        for t in grads:
            assert bool(torch.isfinite(t).all()) and bool(t.any())
        assert all(np.isfinite(float(v)) and float(v) > 0 for v in vals)
        runs.append([bits(v) for v in vals] + [bits(t) for t in grads])
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------- composition with the renderer
def _patch_and_draws():
    """An 8 x 8 HR raster of 64 rays and seeded draws for 64 + 64 samples (tests/test_gpu_train_autograd.py's patch)."""
    from nerf_sr_amd import ops, cameras
    patch = ops.subpixel_rays(cameras.spiral_pose(0.5), (64, 48), cameras.llff_focal(64), 2, True)
    patch = patch.reshape(24, 32, 2, 2, 8)[4:8, 4:8].permute(0, 2, 1, 3, 4).reshape(-1, 8).contiguous()
    gen = torch.Generator().manual_seed(2)
    draws = {"u_coarse": torch.rand(64, 64, generator=gen), "noise_coarse": torch.randn(64, 64, generator=gen),
             "u_fine": torch.rand(64, 64, generator=gen), "noise_fine": torch.randn(64, 128, generator=gen)}
    return patch, {k: v.cuda() for k, v in draws.items()}


def _trainer(**kw):
    from nerf_sr_amd import train
    return train.Trainer(make_state_dict(3), make_state_dict(4), downscale=2, randomized=True, noise_std=1.0, precision="f16x3", **kw)


def test_composes_with_forward_rays_train():
    """0.7 * bilateral Laplacian of the fine depth + TV of the fine colours over a rendered 8 x 8 patch: the weight gradients
    through the device losses against the same loss written in fp32 torch ops (tests/losses_ref.py) over the same forward,
    within the per-tensor training bounds of tests/test_gpu_train_autograd.py (2e-3 of each tensor's norm, 5e-4 on the heads,
    2e-3 on the whole network).  Shows that the upstream gradients arrive in the right layout; no new accuracy claim."""
    from nerf_sr_amd import losses
    patch, draws = _patch_and_draws()
    target = torch.rand(64, 3, generator=torch.Generator().manual_seed(5)).cuda()
    grads, outs = [], []
    for device_losses in (True, False):
        t = _trainer()
        out = t.forward(draws, rays=patch)
        depth, rgb, guide = out["fine_depth"].view(1, 8, 8), out["fine_comp_rgbs"].view(8, 8, 3), target.view(1, 8, 8, 3)
        if device_losses:
            loss = 0.7 * losses.BilateralLaplacianLoss()(depth, guide) + losses.TVLoss()(rgb)
        else:
            loss = 0.7 * ref.laplacian(depth, guide, 0.1) + ref.tv(rgb)
        t.backward(loss)
        grads.append([{k: v.detach().cpu().double() for k, v in t.grads[n].items()} for n in range(2)])
        outs.append((out["fine_depth"].detach(), out["fine_comp_rgbs"].detach(), float(loss.detach())))
    assert bits(outs[0][0]) == bits(outs[1][0]) and bits(outs[0][1]) == bits(outs[1][1])       # the same forward
    assert abs(outs[0][2] - outs[1][2]) <= 1e-5 * abs(outs[1][2])
    got, want = grads
    live = 0
    for n in range(2):
        num = den = 0.0
        for k in STATE_DICT_SPEC:
            err, nrm = float((got[n][k] - want[n][k]).norm()), float(want[n][k].norm())
            num, den = num + err ** 2, den + nrm ** 2
            live += int(nrm > 0)
            assert err <= 2e-3 * nrm + 1e-9, (n, k, err / max(nrm, 1e-30))
            if k in HEAD:
                assert err <= 5e-4 * nrm + 1e-9, (n, k, err / max(nrm, 1e-30))
        assert den == 0.0 or (num / den) ** 0.5 < 2e-3, (n, (num / den) ** 0.5)
        print(f"network {n}: |got - want| / |want| over all tensors = {(num / den) ** 0.5 if den else 0.0:.2e}")
    assert live >= 20                           # the fine network moves (the coarse one only feeds detached weights)


def test_regularize_patch_fused_tv():
    """Trainer.regularize_patch(fused_tv=True) against fused_tv=False from the same state and draws: the returned
    [tv_coarse, tv_fine] agree to 2e-5 relative -- torch's own fp32 sum of 192 terms, n 2^-24."""
    patch, draws = _patch_and_draws()
    tv = {}
    for fused in (False, True):
        t = _trainer()
        tv[fused] = t.regularize_patch(patch, 4, 0.7, draws=draws, fused_tv=fused).cpu().double()
        assert t.step == 1 and tuple(tv[fused].shape) == (2,)
    rel = ((tv[True] - tv[False]).abs() / tv[False].abs()).tolist()
    print(f"tv fused {tv[True].tolist()} torch {tv[False].tolist()} rel {rel}")
    assert all(v > 0 for v in tv[False].tolist()) and max(rel) <= 2e-5
