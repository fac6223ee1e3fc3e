"""CPU-side checks of the image-space regularisers (include/nsr_losses.h, nerf_sr_amd/losses.py): the plain-torch restatement
tests/losses_ref.py against the reference's own classes (tests/golden/losses.npz), the new entry points' argument checks
(nothing is launched: validation comes first), and the Python classes' refusals."""
import inspect
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib, build as nsr_build
from . import losses_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["nsr_loss_workspace_bytes", "nsr_tv_loss", "nsr_tv_loss_backward", "nsr_gradient_loss", "nsr_gradient_loss_backward",
               "nsr_laplacian_loss", "nsr_laplacian_loss_backward"]
INVALID, WORKSPACE = -1, -4
RTOL = 1e-12        # the same arithmetic in the same precision: only the order of a few additions may differ


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "losses.npz"))


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(np.abs(want).max()) if want.size else 0.0
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= RTOL * scale, (what, err, scale)


def _check(g, prefix, fn, names, wrt):
    """fn over the fixture's fp32 inputs cast to double reproduces loss64 and the gradients of upstream * loss."""
    inputs = [torch.from_numpy(g[f"{prefix}_{n}"]).double().requires_grad_(n in wrt) for n in names]
    loss = fn(*inputs)
    _close(loss.detach().numpy(), g[f"{prefix}_loss64"], f"{prefix} loss")
    grads = torch.autograd.grad(float(g["upstream"]) * loss, [t for t in inputs if t.requires_grad], allow_unused=True)
    for n, gr in zip(wrt, grads):
        want = g[f"{prefix}_g{n}64"]
        _close(np.zeros_like(want) if gr is None else gr.numpy(), want, f"{prefix} d/d{n}")
        # the stated exact zeros of the fixture are exact zeros of the restatement too (sign(0) = 0)
        if gr is not None:
            assert np.array_equal(gr.numpy() == 0, want == 0), f"{prefix} d/d{n}: zeros differ"


def test_fixture_has_every_case(g):
    assert list(g["tv_tags"]) == ["2x2x3", "3x5x1", "8x8x3", "33x35x3", "const"]
    assert list(g["gradient_tags"]) == ["3d", "2x3x2x2", "1x1x1x1", "1x3x33x34", "half", "quant"]
    assert list(g["laplacian_tags"]) == ["1x3x3", "2x3x5", "3x4x4", "1x33x35", "ramp", "quant"]
    assert set(g["laplacian_tags"]) <= set(g["bilateral_tags"]) and len(g["bilateral_tags"]) == 9
    assert g["gradient_3d_a"].shape == (3, 1, 4) and g["bilateral_3x4x4_c1_guide"].shape == (3, 4, 4, 1)
    assert sorted({float(g[f"bilateral_{t}_gamma"]) for t in g["bilateral_tags"]}) == [0.1, 1.0]
    # the cases that exist for sign(0) = 0 do have exact zeros: everywhere, or on part of the image
    assert float(g["tv_const_loss64"]) == 0 and not g["tv_const_gx64"].any()
    assert float(g["laplacian_ramp_loss64"]) == 0 and not g["laplacian_ramp_gd64"].any() and not g["bilateral_ramp_gd64"].any()
    for key in ("gradient_half_ga64", "gradient_quant_ga64", "laplacian_quant_gd64"):
        zeros = int((g[key] == 0).sum())
        assert 0 < zeros < g[key].size, (key, zeros)


def test_restatement_reproduces_the_reference_classes(g):
    for tag in g["tv_tags"]:
        _check(g, f"tv_{tag}", ref.tv, ["x"], ["x"])
    for tag in g["gradient_tags"]:
        _check(g, f"gradient_{tag}", ref.gradient, ["a", "b"], ["a", "b"])
    for tag in g["laplacian_tags"]:
        _check(g, f"laplacian_{tag}", ref.laplacian, ["d"], ["d"])
    for tag in g["bilateral_tags"]:
        gamma = float(g[f"bilateral_{tag}_gamma"])
        _check(g, f"bilateral_{tag}", lambda d, guide: ref.laplacian(d, guide, gamma), ["d", "guide"], ["d"])


def test_new_symbols_declared_exported_and_bound(lib):
    text = open(os.path.join(REPO, "include", "nsr_losses.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(nsr_[a-z_0-9]+)\s*\(", text))) == sorted(NEW_SYMBOLS)
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert (_lib.NSR_LOSS_TV, _lib.NSR_LOSS_GRADIENT, _lib.NSR_LOSS_LAPLACIAN) == (0, 1, 2)
    for name, value in (("NSR_LOSS_TV", 0), ("NSR_LOSS_GRADIENT", 1), ("NSR_LOSS_LAPLACIAN", 2)):
        assert re.search(rf"#define {name} {value}\b", text), name


def test_workspace_sizes(lib):
    ws = lib.nsr_loss_workspace_bytes
    TV, GR, LAP = _lib.NSR_LOSS_TV, _lib.NSR_LOSS_GRADIENT, _lib.NSR_LOSS_LAPLACIAN
    # one double per (plane, 32 x 32 tile, partial sum): two sums for TV and gradient, four for the Laplacian
    assert ws(TV, 1, 3, 8, 8) == 3 * 2 * 8 and ws(TV, 1, 3, 33, 65) == 3 * 2 * 3 * 2 * 8
    assert ws(GR, 32, 3, 64, 64) == 32 * 3 * 4 * 2 * 8 and ws(GR, 1, 1, 1, 1) == 16
    assert ws(LAP, 16, 3, 64, 64) == 16 * 4 * 4 * 8 == ws(LAP, 16, 1, 64, 64)
    # grows with the tile count
    assert ws(GR, 1, 1, 32, 32) < ws(GR, 1, 1, 32, 33) < ws(GR, 1, 1, 33, 33) < ws(GR, 2, 1, 33, 33)
    # 0 for an unknown kind and for sizes the entry points refuse
    assert ws(3, 1, 3, 8, 8) == 0 and ws(-1, 1, 3, 8, 8) == 0
    for bad in ((TV, 0, 3, 8, 8), (TV, 1, 0, 8, 8), (TV, 1, 3, 1, 8), (TV, 1, 3, 8, 1), (GR, 0, 3, 8, 8), (GR, 1, 3, 0, 8), (GR, 1, 3, 8, -1),
                (GR, 1, 0, 8, 8), (LAP, 0, 1, 8, 8), (LAP, 1, 1, 2, 8), (LAP, 1, 1, 8, 2)):
        assert ws(*bad) == 0, bad


def test_entry_points_validate_before_any_launch(lib):
    null, one = c_void_p(0), c_void_p(256)          # non-null, never dereferenced: validation happens first
    big = 1 << 30
    # ---- TV
    assert lib.nsr_tv_loss(null, 8, 8, 3, one, one, big, null) == INVALID
    assert lib.nsr_tv_loss(one, 8, 8, 3, null, one, big, null) == INVALID
    assert lib.nsr_tv_loss(one, 8, 8, 3, one, null, big, null) == INVALID
    for H, W, C in ((1, 8, 3), (8, 1, 3), (8, 8, 0), (0, 8, 3), (8, -2, 3)):
        assert lib.nsr_tv_loss(one, H, W, C, one, one, big, null) == INVALID, (H, W, C)
        assert lib.nsr_tv_loss_backward(one, H, W, C, one, one, null) == INVALID, (H, W, C)
    assert lib.nsr_tv_loss(one, 33, 35, 3, one, one, lib.nsr_loss_workspace_bytes(0, 1, 3, 33, 35) - 1, null) == WORKSPACE
    for args in ((null, one, one), (one, null, one), (one, one, null)):
        x, up, grad = args
        assert lib.nsr_tv_loss_backward(x, 8, 8, 3, up, grad, null) == INVALID
    # ---- gradient
    for a, b, loss, ws in ((null, one, one, one), (one, null, one, one), (one, one, null, one), (one, one, one, null)):
        assert lib.nsr_gradient_loss(a, b, 2, 3, 8, 8, loss, ws, big, null) == INVALID
    for B, C, H, W in ((0, 3, 8, 8), (2, 0, 8, 8), (2, 3, 0, 8), (2, 3, 8, 0), (-1, 3, 8, 8)):
        assert lib.nsr_gradient_loss(one, one, B, C, H, W, one, one, big, null) == INVALID, (B, C, H, W)
        assert lib.nsr_gradient_loss_backward(one, one, B, C, H, W, one, one, one, null) == INVALID, (B, C, H, W)
    assert lib.nsr_gradient_loss(one, one, 2, 3, 8, 8, one, one, lib.nsr_loss_workspace_bytes(1, 2, 3, 8, 8) - 1, null) == WORKSPACE
    assert lib.nsr_gradient_loss_backward(one, one, 2, 3, 8, 8, one, null, null, null) == INVALID      # both gradients null
    assert lib.nsr_gradient_loss_backward(null, one, 2, 3, 8, 8, one, one, one, null) == INVALID
    assert lib.nsr_gradient_loss_backward(one, null, 2, 3, 8, 8, one, one, null, null) == INVALID
    assert lib.nsr_gradient_loss_backward(one, one, 2, 3, 8, 8, null, one, one, null) == INVALID       # no upstream scalar
    # ---- Laplacian, plain (guide null) and bilateral
    for guide in (null, one):
        assert lib.nsr_laplacian_loss(null, guide, 2, 8, 8, 3, 0.1, one, one, big, null) == INVALID
        assert lib.nsr_laplacian_loss(one, guide, 2, 8, 8, 3, 0.1, null, one, big, null) == INVALID
        assert lib.nsr_laplacian_loss(one, guide, 2, 8, 8, 3, 0.1, one, null, big, null) == INVALID
        for N, H, W, gamma in ((0, 8, 8, 0.1), (2, 2, 8, 0.1), (2, 8, 2, 0.1), (2, 8, 8, 0.0), (2, 8, 8, -1.0), (2, 8, 8, float("nan"))):
            assert lib.nsr_laplacian_loss(one, guide, N, H, W, 3, gamma, one, one, big, null) == INVALID, (N, H, W, gamma)
            assert lib.nsr_laplacian_loss_backward(one, guide, N, H, W, 3, gamma, one, one, null) == INVALID, (N, H, W, gamma)
        assert lib.nsr_laplacian_loss(one, guide, 2, 33, 8, 3, 0.1, one, one, lib.nsr_loss_workspace_bytes(2, 2, 3, 33, 8) - 1, null) == WORKSPACE
        assert lib.nsr_laplacian_loss_backward(null, guide, 2, 8, 8, 3, 0.1, one, one, null) == INVALID
        assert lib.nsr_laplacian_loss_backward(one, guide, 2, 8, 8, 3, 0.1, null, one, null) == INVALID
        assert lib.nsr_laplacian_loss_backward(one, guide, 2, 8, 8, 3, 0.1, one, null, null) == INVALID
    assert lib.nsr_laplacian_loss(one, one, 2, 8, 8, 0, 0.1, one, one, big, null) == INVALID          # a guide without channels
    assert lib.nsr_laplacian_loss_backward(one, one, 2, 8, 8, 0, 0.1, one, one, null) == INVALID


def test_classes_refuse_before_touching_the_device():
    from nerf_sr_amd import losses
    cpu = torch.zeros(8, 8, 3)
    with pytest.raises(ValueError, match="no CPU path"):
        losses.TVLoss()(cpu)
    with pytest.raises(ValueError, match="no CPU path"):
        losses.GradientLoss(None)(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        losses.LaplacianLoss()(torch.zeros(1, 8, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        losses.BilateralLaplacianLoss()(torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError, match="no gradient"):
        losses.BilateralLaplacianLoss()(torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 3, requires_grad=True))
    # gamma: the argument, else opt.bilateral_gamma, else the reference's default
    import types
    assert losses.BilateralLaplacianLoss().gamma == 0.1
    assert losses.BilateralLaplacianLoss(types.SimpleNamespace(bilateral_gamma=0.5)).gamma == 0.5
    assert losses.BilateralLaplacianLoss(types.SimpleNamespace(bilateral_gamma=0.5), gamma=2.0).gamma == 2.0
    with pytest.raises(ValueError, match="gamma"):
        losses.BilateralLaplacianLoss(gamma=0.0)


def test_regularize_patch_keeps_its_default():
    from nerf_sr_amd.train import Trainer
    p = inspect.signature(Trainer.regularize_patch).parameters
    assert "fused_tv" in p and p["fused_tv"].default is False
