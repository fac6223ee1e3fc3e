"""CPU-side checks of the differentiable SSIM (include/nsr_metrics.h ``nsr_ssim_backward``, ``metrics.SSIM`` under autograd,
``RefineTrainer(refine_with_ssim=True)``):

* ``nsr_ssim_backward`` is exported, bound, and rejects bad arguments before any launch;
* tests/metrics_ref.py in fp64 under autograd -- the oracle of tests/test_gpu_metrics_grad.py -- reproduces the gradients the
  reference's own ``SSIM`` class gave in fp64 (tests/golden/metrics_grad.npz) to 1e-12 of their largest magnitude;
* ``RefineTrainer``'s option checks count the SSIM loss, before a device is touched.
"""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib, build as nsr_build, refine
from nerf_sr_amd.refine import make_refine_state_dict
from . import metrics_ref as ref
from .metrics_ref import ssim_options

GRAD_TAGS = ["tiny", "gray", "box"]


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


@pytest.fixture(scope="module")
def gg(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics_grad.npz"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


def test_backward_entry_point_is_exported_and_bound(lib):
    assert "nsr_ssim_backward" in _lib.SIGNATURES and hasattr(lib, "nsr_ssim_backward")
    assert len(_lib.SIGNATURES["nsr_ssim_backward"][1]) == 17
    assert lib.nsr_version() == 131                      # additive: the version stays


def test_backward_entry_point_validates_before_any_launch(lib):
    null, one = c_void_p(0), c_void_p(256)
    ok = lambda **kw: {**dict(o=one, t=one, B=1, C=3, H=16, W=16, layout=0, w=one, kh=11, kw=11, gs=one, gm=null, go=one, gt=null), **kw}
    call = lambda a: lib.nsr_ssim_backward(a["o"], a["t"], a["B"], a["C"], a["H"], a["W"], a["layout"], a["w"], a["kh"], a["kw"], 1e-4, 9e-4,
                                           a["gs"], a["gm"], a["go"], a["gt"], null)
    for bad in (dict(layout=2), dict(layout=-1),                                                    # layout
                dict(kh=10), dict(kw=4), dict(kh=0), dict(kw=-3),                                   # even / non-positive windows
                dict(H=5), dict(W=5), dict(H=1, kh=3),                                              # a window too tall / wide: pad >= H or W
                dict(B=-1), dict(C=0), dict(C=-3), dict(H=-16), dict(W=0),                          # sizes
                dict(o=null), dict(t=null), dict(w=null),                                           # null images / window with B > 0
                dict(gs=null, gm=null),                                                             # no upstream gradient
                dict(go=null, gt=null)):                                                            # no gradient requested
        assert call(ok(**bad)) == -1, bad
    assert call(ok(kh=61, kw=61, H=64, W=64)) == -2                 # the staging of a 61 x 61 window exceeds the LDS
    assert call(ok(kh=15, kw=15, H=64, W=64)) == -2 and call(ok(kh=61, kw=61, H=8, W=8)) == -1      # ... argument errors come first
    assert call(ok(B=0)) == 0                                       # empty batch: no-op ...
    assert call(ok(B=0, o=null, t=null, w=null, gs=null, go=null)) == 0        # ... whatever the pointers
    assert call(ok(B=0, layout=3)) == -1 and call(ok(B=0, kh=4)) == -1         # but its options are still checked


@pytest.mark.parametrize("tag", GRAD_TAGS)
def test_restatement_under_autograd_matches_the_reference_class(g, gg, tag):
    assert list(gg["tags"]) == GRAD_TAGS
    x = torch.from_numpy(g[f"x_{tag}"]).double().requires_grad_(True)
    y = torch.from_numpy(g[f"y_{tag}"]).double().requires_grad_(True)
    v = torch.from_numpy(gg[f"v_{tag}"])
    assert v.dtype == torch.float32 and tuple(v.shape) == (x.shape[0],)
    (ref.ssim(x, y, **ssim_options(g, tag)) * v.double()).sum().backward()
    for got, name in ((x.grad, "gx"), (y.grad, "gy")):
        want = torch.from_numpy(gg[f"{name}64_{tag}"])
        assert want.dtype == torch.float64 and tuple(want.shape) == tuple(got.shape)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (tag, name)
        # the recorded fp32 gradients of the class are what the fixture says they are: its own fp32 error
        gap = float((torch.from_numpy(gg[f"{name}32_{tag}"]).double() - want).abs().max() / want.abs().max())
        assert gap <= float(gg[f"gap_{tag}"]) <= 1e-4


def test_trainer_counts_the_ssim_loss_in_its_option_checks():
    """Checked before a device is touched: with SSIM as the only loss the constructor gets past "no loss selected" (and stops
    at the incomplete state_dict, the first check after the options); the unsupported losses still raise."""
    sd = make_refine_state_dict(7)
    short = {k: v for k, v in sd.items() if k != "D.conv9.bias"}
    with pytest.raises(KeyError):
        refine.RefineTrainer(short, refine_with_l1=False, refine_with_mse=False, refine_with_ssim=True, lambda_refine_ssim=0.5)
    with pytest.raises(ValueError, match="no loss"):
        refine.RefineTrainer(short, refine_with_l1=False, refine_with_mse=False)
    with pytest.raises(ValueError, match="no loss"):
        refine.RefineTrainer(short, refine_with_l1=False, refine_with_mse=False, refine_with_ssim=False, lambda_refine_ssim=2.0)
    with pytest.raises(NotImplementedError, match="forward_train"):
        refine.RefineTrainer(sd, refine_with_ssim=True, refine_with_vgg=True)
    with pytest.raises(TypeError):
        refine.RefineTrainer(sd, 5e-4, 0.9, True, False, 1.0, 10.0, "cuda", True)      # keyword-only, like the other additions
