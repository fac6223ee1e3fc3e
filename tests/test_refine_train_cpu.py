"""Training of the refinement network, the checks that need no GPU: the plain-torch restatement against the reference's
own recorded train-mode run (tests/golden/refine_train.npz), argument validation of the four entry points before any
launch, and RefineTrainer's option errors."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib, build as nsr_build, refine
from nerf_sr_amd.refine import RUNNING_KEYS, TRAIN_PARAM_KEYS, make_refine_state_dict

from . import refine_train_ref as ref

CASES = ("A", "B", "C")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "refine_train.npz"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


def test_key_lists_match_the_reference(fx):
    assert list(fx["param_keys"]) == TRAIN_PARAM_KEYS and list(fx["running_keys"]) == RUNNING_KEYS
    assert len(ref.LIVE) == 55 and set(ref.CANCELLED) < set(TRAIN_PARAM_KEYS)


def test_fixture_cases_are_clean(fx):
    """The generator's assert, re-read: the reference's fp32 gradients are within 2e-5 of its fp64 ones on every
    non-cancelled tensor, and the cancelled biases' true gradient is zero."""
    for tag in CASES:
        assert float(fx[f"{tag}_grad_gap"].max()) <= 2e-5 and float(fx[f"{tag}_cancelled_max64"]) <= 1e-12


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_the_reference_in_fp64(fx, tag):
    """y, running statistics, gradient norms and sampled gradient entries to 1e-10 relative."""
    l1, mse = fx[f"{tag}_lambdas"]
    y, running, loss, g = ref.grads_fp64(make_refine_state_dict(int(fx["weights_seed"])), fx[f"{tag}_x"], fx[f"{tag}_c"], fx[f"{tag}_gt"], l1, mse)
    tol = 1e-10
    assert tuple(y.shape) == tuple(fx[f"{tag}_y64"].shape)
    assert float((y - torch.from_numpy(fx[f"{tag}_y64"])).abs().max()) <= tol
    assert abs(float(loss) - float(fx[f"{tag}_loss64"])) <= tol * abs(float(fx[f"{tag}_loss64"]))
    run = torch.cat([running[k] for k in RUNNING_KEYS])
    want = torch.from_numpy(fx[f"{tag}_running64"])
    assert float(((run - want).abs() / want.abs().clamp_min(1e-3)).max()) <= tol
    for i, k in enumerate(TRAIN_PARAM_KEYS):
        norm = float(fx[f"{tag}_grad_norm64"][i])
        if k in ref.CANCELLED:
            assert float(g[k].abs().max()) <= 1e-12 and norm <= 1e-12, k
            continue
        assert abs(float(g[k].norm()) - norm) <= tol * norm, k
        got = g[k].flatten()[torch.from_numpy(fx[f"{tag}_grad_idx"][i])]
        assert float((got - torch.from_numpy(fx[f"{tag}_grad_entries64"][i])).abs().max()) <= tol * norm, k


def test_train_entry_points_validate_before_any_launch(lib):
    """include/nsr_refine.h, training: sizes and argument checks that need no GPU."""
    null, one = c_void_p(0), c_void_p(256)
    big = 1 << 44
    ws, sv = lib.nsr_refine_train_workspace_bytes, lib.nsr_refine_train_saved_bytes
    # sizes: 0 on shapes the pair does not take
    assert ws(2, 8, 64, 64, 0) > 0 and sv(2, 8, 64, 64) > 0
    assert ws(1, 8, 64, 60, 0) == 0 and sv(1, 8, 64, 60) == 0            # H, W multiples of 8
    assert ws(1, 1, 8, 8, 0) == 0 and sv(1, 1, 8, 8) == 0                # B H W / 64 = 1: one value per channel
    assert ws(0, 8, 64, 64, 0) == 0 and sv(2, 0, 64, 64) == 0 and sv(2, 8, -8, 64) == 0 and sv(2, 256, 64, 64) == 0
    # the saved state: (787 R + 2398) H W floats + 232 H W bytes per patch set, plus header and per-layer statistics
    per_set = (787 * 8 + 2398) * 4096 * 4 + 232 * 4096
    assert 32 * per_set <= sv(32, 8, 64, 64) <= 32 * per_set + (1 << 20)
    # img_chunk bounds the workspace; the saved state does not depend on it
    assert ws(32, 8, 64, 64, 1) < ws(32, 8, 64, 64, 8) < ws(32, 8, 64, 64, 64) and ws(2, 2, 16, 16, 4) == ws(2, 2, 16, 16, 100)
    t106 = (c_void_p * 106)(*[one] * 106)
    r34 = (c_void_p * 34)(*[one] * 34)
    g72 = (c_void_p * 72)(*[one] * 72)
    fwd = lambda B=2, R=2, H=16, W=16, t=t106, r=r34, x=one, c=one, out=one, w=one, wb=big, s=one, sb=big, mom=0.1: \
        lib.nsr_refine_train_forward(t, r, mom, x, c, B, R, H, W, 0, out, w, wb, s, sb, null)
    assert fwd(H=60) == -2 and fwd(W=20) == -2
    assert fwd(B=1, R=1, H=8, W=8) == -1                                # one value per channel
    assert fwd(B=0) == -1 and fwd(R=0) == -1 and fwd(R=256) == -1
    assert fwd(x=null) == -1 and fwd(c=null) == -1 and fwd(out=null) == -1 and fwd(w=null) == -1 and fwd(s=null) == -1
    assert fwd(t=None) == -1 and fwd(mom=1.5) == -1
    hole = (c_void_p * 106)(*[one] * 106)
    hole[50] = None
    assert fwd(t=hole) == -1
    rhole = (c_void_p * 34)(*[one] * 34)
    rhole[33] = None
    assert fwd(r=rhole) == -1
    assert fwd(w=c_void_p(264)) == -1                                   # misaligned workspace
    assert fwd(wb=ws(2, 2, 16, 16, 0) - 1) == -4                        # short workspace
    assert fwd(sb=sv(2, 2, 16, 16) - 1) == -4                           # short saved state
    bwd = lambda t=t106, go=one, g=g72, w=one, wb=big, s=one, sb=big: lib.nsr_refine_train_backward(t, go, g, w, wb, s, sb, null)
    assert bwd(t=None) == -1 and bwd(go=null) == -1 and bwd(g=None) == -1 and bwd(w=null) == -1 and bwd(s=null) == -1
    ghole = (c_void_p * 72)(*[one] * 72)
    ghole[71] = None
    assert bwd(g=ghole) == -1 and bwd(t=hole) == -1
    assert bwd(sb=16) == -4                                             # shorter than the header itself


def test_trainer_option_errors():
    """Checked before a device is touched."""
    sd = make_refine_state_dict(7)
    for opt in ("refine_with_vgg", "refine_with_grad", "refine_as_gan"):
        with pytest.raises(NotImplementedError, match="forward_train"):
            refine.RefineTrainer(sd, **{opt: True})
    with pytest.raises(NotImplementedError, match="not_use_ref"):
        refine.RefineTrainer(sd, not_use_ref=True)
    for prec in ("f16x3", "bf16", "f16"):
        with pytest.raises(ValueError, match="fp32"):
            refine.RefineTrainer(sd, precision=prec)
    with pytest.raises(ValueError, match="no loss"):
        refine.RefineTrainer(sd, refine_with_l1=False, refine_with_mse=False)
    with pytest.raises(KeyError):
        refine.RefineTrainer({k: v for k, v in sd.items() if k != "D.conv9.bias"})


def test_forward_train_rejects_cpu_tensors():
    sd = {k: torch.from_numpy(v) for k, v in make_refine_state_dict(7).items()}
    with pytest.raises(ValueError, match="no CPU path"):
        refine.forward_train(sd, sd, torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 3, 16, 16))
