"""The refinement network's split-fp16 training precision, the checks that need no GPU: argument validation of
nsr_refine_train_forward_p / _backward_p before anything touches a device, the Python layer's option errors, and the numpy
forms of the GPU unit tests (tests/refine_mixed_ref.py) against torch fp64 -- with the project's usual proof that the unit tests'
own case lists can tell a wrong formula from the right one."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nerf_sr_amd import _lib, build as nsr_build, refine
from nerf_sr_amd.refine import make_refine_state_dict

from . import refine_mixed_ref as ref


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


def test_signatures_and_version(lib):
    assert "nsr_refine_train_forward_p" in _lib.SIGNATURES and "nsr_refine_train_backward_p" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nsr_refine_train_forward_p"][1]) == len(_lib.SIGNATURES["nsr_refine_train_forward"][1]) + 1
    assert len(_lib.SIGNATURES["nsr_refine_train_backward_p"][1]) == len(_lib.SIGNATURES["nsr_refine_train_backward"][1]) + 1
    assert lib.nsr_version() == 131
    assert refine.TRAIN_PRECISIONS == {"fp32": _lib.NSR_FP32, "f16x3_mixed": _lib.NSR_F16X3}


def test_entry_points_validate_before_any_launch(lib):
    null, one = c_void_p(0), c_void_p(256)
    big = 1 << 44
    ws, sv = lib.nsr_refine_train_workspace_bytes, lib.nsr_refine_train_saved_bytes
    t106, r34, g72 = (c_void_p * 106)(*[one] * 106), (c_void_p * 34)(*[one] * 34), (c_void_p * 72)(*[one] * 72)
    hole = (c_void_p * 106)(*[one] * 106)
    hole[50] = None
    ghole = (c_void_p * 72)(*[one] * 72)
    ghole[71] = None
    for prec in (_lib.NSR_FP32, _lib.NSR_F16X3):
        fwd = lambda B=2, R=2, H=16, W=16, t=t106, r=r34, x=one, c=one, out=one, w=one, wb=big, s=one, sb=big, mom=0.1, p=prec: \
            lib.nsr_refine_train_forward_p(p, t, r, mom, x, c, B, R, H, W, 0, out, w, wb, s, sb, null)
        assert fwd(H=60) == -2 and fwd(W=20) == -2 and fwd(B=1, R=1, H=8, W=8) == -1
        assert fwd(B=0) == -1 and fwd(R=0) == -1 and fwd(R=256) == -1
        assert fwd(x=null) == -1 and fwd(c=null) == -1 and fwd(out=null) == -1 and fwd(w=null) == -1 and fwd(s=null) == -1
        assert fwd(t=None) == -1 and fwd(mom=1.5) == -1 and fwd(t=hole) == -1
        assert fwd(w=c_void_p(264)) == -1 and fwd(s=c_void_p(264)) == -1        # misaligned
        assert fwd(wb=ws(2, 2, 16, 16, 0) - 1) == -4                             # the same workspace for both precisions
        assert fwd(sb=sv(2, 2, 16, 16) - 1) == -4                                # ... and the same saved state
        bwd = lambda t=t106, go=one, g=g72, w=one, wb=big, s=one, sb=big, p=prec: lib.nsr_refine_train_backward_p(p, t, go, g, w, wb, s, sb, null)
        assert bwd(t=None) == -1 and bwd(go=null) == -1 and bwd(g=None) == -1 and bwd(w=null) == -1 and bwd(s=null) == -1
        assert bwd(g=ghole) == -1 and bwd(t=hole) == -1 and bwd(w=c_void_p(264)) == -1
        assert bwd(sb=16) == -4
        # an unknown precision is refused first, whatever else is wrong
        for bad in (1, 3, 18, -1, 99):                                           # NSR_BF16, NSR_F16, NSR_F16X3_GEMM, ...
            assert fwd(p=bad) == -2 and fwd(p=bad, x=null) == -2 and bwd(p=bad) == -2 and bwd(p=bad, t=None) == -2


def test_option_errors():
    """Checked before a device is touched: an unknown precision raises, "f16x3" (kept free for a pair whose weight gradient is
    16-bit too) still raises, with `fp32` in the message; "f16x3_mixed" is accepted."""
    sd = make_refine_state_dict(7)
    for prec in ("f16x3", "bf16", "f16", "mixed", "", None, 2):
        with pytest.raises(ValueError, match="fp32"):
            refine.RefineTrainer(sd, precision=prec)
        with pytest.raises(ValueError, match="fp32"):
            refine.forward_train({}, {}, torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 3, 16, 16), precision=prec)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    with pytest.raises(ValueError, match="no CPU path"):                         # past the precision check
        refine.forward_train(tsd, tsd, torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 3, 16, 16), precision="f16x3_mixed")
    with pytest.raises(NotImplementedError, match="not_use_ref"):
        refine.RefineTrainer(sd, precision="f16x3_mixed", not_use_ref=True)


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("case", ref.FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_form_is_torch_conv2d(case):
    x, w, b = ref.fwd_inputs(case)
    xin = _nchw(x)
    if case[6]:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    want = F.conv2d(xin, torch.from_numpy(w), torch.from_numpy(b), stride=case[5], padding=1)
    got = ref.fwd_expected(case)
    assert np.array_equal(got, _nhwc(want)) and np.abs(got).max() < 2 ** 24


@pytest.mark.parametrize("case", ref.DGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_input_gradient_form_is_torch_autograd(case):
    H, W, n, cin, cout, up = case
    dz, w = ref.dgrad_inputs(case)
    x = torch.zeros(n, cin, H, W, dtype=torch.float64, requires_grad=True)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    F.conv2d(xin, torch.from_numpy(w), padding=1).backward(_nchw(dz[..., :cout]))
    got = ref.dgrad_expected(case)
    assert np.array_equal(got, _nhwc(x.grad)) and np.abs(got).max() < 2 ** 24
    if not up:
        direct = torch.nn.grad.conv2d_input((n, cin, H, W), torch.from_numpy(w), _nchw(dz[..., :cout]), padding=1)
        assert np.array_equal(got, _nhwc(direct))
    # the operand the kernel multiplies by: a plain 3 x 3 / pad 1 convolution of dZ with B' read as tap-major weights
    b = ref.flip_pack(w, dz.shape[-1]).reshape(cin, 3, 3, dz.shape[-1]).transpose(0, 3, 1, 2) / 64.0      # (cin, np, 3, 3)
    g = ref.conv_fwd(dz, b)
    assert np.array_equal(ref.fold2x2(g) if up else g, got)


def test_wrong_forms_change_the_unit_tests_expectations():
    """Each deliberately wrong form changes the expected result of at least one case of the GPU unit tests' own lists."""
    def moved(cases, expected, wrong):
        hits = []
        for c in cases:
            a, b = expected(c), expected(c, wrong)
            hits.append(a.shape != b.shape or not np.array_equal(a, b))
        return any(hits)
    assert moved(ref.DGRAD_CASES, ref.dgrad_expected, "no_flip")
    assert moved(ref.DGRAD_CASES, ref.dgrad_expected, "swap")                    # cin / cout swapped (the square cases)
    assert moved(ref.DGRAD_CASES, ref.dgrad_expected, "one_pixel")               # fold taking one of the four pixels
    assert moved(ref.DGRAD_CASES, ref.dgrad_expected, "scaled")                  # range scale not removed
    assert moved(ref.FWD_CASES, ref.fwd_expected, "no_upsample")                 # upsample ignored
    for hs, ws, n, c in ref.FOLD_CASES:
        g = ref.ints(np.random.default_rng(5), (n, 2 * hs, 2 * ws, c), 1 << 20)
        assert not np.array_equal(ref.fold2x2(g), ref.fold2x2(g, "one_pixel"))
    w = ref.weights(128, 128)
    assert not np.array_equal(w, w.transpose(1, 0, 2, 3)) and not np.array_equal(w, w[:, :, ::-1, ::-1])
    assert w.min() == -3 and w.max() == 3
    assert ref.range_exponent(8 * ref.DZ_UNIT) == 40 and ref.range_exponent(0.0) == 0
