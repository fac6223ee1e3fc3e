"""The refinement network's implicit split-fp16 weight gradient, the checks that need no GPU: the numpy form of the GPU unit
tests (tests/refine_wgrad_ref.py) against torch fp64, the project's usual proof that the unit tests' own case list can tell a
wrong formula from the right one, the Python layer's option errors, and the argument validation of
nsr_refine_train_backward_w before anything touches a device."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nerf_sr_amd import _lib, build as nsr_build, refine
from nerf_sr_amd.refine import make_refine_state_dict

from . import refine_wgrad_ref as ref


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_form_is_torch_autograd(case):
    """autograd through F.interpolate / F.conv2d in fp64, and torch.nn.grad.conv2d_weight where there is no upsample"""
    dz, x, _ = ref.inputs(case)
    got = ref.wgrad(dz, x, case.stride, case.up, case.cout)
    assert np.abs(got).max() < 2 ** 24 and np.abs(ref.expected(case)).max() < 2 ** 24
    w = torch.zeros(case.cout, case.cin, 3, 3, dtype=torch.float64, requires_grad=True)
    xin = _nchw(x)
    if case.up:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    g = _nchw(dz[..., :case.cout])
    F.conv2d(xin, w, stride=case.stride, padding=1).backward(g)
    assert np.array_equal(got, w.grad.numpy())
    direct = torch.nn.grad.conv2d_weight(xin, (case.cout, case.cin, 3, 3), g, stride=case.stride, padding=1)
    assert np.array_equal(got, direct.numpy())


def test_exact_inputs_are_exact():
    """what makes the GPU comparison bit for bit: every operand splits into fp16 halves without a remainder, the lo x lo term the
    kernel leaves out is zero in every case, and the wide cases do have a non-zero lo half in the operand they name"""
    for c in ref.CASES:
        dz, x, _ = ref.inputs(c)
        s = 2.0 ** ref.range_exponent(np.abs(dz).max() * ref.DZ_UNIT) * ref.DZ_UNIT
        zh, zl = ref.split16(dz * s)
        xh, xl = ref.split16(x)
        assert np.array_equal(zh + zl, dz * s) and np.array_equal(xh + xl, x)
        assert 2.0 ** 13 <= np.abs(dz * s).max() < 2.0 ** 14
        assert not (zl.any() and xl.any())
        assert zl.any() == (c.wide == "dz") and xl.any() == (c.wide == "x")


@pytest.mark.parametrize("wrong", ref.WRONG_FORMS)
def test_wrong_forms_change_the_unit_tests_expectations(wrong):
    """Each deliberately wrong form changes the expected result of at least one case of the GPU unit tests' own list."""
    assert any(not np.array_equal(ref.expected(c), ref.expected(c, wrong)) for c in ref.CASES)


def test_case_list_covers_what_it_claims():
    cs = ref.CASES
    assert {(c.cin, c.cout) for c in cs} == {(128, 128), (256, 128), (128, 3)}
    assert {c.n for c in cs} == {1, 3} and {c.stride for c in cs} == {1, 2} and {c.up for c in cs} == {0, 1} and {c.acc for c in cs} == {0, 1}
    assert min(c.H * c.W for c in cs) == 6 and max(c.H * c.W for c in cs) == 16 * 24
    K = lambda c: c.n * ref.out_extent(c)[0] * ref.out_extent(c)[1]
    n_slices = lambda c: -(-K(c) // ref.used_slice_len(c))
    assert any(K(c) % 32 for c in cs)                                            # a pixel count that is no multiple of the K tile
    assert any(c.slice_len and n_slices(c) >= 3 for c in cs)                     # >= 3 slices by the override
    assert any(c.slice_len and K(c) % c.slice_len for c in cs)                   # one ending inside a slice
    assert any(not c.slice_len and n_slices(c) >= 3 for c in cs)                 # ... and several at the product's own length
    assert any(c.part_slices and n_slices(c) > c.part_slices for c in cs)        # more than one pass over the partial buffer
    assert {c.wide for c in cs} == {"", "dz", "x"}
    # the slice length is a function of the shape alone, a multiple of the K tile, 8 .. 128 K tiles long
    for cin, cout, k in ((128, 128, 6), (128, 128, 1 << 20), (1536, 512, 8192), (128, 3, 131072), (512, 512, 65536)):
        n = ref.slice_len(cin, cout, k)
        assert n % 32 == 0 and 256 <= n <= 4096


def test_signature_and_names(lib):
    assert "nsr_refine_train_backward_w" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nsr_refine_train_backward_w"][1]) == len(_lib.SIGNATURES["nsr_refine_train_backward_p"][1]) + 1
    assert hasattr(lib, "nsr_refine_train_backward_w")
    assert lib.nsr_version() == 131
    assert refine.TRAIN_PRECISIONS == {"fp32": _lib.NSR_FP32, "f16x3_mixed": _lib.NSR_F16X3}
    assert refine.WEIGHT_GRADS == {"fp32": _lib.NSR_FP32, "f16x3": _lib.NSR_F16X3}


def test_entry_point_validates_before_any_launch(lib):
    null, one = c_void_p(0), c_void_p(256)
    big = 1 << 44
    t106, g72 = (c_void_p * 106)(*[one] * 106), (c_void_p * 72)(*[one] * 72)
    hole = (c_void_p * 106)(*[one] * 106)
    hole[50] = None
    ghole = (c_void_p * 72)(*[one] * 72)
    ghole[71] = None
    for prec in (_lib.NSR_FP32, _lib.NSR_F16X3):
        for wg in (_lib.NSR_FP32, _lib.NSR_F16X3):
            bwd = lambda t=t106, go=one, g=g72, w=one, wb=big, s=one, sb=big, p=prec, q=wg: \
                lib.nsr_refine_train_backward_w(p, q, t, go, g, w, wb, s, sb, null)
            # the same argument validation as nsr_refine_train_backward_p
            assert bwd(t=None) == -1 and bwd(go=null) == -1 and bwd(g=None) == -1 and bwd(w=null) == -1 and bwd(s=null) == -1
            assert bwd(g=ghole) == -1 and bwd(t=hole) == -1 and bwd(w=c_void_p(264)) == -1 and bwd(s=c_void_p(264)) == -1
            assert bwd(sb=16) == -4
            for bad in (1, 3, 18, -1, 99):
                assert bwd(p=bad) == -2 and bwd(p=bad, t=None) == -2
        # an unknown weight_grad is refused first, whatever else is wrong -- the precision included
        for bad in (1, 3, 18, 19, -1, 99):                                       # NSR_BF16, NSR_F16, NSR_F16X3_GEMM, ...
            for p in (prec, 99):
                assert lib.nsr_refine_train_backward_w(p, bad, t106, one, g72, one, big, one, big, null) == -2
                assert lib.nsr_refine_train_backward_w(p, bad, None, null, None, null, 0, null, 0, null) == -2


def test_option_errors():
    """Checked before a device is touched: an unknown weight_grad raises; "fp32" and "f16x3" pass the check, with either
    precision; the precision's own names are what they were."""
    sd = make_refine_state_dict(7)
    for wg in ("bf16", "f16", "", None, 2, "f16x3_mixed"):
        with pytest.raises(ValueError, match="weight_grad"):
            refine.RefineTrainer(sd, weight_grad=wg)
        with pytest.raises(ValueError, match="weight_grad"):
            refine.RefineTrainer(sd, precision="f16x3_mixed", weight_grad=wg)
        with pytest.raises(ValueError, match="weight_grad"):
            refine.forward_train({}, {}, torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 3, 16, 16), weight_grad=wg)
    with pytest.raises(ValueError, match="fp32"):                                # `precision` keeps refusing the short name
        refine.forward_train({}, {}, torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 3, 16, 16), precision="f16x3", weight_grad="f16x3")
    with pytest.raises(TypeError):                                               # keyword-only
        refine.forward_train({}, {}, torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 3, 16, 16), 0.1, None, "fp32", "f16x3")
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    for prec in ("fp32", "f16x3_mixed"):
        for wg in ("fp32", "f16x3"):
            with pytest.raises(ValueError, match="no CPU path"):                 # past both option checks
                refine.forward_train(tsd, tsd, torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 3, 16, 16), precision=prec, weight_grad=wg)
    with pytest.raises(NotImplementedError, match="not_use_ref"):
        refine.RefineTrainer(sd, precision="f16x3_mixed", weight_grad="f16x3", not_use_ref=True)
