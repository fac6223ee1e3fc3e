"""Early ray termination (include/nsr.h, "early ray termination"), everything that needs no GPU:

1. the two entry points are declared, exported and bound, and make their argument checks before anything touches the device
   (null device pointers, no GPU);
2. the derivation of the bound, pinned independently of any kernel: the rule (tests/early_stop_ref.py) applied to the
   oracle's own render, full and truncated arrays composited by the oracle, the three bounds asserted;
3. the Python mirror: ``default_options(early_stop=...)`` and the ValueErrors raised before a device is touched.

Parts 1 and 3 need the feature.  Part 2 depends on the helper and the oracle alone -- that is what makes it independent of
any kernel -- so it pins the bound's derivation whether or not the library has the option."""
import os
import re
from ctypes import c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib, cameras
from nerf_sr_amd.weights import make_state_dict
from oracle import nerf_oracle as oc
from tests import early_stop_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nsr_render_rays_composited_ert", "nsr_forward_rays_ert")
OK, INVALID, UNSUPPORTED = 0, -1, -2
F32, BF16, F16X3, F16 = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ 1. header and ABI
def test_entry_points_are_declared_exported_and_bound():
    with open(os.path.join(REPO, "include", "nsr.h")) as f:
        header = f.read()
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name in doc
    assert lib.nsr_version() == 131
    for word in ("-ln(eps)", "eps + 2e-6", "NSR_SIGMA_SOFTPLUS", "NSR_OPT_COLOR_NONE", "caller's responsibility"):
        assert word in header, word


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    null, one = c_void_p(0), c_void_p(16)

    def comp(eps, prec=F16X3, n=128, flags=0, R=10):
        return lib.nsr_render_rays_composited_ert(null, prec, null, 8, null, R, n, flags, eps, null, null, null, null, null, null)

    def fwd(eps, prec=F16X3, nc=64, ni=64, flags=0):
        return lib.nsr_forward_rays_ert(null, null, prec, null, 8, 10, nc, ni, flags, 0, None, null, 0, null, None, eps, null)

    for call in (comp, fwd):
        for bad in (float("nan"), -1e-3, 1.0, 2.0, float("inf"), -float("inf")):
            assert call(bad) == INVALID, (call.__name__, bad)
            assert call(bad, prec=F32) == INVALID            # the threshold is checked first
        for prec in (F32, BF16, F16):
            assert call(1e-4, prec=prec) == UNSUPPORTED, (call.__name__, prec)
        assert call(1e-4, flags=2) == UNSUPPORTED and call(1e-4, flags=3) == UNSUPPORTED     # NSR_SIGMA_SOFTPLUS
        assert call(1e-4) == INVALID                         # only now the null pointers are looked at
    for n in (32, 96, 192, 256):
        assert comp(1e-4, n=n) == UNSUPPORTED, n
    assert fwd(1e-4, nc=64, ni=32) == UNSUPPORTED            # the LAST pass has 96 samples
    assert fwd(1e-4, nc=96, ni=0) == UNSUPPORTED             # ... the coarse pass, when it is the last one
    assert fwd(1e-4, nc=32, ni=32) == INVALID                # 64 samples in the last pass: accepted, then the null pointers
    assert fwd(1e-4, nc=64, ni=0) == INVALID
    # 0 = off: the parents' own checks and results
    assert comp(0.0, prec=F32, n=64, R=0) == INVALID                                               # (null packed blob)
    assert lib.nsr_render_rays_composited_ert(one, F16X3, null, 8, null, 0, 96, 0, 0.0, null, null, null, null, null, null) == UNSUPPORTED
    assert lib.nsr_render_rays_composited_ert(one, F32, null, 8, null, 0, 64, 0, 0.0, null, null, null, null, null, null) == OK
    assert lib.nsr_render_rays_composited_ert(one, F16X3, null, 8, null, 0, 64, 0, 1e-4, null, null, null, null, null, null) == OK   # empty batch
    assert lib.nsr_render_rays_composited_ert(one, F16X3, null, 8, null, 0, 64, 4, 1e-4, null, null, null, null, null, null) == INVALID  # unknown flag bit


# ------------------------------------------------------------------------------------------------ 2. the rule and its bound
def test_the_rule_on_hand_made_rays():
    """tau per window 5 for three rays and 2.5 for the fourth: with -ln(1e-3) = 6.9 the group stops when the SLOWEST ray
    passes it (after window 2: 7.5), a lone ray of the first kind after window 1."""
    N = 128
    z = np.tile(np.arange(N, dtype=np.float32) * np.float32(5 / 2048), (4, 1))
    sigma = np.full((4, N), 64, np.float32)
    sigma[3] = 32
    rgb = np.full((4, N, 3), 0.5, np.float32)
    t = ref.truncate(rgb, sigma, z, 1e-3)
    assert t.n_cut == 1 and list(t.last_window) == [2] and not t.marginal and t.n_cut_lo == t.n_cut_hi == 1
    assert (t.sigma[:, 96:] == 0).all() and (t.sigma[:, :96] == sigma[:, :96]).all() and (t.rgb[:, 96:] == 0).all()
    assert t.n_cut_single_ray == 3 * 2 + 1
    t = ref.truncate(rgb[:3], sigma[:3], z[:3], 1e-3)             # a ragged group: the missing ray counts as terminated
    assert t.n_cut == 2 and list(t.last_window) == [1]
    sigma[0, 5] = np.nan                                           # a NaN optical depth never terminates
    assert ref.truncate(rgb, sigma, z, 1e-3).n_cut == 0
    sigma[0, 5] = 64
    sigma[:, :32] = -7                                             # an empty first window contributes 0
    assert list(ref.truncate(rgb, sigma, z, 1e-3).last_window) == [3]
    # a comparison within 1e-4 of the threshold is reported, and the count is bracketed
    thr = float(ref.threshold(1e-3))
    sigma = np.full((4, N), thr / 32 * 2048 / 5 * (1 + 2e-5), np.float32)
    t = ref.truncate(rgb, sigma, z, 1e-3)
    assert (0, 0) in t.marginal and t.n_cut_lo == 2 and t.n_cut_hi == 3 and t.n_cut in (2, 3)


@pytest.fixture(scope="module")
def oracle_render():
    """512 consecutive rays of BASELINE config #2 (504 x 378 <- 252 x 189, NDC) from the middle of the frame, rendered by the
    oracle: the 64-sample coarse pass and the 128-sample fine pass of the `sharp` field, of a dense one (sigma.bias = 1e3:
    transmittance exactly 0 after one window) and of a `thick` one (sigma.bias = 16: tau grows by ~8 per coarse window, so groups
    stop at different windows with a residual transmittance near eps -- where the bound has something to hold)."""
    rays = oc.subpixel_ray_grid(torch.from_numpy(cameras.spiral_pose(0.4)), 378, 504, cameras.llff_focal(504), 2, True, 0.0, 1.0)
    rays = rays.reshape(-1, 8)[4 * (252 * 95 + 100):][:512]
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    de = oc.posenc(d, 4)
    out = {}
    with torch.no_grad():
        for field in ("sharp", "dense", "thick"):
            sds = [make_state_dict(seed, "sharp" if field == "sharp" else "smooth") for seed in (99, 100)]
            if field == "dense":
                for sd in sds:
                    sd["sigma.bias"] = np.full((1,), 1e3, dtype=np.float32)
            if field == "thick":
                for sd in sds:
                    sd["sigma.bias"] = np.full((1,), 16, dtype=np.float32)
            sd_c, sd_f = (oc.to_torch_sd(sd) for sd in sds)
            z, xyz = oc.sample_coarse(o, d, near, far, 64, False)
            rgb, sig = oc.render_points(sd_c, xyz, de)
            z2, xyz2 = oc.resample_fine(o, d, z, oc.composite(rgb, sig, z, False)[3], 64)
            rgb2, sig2 = oc.render_points(sd_f, xyz2, de)
            out[field] = {64: (rgb, sig, z), 128: (rgb2, sig2, z2)}
    return out


@pytest.mark.parametrize("field", ["sharp", "dense", "thick"])
def test_bound_holds_on_the_oracle_render(oracle_render, field):
    """(The `sharp` field is thin along these rays -- tau stays below -ln(1e-3) -- so nothing is cut on it and its outputs
    do not move: scripts/early_stop_stats.py finds the same over whole frames.)"""
    cut_any, moved = 0, 0.0
    for N, (rgb, sig, z) in oracle_render[field].items():
        assert bool(((rgb >= 0) & (rgb <= 1)).all())           # the bound's precondition
        for eps in (1e-3, 1e-4, 1e-5):
            t = ref.truncate(rgb.numpy(), sig.numpy(), z.numpy(), eps)
            b, b_depth = ref.bounds(eps, z.numpy())
            for white in (False, True):
                full = oc.composite(rgb, sig, z, white)
                cut = oc.composite(torch.from_numpy(t.rgb), torch.from_numpy(t.sigma), z, white)
                d_rgb = float((full[0] - cut[0]).abs().max())
                d_op = float((full[2] - cut[2]).abs().max())
                d_depth = (full[1] - cut[1]).abs().numpy()
                print(f"{field} N {N} eps {eps:g} white {white}: {t.n_cut} windows cut, |dRGB| {d_rgb:.2e} |dopacity| {d_op:.2e} "
                      f"|ddepth| / bound {float((d_depth / b_depth).max()):.2e}")
                assert d_rgb <= b and d_op <= b and bool((d_depth <= b_depth).all())
                moved = max(moved, d_rgb)
                # weights in front of the cut are untouched, behind it exactly zero
                w_full, w_cut = full[3].numpy(), cut[3].numpy()
                for g, last in enumerate(t.last_window):
                    k = 32 * (int(last) + 1)
                    assert np.array_equal(w_cut[4 * g:4 * g + 4, :k], w_full[4 * g:4 * g + 4, :k])
                    assert not w_cut[4 * g:4 * g + 4, k:].any()
            cut_any += t.n_cut
            if field == "dense":                                # every window but the first of every group
                assert t.n_cut == 128 * (N // 32 - 1)
    if field == "sharp":
        assert cut_any == 0 and moved == 0.0
    else:
        assert cut_any > 0
    if field == "thick":        # partial cuts with a visible residual: the bound is not met trivially
        assert moved > 1e-6


# ------------------------------------------------------------------------------------------------ 3. the Python mirror
def test_default_options_and_refusals_before_any_device():
    from nerf_sr_amd import ops
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    assert default_options().early_stop == 0.0 and default_options(early_stop=1e-4).early_stop == 1e-4
    good = dict(early_stop=1e-4, precision="f16x3")
    for kw, word in ((dict(good, precision="fp32"), "f16x3"), (dict(good, precision="f16"), "f16x3"),
                     (dict(good, sigma_activation="softplus"), "softplus"), (dict(good, color_activation="none"), "color_activation"),
                     (dict(good, N_importance=32), "64 or 128"), (dict(good, N_coarse=96, N_importance=0), "64 or 128"),
                     (dict(good, D=4), "architecture"),
                     (dict(good, early_stop=1.0), "[0, 1)"), (dict(good, early_stop=-0.1), "[0, 1)"),
                     (dict(good, early_stop=float("nan")), "[0, 1)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            NeRFDownXModel(default_options(**kw), device="cuda")
    # the per-call check of ops.render_rays_composited / ops.forward_rays, on a network object that owns no device memory
    net = object.__new__(ops.VanillaMLP)
    net.precision, net.color_activation = "f16x3", "sigmoid"
    assert ops.check_early_stop(0.0, None, 96, "softplus") == 0.0 and ops.check_early_stop(1e-4, net, 128) == 1e-4
    for args, word in (((1.0, net, 128), "[0, 1)"), ((float("nan"), net, 128), "[0, 1)"), ((-1e-9, net, 128), "[0, 1)"),
                       ((1e-4, net, 96), "64 or 128"), ((1e-4, net, 128, "softplus"), "softplus"),
                       ((1e-4, SimpleNamespace(precision="f16x3"), 128), "f16x3")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.check_early_stop(*args)
    net.precision = "fp32"
    with pytest.raises(ValueError, match="f16x3"):
        ops.check_early_stop(1e-4, net, 128)
    net.precision, net.color_activation = "f16x3", "none"
    with pytest.raises(ValueError, match="color_activation"):
        ops.check_early_stop(1e-4, net, 128)
