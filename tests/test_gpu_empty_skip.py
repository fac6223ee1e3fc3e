"""The split-fp16 render kernel of ``nsr_render_rays_composited`` (csrc/nsr_mlp_f16.hip, "COMP") tiles a launch into groups
of 4 consecutive rays x windows of 32 samples and ends a window after the density head when none of its 128 samples has a
raw density above zero: their weights are exactly +0 under the relu density, so the colours it leaves out cannot reach any
output.  The two-call route (``nsr_render_rays`` + the stand-alone compositor) evaluates every colour, so ``torch.equal``
against it proves the skip exact.  That the skip HAPPENS is shown by a counter the test-hook library passes to the same
launch (tests/csrc/nsr_test_hooks_render.hip: ``nsr_test_f16x3_render_composite``; libnsr.so itself always passes null): every
window on a field whose density is negative everywhere, none on a field whose density is positive everywhere, none under
the softplus density (where a negative raw density still has weight), and on the benchmark's fields exactly the windows
whose 128 raw densities -- read from the two-call route's (R, N, 4) output -- are all <= 0."""
from ctypes import c_int, c_int64, c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import make_state_dict
from tests import hooks

pytestmark = pytest.mark.gpu

RAY_COUNTS = (1, 2, 3, 5, 4099)
SAMPLES = (64, 128)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def counted():
    """(packed net, rays, z, white, sigma_activation) -> (comp, depth, opacity, weights, skipped windows) through the hooks."""
    lib = hooks.load()
    fn = lib.nsr_test_f16x3_render_composite
    fn.restype = c_int
    fn.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int] + [c_void_p] * 7

    def run(ops, net, rays, z, white, sigma_activation="relu"):
        R, N = z.shape
        comp = torch.full((R, 3), float("nan"), device="cuda")
        depth = torch.full((R,), float("nan"), device="cuda")
        opac = torch.full((R,), float("nan"), device="cuda")
        w = torch.full((R, N), float("nan"), device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = fn(hooks.ptr(net.packed), hooks.ptr(rays), rays.shape[1], hooks.ptr(z), R, N, ops.renderer_flags(white, sigma_activation),
                None, hooks.ptr(comp), hooks.ptr(depth), hooks.ptr(opac), hooks.ptr(w), hooks.ptr(count), hooks.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return comp, depth, opac, w, int(count.item())
    return run


def _rays(n):
    """n consecutive rays from the middle of the benchmark's frame (BASELINE config #2: 504x378 <- 252x189, NDC): every 4
    consecutive ones are the sub-pixel rays of one LR pixel."""
    from nerf_sr_amd import cameras, ops
    lo = 252 * 95 + 100
    r = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, 0.0, 1.0, device="cuda",
                          lr_range=(lo, lo + (n + 3) // 4)).view(-1, 8)
    return r[:n].contiguous()


def _z(ops, rays, N):
    z, _ = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)
    return z.contiguous()


def _field(name):
    if name in ("smooth", "sharp"):
        return make_state_dict(99, name)
    sd = make_state_dict(99, "smooth")
    sd["sigma.bias"] = np.full((1,), -1e3 if name == "empty" else 1e3, dtype=np.float32)
    return sd


def _n_windows(R, N):
    return ((R + 3) // 4) * (N // 32)


def _empty_windows(sig):
    """Windows (4 consecutive rays x 32 consecutive samples; the last group may hold fewer rays) whose densities are all <= 0,
    counted on the (R, N) raw densities of the two-call route.  NaN is not <= 0."""
    R, N = sig.shape
    pad = (-R) % 4
    dead = sig <= 0
    if pad:
        dead = torch.cat([dead, torch.ones(pad, N, dtype=torch.bool, device=sig.device)])
    return int(dead.reshape(-1, 4, N // 32, 32).permute(0, 2, 1, 3).reshape(-1, 128).all(-1).sum().item())


def _check(ops, counted, net, rays, z, white, sigma_activation="relu", want_count=None):
    rend = ops.VolumetricRenderer(SimpleNamespace(sigma_activation=sigma_activation))
    rgb, sig = ops.render_rays(net, rays, z)
    assert bool(torch.isfinite(rgb).all()), "the exactness argument needs finite colours"
    want = rend(rgb.contiguous(), sig.contiguous(), z, white)
    got = ops.render_rays_composited(net, rays, z, white, sigma_activation=sigma_activation)
    hooked = counted(ops, net, rays, z, white, sigma_activation)
    names = ("comp_rgb", "depth", "opacity", "weights")
    for name, a, b, c in zip(names, got, hooked[:4], want):
        assert torch.equal(a, c), name
        assert torch.equal(b, c), name + " (hook library)"
    n_win = _n_windows(*z.shape)
    n_dead = _empty_windows(sig)
    count = hooked[4]
    print(f"R {z.shape[0]} N {z.shape[1]} white {white} {sigma_activation}: {count} of {n_win} windows skipped ({n_dead} all-empty)")
    assert count == (n_dead if want_count is None else want_count), (count, n_dead, n_win)
    return count, n_win


@pytest.mark.parametrize("field", ["smooth", "sharp", "empty", "dense"])
def test_fused_render_equals_the_two_call_route_and_skips_exactly_the_empty_windows(ops, counted, field):
    net = ops.VanillaMLP(precision="f16x3").load_state_dict(_field(field))
    for N in SAMPLES:
        for R in RAY_COUNTS:
            rays = _rays(R)
            z = _z(ops, rays, N)
            for white in (False, True):
                count, n_win = _check(ops, counted, net, rays, z, white)
                if field == "empty":
                    assert count == n_win
                if field == "dense":
                    assert count == 0
    if field == "smooth":      # the benchmark's field does skip on ray bundles like an image's
        count, n_win = _check(ops, counted, net, _rays(4099), _z(ops, _rays(4099), 128), False)
        assert 0 < count < n_win


@pytest.mark.parametrize("option", ["gamma_correct", "color_none"])
def test_colour_options_with_the_skip(ops, counted, option):
    """--gamma_correct (a skipped window's colour 0 stands for pow(rgb, 1 / 2.2) of a sigmoid output: finite) and
    --color_activation none (finite colours of either sign: +0 * rgb = +-0, and an accumulator that starts at +0 stays +0)."""
    opt = SimpleNamespace(color_activation="none") if option == "color_none" else None
    net = ops.VanillaMLP(opt, precision="f16x3").load_state_dict(_field("smooth"))
    if option == "gamma_correct":
        net.set_gamma_correct(True)
    for N in SAMPLES:
        for R in (5, 4099):
            rays = _rays(R)
            for white in (False, True):
                _check(ops, counted, net, rays, _z(ops, rays, N), white)


@pytest.mark.parametrize("field", ["smooth", "empty"])
def test_softplus_density_never_skips(ops, counted, field):
    """log(1 + exp(sigma - 1)) > 0 for every finite raw density: a sample with sigma <= 0 still has weight, the skip is off."""
    net = ops.VanillaMLP(precision="f16x3").load_state_dict(_field(field))
    for N in SAMPLES:
        for R in RAY_COUNTS:
            rays = _rays(R)
            _check(ops, counted, net, rays, _z(ops, rays, N), True, "softplus", want_count=0)
