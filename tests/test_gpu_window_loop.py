"""The split-fp16 render kernel of ``nsr_render_rays_composited`` (csrc/nsr_mlp_f16.hip, "COMP") walks the N / 32 depth
windows of a wave's ray in a loop.  What depends on the ray alone -- the ray fetch, the range check of the encoded direction,
its encoding -- is done once before that loop, and the wave index the chunk addresses derive from is re-read once per
window.  None of it may change a bit: the two-call route (``nsr_render_rays`` + the
stand-alone compositor) does all of it per 128-point tile, so ``torch.equal`` against it on inputs chosen to tell the waves
and the windows apart is the check:

  * every ray of a 4-ray group has its own origin and direction (a wave that used another wave's hoisted ray would show);
  * the depths are jittered per sample (randomized stratified sampling), so no two windows of a ray share their depths
    (depths taken from the wrong window would show);
  * 11-wide rays, whose ENCODED direction (columns 8:11) is not the marching direction (columns 3:6);
  * a bundle on which some ray groups have an all-empty window directly followed by a live one and others the reverse:
    the skipped window restarts the weight ring, the live one streams it through, the hoisted ray state crosses both;
  * the numerics status word: a NaN or out-of-range direction is now caught before the loop, a position inside it.
"""
from ctypes import c_int, c_int64, c_void_p

import pytest
import torch

from nerf_sr_amd.weights import make_state_dict
from tests import hooks

pytestmark = pytest.mark.gpu

RAY_COUNTS = (1, 3, 4, 5, 9)      # whole groups, clamped last groups, one wave alone
SAMPLES = (64, 128)
NAMES = ("comp_rgb", "depth", "opacity", "weights")
INPUT_RANGE = 2                   # NSR_FLAG_INPUT_RANGE (include/nsr.h)
# the skip-pattern bundle: 1,025 groups of the benchmark's frame.  On the fp32 CPU oracle (oracle/nerf_oracle.py: the same rays,
# jitter and field) 2,140 of its 4,100 windows are all-empty, 360 groups have an empty window directly followed by a live
# one and 278 the reverse: far from the edge of either being absent.
PATTERN_RAYS, PATTERN_N = 4099, 128


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def nets(ops):
    return {f: ops.VanillaMLP(precision="f16x3").load_state_dict(make_state_dict(99, f)) for f in ("smooth", "sharp")}


@pytest.fixture(scope="module")
def counted(ops):
    """(net, rays, z, white) -> the four outputs + the skipped-window count, through the test-hook library."""
    fn = hooks.load().nsr_test_f16x3_render_composite
    fn.restype = c_int
    fn.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int] + [c_void_p] * 7

    def run(net, rays, z, white):
        R, N = z.shape
        comp = torch.full((R, 3), float("nan"), device="cuda")
        depth = torch.full((R,), float("nan"), device="cuda")
        opac = torch.full((R,), float("nan"), device="cuda")
        w = torch.full((R, N), float("nan"), device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = fn(hooks.ptr(net.packed), hooks.ptr(rays), rays.shape[1], hooks.ptr(z), R, N, ops.renderer_flags(white), None,
                hooks.ptr(comp), hooks.ptr(depth), hooks.ptr(opac), hooks.ptr(w), hooks.ptr(count), hooks.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return comp, depth, opac, w, int(count.item())
    return run


def _rays(ops, n, seed=0):
    """n consecutive rays from the middle of the benchmark's frame (every 4 = the sub-pixel rays of one LR pixel), each
    nudged by its own small offset in origin and direction so that no two rays of a group share either."""
    from nerf_sr_amd import cameras
    lo = 252 * 95 + 100
    r = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, 0.0, 1.0, device="cuda",
                          lr_range=(lo, lo + (n + 3) // 4)).view(-1, 8)[:n].clone()
    g = torch.Generator().manual_seed(1000 + seed)
    r[:, 0:6] += (1e-3 * torch.randn(n, 6, generator=g)).cuda()
    group = torch.arange(n, device="cuda") // 4
    for k in (1, 2, 3):                        # rays k apart in the same group: distinct origins, distinct directions
        other = group[k:] != group[:-k]
        assert bool(((r[k:, 0:3] != r[:-k, 0:3]).any(1) | other).all()) and bool(((r[k:, 3:6] != r[:-k, 3:6]).any(1) | other).all())
    return r.contiguous()


def _z(ops, rays, N, seed=0):
    """Randomized stratified depths: every sample has its own jitter, so the 32 depths of a window are no other window's."""
    u = torch.rand(rays.shape[0], N, generator=torch.Generator().manual_seed(2000 + seed)).cuda()
    z, _ = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, True, False, u=u)
    w = z.view(z.shape[0], N // 32, 32)
    assert bool((w[:, 1:] - w[:, :-1] > 0).all()), "every window's depths lie behind the previous window's"
    step = w[:, :, 1:] - w[:, :, :-1]
    assert float(step.std()) > 0.1 * float(step.mean()), "the depths are not jittered"
    return z.contiguous()


def _dead_windows(sig):
    """(groups, N / 32) bool: the window's densities (4 rays x 32 samples; rays past the end count as empty) are all <= 0, on
    the (R, N) raw densities of the two-call route -- the definition of tests/test_gpu_empty_skip.py.  NaN is not <= 0."""
    R, N = sig.shape
    dead = sig <= 0
    if (-R) % 4:
        dead = torch.cat([dead, torch.ones((-R) % 4, N, dtype=torch.bool, device=sig.device)])
    return dead.view(-1, 4, N // 32, 32).permute(0, 2, 1, 3).reshape(-1, N // 32, 128).all(-1)


def _check(ops, counted, net, rays, z, white):
    rgb, sig = ops.render_rays(net, rays, z)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(sig).all())
    want = ops.VolumetricRenderer()(rgb.contiguous(), sig.contiguous(), z, white)
    got = ops.render_rays_composited(net, rays, z, white)
    hooked = counted(net, rays, z, white)
    for name, a, b, c in zip(NAMES, got, hooked[:4], want):
        assert torch.equal(a, c), name
        assert torch.equal(b, c), name + " (hook library)"
    dead = _dead_windows(sig)
    print(f"R {z.shape[0]} N {z.shape[1]} stride {rays.shape[1]} white {white}: {hooked[4]} of {dead.numel()} windows skipped "
          f"({int(dead.sum())} all-empty)")
    assert hooked[4] == int(dead.sum()), (hooked[4], int(dead.sum()), dead.numel())
    return dead


@pytest.mark.parametrize("field", ["smooth", "sharp"])
def test_fused_render_equals_the_two_call_route(ops, nets, counted, field):
    for N in SAMPLES:
        for R in RAY_COUNTS:
            rays = _rays(ops, R, seed=R)
            z = _z(ops, rays, N, seed=R)
            for white in (False, True):
                _check(ops, counted, nets[field], rays, z, white)


def _with_view_direction(rays):
    """(R, 8) -> (R, 11): a unit view direction in columns 8:11 that is not the marching direction."""
    v = torch.nn.functional.normalize(rays[:, 3:6].flip(1) + 0.3, dim=1)
    assert bool((v != rays[:, 3:6]).any(1).all())
    return torch.cat([rays, v], 1).contiguous()


def test_encoded_direction_of_11_wide_rays(ops, nets, counted):
    rays = _with_view_direction(_rays(ops, 9, seed=11))
    for N in SAMPLES:
        _check(ops, counted, nets["smooth"], rays, _z(ops, rays[:, :8], N, seed=11), True)


def test_empty_then_live_and_live_then_empty_windows(ops, nets, counted):
    rays = _rays(ops, PATTERN_RAYS, seed=7)
    dead = _check(ops, counted, nets["smooth"], rays, _z(ops, rays, PATTERN_N, seed=7), False)
    empty_then_live = int((dead[:, :-1] & ~dead[:, 1:]).any(1).sum())
    live_then_empty = int((~dead[:, :-1] & dead[:, 1:]).any(1).sum())
    print(f"groups with an all-empty window directly followed by a live one: {empty_then_live}; the reverse: {live_then_empty}")
    assert empty_then_live > 0 and live_then_empty > 0, (empty_then_live, live_then_empty)


@pytest.mark.parametrize("what", ["nan_direction", "nan_view_direction", "position_over_65504", "view_direction_over_65504"])
def test_input_range_flag_equals_the_two_call_route(ops, nets, what):
    """The bad ray is wave 2 of the second group; the status word is the whole launch's (sticky, read and cleared here)."""
    net = nets["smooth"]
    rays = _rays(ops, 9, seed=13)
    z = _z(ops, rays, 128, seed=13)
    if "view" in what:
        rays = _with_view_direction(rays)
    if what == "nan_direction":
        rays[6, 4] = float("nan")
    elif what == "nan_view_direction":
        rays[6, 9] = float("nan")
    elif what == "position_over_65504":
        rays[6, 0] = 7.0e4
    else:
        rays[6, 10] = -7.0e4
    net.status(clear=True)
    ops.render_rays(net, rays, z)
    two_call = net.status(clear=True)
    ops.render_rays_composited(net, rays, z, False)
    fused = net.status(clear=True)
    print(f"{what}: status {fused:#x} (two-call route {two_call:#x})")
    assert fused & INPUT_RANGE
    assert fused == two_call
