"""The weight DMA of the split-fp16 render kernels by constant per-wave shares (csrc/nsr_f16x3_core.h, "constant shares";
DESIGN 3.1): every wave moves K fragment pieces and a quarter of the bias piece of every chunk, K a constant of the code that
fetches the chunk.  A piece in the wrong place, a missing one or a wait that lets a chunk be read too early changes the
network, so every case runs random weights and asserts

1. the fused launch ``torch.equal`` to the two-call route ``nsr_render_rays`` + the stand-alone compositor, which runs another
   chunk sequence (one 128-point tile, no window loop, nothing fetched behind the last two dir_encoding blocks) through the
   same loader;
2. the composited colour (the density pass: the opacity) within the per-ray contract of tests/util.py -- max(1e-4, 2 x the
   oracle's own fp32-vs-fp64 gap) -- of the CPU oracle, and a clear status word.

Fields: ``sigma.bias`` -1e3 (every window empty: the ring is restarted behind every density block), +1e3 (none is) and as
generated (both).  Ray counts 1, 3, 4, 5, 9: a single ragged group, a full one, groups whose later waves idle.  64, 128, 192 and
256 samples; the density-only pass once through ``forward_rays(coarse_rgb=False)``; early ray termination once on the dense
field, where the loop breaks behind the first window and drains the L1 chunks it had fetched for the second."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import make_state_dict
from oracle import nerf_oracle as oc

pytestmark = pytest.mark.gpu

RAY_COUNTS = (1, 3, 4, 5, 9)
SAMPLES = (64, 128, 192, 256)
FIELDS = {"empty": -1e3, "dense": 1e3, "mixed": None}
NAMES = ("comp_rgb", "depth", "opacity", "weights")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


def _state(field, seed=99):
    sd = make_state_dict(seed)
    if FIELDS[field] is not None:
        sd["sigma.bias"] = np.full((1,), FIELDS[field], dtype=np.float32)
    return sd


@pytest.fixture(scope="module")
def nets(ops):
    made = {}

    def get(field, seed=99):
        if (field, seed) not in made:
            made[(field, seed)] = ops.VanillaMLP(precision="f16x3").load_state_dict(_state(field, seed))
        return made[(field, seed)]
    return get


@pytest.fixture(scope="module")
def rays9():
    """nine consecutive rays from the middle of the benchmark's frame (config #2), as tests/test_gpu_testtime.py takes them"""
    from nerf_sr_amd import cameras, ops
    lo = 252 * 95 + 100
    return ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, 0.0, 1.0, device="cuda",
                             lr_range=(lo, lo + 3)).view(-1, 8)[:9].contiguous()


def _z(ops, rays, N):
    z, _ = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)
    return z.contiguous()


_ORACLE = {}


def _oracle(field, rays, z, white, seed=99):
    """(fp32, fp64) composited outputs of the CPU oracle on the nine rays at the kernel's own depths; once per case, shared"""
    key = (field, seed, z.shape[1], white)
    if key not in _ORACLE:
        out = []
        for dt in (torch.float32, torch.float64):
            sd = oc.to_torch_sd(_state(field, seed), dt)
            r, zz = rays.cpu().to(dt), z.cpu().to(dt)
            with torch.no_grad():
                rgb, sig = oc.render_points(sd, oc.points_on_rays(r[:, 0:3], r[:, 3:6], zz), oc.posenc(r[:, 3:6], 4))
                out.append(oc.composite(rgb, sig, zz, white))
        _ORACLE[key] = out
    return _ORACLE[key]


def _assert_contract(got, ref32, ref64, what):
    """per ray: |got - fp32 oracle| <= max(1e-4, 2 |fp32 oracle - fp64 oracle|)"""
    got, a, b = (t.detach().cpu().double().reshape(got.shape[0], -1) for t in (got, ref32, ref64))
    err = (got - a).abs().max(1)[0]
    tol = torch.clamp(2.0 * (a - b).abs().max(1)[0], min=1e-4)
    print(f"{what}: worst ray {float(err.max()):.3e} (bound {float(tol[err.argmax()]):.3e})")
    assert bool((err <= tol).all()), (what, err.tolist(), tol.tolist())


@pytest.mark.parametrize("N", SAMPLES)
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_fused_render_equals_the_two_call_route_and_meets_the_oracle(ops, nets, rays9, field, N):
    net = nets(field)
    z9 = _z(ops, rays9, N)
    rend = ops.VolumetricRenderer()
    for white in (False, True):
        ref32, ref64 = _oracle(field, rays9, z9, white)
        for R in RAY_COUNTS:
            rays, z = rays9[:R].contiguous(), z9[:R].contiguous()
            rgb, sig = ops.render_rays(net, rays, z)
            want = rend(rgb.contiguous(), sig.contiguous(), z, white)
            got = ops.render_rays_composited(net, rays, z, white)
            for name, a, c in zip(NAMES, got, want):
                assert torch.equal(a, c), (name, field, N, R, white)
            if field == "empty":
                assert not bool(got[3].any())
            _assert_contract(got[0], ref32[0][:R], ref64[0][:R], f"{field} N {N} R {R} white {white} comp_rgb")
            assert net.status(clear=True) == 0


def _staged(ops, coarse, fine, rays, Nc, Ni, white):
    """sample -> render -> composite -> resample -> render -> composite through the stand-alone calls"""
    rend = ops.VolumetricRenderer()
    z = _z(ops, rays, Nc)
    rgb, sig = ops.render_rays(coarse, rays, z)
    c = rend(rgb.contiguous(), sig.contiguous(), z, white)
    z2, _ = ops.resample_along_rays(rays[:, 0:3], rays[:, 3:6], z, c[3], Ni, False)
    z2 = z2.contiguous()
    rgb2, sig2 = ops.render_rays(fine, rays, z2)
    return dict(zip(ops.OUT_KEYS, c + rend(rgb2.contiguous(), sig2.contiguous(), z2, white))), z2


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_density_only_coarse_pass(ops, nets, rays9, field):
    """``coarse_rgb=False``: the coarse launch is the density-only instantiation, the fine one the 128-sample launch"""
    coarse, fine = nets(field), nets(field, 100)
    for R in RAY_COUNTS:
        rays = rays9[:R].contiguous()
        want, z2 = _staged(ops, coarse, fine, rays, 64, 64, True)
        got = ops.forward_rays(coarse, fine, rays, 64, 64, True, coarse_rgb=False)
        assert sorted(got) == sorted(k for k in ops.OUT_KEYS if k != "coarse_comp_rgbs")
        for k in got:
            assert torch.equal(got[k], want[k]), (k, field, R)
        assert coarse.status(clear=True) == 0 and fine.status(clear=True) == 0
    # R = 9 is the last of the loop: its depths are the oracle's inputs
    z = _z(ops, rays9, 64)
    ref32, ref64 = _oracle(field, rays9, z, True)
    _assert_contract(got["coarse_opacity"], ref32[2], ref64[2], f"{field} density pass opacity")
    f32, f64 = _oracle(field, rays9, z2, True, seed=100)
    _assert_contract(got["fine_comp_rgbs"], f32[0], f64[0], f"{field} fine comp_rgb behind the density pass")


@pytest.mark.parametrize("N", (64, 128))
def test_early_stop_breaks_behind_the_first_window_and_drains(ops, nets, rays9, N):
    """Dense field: the transmittance is exactly 0 behind the first window (tau > 100 there), so the cut launch equals the uncut
    one bit for bit, and every group cuts every window but its first."""
    net = nets("dense")
    z9 = _z(ops, rays9, N)
    ref32, ref64 = _oracle("dense", rays9, z9, False)
    rend = ops.VolumetricRenderer()
    for R in RAY_COUNTS:
        rays, z = rays9[:R].contiguous(), z9[:R].contiguous()
        rgb, sig = ops.render_rays(net, rays, z)
        want = rend(rgb.contiguous(), sig.contiguous(), z, False)
        assert not bool(want[3][:, 32:].any()), "the exactness argument needs a spent ray behind the first window"
        got = ops.render_rays_composited(net, rays, z, False, early_stop=1e-4, want_cut_count=True)
        for name, a, c in zip(NAMES, got[:4], want):
            assert torch.equal(a, c), (name, N, R)
        assert int(got[4].item()) == ((R + 3) // 4) * (N // 32 - 1)
        _assert_contract(got[0], ref32[0][:R], ref64[0][:R], f"early stop N {N} R {R} comp_rgb")
        assert net.status(clear=True) == 0
