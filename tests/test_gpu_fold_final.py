"""The split-fp16 inference kernels evaluate ``dir_encoding`` on L8's output directly: ``xyz_encoding_final`` (a bare Linear whose
output feeds ``dir_encoding`` alone) is folded into it at pack time, ``W' = W_dir[:, :256] W_f``, ``b' = b_dir +
W_dir[:, :256] b_f`` (csrc/nsr_mlp_layout.h, "Folded dir_encoding").  What that must keep and what it adds:

  * colours against the oracle at the tolerance tests/test_gpu_parity.py::test_f16x3_mlp_vs_golden holds the same quantity to,
    on the benchmark's network, on one whose ``xyz_encoding_final`` is a bias alone (``b'`` on its own) and on a ``--no_dir``
    network; the density bit for bit what the density-only launch returns;
  * rays against the fp32 and fp64 oracles under the per-ray rule max(1e-4, 2 x the oracle's own gap), no ray exempt; the
    compositing weights a function of the densities alone;
  * the fused launch bit for bit the two-call route, also with a white background, 11-wide rays and gamma;
  * the folded matrix enters the fp16 stream like every weight: its own range check;
  * a module loaded twice serves the second network (no stale folded region).

Shapes: 160 points (one 128-point tile + a ragged 32), 6 rays (one group of 4 + a ragged 2) at 64 and 128 samples.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib, cameras
from nerf_sr_amd.weights import make_state_dict
from oracle import nerf_oracle as oc

pytestmark = pytest.mark.gpu

RGB_POINT_TOL = 3e-6      # tests/test_gpu_parity.py::test_f16x3_mlp_vs_golden: sigmoid colours of the f16x3 kernel vs the oracle
RGB_TOL = 1e-4            # the per-ray contract (tests/util.py): max(1e-4, 2 x the oracle's own fp32-vs-fp64 gap)
P, R = 160, 6
FINAL_W, FINAL_B, DIR_W = "xyz_encoding_final.weight", "xyz_encoding_final.bias", "dir_encoding.0.weight"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


def _bias_only(sd, seed=5):
    """xyz_encoding_final = a bias alone, large against the network's own (make_state_dict: 0.05): b' carries the layer."""
    out = dict(sd)
    out[FINAL_W] = np.zeros_like(sd[FINAL_W])
    out[FINAL_B] = np.random.default_rng(seed).uniform(-2.0, 2.0, sd[FINAL_B].shape).astype(np.float32)
    return out


def _narrow(sd):
    out = dict(sd)
    out[DIR_W] = np.ascontiguousarray(sd[DIR_W][:, :256])
    return out


CASES = {"bench": (lambda: make_state_dict(99), None),
         "bias_only": (lambda: _bias_only(make_state_dict(99)), None),
         "no_dir": (lambda: _narrow(make_state_dict(99)), SimpleNamespace(no_dir=True))}


@pytest.fixture(scope="module")
def points():
    gen = torch.Generator().manual_seed(3)
    return torch.cat([oc.posenc(torch.rand(P, 3, generator=gen) * 2 - 1, 10),
                      oc.posenc(torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1), 4)], -1)


@pytest.mark.parametrize("case", list(CASES))
def test_points_against_the_oracle(ops, points, case):
    make, opt = CASES[case]
    sd = make()
    net = ops.VanillaMLP(opt, precision="f16x3").load_state_dict(sd)
    want = oc.mlp_forward(oc.to_torch_sd(sd), points)
    out = net(points.cuda())
    err = float((out[:, :3].cpu() - want[:, :3]).abs().max())
    print(f"{case}: max |dRGB| vs the fp32 oracle {err:.3e} (tolerance {RGB_POINT_TOL:.0e})")
    assert out.shape == (P, 4) and err <= RGB_POINT_TOL
    assert torch.equal(out[:, 3], net(points.cuda(), sigma_only=True)[:, 0])
    assert net.status(clear=True) == 0


def _rays(ops, n, wide=False):
    """n consecutive rays from the middle of the benchmark's frame (every 4 = the sub-pixel rays of one LR pixel)."""
    lo = 252 * 95 + 100
    r = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, 0.0, 1.0, device="cuda",
                          lr_range=(lo, lo + (n + 3) // 4)).view(-1, 8)[:n].contiguous()
    if wide:     # (R, 11): a unit view direction in columns 8:11 that is not the marching direction
        r = torch.cat([r, torch.nn.functional.normalize(r[:, 3:6].flip(1) + 0.3, dim=1)], 1).contiguous()
    return r


@pytest.fixture(scope="module")
def pair(ops):
    sd_c, sd_f = make_state_dict(99), make_state_dict(100)
    return (sd_c, sd_f, ops.VanillaMLP(precision="f16x3").load_state_dict(sd_c), ops.VanillaMLP(precision="f16x3").load_state_dict(sd_f))


def test_rays_against_the_oracles(ops, pair):
    sd_c, sd_f, net_c, net_f = pair
    rays = _rays(ops, R)
    hip = {k: v.cpu().double() for k, v in ops.forward_rays(net_c, net_f, rays, 64, 64, False).items()}
    cpu = rays.cpu()
    with torch.no_grad():
        o32 = oc.forward_rays(oc.to_torch_sd(sd_c), oc.to_torch_sd(sd_f), cpu, 64, 64, False)
        o64 = oc.forward_rays(oc.to_torch_sd(sd_c, torch.float64), oc.to_torch_sd(sd_f, torch.float64), cpu.double(), 64, 64, False)
    for k in ("coarse_comp_rgbs", "fine_comp_rgbs"):
        gap = (o32[k].double() - o64[k]).abs().amax(-1)
        bound = torch.maximum(torch.full_like(gap, RGB_TOL), 2 * gap)
        e32 = (hip[k] - o32[k].double()).abs().amax(-1)
        e64 = (hip[k] - o64[k]).abs().amax(-1)
        print(f"{k}: max |dRGB| vs fp32 oracle {float(e32.max()):.3e}, vs fp64 oracle {float(e64.max()):.3e}; oracle gap {float(gap.max()):.3e}")
        assert float(gap.max()) < RGB_TOL            # the fp32 oracle itself is inside the contract on these rays
        assert bool((e32 <= bound).all()) and bool((e64 <= bound).all()), (k, e32, e64, bound)
    # what the density alone decides, at the tolerances tests/test_gpu_parity.py::test_f16x3_forward_rays_vs_golden holds it to
    # (far = 1 on these NDC rays), and the s^2 mean of the first LR pixel (its four sub-pixel rays) under the colour contract
    far = float(cpu[0, 7])
    for k in ("coarse_opacity", "fine_opacity", "coarse_depth", "fine_depth"):
        err = float((hip[k] - o32[k].double()).abs().max())
        print(f"{k}: max err vs fp32 oracle {err:.3e}")
        assert err <= 1e-4 * (far if k.endswith("depth") else 1.0), k
    lr = ops.sr_mean(ops.forward_rays(net_c, net_f, rays, 64, 64, False)["fine_comp_rgbs"][:4].contiguous(), 1, 4).cpu()
    assert float((lr - oc.sr_mean(o32["fine_comp_rgbs"][:4], 1, 4)).abs().max()) <= RGB_TOL


@pytest.mark.parametrize("which", ["coarse", "fine"])
@pytest.mark.parametrize("N", [64, 128])
def test_weights_come_from_the_densities_alone(ops, pair, N, which):
    """Two density-only routes fed the same z.  (1) The raw launch's densities, composited with every colour set to zero: the
    fused launch's weights, depth and opacity must be those bit for bit.  (2) The density-only launch (``sigma_only``: an
    instantiation that never reads the folded chunks) on the rays' encoded points.  It takes embedded rows, made by the
    stand-alone encoder (sinf / cosf), while the ray launches encode in the kernel (nsr_sincos, abs error < 1.5e-7): the two
    are not the same bits, so this route is held to a bound instead: densities within 2e-4 (each route is held to 1e-4 of the
    same golden densities by tests/test_gpu_parity.py::test_f16x3_mlp_vs_golden), hence weights of every sample but the
    last (whose delta is 1e10: alpha jumps at sigma = 0) within 2e-4 x (z_last - z_first) + 1e-6, since
    |dw_k| <= delta_k |dsigma_k| + sum_{j<k} delta_j |dsigma_j|."""
    net = pair[2] if which == "coarse" else pair[3]
    rays = _rays(ops, R)
    z, _ = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)
    comp, depth, opac, w = ops.render_rays_composited(net, rays, z, False)
    rgb, sig = ops.render_rays(net, rays, z)
    _, depth0, opac0, w0 = ops.VolumetricRenderer()(torch.zeros_like(rgb), sig.contiguous(), z, False)
    assert float(w.max()) > 0.0
    assert torch.equal(w, w0) and torch.equal(depth, depth0) and torch.equal(opac, opac0)
    xyz = ops.cast_rays(rays[:, 0:3], rays[:, 3:6], z)
    x = torch.cat([ops.PositionalEncoding(3, 10)(xyz.reshape(-1, 3).contiguous()),
                   ops.PositionalEncoding(3, 4)(rays[:, 3:6].contiguous()).repeat_interleave(N, dim=0)], -1).contiguous()
    sig1 = net(x, sigma_only=True)[:, 0].view(R, N)
    d_sig = float((sig1 - sig).abs().max())
    _, _, _, w1 = ops.VolumetricRenderer()(torch.zeros_like(rgb), sig1.contiguous(), z, False)
    d_w = float((w1[:, :-1] - w[:, :-1]).abs().max())
    bound = 2e-4 * float((z[:, -1] - z[:, 0]).max()) + 1e-6
    print(f"{which} N {N}: density-only launch vs the ray launch: max |dsigma| {d_sig:.3e}, max |dweight| {d_w:.3e} (bound {bound:.3e})")
    assert d_sig <= 2e-4 and d_w <= bound


@pytest.mark.parametrize("what", ["plain", "white_bkgd", "wide_rays", "gamma"])
def test_fused_equals_the_two_call_route(ops, what):
    net = ops.VanillaMLP(precision="f16x3").load_state_dict(make_state_dict(100))
    if what == "gamma":
        net.set_gamma_correct(True)
    rays = _rays(ops, R, wide=(what == "wide_rays"))
    white = what == "white_bkgd"
    for N in (64, 128):
        z, _ = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)
        rgb, sig = ops.render_rays(net, rays, z)
        assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(sig).all())
        want = ops.VolumetricRenderer()(rgb.contiguous(), sig.contiguous(), z, white)
        got = ops.render_rays_composited(net, rays, z, white)
        for name, a, b in zip(("comp_rgb", "depth", "opacity", "weights"), got, want):
            assert torch.equal(a, b), (what, N, name)
        assert float(got[0].abs().max()) > 0.0
    assert net.status(clear=True) == 0


def test_folded_matrix_range_rule(ops):
    """Each of the 24 tensors passes the raw check (|w| = 40 < 1023.75) but W' = 256 x 40 x 40 = 409,600 does not."""
    sd = make_state_dict(99)
    sd[FINAL_W] = np.full_like(sd[FINAL_W], 40.0)
    sd[DIR_W] = sd[DIR_W].copy()
    sd[DIR_W][:, :256] = 40.0
    with pytest.raises(_lib.NsrNumericsError):
        ops.VanillaMLP(precision="f16x3").load_state_dict(sd)
    assert ops.VanillaMLP(precision="fp32").load_state_dict(sd).status() == 0
    # the blob's own word, without the exception in between
    blob = torch.empty(_lib.load().nsr_packed_weights_bytes(_lib.NSR_F16X3), dtype=torch.uint8, device="cuda")
    dev = [torch.from_numpy(np.ascontiguousarray(v)).float().cuda() for v in sd.values()]
    import ctypes
    ptrs = (ctypes.c_void_p * len(dev))(*[ctypes.c_void_p(t.data_ptr()) for t in dev])
    assert _lib.load().nsr_pack_weights(ptrs, ctypes.c_void_p(blob.data_ptr()), _lib.NSR_F16X3, None) == _lib.NSR_ERR_RANGE
    flags = ctypes.c_uint(0)
    assert _lib.load().nsr_weights_status(ctypes.c_void_p(blob.data_ptr()), _lib.NSR_F16X3, 0, ctypes.byref(flags), None) == 0
    assert flags.value & 1                              # NSR_FLAG_WEIGHT_RANGE
    # finite tensors that each pass the raw check, W' = 0 in range, but b' = b_dir + 256 x 40 x 1e37 overflows fp32
    big = make_state_dict(99)
    big[FINAL_W] = np.zeros_like(big[FINAL_W])
    big[FINAL_B] = np.full_like(big[FINAL_B], 1e37)
    big[DIR_W] = big[DIR_W].copy()
    big[DIR_W][:, :256] = 40.0
    with pytest.raises(_lib.NsrNumericsError):
        ops.VanillaMLP(precision="f16x3").load_state_dict(big)
    assert ops.VanillaMLP(precision="fp32").load_state_dict(big).status() == 0
    nan = make_state_dict(99)
    nan[FINAL_B] = nan[FINAL_B].copy()
    nan[FINAL_B][7] = float("nan")
    with pytest.raises(_lib.NsrNumericsError):
        ops.VanillaMLP(precision="f16x3").load_state_dict(nan)


def test_repack_leaves_no_stale_fold(ops, points):
    a, b = make_state_dict(99), _bias_only(make_state_dict(100), seed=9)
    rays = _rays(ops, R)
    z, _ = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], 128, False, False)
    net = ops.VanillaMLP(precision="f16x3").load_state_dict(a)
    first = net(points.cuda()).clone()
    net.load_state_dict(b)
    fresh = ops.VanillaMLP(precision="f16x3").load_state_dict(b)
    again, want = net(points.cuda()), fresh(points.cuda())
    assert torch.equal(again, want) and not torch.equal(again[:, :3], first[:, :3])
    for x, y in zip(ops.render_rays_composited(net, rays, z, False), ops.render_rays_composited(fresh, rays, z, False)):
        assert torch.equal(x, y)
