"""Unit layer over the ray-side forward stages, bit for bit: sample_kernel, sr_mean_kernel, unflatten_kernel
(csrc/nsr_rays.hip), composite_kernel<K> and resample_kernel (csrc/nsr_render.hip), each launched on its own through its exported
entry point (nerf_sr_amd/_lib.py), with the arguments nerf_sr_amd.ops does not expose: ray stride 11, rgb / sigma strides, null
outputs.  Restatements and inputs: tests/ray_stages_ref.py, itself pinned on the CPU by tests/test_ray_stages_cpu.py.

Every output buffer is NaN-filled with a guard region behind it that must survive, no NaN may remain in the written region, and
every element of every output is compared in every bit.  The only inexact calls on these paths are the compositor's expf and
softplus logf / expf, all inside alpha: a probe launch reads the device's alpha of every sample (ray_stages_ref.probe_inputs),
which is (a) held to the bound train_heads_ref.forward_bounds derives against the fp64 value, and (b) fed to the emulation of
everything behind it, which the device must equal in every bit.  Lines starting RAY_STAGES_RECORD (run with -s) are the figures
of profiles/ray_stages_units.json."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib as nsr_lib
from tests import ray_stages_ref as rs

pytestmark = pytest.mark.gpu

GUARD = 1024                    # elements behind every output region
f32 = np.float32
OUTPUTS = ("comp_rgb", "depth", "opacity", "weights")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return nsr_lib.load()       # raises if libnsr.so is missing: no fallback


def record(**kw):
    print("RAY_STAGES_RECORD " + json.dumps(kw, sort_keys=True))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t, offset_elems=0):
    return None if t is None else t.data_ptr() + offset_elems * t.element_size()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def out_buf(n):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")


def take(buf, shape, what, written=True):
    """the written region of an output buffer as a host array; asserts the guard behind it and that every element was written
    (written=False: that none was)"""
    if buf is None:
        return None
    a = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert a.size == n + GUARD
    assert np.isnan(a[n:]).all(), f"floats behind {what} were written"
    if written:
        assert not np.isnan(a[:n]).any(), f"{what}: {int(np.isnan(a[:n]).sum())} elements were not written (or are NaN)"
    else:
        assert np.isnan(a[:n]).all(), f"a refused call wrote {what}"
    return a[:n].reshape(shape).copy()


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == f32, what
    bad = rs.bits(got) != rs.bits(want)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in their bits; first at {i}: device "
                             f"{got[i]!r} ({rs.bits(got)[i]:#010x}) restatement {want[i]!r} ({rs.bits(want)[i]:#010x})")


# ------------------------------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------------------------------
def run_sample(lib, rays, N, lindisp, u, with_pts, expect=rs.NSR_OK):
    R, stride = rays.shape
    d_rays, d_u = dev(rays), dev(u)
    z, pts = out_buf(R * N), out_buf(R * N * 3) if with_pts else None
    rc = lib.nsr_sample_along_rays(ptr(d_rays), stride, R, N, int(lindisp), ptr(d_u), ptr(z), ptr(pts), stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    ok = rc == rs.NSR_OK
    return take(z, (R, N), "z", ok), take(pts, (R, N, 3), "pts", ok)


@pytest.mark.parametrize("N", rs.SAMPLER_N)
@pytest.mark.parametrize("R", rs.SAMPLER_R)
def test_sample_bit_for_bit(lib, R, N):
    """R N on both sides of a 256-thread block; lindisp off / on; u null / given (0, the largest fp32 below 1, random); pts null /
    non-null; ray stride 8 / 11 (columns 8..10 NaN: never read into a result)"""
    for stride in (8, 11):
        rays = rs.sampler_rays(R, stride)
        for lindisp in (False, True):
            for u in (None, rs.sampler_u(R, N)):
                want_z, want_pts = rs.sample_numpy(rays, N, lindisp, u)
                for with_pts in (True, False):
                    z, pts = run_sample(lib, rays, N, lindisp, u, with_pts)
                    what = f"stride {stride} lindisp {lindisp} u {'given' if u is not None else 'null'}"
                    assert_bits(z, want_z, "z, " + what)
                    if with_pts:
                        assert_bits(pts, want_pts, "pts, " + what)


def test_sample_near_equals_far(lib):
    for N in (1, 3, 65):
        rays = rs.sampler_rays(5, 8, near_eq_far=True)
        for lindisp in (False, True):
            for u in (None, rs.sampler_u(5, N)):
                want_z, want_pts = rs.sample_numpy(rays, N, lindisp, u)
                z, pts = run_sample(lib, rays, N, lindisp, u, True)
                assert_bits(z, want_z, f"z N {N} lindisp {lindisp}")
                assert_bits(pts, want_pts, f"pts N {N} lindisp {lindisp}")
                if not lindisp:          # at most 8 roundings between near and any depth (4 in nsr_coarse_z, 4 in the jitter)
                    assert (np.abs(z - rays[:, 6:7]) <= 8 * rs.hr.U * rays[:, 6:7]).all()


def test_sample_equals_the_fixtures(lib, golden_dir):
    """z_coarse of both path fixtures, z_coarse_rand and z_coarse_lindisp of the edge fixture: every bit (the restatement
    reproduces all four on the CPU, tests/test_ray_stages_cpu.py)"""
    counts = {}
    for name in ("path_llff", "path_blender"):
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        z, _ = run_sample(lib, g["rays"], 64, False, None, False)
        counts[name + ":z_coarse"] = [int((rs.bits(z) == rs.bits(g["z_coarse"])).sum()), int(z.size)]
        assert_bits(z, g["z_coarse"], name + " z_coarse")
    e = np.load(os.path.join(golden_dir, "edge_cases.npz"))
    rays = np.zeros((e["z"].shape[0], 8), dtype=f32)
    rays[:, 5], rays[:, 6], rays[:, 7] = -1.0, 2.0, 6.0
    zr, _ = run_sample(lib, rays, 64, False, e["u_coarse"], False)
    zl, _ = run_sample(lib, rays, 64, True, None, False)
    for key, z in (("z_coarse_rand", zr), ("z_coarse_lindisp", zl)):
        counts["edge_cases:" + key] = [int((rs.bits(z) == rs.bits(e[key])).sum()), int(z.size)]
        assert rs.EDGE_FIXTURE_BIT_EQUAL[key]
        assert_bits(z, e[key], key)
    record(test="sample_fixtures", bit_equal_entries=counts)


# ------------------------------------------------------------------------------------------------------------------------
# compositor
# ------------------------------------------------------------------------------------------------------------------------
def run_composite(lib, rgb4, sigma, z, flags, strides=(4, 1), null=None, expect=rs.NSR_OK, n_samples=None):
    """one launch of nsr_composite -> dict of the four outputs (None where `null` names it).  rgb4 (R, N, 4) with NaN in column
    3; strides: (3, 1) packed colours, (4, 1) the NaN column in between, (4, 4) one interleaved (R, N, 4) buffer with sigma in
    column 3"""
    R, N = sigma.shape
    if strides == (4, 4):
        inter = rgb4.copy()
        inter[:, :, 3] = sigma
        d_rgb = dev(inter)
        p_rgb, p_sigma = ptr(d_rgb), ptr(d_rgb, 3)
    else:
        d_rgb, d_sigma = dev(rgb4 if strides[0] == 4 else rgb4[:, :, :3]), dev(sigma)
        p_rgb, p_sigma = ptr(d_rgb), ptr(d_sigma)
    d_z = dev(z)
    shapes = {"comp_rgb": (R, 3), "depth": (R,), "opacity": (R,), "weights": (R, N)}
    bufs = {k: (None if k == null else out_buf(int(np.prod(s)))) for k, s in shapes.items()}
    rc = lib.nsr_composite(p_rgb, strides[0], p_sigma, strides[1], ptr(d_z), R, N if n_samples is None else n_samples, flags,
                           *[ptr(bufs[k]) for k in OUTPUTS], stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    return {k: take(bufs[k], shapes[k], k, rc == rs.NSR_OK) for k in OUTPUTS}


def probe_alpha(lib, sigma, z, flags):
    """the device's alpha of every sample of the case, by the probe launch (same flag word)"""
    prgb, ps, pz = rs.probe_inputs(sigma, z)
    P = ps.shape[0]
    d = [dev(a) for a in (prgb, ps, pz)]
    w = out_buf(P * 2)
    rc = lib.nsr_composite(ptr(d[0]), 3, ptr(d[1]), 1, ptr(d[2]), P, 2, flags, None, None, None, ptr(w), stream())
    assert rc == rs.NSR_OK, rc
    torch.cuda.synchronize()
    return np.ascontiguousarray(take(w, (P, 2), "probe weights")[:, 0]).reshape(sigma.shape)


def check_alpha(alpha, rgb4, sigma, z, flags):
    """(a): the probed alpha within the derived bound of its fp64 value -> largest err / bound"""
    val, E = rs.composite_output_bounds(rgb4, sigma, z, flags)["alpha"]
    err = np.abs(alpha.astype(np.float64) - val)
    nz = E > 0
    ratio = float((err[nz] / E[nz]).max())
    assert (err <= E).all(), f"alpha outside the derived bound: largest err / bound {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("N", rs.COMPOSITE_N)
def test_composite_bit_for_bit(lib, N):
    """every R of COMPOSITE_R x every flag word x the three stride forms; with R = 5 each of the four outputs null in turn"""
    ratios = {}
    for R in rs.COMPOSITE_R:
        rgb4, sigma, z = rs.composite_inputs(R, N)
        for flags in rs.COMPOSITE_FLAGS:
            alpha = probe_alpha(lib, sigma, z, flags)
            name = rs.hr.flag_name(flags)
            ratios[name] = max(ratios.get(name, 0.0), check_alpha(alpha, rgb4, sigma, z, flags))
            want = dict(zip(OUTPUTS, rs.emulate_composite(rgb4, sigma, z, flags, alpha)))
            for strides in ((3, 1), (4, 1), (4, 4)):
                got = run_composite(lib, rgb4, sigma, z, flags, strides)
                for k in OUTPUTS:
                    assert_bits(got[k], want[k], f"{k}, R {R} N {N} {name} strides {strides}")
            if R == 5:
                for null in OUTPUTS:
                    got = run_composite(lib, rgb4, sigma, z, flags, (4, 1), null=null)
                    for k in OUTPUTS:
                        if k != null:
                            assert_bits(got[k], want[k], f"{k} with {null} null, R {R} N {N} {name}")
    record(test="composite", N=N, K=rs.lanes_K(N), alpha_err_over_bound=ratios)


def test_composite_product_order_ray(lib):
    """the ray on which the association of the fp64 transmittance product would show in fp32 (ray_stages_ref.product_order_case)"""
    rgb4, sigma, z = rs.product_order_case()
    for flags in (0, rs.WHITE):
        alpha = probe_alpha(lib, sigma, z, flags)
        ratio = check_alpha(alpha, rgb4, sigma, z, flags)
        want = dict(zip(OUTPUTS, rs.emulate_composite(rgb4, sigma, z, flags, alpha)))
        got = run_composite(lib, rgb4, sigma, z, flags, (4, 1))
        for k in OUTPUTS:
            assert_bits(got[k], want[k], f"{k}, product-order ray, flags {flags}")
    seq = rs.emulate_composite(rgb4, sigma, z, 0, alpha, wrong="sequential_product")[3]
    record(test="composite_product_order", alpha_err_over_bound=ratio,
           sequential_product_would_differ_with_device_alpha=not rs.same_bits(seq, want["weights"]))


def test_composite_return_codes(lib):
    rgb4, sigma, z = rs.composite_inputs(4, 64)
    run_composite(lib, rgb4, sigma, z, 0, expect=rs.NSR_ERR_UNSUPPORTED, n_samples=513)
    run_composite(lib, rgb4, sigma, z, 0, expect=rs.NSR_ERR_INVALID_ARG, n_samples=0)
    for flags in (4, 8, -1, rs.WHITE | 4):
        run_composite(lib, rgb4, sigma, z, flags, expect=rs.NSR_ERR_INVALID_ARG)


# ------------------------------------------------------------------------------------------------------------------------
# resampler
# ------------------------------------------------------------------------------------------------------------------------
def run_resample(lib, rays, z, w, Ni, u, with_pts, expect=rs.NSR_OK, n_coarse=None):
    R, Nc = z.shape
    M = Nc + Ni
    d = [dev(a) for a in (rays, z, w, u)]
    z_out, pts = out_buf(R * M), out_buf(R * M * 3) if with_pts else None
    rc = lib.nsr_resample_along_rays(ptr(d[0]), rays.shape[1], ptr(d[1]), ptr(d[2]), R, Nc if n_coarse is None else n_coarse, Ni,
                                     ptr(d[3]), ptr(z_out), ptr(pts), stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    ok = rc == rs.NSR_OK
    return take(z_out, (R, M), "z_out", ok), take(pts, (R, M, 3), "pts", ok)


def resample_case_inputs(R, Nc, Ni, with_u):
    """as tests/test_ray_stages_cpu.py: the seed rotates the planted kinds of ray through the ray slots"""
    z, w = rs.resample_case(R, Nc, seed=Ni % rs.RS_KINDS)
    return z, w, (rs.resample_u(z, w, Ni) if with_u else None)


@pytest.mark.parametrize("Nc", rs.RESAMPLE_NC)
def test_resample_bit_for_bit(lib, Nc):
    """every Ni x R x (u null, u given with 0, 1, cdf entries, a value above the last cdf entry) as ray stride 8 with pts, ray
    stride 11 with pts and pts null.  No conditioning allowance: rays on the snap included.  The exact-sum precondition is
    asserted on every case (resample_numpy), and a ray's output being the restatement's in every bit with no NaN left is every
    value of [z, z_new] in exactly one slot."""
    for Ni in rs.RESAMPLE_NI:
        for R in rs.RESAMPLE_R:
            for with_u in (False, True):
                z, w, u = resample_case_inputs(R, Nc, Ni, with_u)
                for stride, with_pts in ((8, True), (11, True), (8, False)):
                    rays = rs.sampler_rays(R, stride, seed=Nc)
                    want_z, want_pts = rs.resample_numpy(z, w, Ni, u, rays)
                    got_z, got_pts = run_resample(lib, rays, z, w, Ni, u, with_pts)
                    what = f"Nc {Nc} Ni {Ni} R {R} u {'given' if with_u else 'null'} stride {stride}"
                    assert_bits(got_z, want_z, "z_out, " + what)
                    if with_pts:
                        assert_bits(got_pts, want_pts, "pts, " + what)


def test_resample_on_the_path_fixtures(lib, golden_dir):
    """the device equals the restatement on the fixtures' coarse weights in every bit, and so reproduces the same rays of the
    fixtures' z_fine (the rest: one ulp of torch's fp32 order in w.sum)"""
    counts = {}
    for name, at_least in (("path_llff", 150), ("path_blender", 119)):
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        want, _ = rs.resample_numpy(g["z_coarse"], g["coarse_weights"], 64)
        got, _ = run_resample(lib, g["rays"], g["z_coarse"], g["coarse_weights"], 64, None, False)
        assert_bits(got, want, name)
        counts[name] = [int((rs.bits(got) == rs.bits(g["z_fine"])).all(1).sum()), int(got.shape[0])]
        assert counts[name][0] >= at_least
    record(test="resample_fixtures", bit_equal_rays=counts)


def test_resample_return_codes(lib):
    rays = rs.sampler_rays(4, 8)
    z, w = rs.resample_case(4, 256)
    run_resample(lib, rays, z, w, 64, None, True, expect=rs.NSR_ERR_INVALID_ARG, n_coarse=2)
    run_resample(lib, rays, z, w, 64, None, True, expect=rs.NSR_ERR_UNSUPPORTED, n_coarse=257)
    run_resample(lib, rays, z, w, 257, None, True, expect=rs.NSR_ERR_UNSUPPORTED)


# ------------------------------------------------------------------------------------------------------------------------
# s^2 mean, un-flatten
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s2", (1, 4, 16))
def test_sr_mean_bit_for_bit(lib, s2):
    for c in (1, 3, 4):
        for n_lr in (1, 85, 257):
            x = rs.sr_mean_data(n_lr, s2, c)
            d_x, out = dev(x), out_buf(n_lr * c)
            assert lib.nsr_sr_mean(ptr(d_x), n_lr, s2, c, ptr(out), stream()) == rs.NSR_OK
            torch.cuda.synchronize()
            assert_bits(take(out, (n_lr, c), "lr"), rs.sr_mean_numpy(x, n_lr, s2, c), f"s2 {s2} c {c} n_lr {n_lr}")


@pytest.mark.parametrize("s", (1, 2, 4))
def test_unflatten_is_the_permutation(lib, s):
    for H, W in ((3 * s, 5 * s), (7 * s, 11 * s), (20, 12)):
        for c in (1, 3, 4):
            assert (H * W * c) % 256 != 0
            x = np.arange(1, H * W * c + 1, dtype=f32).reshape(-1, c)        # every element its own value
            d_x, out = dev(x), out_buf(H * W * c)
            assert lib.nsr_unflatten(ptr(d_x), H, W, s, c, ptr(out), stream()) == rs.NSR_OK
            torch.cuda.synchronize()
            assert_bits(take(out, (H, W, c), "hr"), rs.unflatten_numpy(x, H, W, s, c), f"s {s} H {H} W {W} c {c}")
