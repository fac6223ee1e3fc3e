"""Pins tests/ray_stages_ref.py without a device: the restatements of the sampler, the compositor and the resampler against
torch, the oracle and the committed fixtures; the exact-sum precondition of the resampler with exact rationals; and, for each
deliberately wrong restatement, that it changes the expected bits of at least one case tests/test_gpu_ray_stages.py runs."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as oc
from tests import ray_stages_ref as rs
from tests import train_heads_ref as hr
from tests.util import assert_resample_close

f32 = np.float32


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


# ------------------------------------------------------------------------------------------------------------------------
# linspace and the sampler
# ------------------------------------------------------------------------------------------------------------------------
def test_linspace01_equals_torch_linspace():
    """the single-rounding upper half is torch.linspace(0, 1, n) in every bit for n = 1..600; the two-rounding form the kernel
    held before is not (one ulp off on some entries of most n)"""
    off_n, off_64 = 0, None
    for n in range(1, 601):
        want = torch.linspace(0, 1, n).numpy()
        assert rs.same_bits(rs.linspace01(n), want), n
        bad = int((rs.bits(rs.linspace01(n, two_rounding=True)) != rs.bits(want)).sum())
        off_n += bad > 0
        if n == 64:
            off_64 = bad
    print(f"two-rounding form: differs from torch.linspace for {off_n} of the n in 1..600, {off_64} entries at n = 64")
    assert off_n > 0 and off_64 > 0


@pytest.mark.parametrize("name", ("path_llff", "path_blender"))
def test_sampler_restatement_equals_fixture_z_coarse(golden_dir, name):
    g = _golden(golden_dir, name)
    z, _ = rs.sample_numpy(g["rays"], 64, False)
    assert rs.same_bits(z, g["z_coarse"])
    z2, _ = rs.sample_numpy(g["rays"], 64, False, wrong="two_rounding_linspace")
    assert not rs.same_bits(z2, g["z_coarse"])


def edge_rays(R):
    rays = np.zeros((R, 8), dtype=f32)
    rays[:, 5], rays[:, 6], rays[:, 7] = -1.0, 2.0, 6.0
    return rays


def test_sampler_restatement_on_the_edge_fixture(golden_dir):
    """z_coarse_rand and z_coarse_lindisp of edge_cases.npz: which of them the restatement reproduces bit for bit (the GPU file
    asks the device for the same)"""
    e = _golden(golden_dir, "edge_cases")
    rays = edge_rays(e["z"].shape[0])
    zr, _ = rs.sample_numpy(rays, 64, False, u=e["u_coarse"])
    zl, _ = rs.sample_numpy(rays, 64, True)
    for key, got in (("z_coarse_rand", zr), ("z_coarse_lindisp", zl)):
        n = int((rs.bits(got) != rs.bits(e[key])).sum())
        err = float(np.abs(got.astype(np.float64) - e[key]).max())
        print(f"{key}: {n} of {got.size} entries differ from the restatement, max abs {err:.2e}")
        assert rs.EDGE_FIXTURE_BIT_EQUAL[key] == (n == 0)
        assert err <= 2e-6                                     # the tolerance tests/test_gpu_parity.py holds the device to


@pytest.mark.parametrize("lindisp", (False, True))
def test_sampler_restatement_against_the_oracle(lindisp):
    rays = rs.sampler_rays(5, 8)
    t = [torch.from_numpy(rays[:, a:b].astype(np.float64)) for a, b in ((0, 3), (3, 6), (6, 7), (7, 8))]
    for N in rs.SAMPLER_N:
        for u in (None, rs.sampler_u(5, N)):
            z, pts = rs.sample_numpy(rays, N, lindisp, u)
            zo, po = oc.sample_coarse(*t, N, lindisp, None if u is None else torch.from_numpy(u.astype(np.float64)))
            assert np.abs(z - zo.numpy()).max() <= 8 * hr.U * np.abs(zo.numpy()).max()
            assert np.abs(pts - po.numpy()).max() <= 16 * hr.U * max(1.0, np.abs(po.numpy()).max())


def test_sampler_wrong_restatements_show():
    for what in rs.SAMPLER_WRONG:
        hit = 0
        for N in rs.SAMPLER_N:
            for R in rs.SAMPLER_R:
                for lindisp in (False, True):
                    rays = rs.sampler_rays(R, 8)
                    u = rs.sampler_u(R, N) if what == "midpoint_form" else None
                    hit += not rs.same_bits(rs.sample_numpy(rays, N, lindisp, u)[0], rs.sample_numpy(rays, N, lindisp, u, wrong=what)[0])
        print(f"sampler {what}: expected bits change in {hit} cases")
        assert hit > 0, what


# ------------------------------------------------------------------------------------------------------------------------
# compositor
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", rs.COMPOSITE_N)
def test_composite_emulation_within_the_derived_bound(N):
    """libm exp rounded to fp32 supplies alpha; the emulation of everything behind it stays inside the bound derived by
    train_heads_ref's rules against oracle.composite in float64"""
    R = 5
    rgb4, sigma, z = rs.composite_inputs(R, N)
    worst = {}
    for flags in rs.COMPOSITE_FLAGS:
        alpha = rs.alpha_libm(sigma, z, flags)
        got = dict(zip(("comp_rgb", "depth", "opacity", "weights"), rs.emulate_composite(rgb4, sigma, z, flags, alpha)))
        got["alpha"] = alpha
        t = [torch.from_numpy(a.astype(np.float64)) for a in (rgb4[:, :, :3], sigma, z)]
        want = dict(zip(("comp_rgb", "depth", "opacity", "weights"),
                        oc.composite(*t, bool(flags & rs.WHITE), "softplus" if flags & rs.SOFTPLUS else "relu")))
        bounds = rs.composite_output_bounds(rgb4, sigma, z, flags)
        for name in ("alpha", "weights", "opacity", "depth", "comp_rgb"):
            val, E = bounds[name]
            if name in want and N > 1:                         # the bound's own fp64 value against the oracle's (which builds the
                                                               # last delta from an empty slice at N = 1 and returns no sample)
                ref = want[name].numpy()
                assert np.abs(val - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), name
            err = np.abs(got[name].astype(np.float64) - val)
            assert (err <= E).all(), (N, flags, name, float((err / E).max()))
            nz = E > 0
            worst[name] = max(worst.get(name, 0.0), float((err[nz] / E[nz]).max()))
    print(f"N {N:3d}: largest emulated err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def all_composite_cases():
    """(R, N, flags) of tests/test_gpu_ray_stages.py::test_composite_bit_for_bit"""
    for N in rs.COMPOSITE_N:
        for R in rs.COMPOSITE_R:
            for flags in rs.COMPOSITE_FLAGS:
                yield R, N, flags


def test_composite_wrong_restatements_show():
    """each wrong restatement changes the expected bits of at least one case of the GPU file (alpha: libm's stand-in).  The
    product order shows on the planted ray of product_order_case alone: everywhere else the two associations round to the same
    fp32 transmittance."""
    hits = dict.fromkeys(rs.COMPOSITE_WRONG, 0)
    for R, N, flags in all_composite_cases():
        if R not in (1, 5):
            continue                                           # two of the four ray counts: the rest repeat the same kinds of ray
        rgb4, sigma, z = rs.composite_inputs(R, N)
        good = rs.emulate_composite(rgb4, sigma, z, flags, rs.alpha_libm(sigma, z, flags))
        for what in rs.COMPOSITE_WRONG:
            alpha = rs.alpha_libm(sigma, z, flags, wrong=what if what in ("last_delta_from_z", "lane_boundary_delta") else None)
            bad = rs.emulate_composite(rgb4, sigma, z, flags, alpha, wrong=what)
            hits[what] += not all(rs.same_bits(a, b) for a, b in zip(good, bad))
    rgb4, sigma, z = rs.product_order_case()
    alpha = rs.alpha_libm(sigma, z, 0)
    hits["sequential_product"] += not rs.same_bits(rs.emulate_composite(rgb4, sigma, z, 0, alpha)[3],
                                                   rs.emulate_composite(rgb4, sigma, z, 0, alpha, wrong="sequential_product")[3])
    print("compositor, cases whose expected bits change: " + ", ".join(f"{k} {v}" for k, v in hits.items()))
    for what, n in hits.items():
        assert n > 0, what


def test_probe_inputs_state_the_case():
    rgb4, sigma, z = rs.composite_inputs(5, 65)
    prgb, ps, pz = rs.probe_inputs(sigma, z)
    assert prgb.shape == (325, 2, 3) and ps.shape == pz.shape == (325, 2)
    assert rs.same_bits(rs.composite_deltas(pz)[:, 0], rs.composite_deltas(z).reshape(-1)) and (pz[64::65, 1] == f32(1e10)).all()
    # behind the probe's alpha the emulation returns that alpha as the first weight
    a = rs.alpha_libm(ps, pz, 0)
    assert rs.same_bits(rs.emulate_composite(prgb, ps, pz, 0, a)[3][:, 0], rs.alpha_libm(sigma, z, 0).reshape(-1))


# ------------------------------------------------------------------------------------------------------------------------
# resampler
# ------------------------------------------------------------------------------------------------------------------------
def _kernel_order_sums(terms):
    """the normaliser and the cdf in resample_kernel's own orders, in exact rationals and in fp64: lane-strided partial sums and
    the xor butterfly; Hillis-Steele scans of 64-lane segments with the carry.  -> (all fp64 results equal the rationals)"""
    n = len(terms)
    ok = True
    for typ in (Fraction, float):
        t = [typ(float(v)) for v in terms]
        part = [typ(0)] * 64
        for j in range(n):
            part[j % 64] = part[j % 64] + t[j]
        o = 32
        while o:
            part = [part[l] + part[l ^ o] for l in range(64)]
            o >>= 1
        cdf, carry = [], typ(0)
        for seg in range(0, n, 64):
            v = [t[seg + l] if seg + l < n else typ(0) for l in range(64)]
            o = 1
            while o < 64:
                v = [v[l] + v[l - o] if l >= o else v[l] for l in range(64)]
                o <<= 1
            v = [x + carry for x in v]
            cdf += v[:min(64, n - seg)]
            carry = v[63]
        if typ is Fraction:
            exact = (part[0], cdf)
        else:
            ok = all(Fraction(p) == exact[0] for p in part) and all(Fraction(a) == b for a, b in zip(cdf, exact[1]))
    return ok


@pytest.mark.parametrize("Nc", (3, 66, 130, 256))
def test_resampler_sums_are_exact_in_fp64(Nc):
    """the precondition of the bit-for-bit claim: for weights in [0, 1] and Nc <= 256 every fp64 partial sum of fl(w + 1e-5f) and
    of the pdf is exact (terms >= 2^-17 resp. 2^-25 as fp32, at most 254 of them: under 50 bits), checked with exact rationals in
    the kernel's own summation orders; and sums_are_exact, the cheap criterion asserted on every case, agrees"""
    z, w = rs.resample_case(9, Nc)
    w[6] = 1.0                                                  # the largest total
    w[7, 1:-1] = np.nextafter(f32(1.0), f32(0.0))
    t = (w[:, 1:-1] + rs.EPS).astype(f32)
    wsum = t.astype(np.float64).sum(1).astype(f32)
    pdf = (t / wsum[:, None]).astype(f32)
    assert t.min() >= 2.0 ** -17 and pdf.min() >= 2.0 ** -25
    for r in range(9):
        assert _kernel_order_sums(t[r]) and _kernel_order_sums(pdf[r]), r
    assert rs.sums_are_exact(t) and rs.sums_are_exact(pdf)
    # ... and the criterion does refuse what is not exact
    assert not rs.sums_are_exact(np.array([1.0, 2.0 ** -60]))
    assert not rs.sums_are_exact(np.array([f32(1e30), f32(1e-5)], dtype=f32))
    assert not _kernel_order_sums([1.0, 2.0 ** -60, 1.0])


def all_resample_cases():
    """(R, Nc, Ni, given u?) of tests/test_gpu_ray_stages.py::test_resample_bit_for_bit"""
    for Nc in rs.RESAMPLE_NC:
        for Ni in rs.RESAMPLE_NI:
            for R in rs.RESAMPLE_R:
                for with_u in (False, True):
                    yield R, Nc, Ni, with_u


def resample_case_inputs(R, Nc, Ni, with_u):
    z, w = rs.resample_case(R, Nc, seed=Ni % rs.RS_KINDS)                # the seed rotates the planted kinds through the ray slots
    return z, w, (rs.resample_u(z, w, Ni) if with_u else None)


def test_resample_restatement_against_the_oracle():
    for R, Nc, Ni, with_u in all_resample_cases():
        if R != 5:
            continue
        z, w, u = resample_case_inputs(R, Nc, Ni, with_u)
        got, _ = rs.resample_numpy(z, w, Ni, u)
        assert (np.diff(got, axis=1) >= 0).all()
        zero3 = torch.zeros(R, 3)
        want, _ = oc.resample_fine(zero3, zero3, torch.from_numpy(z), torch.from_numpy(w), Ni, None if u is None else torch.from_numpy(u))
        assert_resample_close(got, want, z, w, Ni, u=u)


@pytest.mark.parametrize("name,at_least", (("path_llff", 150), ("path_blender", 119)))
def test_resample_restatement_on_the_path_fixtures(golden_dir, name, at_least):
    """rays of the fixture whose z_fine the restatement reproduces in every bit (the rest: one ulp of torch's fp32 order in
    w.sum); with the two-rounding linspace almost none"""
    g = _golden(golden_dir, name)
    got, _ = rs.resample_numpy(g["z_coarse"], g["coarse_weights"], 64)
    equal = int((rs.bits(got) == rs.bits(g["z_fine"])).all(1).sum())
    print(f"{name}: z_fine bit-equal on {equal} of {got.shape[0]} rays")
    assert equal >= at_least
    assert_resample_close(got, g["z_fine"], g["z_coarse"], g["coarse_weights"], 64)


def test_resample_planted_rays_fill_every_slot():
    """the ray with repeated depths: every value of [z, z_new] lands in the output exactly once"""
    for Nc, Ni in ((66, 64), (256, 256), (4, 1)):
        z, w = rs.resample_case(9, Nc)
        got, _ = rs.resample_numpy(z, w, Ni)
        assert len(np.unique(z[rs.RS_TIES])) <= (Nc + 2) // 3
        for r in range(9):
            assert np.isfinite(got[r]).all() and (np.diff(got[r]) >= 0).all()
            vals, counts = np.unique(z[r], return_counts=True)
            assert all((got[r] == v).sum() >= c for v, c in zip(vals, counts))


def test_resample_wrong_restatements_show():
    hits = dict.fromkeys(rs.RESAMPLE_WRONG, 0)
    for R, Nc, Ni, with_u in all_resample_cases():
        if R != 5:
            continue
        z, w, u = resample_case_inputs(R, Nc, Ni, with_u)
        good, _ = rs.resample_numpy(z, w, Ni, u)
        for what in rs.RESAMPLE_WRONG:
            hits[what] += not rs.same_bits(good, rs.resample_numpy(z, w, Ni, u, wrong=what, require_exact=False)[0])
    print("resampler, cases whose expected bits change: " + ", ".join(f"{k} {v}" for k, v in hits.items()))
    for what, n in hits.items():
        assert n > 0, what


# ------------------------------------------------------------------------------------------------------------------------
# s^2 mean, un-flatten
# ------------------------------------------------------------------------------------------------------------------------
def test_sr_mean_and_unflatten_restatements(golden_dir):
    g = _golden(golden_dir, "path_llff")
    assert np.abs(rs.sr_mean_numpy(g["fine_comp_rgbs"], 64, 4, 3) - g["lr_fine_rgb_s2"]).max() <= 2 * hr.U
    for H, W, s, c in ((8, 16, 2, 3), (12, 20, 4, 1), (5, 7, 1, 4)):
        x = np.arange(H * W * c, dtype=f32).reshape(-1, c)
        assert rs.same_bits(rs.unflatten_numpy(x, H, W, s, c), oc.unflatten_hr(torch.from_numpy(x), H, W, s).numpy())
    # the order shows: pairwise summation of the same data differs from the left-to-right sum
    d = rs.sr_mean_data(85, 16, 3).reshape(85, 16, 3)
    pair = d
    while pair.shape[1] > 1:
        pair = (pair[:, 0::2] + pair[:, 1::2]).astype(f32)
    assert not rs.same_bits((pair[:, 0] / f32(16)).astype(f32), rs.sr_mean_numpy(d, 85, 16, 3))
