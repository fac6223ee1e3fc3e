"""The numpy restatement of the in-kernel positional encodings (tests/encoding_ref.py), proven without a device:

* ``fma32`` is a correctly rounded fp32 fused multiply-add: equal to exact rational arithmetic on 1e5 random triples
  (cancelling ones included) and on constructed triples whose float64 sum lands exactly on an fp32 rounding midpoint, where a
  float64 ``a * b + c`` cast to fp32 is wrong;
* the constants are the header's, rounded once;
* the restated ``nsr_sincos`` stays within the header's own bound, 1.5e-7 absolute, of float64 sin / cos on every argument set
  of the device test that lies in the claimed range; ``nsr_sincos(+-0)`` is exactly (+0, 1);
* the encoded rows stay within the same bound of ``oracle.posenc`` in float64;
* teeth: each wrong variant of the encoder changes expected bits on the GPU test's own rays;
* the one-hot networks: the construction rules, the expected value per precision, and that on the GPU test's rays every
  sin / cos column takes both signs and at least 32 distinct values.

The figures (largest error per set, elements changed per variant) are recorded in profiles/encoding_units.json; the record is
checked against a fresh computation here."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as oc
from tests import encoding_ref as enc
from tests import mlp_exact_ref as er

F32 = np.float32
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "encoding_units.json")


def _round_f32(q: Fraction) -> float:
    """The fp32 nearest to the rational q, ties to even, subnormals included (no overflow in the cases below)."""
    if q == 0:
        return 0.0
    n, d = abs(q.numerator), q.denominator
    e = n.bit_length() - d.bit_length()
    if Fraction(n, d) < Fraction(2) ** e:
        e -= 1                                               # 2^e <= |q| < 2^(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    return float(round(q / quantum) * quantum)               # round(): half to even; the product is exact in float64


def _exact_fma(a, b, c):
    return np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], dtype=F32)


def _same(got, want):
    """Bit equality; an exact zero may carry either sign in the rational reference."""
    return np.array_equal(enc.bits(got), enc.bits(want)) or \
        (np.array_equal(got, want) and bool(np.all((enc.bits(got) == enc.bits(want)) | (want == 0))))


def test_fma32_is_correctly_rounded_on_random_triples():
    rng = np.random.Generator(np.random.PCG64([21]))
    n = 100_000
    a = (rng.uniform(1, 2, n) * np.exp2(rng.integers(-30, 30, n)) * rng.choice([-1, 1], n)).astype(F32)
    b = (rng.uniform(1, 2, n) * np.exp2(rng.integers(-30, 30, n)) * rng.choice([-1, 1], n)).astype(F32)
    c = (rng.uniform(1, 2, n) * np.exp2(rng.integers(-60, 60, n)) * rng.choice([-1, 1], n)).astype(F32)
    # a third cancel almost entirely (c = -fl(a b) moved by a few ulps), a third land in the subnormals
    third = n // 3
    near = -(a[:third].astype(np.float64) * b[:third].astype(np.float64)).astype(F32)
    for _ in range(3):
        near = np.where(rng.random(third) < 0.5, np.nextafter(near, F32(np.inf)), near)
    c[:third] = near
    a[third:2 * third] = (rng.uniform(1, 2, third) * 2.0 ** -70).astype(F32)
    b[third:2 * third] = (rng.uniform(1, 2, third) * np.exp2(rng.integers(-62, -54, third)) * rng.choice([-1, 1], third)).astype(F32)
    c[third:2 * third] = (rng.uniform(-1, 1, third) * 2.0 ** -128).astype(F32)
    got, want = enc.fma32(a, b, c), _exact_fma(a, b, c)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], a[bad[:5]], b[bad[:5]], c[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert (np.abs(want[third:2 * third]) < 2.0 ** -126).sum() > 1000      # the subnormal third is one


def test_fma32_on_float64_midpoints():
    """c has an odd last bit; a b = +-(half an ulp of c) (1 - 2^-46): the exact sum lies just inside the half-ulp, float64
    rounds it ONTO the midpoint, and the second rounding (ties to even) then leaves c -- the correctly rounded result."""
    rng = np.random.Generator(np.random.PCG64([22]))
    n = 4096
    c = ((rng.integers(1 << 23, 1 << 24, n) | 1).astype(np.float64) * np.exp2(rng.integers(-40, 40, n).astype(np.float64)))
    c = (c * rng.choice([-1.0, 1.0], n)).astype(F32)
    h = np.frexp(c.astype(np.float64))[1] - 25             # half an ulp of c is 2^h
    a = (np.exp2((h // 2).astype(np.float64)) * (1 + 2.0 ** -23)).astype(F32)
    b = (np.exp2((h - h // 2).astype(np.float64)) * (1 - 2.0 ** -23) * rng.choice([-1.0, 1.0], n)).astype(F32)
    exact = _exact_fma(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert _same(enc.fma32(a, b, c), exact)
    assert (naive != exact).sum() > n // 4, "the constructed cases do not reach a float64 midpoint"
    # the hand-made one of the docstring
    a1, b1, c1 = F32(2.0 ** -12 * (1 + 2.0 ** -23)), F32(2.0 ** -12 * (1 - 2.0 ** -23)), F32(1 + 2.0 ** -23)
    assert enc.fma32(a1, b1, c1) == c1 and F32(float(a1) * float(b1) + float(c1)) != c1


def test_constants_are_the_headers():
    """pi/2 = 0x3FC90FDA + 0x33A22168 + 0x27C234C4 (the comment in csrc/nsr_common.h), 2/pi to nearest."""
    assert [int(v.view(np.uint32)) for v in enc.PIO2] == [0x3FC90FDA, 0x33A22168, 0x27C234C4]
    assert enc.TWO_OVER_PI == F32(2 / np.pi)
    src = open(os.path.join(os.path.dirname(PROFILE), "..", "nerf_sr_amd", "csrc", "nsr_common.h")).read()
    for text in ("0.636619772367581343f", "-1.57079625129699707031f", "-7.54978941586159635335e-08f", "-5.39030252995776476554e-15f",
                 "-1.9515295891e-4f", "8.3321608736e-3f", "-1.6666654611e-1f", "2.443315711809948e-5f", "-1.388731625493765e-3f",
                 "4.166664568298827e-2f"):
        assert text in src, text
    # a float64 detour would give the same values here (so numpy's own parsing agrees with the single rounding)
    for text in ("1.57079625129699707031", "7.54978941586159635335e-08", "-1.9515295891e-4", "4.166664568298827e-2"):
        assert enc.f32_literal(text) == F32(float(text))


def test_sincos_within_the_headers_bound():
    errs = enc.sincos_errors()
    for name, e in errs.items():
        print(f"{name}: {enc.sincos_sets()[name].size} arguments, max abs error {e:.4e}")
    assert set(errs) == set(enc.ACCURACY_SETS) and all(e <= enc.SINCOS_BOUND for e in errs.values()), errs
    n = sum(v.size for v in enc.sincos_sets().values())
    assert 2_500_000 <= n <= 3_500_000
    sets = enc.sincos_sets()
    assert np.all(np.abs(sets["half_pi_multiples"]) < 2.0 ** 15 + 1) and (np.abs(sets["log_uniform"]) < 2.0 ** -126).sum() > 10_000
    assert np.all((np.abs(sets["beyond"]) >= 2.0 ** 15) & (np.abs(sets["beyond"]) < 2.0 ** 20))


def test_sincos_of_zero_and_nonfinite():
    sn, cs = enc.nsr_sincos(np.array([0.0, -0.0], dtype=F32))
    assert enc.bits(sn).tolist() == [0, 0] and enc.bits(cs).tolist() == [0x3F800000] * 2
    sn, cs = enc.nsr_sincos(enc.sincos_sets()["nonfinite"])
    assert np.isnan(sn).all() and np.isnan(cs).all()
    den = enc.sincos_sets()["special"][2:4]
    sn, cs = enc.nsr_sincos(den)
    assert np.array_equal(enc.bits(sn), enc.bits(den)) and np.all(cs == 1)        # sin x = x on a denormal: nothing flushed


def test_rows_against_the_oracle():
    """encode_rays against oracle.posenc in float64 on the float32 points and directions: the header's bound on every sin / cos
    column, the raw coordinates exact."""
    for rays, z in enc.ray_sets():
        rows = enc.encode_rays(rays, z)
        N = z.shape[1]
        v = torch.from_numpy(enc.cast_rays(rays, z)).double()
        d = torch.from_numpy(np.repeat(enc.view_direction(rays), N, 0)).double()
        want = torch.cat([oc.posenc(v, 10), oc.posenc(d, 4)], -1).numpy()
        assert rows.shape == want.shape == (rays.shape[0] * N, 90) and rows.dtype == F32
        err = np.abs(rows.astype(np.float64) - want)
        assert err.max() <= enc.SINCOS_BOUND, err.max()
        assert np.array_equal(rows[:, :3].astype(np.float64), want[:, :3]) and np.array_equal(rows[:, 63:66].astype(np.float64), want[:, 63:66])
    # cast_rays is two fp32 roundings, not one
    rays, z = enc.make_rays(5, 64, 8)
    one = (rays[:, None, 0:3].astype(np.float64) + z[:, :, None].astype(np.float64) * rays[:, None, 3:6]).astype(F32).reshape(-1, 3)
    assert (one != enc.cast_rays(rays, z)).any()


def test_planted_rays():
    for stride in enc.STRIDES:
        rays, z = enc.make_rays(5, 64, stride)
        v = enc.cast_rays(rays, z).reshape(5, 64, 3)
        d = enc.view_direction(rays)
        assert not rays[1, :6].any() and not d[1].any() and not v[1].any()                                      # o = d = 0
        assert np.array_equal(v[2, -1], [60.0, -60.0, -60.0]) and np.ldexp(60.0, 9) == 30720 and np.abs(v).max() < 64
        assert set(np.abs(rays[3, 0:6]).tolist()) == {0.0, float(enc.TINY)} and np.signbit(rays[3, 1]) and 0 < enc.TINY < 2.0 ** -126
        assert d[4].tolist() == [float(enc.PI_2), float(enc.PI_8), 1.0]
        assert np.all(np.diff(z, axis=1) >= 0) and z.min() >= 2 and z.max() <= 6
        if stride == 11:
            assert not np.array_equal(rays[:, 3:6], rays[:, 8:11])
        rays2, z2 = enc.make_rays(2, 128, stride)
        assert np.array_equal(enc.cast_rays(rays2, z2)[-1], [60.0, -60.0, -60.0])


def test_encode_arch_is_the_row_cut_and_padded():
    rays, z = enc.make_rays(5, 64, 11)
    rows = enc.encode_rays(rays, z)
    full = enc.encode_arch(rays, z, 64, 10, 0, 16)
    assert np.array_equal(enc.bits(full[:, :63]), enc.bits(rows[:, :63])) and not full[:, 63:].any()
    dirs = enc.encode_arch(rays, None, 64, 4, 1, 8)
    assert np.array_equal(enc.bits(dirs[:, :27]), enc.bits(rows[:, 63:])) and not dirs[:, 27:].any()
    assert np.array_equal(enc.encode_arch(rays, z, 64, 0, 0, 1)[:, :3], rows[:, :3])
    assert enc.encode_arch(rays, z, 64, 16, 0, 25).shape == (320, 100)


def test_every_wrong_variant_changes_expected_bits():
    counts = enc.teeth_counts()
    print(counts)
    assert tuple(counts) == enc.VARIANTS and len(counts) == 9 and all(n > 0 for n in counts.values()), counts
    # each variant is visible on EVERY shape and stride it can touch, not only in the sum
    for rays, z in enc.ray_sets():
        base = enc.bits(enc.encode_rays(rays, z))
        for v in enc.VARIANTS:
            if v == "view_from_d" and rays.shape[1] == 8:
                continue
            if v == "flush_denormal" and rays.shape[0] < 5:
                continue                                       # the denormal ray is planted from five rays up
            assert (enc.bits(enc.encode_rays(rays, z, variant=v)) != base).any(), (v, rays.shape, z.shape)


def test_profile_records_these_figures():
    with open(PROFILE) as f:
        doc = json.load(f)
    fresh = enc.cpu_figures()
    assert doc["cpu"]["teeth_expected_elements_changed"] == fresh["teeth_expected_elements_changed"]
    assert doc["cpu"]["arguments"] == fresh["arguments"]
    for name, e in fresh["nsr_sincos_max_abs_error"].items():
        assert doc["cpu"]["nsr_sincos_max_abs_error"][name] == pytest.approx(e, rel=1e-6)      # libm's sin / cos may differ in the last bit


# ---------------------------------------------------------------------------------------------------------------------
# one-hot networks
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_raw(sd, rows):
    sd_t = oc.to_torch_sd(sd, torch.float64)
    return oc.mlp_forward(sd_t, torch.from_numpy(rows).double(), color_activation="none").numpy()


def test_onehot_networks_follow_the_rules_and_cover_every_column():
    seen = {p: [] for p in enc.PLACES}
    reads = {"l1": ("xyz_encoding_1.0.weight", slice(0, 63)), "skip": ("xyz_encoding_5.0.weight", slice(0, 63)),
             "dir": ("dir_encoding.0.weight", slice(256, 283))}
    for place in enc.PLACES:
        nets = enc.onehot_networks(place)
        assert len(nets) == {"l1": 15, "skip": 15, "dir": 8}[place]
        for name, sd, taps in nets:
            assert all(not sd[k].any() for k in sd if k.endswith(".bias"))
            for key, cols in reads.values():
                w = sd[key][:, cols]
                assert ((w != 0).sum(1) <= 1).all() and set(np.unique(w)) <= {-1.0, 0.0, 1.0} and not w[:, :3].any()
            if place == "skip":
                assert all(not sd[f"xyz_encoding_{i}.0.weight"].any() for i in range(1, 5))
            key, cols = reads[place]
            used = np.flatnonzero(np.abs(sd[key][:, cols]).sum(0))
            seen[place] += used.tolist()
            n_here = 3 if place == "dir" else 4
            assert len(used) == n_here
            want_cols = sorted(c - (63 if place == "dir" else 0) for c, _ in taps[:3]) + ([] if place == "dir" else [taps[3][0]])
            assert sorted(used.tolist()) == sorted(want_cols)
    assert sorted(seen["l1"]) == list(enc.SINCOS_POS) and sorted(seen["skip"]) == list(enc.SINCOS_POS)
    assert sorted(seen["dir"]) == list(enc.SINCOS_DIR)


def test_onehot_expected_values():
    """fp32: the network's exact (float64) output is the encoded column itself with its sign -- the taps are right; f16x3:
    within 2^-21 relative of it; f16 / bf16: the format's rounding; and the true-format split agrees with the exponent-free
    emulation of mlp_exact_ref wherever fp16 is normal."""
    rays, z = enc.make_rays(5, 64, 11)
    rows = enc.encode_rays(rays, z)
    for place in enc.PLACES:
        for name, sd, taps in enc.onehot_networks(place)[::4]:
            want = _oracle_raw(sd, rows)
            got = enc.onehot_expected(rows, taps, "fp32")
            assert np.array_equal(got.astype(np.float64), want), name
            for c, s in taps:
                assert np.array_equal(enc.bits(enc.onehot_expected(rows, taps, "fp32")[:, [t[0] for t in taps].index(c)]),
                                      enc.bits(F32(s) * rows[:, c]))
    v = np.concatenate([rows[:, 3:63].ravel(), rows[:, 66:].ravel()])
    x3 = enc.operand(v, "f16x3").astype(np.float64)
    big = np.abs(v) >= 2.0 ** -3                     # 22 significant bits are all above fp16's subnormal floor 2^-24
    assert big.sum() > v.size // 2
    assert (np.abs(x3[big] - v[big]) <= 2.0 ** -21 * np.abs(v[big])).all()
    assert (np.abs(x3 - v) <= np.maximum(2.0 ** -21 * np.abs(v), 2.0 ** -25)).all()          # below: the floor's half quantum
    hi, lo = er._split(v[big].astype(np.float64))
    normal = (np.abs(lo) >= 2.0 ** -14) | (lo == 0)      # the emulation of mlp_exact_ref has no exponent range: compare where lo is normal
    assert normal.sum() > big.sum() // 2 and np.array_equal(x3[big][normal], (hi + lo)[normal])
    assert np.array_equal(enc.operand(v[big], "f16").astype(np.float64), er._rne(v[big].astype(np.float64), 11))
    assert np.array_equal(enc.operand(v[big], "bf16").astype(np.float64), er._rne(v[big].astype(np.float64), 8))
    assert np.array_equal(enc.rn_bf16(torch.tensor([1.00390625, -3.0e-40, 0.0]).numpy()),
                          torch.tensor([1.00390625, -3.0e-40, 0.0]).bfloat16().float().numpy())


def test_every_column_takes_both_signs_and_many_values():
    """The condition on the rays: over the ray sets a place's networks run on -- the two shapes at both strides; for the
    direction part also the 37-ray set, since a direction column has one value per ray -- every sin / cos column is positive
    somewhere, negative somewhere and takes at least 32 distinct values."""
    rows = np.concatenate([enc.encode_rays(r, z) for r, z in enc.ray_sets()], 0)
    small = np.concatenate([enc.encode_rays(*enc.make_rays(R, N, s)) for (R, N) in enc.SHAPES for s in enc.STRIDES], 0)
    for c in enc.SINCOS_POS:
        assert (small[:, c] > 0).any() and (small[:, c] < 0).any() and len(np.unique(small[:, c])) >= 32, c
    for c in enc.SINCOS_DIR:
        col = rows[:, 63 + c]
        assert (col > 0).any() and (col < 0).any() and len(np.unique(col)) >= 32, c
