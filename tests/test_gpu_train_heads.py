"""Unit layer under the training step's head: the kernels between the rendered colours and the network's backward
(csrc/nsr_train.hip) -- composite_bwd_kernel<K, FULL>, lr_loss_kernel, loss_finish_kernel, sigma_noise_kernel,
gamma_points_kernel -- launched on their own through the test-hook library (tests/hooks.py,
tests/csrc/nsr_test_hooks_heads.hip).  Reference, error model and inputs: tests/train_heads_ref.py, itself pinned on the CPU by
tests/test_train_heads_cpu.py.

Every output buffer is NaN- or pattern-filled with a guard region behind it that must survive; every element of every output is
compared.  The real-valued compositing cases hold the kernel to the DERIVED elementwise bound of
train_heads_ref.error_bounds, no factor on top; the largest err / bound per (K, option) is printed (run with -s) and recorded
in DESIGN.md.  The exact checks are bit for bit.

One check is stated differently from "a ray opaque at k = 0 gives d_rgb nonzero at k = 0 only": with f = 1 - alpha + 1e-10 the
transmittance behind an opaque sample is 1e-10, not 0, so every later sample with a positive density has w = alpha 1e-10 and a
d_rgb of that order on the device and in the fp64 reference alike.  test_composite_bwd_exact_rays asserts what does hold
exactly: d_rgb is nonzero at k = 0, exactly 0 at every later sample with sigma <= 0, and at most |g_comp| fl(1e-10) elsewhere.
"""
import ctypes

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib as nsr_lib
from tests import hooks
from tests import train_heads_ref as hr

pytestmark = pytest.mark.gpu

GUARD = 1024                    # elements behind every output region
GMAX_GARBAGE = 0x7F7F7F7F
U = hr.U
f32 = np.float32


@pytest.fixture(scope="module")
def hk():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    lib = hooks.load()
    # the product's own forward compositor, out of the same library (it links the product's objects)
    lib.nsr_composite.restype, lib.nsr_composite.argtypes = nsr_lib.SIGNATURES["nsr_composite"]
    return lib


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def out_buf(n, dtype=torch.float32, fill=float("nan")):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------------------------------
# compositing backward
# ------------------------------------------------------------------------------------------------------------------------
_cases = {}


def case_of(R, N):
    if (R, N) not in _cases:
        c = hr.composite_case(R, N)
        c["dev"] = {k: dev(v) for k, v in c.items()}
        _cases[(R, N)] = c
    return _cases[(R, N)]


def run_bwd(hk, c, R, N, flags, names=(), gmax=True, bias=True, expect=hooks.NSR_OK, override=None):
    """one launch -> (d4 (P, 4) fp32, bias_part (R, 4) fp32 or None); asserts the guards and the gmax contract.
    override: {name: host array} replacing the case's arrays of that name"""
    d = dict(c["dev"])
    for k, v in (override or {}).items():
        d[k] = dev(v)
    P = R * N
    d4 = out_buf(P * 4)
    gm = torch.full((11 + GUARD,), GMAX_GARBAGE, dtype=torch.int32, device="cuda") if gmax else None
    bp = out_buf(R * 4) if bias else None
    up = [hooks.ptr(d[n]) if n in names else None for n in ("g_depth", "g_opacity", "g_weights")]
    rc = hk.nsr_test_composite_bwd(hooks.ptr(d["rgb4"]), hooks.ptr(d["sigma"]), hooks.ptr(d["z"]), hooks.ptr(d["g_comp"]), R, N, flags,
                                   hooks.ptr(d4), hooks.ptr(gm), hooks.ptr(bp), up[0], up[1], up[2], hooks.stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    out = d4.cpu().numpy()
    if rc != hooks.NSR_OK:
        assert np.isnan(out).all(), "a refused call wrote d4"
        assert gm is None or (gm.cpu().numpy() == GMAX_GARBAGE).all(), "a refused call wrote gmax"
        assert bp is None or np.isnan(bp.cpu().numpy()).all(), "a refused call wrote bias_part"
        return None, None
    assert np.isnan(out[P * 4:]).all(), "floats behind d4 were written"
    if gm is not None:
        g = gm.cpu().numpy()
        assert (g[:10] == 0).all(), "the ten gmax words were not cleared"
        assert (g[10:] == GMAX_GARBAGE).all(), "gmax word 10 or the words behind it were written"
    b = None
    if bp is not None:
        b = bp.cpu().numpy()
        assert np.isnan(b[R * 4:]).all(), "floats behind bias_part were written"
        b = b[:R * 4].reshape(R, 4).copy()
    return out[:P * 4].reshape(P, 4).copy(), b


def host_args(c, flags):
    return (c["rgb4"], c["sigma"], c["z"], c["g_comp"], flags)


@pytest.mark.parametrize("R,N", hr.SHAPES)
def test_composite_bwd_within_derived_bound(hk, R, N):
    """|d4 - fp64 reference| <= train_heads_ref.error_bounds elementwise, no factor; bias_part within the sum of its points'
    bounds plus N fp32 additions.  Every option set of train_heads_ref.option_sets(); gmax and bias_part null and non-null in
    turn.  Measured on one MI355X (2026-10-19), largest err / bound: see DESIGN.md."""
    c = case_of(R, N)
    K = (N + 63) // 64
    worst, fails = {}, []
    for idx, (flags, names) in enumerate(hr.option_sets()):
        up = hr.upstream(c, names)
        ref, ref_bias = hr.ref_composite_bwd(*host_args(c, flags), **up)
        bound, bound_bias = hr.error_bounds(*host_args(c, flags), **up)
        got, bias = run_bwd(hk, c, R, N, flags, names, gmax=idx % 2 == 0, bias=idx % 3 != 0)
        assert np.isfinite(got).all(), (flags, names, "an element of d4 was not written")
        err = np.abs(got.astype(np.float64) - ref)
        nz = bound > 0
        ratio = float((err[nz] / bound[nz]).max())
        key = (K, hr.flag_name(flags), "FULL" if ("g_opacity" in names or "g_weights" in names) else "plain")
        worst[key] = max(worst.get(key, 0.0), ratio)
        if not (err <= bound).all():
            p, col = np.unravel_index(np.argmax(np.where(nz, err / np.where(nz, bound, 1.0), 0.0)), err.shape)
            fails.append((flags, names, ratio, f"ray {p // N} sample {p % N} column {col}: {got[p, col]!r} vs {ref[p, col]!r}"))
        if bias is not None:
            berr = np.abs(bias.astype(np.float64) - ref_bias)
            if not (berr <= bound_bias).all():
                fails.append((flags, names, "bias_part", float((berr / bound_bias).max())))
    for (k, opt, inst), v in worst.items():
        print(f"composite_bwd R {R} N {N:3d} K {k} {inst:5s} {opt:15s}: largest err / bound {v:.4f}")
    assert not fails, fails


def test_composite_bwd_unsupported_n_writes_nothing(hk):
    c = hr.composite_case(5, 257)
    c["dev"] = {k: dev(v) for k, v in c.items()}
    run_bwd(hk, c, 5, 257, 0, ("g_depth",), expect=hooks.NSR_ERR_UNSUPPORTED)
    run_bwd(hk, c, 5, 257, 0, ("g_opacity", "g_weights"), expect=hooks.NSR_ERR_UNSUPPORTED)


@pytest.mark.parametrize("N", hr.ALL_N)
def test_composite_bwd_reproduces_the_forward_weights(hk, N):
    """NSR_TRAIN_COLOR_NONE and g_comp = (1, 2, 4): d4[:, 0:3] = (w, 2 w, 4 w) with w the BITS of nsr_composite's weights on the same
    inputs -- the backward recomputes the forward with the same code.  Both density modes."""
    R = 5
    c = case_of(R, N)
    g = np.tile(np.array([1.0, 2.0, 4.0], dtype=f32), (R, 1))
    for soft in (0, hr.SOFTPLUS):
        wts = out_buf(R * N)
        d = c["dev"]
        rc = hk.nsr_composite(hooks.ptr(d["rgb4"]), 4, hooks.ptr(d["sigma"]), 1, hooks.ptr(d["z"]), R, N, soft, None, None, None,
                              hooks.ptr(wts), hooks.stream())
        assert rc == hooks.NSR_OK, rc
        torch.cuda.synchronize()
        w = wts.cpu().numpy()[:R * N]
        assert np.isfinite(w).all() and (w >= 0).all() and w.max() > 0.01
        for full in ((), ("g_opacity",)):       # gw does not enter d_rgb: the FULL instantiation stores the same colours
            got, _ = run_bwd(hk, c, R, N, hr.COLOR_NONE | soft, full, override={"g_comp": g})
            for col, s in enumerate((1.0, 2.0, 4.0)):
                bad = np.flatnonzero(bits(got[:, col].copy()) != bits(f32(s) * w))
                assert bad.size == 0, (N, soft, full, col, bad[:8], got[bad[:8], col], w[bad[:8]])


@pytest.mark.parametrize("N", (3, 65, 193))
def test_composite_bwd_exact_rays(hk, N):
    """the planted rays of train_heads_ref.composite_case under relu: an all-transparent ray gives d4 = 0 exactly; a masked sample's
    d_sigma is +0; behind a sample opaque at k = 0 (see the module docstring)"""
    R = 5
    c = case_of(R, N)
    sigma = c["sigma"].reshape(R, N)
    tiny = float(f32(1e-10)) * (1.0 + 4.0 * U)
    for flags in (0, hr.WHITE, hr.GAMMA, hr.COLOR_NONE):
        for names in ((), ("g_depth",), ("g_depth", "g_opacity", "g_weights")):
            got, bias = run_bwd(hk, c, R, N, flags, names)
            got = got.reshape(R, N, 4)
            assert (got[hr.RAY_TRANSPARENT] == 0).all() and (bias[hr.RAY_TRANSPARENT] == 0).all()
            assert (bits(got[:, :, 3].copy())[sigma <= 0] == 0).all(), "a masked sample's d_sigma is not +0"
            assert (got[:, :, 3][sigma > 0] != 0).any()
            op = got[hr.RAY_OPAQUE_AT_0]
            assert (op[0, :3] != 0).all()
            later, gc = op[1:, :3], np.abs(c["g_comp"][hr.RAY_OPAQUE_AT_0])[None, :]
            assert (later[sigma[hr.RAY_OPAQUE_AT_0, 1:] <= 0] == 0).all()
            assert (np.abs(later) <= gc * tiny).all()
            assert (np.abs(op[0, :3]) > 1e6 * np.abs(later).max(0)).all()


@pytest.mark.parametrize("N", (2, 64, 129, 192, 256))
def test_composite_bwd_full_with_zero_upstreams_stores_the_plain_bits(hk, N):
    R = 5
    c = case_of(R, N)
    zeros = {"g_opacity": np.zeros(R, dtype=f32), "g_weights": np.zeros((R, N), dtype=f32)}
    for flags in (0, hr.WHITE | hr.SOFTPLUS, hr.WHITE | hr.GAMMA):
        for depth in ((), ("g_depth",)):
            plain, pb = run_bwd(hk, c, R, N, flags, depth)
            for names in (("g_opacity",), ("g_weights",), ("g_opacity", "g_weights")):
                full, fb = run_bwd(hk, c, R, N, flags, depth + names, override=zeros)
                assert np.array_equal(bits(full), bits(plain)) and np.array_equal(bits(fb), bits(pb)), (N, flags, depth, names)


def test_composite_bwd_wrong_references_are_told_apart(hk):
    """teeth: ONE device output against five deliberately wrong references"""
    R, N = 5, 193
    c = case_of(R, N)
    up = hr.upstream(c, ("g_depth",))
    got, _ = run_bwd(hk, c, R, N, hr.WHITE, ("g_depth",))
    got = got.astype(np.float64)
    bound, _ = hr.error_bounds(*host_args(c, hr.WHITE), **up)
    ref, _ = hr.ref_composite_bwd(*host_args(c, hr.WHITE), **up)
    assert (np.abs(got - ref) <= bound).all()
    for what in hr.WRONG:
        bad, _ = hr.ref_composite_bwd(*host_args(c, hr.WHITE), **up, wrong=what)
        n = int((np.abs(got - bad) > bound).sum())
        print(f"{what}: {n} elements beyond the bound")
        assert n > 0, what


# ------------------------------------------------------------------------------------------------------------------------
# loss head
# ------------------------------------------------------------------------------------------------------------------------
def run_lr_loss(hk, comp, target, s2, scale, lam, lam_var, lam_dvar, far, depth, with_g_depth):
    """-> lr_out (n_lr, 3), g_comp (n_lr s2, 3), block_sums (3, nblk) fp64, g_depth (n_lr s2,) or None; asserts the guards"""
    n_lr = target.shape[0]
    nblk = (n_lr + 255) // 256
    lr, gc = out_buf(n_lr * 3), out_buf(n_lr * s2 * 3)
    bs = out_buf(3 * nblk, torch.float64)
    gd = out_buf(n_lr * s2) if with_g_depth else None
    t_comp, t_target, t_depth = dev(comp), dev(target), dev(depth)
    rc = hk.nsr_test_lr_loss(hooks.ptr(t_comp), hooks.ptr(t_target), n_lr, s2, scale, lam, hooks.ptr(lr), hooks.ptr(gc), hooks.ptr(bs),
                             lam_var, lam_dvar, far, hooks.ptr(t_depth), hooks.ptr(gd), hooks.stream())
    assert rc == hooks.NSR_OK, rc
    torch.cuda.synchronize()
    lr, gc, bs = lr.cpu().numpy(), gc.cpu().numpy(), bs.cpu().numpy()
    assert np.isnan(lr[n_lr * 3:]).all() and np.isnan(gc[n_lr * s2 * 3:]).all() and np.isnan(bs[3 * nblk:]).all(), "guard written"
    g_depth = None
    if gd is not None:
        gd = gd.cpu().numpy()
        assert np.isnan(gd[n_lr * s2:]).all(), "floats behind g_depth were written"
        g_depth = gd[:n_lr * s2].copy()
    return lr[:n_lr * 3].reshape(n_lr, 3).copy(), gc[:n_lr * s2 * 3].reshape(-1, 3).copy(), bs[:3 * nblk].reshape(3, nblk).copy(), g_depth


def lr_branches(s2):
    """(lambda_var, lambda_dvar, depth given, g_depth asked for): lambda_var 0 and nonzero; g_depth null; non-null with
    lambda_dvar = 0 (must come back as zeros).  One sub-ray has no variance: its lambdas are 0"""
    lv, ld = float(f32(0.25)), float(f32(0.125))
    out = [(0.0, 0.0, False, False), (0.0, 0.0, True, True)]
    if s2 > 1:
        out += [(lv, 0.0, False, False), (lv, ld, True, True), (0.0, ld, True, True), (lv, 0.0, True, True)]
    return out


N_LR = (1, 255, 256, 257, 600)


@pytest.mark.parametrize("n_lr", N_LR)
@pytest.mark.parametrize("s2", (1, 4, 16))
def test_lr_loss_exact(hk, s2, n_lr):
    """comp, target, depth: small integers times 2^-8, s2 and far powers of two: every fp32 step of the kernel is exact and the
    fp64 reference in the kernel's operation order gives its bits: lr_out, the three block_sums rows at [q nblk + block], g_comp
    and g_depth as float32(fp64 expression)"""
    rng = np.random.default_rng(100 * s2 + n_lr)
    comp = (rng.integers(0, 257, (n_lr * s2, 3)) / 256.0).astype(f32)
    target = (rng.integers(0, 257, (n_lr, 3)) / 256.0).astype(f32)
    depth = (rng.integers(512, 1536, n_lr * s2) / 256.0).astype(f32)
    scale, lam, far = 1.0 / (3.0 * n_lr), 0.5, 4.0
    for lv, ld, has_depth, want_gd in lr_branches(s2):
        lr, gc, bs, gd = run_lr_loss(hk, comp, target, s2, scale, lam, lv, ld, far, depth if has_depth else None, want_gd)
        r_lr, r_gc, r_gd, r_bs = hr.ref_lr_loss(comp, target, s2, scale, lam, lv, ld, far, depth if want_gd else None)
        tag = (s2, n_lr, lv, ld, want_gd)
        assert np.array_equal(bits(lr), bits(r_lr.astype(f32))), tag
        assert np.array_equal(bits(bs), bits(r_bs)), (tag, bs, r_bs)
        assert np.array_equal(bits(gc), bits(r_gc.astype(f32))), tag
        if want_gd:
            assert np.array_equal(bits(gd), bits(r_gd.astype(f32))), tag
            if ld == 0.0:
                assert (bits(gd) == 0).all(), "g_depth with lambda_dvar = 0 is not written as zeros"
            else:
                assert gd.any() and bs[2].any()
        assert bs[1].any() == (lv != 0.0) and bs[0].any()


@pytest.mark.parametrize("n_lr", N_LR)
@pytest.mark.parametrize("s2", (1, 4, 9, 16))
def test_lr_loss_real(hk, s2, n_lr):
    """lr_out: the fp32 left-to-right sum and one division, bit for bit; g_comp and g_depth within 1 fp32 ulp of the fp64
    reference; block_sums within the rounding of their fp64 additions in any order ((additions per block) 2^-53, relative:
    every term is a square)"""
    rng = np.random.default_rng(100 * s2 + n_lr + 7)
    comp = rng.uniform(0, 1, (n_lr * s2, 3)).astype(f32)
    target = rng.uniform(0, 1, (n_lr, 3)).astype(f32)
    depth = rng.uniform(2, 6, n_lr * s2).astype(f32)
    scale, lam, far = 1.0 / (3.0 * n_lr), float(f32(0.7)), float(f32(6.3))
    acc = np.zeros((n_lr, 3), dtype=f32)
    for k in range(s2):
        acc = acc + comp.reshape(n_lr, s2, 3)[:, k]
    want_lr = acc / f32(s2)
    for lv, ld, has_depth, want_gd in lr_branches(s2):
        lv, ld = float(f32(lv * 1.3)), float(f32(ld * 1.7))      # not powers of two (0 stays 0)
        lr, gc, bs, gd = run_lr_loss(hk, comp, target, s2, scale, lam, lv, ld, far, depth if has_depth else None, want_gd)
        _, r_gc, r_gd, r_bs = hr.ref_lr_loss(comp, target, s2, scale, lam, lv, ld, far, depth if want_gd else None)
        tag = (s2, n_lr, lv, ld, want_gd)
        assert np.array_equal(bits(lr), bits(want_lr)), tag
        assert (np.abs(gc.astype(np.float64) - r_gc) <= hr.ulp32(r_gc)).all(), tag
        if want_gd:
            assert (np.abs(gd.astype(np.float64) - r_gd) <= hr.ulp32(r_gd)).all(), tag
            assert ld != 0.0 or (bits(gd) == 0).all()
        assert (np.abs(bs - r_bs) <= 256 * (4 * s2 + 8) * 2.0 ** -53 * np.abs(r_bs)).all(), (tag, bs, r_bs)


@pytest.mark.parametrize("var", (False, True))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 1000))
def test_loss_finish(hk, n, var):
    """integer-valued block_sums: the carry is exact in any order.  Slot 0, slot 1, slot 0 again: the carry accumulates, the other
    slot's words and the two words behind the six carries stay, losses = float32(lambda carry scale) bit for bit"""
    rng = np.random.default_rng(n)
    scale, lam, lv, ld = 1.0 / 3000.0, 0.5, float(f32(0.25)), float(f32(0.125))
    carry0 = np.array([10, 20, 30, 40, 50, 60, 7777, 8888], dtype=np.float64)
    carry = torch.cat([dev(carry0), out_buf(0, torch.float64)])
    losses, var_losses = out_buf(2), (out_buf(4) if var else None)
    want_carry = carry0[:6].copy()
    want_losses, want_var = np.full(2, np.nan, dtype=f32), np.full(4, np.nan, dtype=f32)
    for call, slot in enumerate((0, 1, 0)):
        sums = rng.integers(0, 1 << 20, 3 * n).astype(np.float64)
        t = dev(sums)
        rc = hk.nsr_test_loss_finish(hooks.ptr(t), n, scale, lam, hooks.ptr(losses), slot, hooks.ptr(carry), lv, ld,
                                     hooks.ptr(var_losses), hooks.stream())
        assert rc == hooks.NSR_OK, rc
        torch.cuda.synchronize()
        want_carry, want_losses[slot], (want_var[slot], want_var[2 + slot]) = hr.ref_loss_finish(sums, n, scale, lam, slot, want_carry,
                                                                                                 lv, ld)
        got = carry.cpu().numpy()
        assert np.array_equal(bits(got[:6].copy()), bits(want_carry)), (n, call, got[:8], want_carry)
        assert got[6] == 7777 and got[7] == 8888 and np.isnan(got[8:]).all(), "words behind the six carries were written"
        got_l = losses.cpu().numpy()
        assert np.array_equal(bits(got_l[:2].copy()), bits(want_losses)) and np.isnan(got_l[2:]).all(), (n, call, got_l[:2], want_losses)
        if var:
            got_v = var_losses.cpu().numpy()
            assert np.array_equal(bits(got_v[:4].copy()), bits(want_var)) and np.isnan(got_v[4:]).all(), (n, call, got_v[:4], want_var)
    assert (want_carry > carry0[:6]).all()                       # both slots of all three sums moved


# ------------------------------------------------------------------------------------------------------------------------
# density noise, per-sample gamma
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (1, 255, 257))
def test_sigma_noise(hk, P):
    """input at stride 4 from column 3 of a (P, 4) array; out = fl(s + fl(noise std)) bit for bit; noise null: a copy"""
    rng = np.random.default_rng(P)
    rows = rng.standard_normal((P, 4)).astype(f32) * f32(3.0)
    noise = rng.standard_normal(P).astype(f32)
    std = f32(0.37)
    t_rows, t_noise = dev(rows), dev(noise)
    for nz in (t_noise, None):
        out = out_buf(P)
        rc = hk.nsr_test_sigma_noise(hooks.ptr(t_rows, 3), 4, hooks.ptr(nz), float(std), P, hooks.ptr(out), hooks.stream())
        assert rc == hooks.NSR_OK, rc
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isnan(got[P:]).all(), "floats behind the output were written"
        want = rows[:, 3] + noise * std if nz is not None else rows[:, 3]
        assert want.dtype == f32 and np.array_equal(bits(got[:P].copy()), bits(want.copy()))


@pytest.mark.parametrize("P", (1, 255, 257))
def test_gamma_points(hk, P):
    """columns 0..2 within the transcendental allowance of c^(1 / 2.2) in fp64 (+ the exponent's own rounding: 1 / 2.2f is
    (1 / 2.2)(1 + d), |d| <= 2 u: relative 2 u |ln c| / 2.2); column 3 bit-identical"""
    rng = np.random.default_rng(P)
    rows = rng.uniform(0.0, 1.0, (P, 4)).astype(f32)
    rows[:, 3] = (rng.standard_normal(P) * 5).astype(f32)
    rows[0, :3] = (0.0, 1.0, 1e-30)[:3]
    if P > 1:
        rows[1, 3] = np.nan
    buf = torch.cat([dev(rows.reshape(-1)), torch.full((GUARD,), 0.5, device="cuda")])
    rc = hk.nsr_test_gamma_points(hooks.ptr(buf), P, hooks.stream())
    assert rc == hooks.NSR_OK, rc
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[P * 4:] == 0.5).all(), "floats behind the rows were written"
    got = got[:P * 4].reshape(P, 4)
    assert np.array_equal(bits(got[:, 3].copy()), bits(rows[:, 3].copy()))
    c = rows[:, :3].astype(np.float64)
    want = c ** (1.0 / 2.2)
    with np.errstate(divide="ignore", invalid="ignore"):
        expo = np.where(c > 0, want * 2.0 * U * np.abs(np.log(c)) / 2.2, 0.0)
    bound = hr.TRANSCENDENTAL_ULPS * hr.ulp32(want) + expo
    err = np.abs(got[:, :3].astype(np.float64) - want)
    print(f"gamma_points P {P}: largest err / bound {float((err / bound).max()):.4f}, largest err in ulp {float((err / hr.ulp32(want)).max()):.3f}")
    assert (err <= bound).all()
    assert got[0, 0] == 0.0 and got[0, 1] == 1.0
