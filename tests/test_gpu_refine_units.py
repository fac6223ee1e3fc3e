"""Unit layer under the refinement network's train-mode pair: every small kernel of csrc/nsr_refine_train.hip ALONE, through
the launcher site_forward / site_backward call (csrc/nsr_refine_train_work.h; hooks: tests/csrc/nsr_test_hooks_refine_train.hip),
against tests/refine_units_ref.py.

Method.  Every output is a NaN frame around the owned region (guard rows, guard columns where the kernel takes a row stride,
ld 384 / ch0 128 -- the network's real slice -- among the cases) and is compared WHOLE, bit for bit (a NaN with a NaN), with
the expected frame: a store outside the region, a read of a NaN the kernel does not own and a wrong value all show.  Inputs
with a stride carry NaN in the columns the kernel must not read.  Each kernel is fed by numpy, never by the kernel before it.

* exact data (small integers, rows a power of two, mirrored halves so that the mean is an integer): the result equals plain
  integer arithmetic, whatever the order;
* real data (seeded normal): the result equals the ORDER-RESTATING fp32 form bit for bit, and lies within the first-order
  bound (ceil(rpp / 4) + 3) 2^-24 sum|terms| + one rounding of the result of the fp64 sum of the same terms (for the centred
  squares and dy xhat also: of the fp64 terms, with three more roundings for the term's own operations);
* only sqrtf (rstd) and tanhf are held to bounds instead of bits.

Measured on an MI355X (pytest -s prints them; largest over all real-data cases), error / bound:
  per-channel sums against the fp64 sum of the same terms: mean 0.299, centred squares 0.368, d beta 0.162, d gamma 0.202,
  bias gradient 0.299; against the fp64 terms: centred squares 0.273, d gamma 0.239.  The largest ratios come from the 8-row
  cases; at 16,384 rows and above every ratio is <= 0.052.
  rstd against 1 / sqrt(var64 + eps): 0.500 of the four-rounding bound, and equal to numpy's correctly rounded sequence
  (np.sqrt, one division) in every case
  tanhf of fwd_reduce against the fp64 tanh: 1.32 ulp at most (5 granted)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import hooks
from tests import refine_units_ref as ru
from tests.refine_units_ref import GE, GR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return hooks.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def framed(v, fill=None):
    """a vector inside GE NaN guard elements, on the device"""
    f = ru.vec_frame(v.size)
    f[GE:-GE] = v.reshape(-1) if fill is None else fill
    return dev(f)


def assert_bits(got, want, what):
    ok = ru.same_bits(got, want)
    if ok.all():
        return
    bad = np.argwhere(~ok)
    first = tuple(bad[0])
    raise AssertionError(f"{what}: {len(bad)} of {want.size} elements differ; first at {first}: got {got[first]!r}, want {want[first]!r}; "
                         f"index ranges {list(zip(bad.min(0).tolist(), bad.max(0).tolist()))} (frames: {GR} guard rows / {GE} guard elements)")


def assert_vec(t, want_inner, what):
    f = ru.vec_frame(want_inner.size)
    f[GE:-GE] = want_inner.reshape(-1)
    assert_bits(host(t), f, what)


def ok(rc, what):
    assert rc == 0, f"{what}: status {rc}"


# ------------------------------------------------------------------------------------------------------------------------
# per-channel reductions and their finishers
# ------------------------------------------------------------------------------------------------------------------------
WORST = {}


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def launch_reduce(hk, mode, c, X, DA, stat, gamma, beta, what):
    nparts = ru.reduce_parts(c.rows)
    part = dev(ru.vec_frame(2 * nparts * c.C))
    n = ctypes.c_int(-1)
    off = GR * c.ld + c.ch0
    ok(hk.nsr_test_refine_col_reduce(mode, hooks.ptr(X, off), c.ld, hooks.ptr(DA, off) if mode == 2 else None, c.ld,
                                     hooks.ptr(stat), hooks.ptr(gamma), hooks.ptr(beta), c.rows, c.C, hooks.ptr(part, GE),
                                     ctypes.byref(n), hooks.stream()), what)
    assert n.value == nparts, f"{what}: the launcher chose {n.value} partitions, the restatement {nparts}"
    return part, nparts


def check_part(part, want, nparts, C, what):
    f = ru.vec_frame(2 * nparts * C)
    f[GE:GE + want.size] = want.reshape(-1)
    assert_bits(host(part), f, what)


@pytest.mark.parametrize("c", ru.REDUCE_CASES, ids=lambda c: f"{c.kind}_{c.rows}x{c.C}")
def test_reductions_and_finishers(hk, c):
    """col_reduce<0|1|2>, fin_mean, fin_var, fin_bn_bwd, fin_bias.

    rstd bound.  fin_var computes fdiv(1, sqrtf(fadd(fl(ss / rows), eps))) from the double sum ss of its partials; against
    1 / sqrt(var64 + eps), var64 = ss / rows in double, four roundings lie on the path: fl(var) (relative 2^-24 of var <= var +
    eps), the addition (2^-24), sqrtf (HIP documents 1 ulp: 2^-23 of the root) and the division (2^-24).  rstd = (var +
    eps)^(-1/2) halves the first two: (1/2 + 1/2 + 2 + 1) 2^-24 = 2^-22 relative, first order; the factor 1 + 2^-10 covers the
    second-order terms (each below 2^-45)."""
    d = ru.build_reduce(c)
    e = ru.reduce_expected(c, d)
    rows, C, tag = c.rows, c.C, f"{c.kind} {c.rows} x {c.C}"
    X, DA = dev(d["X"]), dev(d["DA"])
    gamma, beta = dev(d["gamma"]), dev(d["beta"])
    x = ru.own(d["X"], rows, c.ch0, C)
    da = ru.own(d["DA"], rows, c.ch0, C)
    x64 = x.astype(np.float64)

    # ---- mode 0 and the mean
    part, nparts = launch_reduce(hk, 0, c, X, DA, None, None, None, tag + " mode 0")
    check_part(part, e["part0"], nparts, C, tag + " mode 0 partials")
    p0 = framed(e["part0"])
    for mom in (0.1, 0.0, 1.0):
        stat, run = dev(ru.vec_frame(2 * C)), framed(d["run_mean0"])
        ok(hk.nsr_test_refine_fin_mean(hooks.ptr(p0, GE), nparts, C, rows, mom, hooks.ptr(stat, GE), hooks.ptr(run, GE), hooks.stream()), tag)
        assert_vec(stat, np.concatenate([e["mean"], np.full(C, ru.NAN)]), f"{tag} mean (momentum {mom})")
        assert_vec(run, e["run_mean"][mom], f"{tag} running_mean (momentum {mom})")
    stat = dev(ru.vec_frame(2 * C))
    ok(hk.nsr_test_refine_fin_mean(hooks.ptr(p0, GE), nparts, C, rows, 0.1, hooks.ptr(stat, GE), None, hooks.stream()), tag)
    assert_vec(stat, np.concatenate([e["mean"], np.full(C, ru.NAN)]), tag + " mean without running statistics")
    mean_gpu = host(stat)[GE:GE + C]

    # ---- mode 1, rstd and the running variance
    stat1 = dev(np.concatenate([e["mean"], np.full(C, ru.NAN)]).astype(np.float32))        # rstd is not there yet: never read
    part, _ = launch_reduce(hk, 1, c, X, DA, stat1, None, None, tag + " mode 1")
    check_part(part, e["part1"], nparts, C, tag + " mode 1 partials")
    p1 = framed(e["part1"])
    ss64 = ru.part_sum64(e["part1"][0])
    rstd_ref = 1.0 / np.sqrt(ss64 / rows + float(ru.EPS))
    for mom in (0.1, 0.0, 1.0):
        stat, run = framed(np.concatenate([e["mean"], np.full(C, ru.NAN)])), framed(d["run_var0"])
        ok(hk.nsr_test_refine_fin_var(hooks.ptr(p1, GE), nparts, C, rows, mom, float(ru.EPS), hooks.ptr(stat, GE), hooks.ptr(run, GE),
                                      hooks.stream()), tag)
        assert_vec(run, e["run_var"][mom], f"{tag} running_var (momentum {mom})")
        s = host(stat)
        assert_bits(s[:GE + C], np.concatenate([np.full(GE, ru.NAN), e["mean"]]).astype(np.float32), tag + " fin_var touched the mean")
        assert np.isnan(s[GE + 2 * C:]).all(), tag + " fin_var wrote behind rstd"
        rstd = s[GE + C:GE + 2 * C].astype(np.float64)
        bound = rstd_ref * 2.0 ** -22 * (1 + 2.0 ** -10)
        err = np.abs(rstd - rstd_ref)
        note("rstd", (err / bound).max())
        note("rstd != numpy", float((s[GE + C:GE + 2 * C] != e["rstd"]).any()))
        assert (err <= bound).all(), f"{tag}: rstd off by {(err / bound).max():.3f} x the four-rounding bound"
    run_var1 = host(run)[GE:GE + C]                                                       # momentum 1: the unbiased variance itself

    # ---- mode 2 and its finisher (stat made in numpy)
    stat2 = dev(d["stat2"])
    part, _ = launch_reduce(hk, 2, c, X, DA, stat2, gamma, beta, tag + " mode 2")
    check_part(part, e["part2"], nparts, C, tag + " mode 2 partials")
    p2 = framed(e["part2"])
    outs = {}
    for acc in (0, 1):
        gg = framed(d["g_gamma0"], None if acc else ru.NAN)            # a store must not read what it overwrites
        gb = framed(d["g_beta0"], None if acc else ru.NAN)
        m = dev(ru.vec_frame(2 * C))
        ok(hk.nsr_test_refine_fin_bn_bwd(hooks.ptr(p2, GE), nparts, C, rows, acc, hooks.ptr(gg, GE), hooks.ptr(gb, GE), hooks.ptr(m, GE),
                                         hooks.stream()), tag)
        assert_vec(gg, e["g_gamma", acc], f"{tag} d gamma (acc {acc})")
        assert_vec(gb, e["g_beta", acc], f"{tag} d beta (acc {acc})")
        assert_vec(m, e["m"], f"{tag} m (acc {acc})")
        outs[acc] = host(gg)[GE:-GE], host(gb)[GE:-GE]

    # ---- bias gradient: elements [0, n_valid) only
    for acc in (0, 1):
        g0 = d["g_bias0"].copy()
        if not acc:
            g0[:c.n_valid] = ru.NAN
        gbias = framed(g0)
        ok(hk.nsr_test_refine_fin_bias(hooks.ptr(p0, GE), nparts, C, c.n_valid, acc, hooks.ptr(gbias, GE), hooks.stream()), tag)
        assert_vec(gbias, e["g_bias", acc], f"{tag} bias gradient (acc {acc}, n_valid {c.n_valid})")
        if not acc:
            bias_gpu = host(gbias)[GE:GE + c.n_valid]

    # ---- against fp64
    mean32 = e["mean"].astype(np.float64)
    if c.kind == "int":
        assert np.array_equal(mean_gpu.astype(np.float64), x64.mean(0))
        assert np.array_equal(ss64, ((x64 - x64.mean(0)) ** 2).sum(0))
        assert np.array_equal(run_var1.astype(np.float64), (ss64 / (rows - 1)).astype(np.float32))
        xhat = (x64 - d["stat2"][:C]) * d["stat2"][C:]                                    # integers x 0.5: exact in any order
        dy = np.where(d["gamma"] * xhat + d["beta"] > 0, da.astype(np.float64), 0.0)
        for acc in (0, 1):
            assert np.array_equal(outs[acc][1].astype(np.float64), dy.sum(0) + acc * d["g_beta0"]), f"{tag} d beta (acc {acc})"
            assert np.array_equal(outs[acc][0].astype(np.float64), (dy * xhat).sum(0) + acc * d["g_gamma0"]), f"{tag} d gamma (acc {acc})"
        assert np.array_equal(bias_gpu.astype(np.float64), x64.sum(0)[:c.n_valid])
        return
    rnd = lambda v: 2.0 ** -24 * np.abs(v)                                                # one rounding of the result
    t2 = [t.astype(np.float64) for t in ru.reduce_terms_f32(2, x, d["stat2"], d["gamma"], d["beta"], da)]
    t1 = ru.reduce_terms_f32(1, x, np.concatenate([e["mean"], e["mean"]]))[0].astype(np.float64)
    s2mean, s2rstd = d["stat2"][:C].astype(np.float64), d["stat2"][C:].astype(np.float64)
    dy = t2[0]
    checks = [
        ("mean", mean_gpu, x64.sum(0) / rows, ru.sum_bound(np.abs(x64).sum(0), rows, nparts) / rows),
        ("centred squares", run_var1, t1.sum(0) / (rows - 1), ru.sum_bound(t1.sum(0), rows, nparts) / (rows - 1)),
        ("centred squares, fp64 terms", run_var1, ((x64 - mean32) ** 2).sum(0) / (rows - 1),
         ru.sum_bound(((x64 - mean32) ** 2).sum(0), rows, nparts, 3) / (rows - 1)),
        ("d beta", outs[0][1], dy.sum(0), ru.sum_bound(np.abs(dy).sum(0), rows, nparts)),
        ("d gamma", outs[0][0], t2[1].sum(0), ru.sum_bound(np.abs(t2[1]).sum(0), rows, nparts)),
        ("d gamma, fp64 terms", outs[0][0], (dy * ((x64 - s2mean) * s2rstd)).sum(0),
         ru.sum_bound(np.abs(dy * ((x64 - s2mean) * s2rstd)).sum(0), rows, nparts, 3)),
        ("bias gradient", bias_gpu, x64.sum(0)[:c.n_valid], ru.sum_bound(np.abs(x64).sum(0), rows, nparts)[:c.n_valid]),
    ]
    line = []
    for name, got, want, bound in checks:
        bound = bound + rnd(want)
        err = np.abs(got.astype(np.float64) - want)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        note(name, ratio)
        line.append(f"{name} {ratio:.3f}")
        assert (err <= bound).all(), f"{tag}: {name} off by {ratio:.3f} x the first-order bound"
    print(f"refine units, reductions {tag} (rpp {ru.rows_per_part(rows, nparts)}): err / bound: " + ", ".join(line))


def test_reductions_report():
    """the largest ratios of the cases above (pytest -s; recorded in the module docstring)"""
    print("refine units, reductions, largest err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


# ------------------------------------------------------------------------------------------------------------------------
# bn_relu / bn_bwd / relu_bwd
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ru.BN_CASES, ids=lambda c: f"{c.rows}x{c.C}")
def test_bn_relu_bn_bwd_relu_bwd(hk, c):
    d = ru.build_bn(c)
    rows, C, tag = c.rows, c.C, f"{c.rows} x {c.C}"
    z, stat, gamma, beta, m, DA = (dev(d[k]) for k in ("z", "stat", "gamma", "beta", "m", "DA"))
    off = GR * c.ld + c.ch0
    dst = dev(ru.frame(rows, c.ld))
    ok(hk.nsr_test_refine_bn_relu(hooks.ptr(z), hooks.ptr(stat), hooks.ptr(gamma), hooks.ptr(beta), rows, C, hooks.ptr(dst, off), c.ld,
                                  hooks.stream()), tag)
    want_a = ru.bn_relu_expected(c, d)
    a = host(dst)
    assert_bits(a, want_a, tag + " bn_relu")
    act = ru.own(a, rows, c.ch0, C)
    # the built entries of row 0: +0, the smallest positive fp32, +0, NaN, +0, 2^-24, +0, +0
    first = act[0, :8]
    assert np.isnan(first[3]) and first[1] == ru.TINY and first[5] == np.float32(2.0 ** -24)
    assert not first[[0, 2, 4, 6, 7]].any() and not np.signbit(first[[0, 2, 4, 6, 7]]).any()

    dz = dev(ru.frame(rows, C))
    ok(hk.nsr_test_refine_bn_bwd(hooks.ptr(z), hooks.ptr(DA, off), c.ld, hooks.ptr(stat), hooks.ptr(gamma), hooks.ptr(beta), hooks.ptr(m),
                                 rows, C, hooks.ptr(dz, GR * C), hooks.stream()), tag)
    got = host(dz)
    assert_bits(got, ru.bn_bwd_expected(c, d), tag + " bn_bwd")
    # the ReLU mask of the backward is exactly (forward output > 0), the forward output being the DEVICE's
    da = ru.own(d["DA"], rows, c.ch0, C)
    mean, rstd = d["stat"][:C], d["stat"][C:]
    with np.errstate(invalid="ignore"):
        dy = np.where(act > 0, da, np.float32(0))
        masked = (d["gamma"] * rstd) * ((dy - d["m"][:C]) - ((d["z"] - mean) * rstd) * d["m"][C:])
    assert_bits(got[GR:GR + rows], masked.astype(np.float32), tag + " bn_bwd mask")

    a_dense, da_dense, want = ru.relu_bwd_expected(c, d)
    out, a_dev, da_dev = dev(ru.frame(rows, C)), dev(a_dense), dev(da_dense)
    ok(hk.nsr_test_refine_relu_bwd(hooks.ptr(a_dev), hooks.ptr(da_dev), rows * C, hooks.ptr(out, GR * C), hooks.stream()), tag)
    assert_bits(host(out), want, tag + " relu_bwd")


# ------------------------------------------------------------------------------------------------------------------------
# tanh_bwd, nhwc3_to_nchw
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ru.TANH_CASES, ids=lambda c: f"{c.B}x{c.H}x{c.W}")
def test_tanh_bwd_and_layout(hk, c):
    d = ru.build_tanh(c)
    px, rows = c.H * c.W, c.B * c.H * c.W
    dz, y, g_out = dev(ru.frame(rows, 32)), dev(d["y"]), dev(d["g_out"])
    ok(hk.nsr_test_refine_tanh_bwd(hooks.ptr(y), hooks.ptr(g_out), px, rows, hooks.ptr(dz, GR * 32), hooks.stream()), "tanh_bwd")
    got = host(dz)
    assert_bits(got, ru.tanh_bwd_expected(c, d), "tanh_bwd")
    pad = got[GR:-GR, 3:]
    assert not pad.any() and not np.signbit(pad).any(), "columns 3..31 are exactly +0.0"
    # the layout kernel on the same non-square shape: (B px, 3) -> (B, 3, px), exact
    out = framed(np.zeros(rows * 3, dtype=np.float32), ru.NAN)
    ok(hk.nsr_test_refine_nhwc3_to_nchw(hooks.ptr(y), px, c.B, hooks.ptr(out, GE), hooks.stream()), "nhwc3_to_nchw")
    assert_vec(out, ru.nhwc3_to_nchw_ref(d["y"], c.B, px), "nhwc3_to_nchw")


# ------------------------------------------------------------------------------------------------------------------------
# max over the references and its routing
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (1, 2, 8, 255))
def test_max_idx_and_route(hk, R):
    cases = [c for c in ru.MAX_CASES if c.R == R]
    assert {c.data for c in cases} == {"random", "ties", "nan", "zeros"} and {c.C for c in cases} == {8, 128}
    for c in cases:
        d = ru.build_max(c)
        n, tag = c.B * c.px, f"R {c.R} C {c.C} px {c.px} B {c.B} {c.data}"
        want_dst, want_win = ru.max_expected(c, d)
        dst = dev(ru.frame(n, c.ld))
        win, src = dev(np.full(n * c.C + 2 * GE, ru.WIN_SENT, dtype=np.uint8)), dev(d["src"])
        ok(hk.nsr_test_refine_max_idx(hooks.ptr(src), c.C, c.R, c.px, c.B, hooks.ptr(dst, GR * c.ld + c.ch0), c.ld, hooks.ptr(win, GE),
                                      hooks.stream()), tag)
        assert_bits(host(dst), want_dst, tag + " maximum")
        assert_bits(host(win), want_win, tag + " winner")
        w = want_win[GE:-GE].reshape(n, c.C)
        if c.data == "nan":
            m = ru.own(want_dst, n, c.ch0, c.C)
            has = np.isnan(d["src"]).any(1).reshape(n, c.C)
            assert has.any() and np.array_equal(np.isnan(m), has), "a NaN among the references is the maximum"
            firstnan = np.isnan(d["src"]).argmax(1).reshape(n, c.C)
            assert np.array_equal(w[has], firstnan[has]), "the first NaN wins"
        # route: the winners made in numpy, g_max a slice of a NaN frame, every element of g_fc overwritten
        G, w_dev = dev(d["G"]), dev(w)
        gfc = dev(ru.frame(c.B * c.R * c.px, c.C))
        ok(hk.nsr_test_refine_route(hooks.ptr(G, GR * c.ld + c.ch0), c.ld, hooks.ptr(w_dev), c.C, c.R, c.px, c.B,
                                    hooks.ptr(gfc, GR * c.C), hooks.stream()), tag)
        got = host(gfc)
        assert_bits(got, ru.route_expected(c, d)[1], tag + " route")
        r = got[GR:-GR].reshape(c.B, c.R, c.px, c.C)
        g = ru.own(d["G"], n, c.ch0, c.C).reshape(c.B, c.px, c.C)
        assert not np.isnan(r).any(), "route left an element of g_fc unwritten"
        assert ((r != 0).sum(1) == (g != 0)).all(), "exactly one non-zero copy per (pixel, channel)"
        assert_bits(r.sum(1, dtype=np.float32), g, tag + " route summed over r")


# ------------------------------------------------------------------------------------------------------------------------
# col2im
# ------------------------------------------------------------------------------------------------------------------------
def run_col2im(hk, c, d):
    n = c.n_img * c.Hs * c.Ws
    dst, dcol = dev(d["dst0"]), dev(d["dcol"])
    ok(hk.nsr_test_refine_col2im(hooks.ptr(dcol), d["kp"], c.cin, c.n_img, c.Hs, c.Ws, c.stride, c.up, d["Ho"], d["Wo"], c.acc,
                                 hooks.ptr(dst, GR * c.ld + c.ch0), c.ld, hooks.stream()), str(c))
    return host(dst), n


@pytest.mark.parametrize("Hs,Ws", ((2, 2), (4, 6), (5, 7), (8, 8)))
def test_col2im_exact(hk, Hs, Ws):
    cases = [c for c in ru.COL_CASES if (c.Hs, c.Ws) == (Hs, Ws)]
    assert len(cases) == 18 and {(c.stride, c.up) for c in cases} == {(1, 0), (2, 0), (1, 1)} and {c.cin for c in cases} == {4, 8, 128}
    for i, c in enumerate(cases):
        d = ru.build_col(c)
        got, n = run_col2im(hk, c, d)
        assert_bits(got, ru.col2im_expected(c, d), f"{c} col2im")
        # ... which is the transpose of im2col, in integers
        t = ru.col2im_transpose64(d["dcol"], c.cin, c.n_img, c.Hs, c.Ws, c.stride, c.up, d["Ho"], d["Wo"])
        if c.acc:
            t = t + ru.own(d["dst0"], n, c.ch0, c.cin)
        assert np.array_equal(ru.own(got, n, c.ch0, c.cin).astype(np.float64), t), f"{c}: not the transpose of im2col"
        if i % 3 == 0:                                                         # real data: the kernel's own order, bit for bit
            d = ru.build_col(c, real=True)
            got, _ = run_col2im(hk, c, d)
            assert_bits(got, ru.col2im_expected(c, d), f"{c} col2im, real data")


# ------------------------------------------------------------------------------------------------------------------------
# wgrad_reduce, fwd_reduce
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", ((3, 128), (128, 3), (8, 8), (64, 32)))
def test_wgrad_reduce_exact(hk, cin, cout):
    cases = [c for c in ru.WGRAD_CASES if (c.cin, c.cout) == (cin, cout)]
    assert len(cases) == 6
    for c in cases:
        d = ru.build_wgrad(c)
        g, part = dev(d["g0"]), dev(d["part"])
        ok(hk.nsr_test_refine_wgrad_reduce(hooks.ptr(part), c.splits, d["split_stride"], d["kp"], c.cin, c.cout, c.acc,
                                           hooks.ptr(g, GE), hooks.stream()), str(c))
        got = host(g)
        assert_bits(got, ru.wgrad_expected(c, d), f"{c} wgrad_reduce")
        blk = d["part"][:, :c.rows * d["kp"]].reshape(c.splits, c.rows, d["kp"])[:, :c.cout, :9 * c.cin].astype(np.float64)
        want = blk.sum(0).reshape(c.cout, 9, c.cin).transpose(0, 2, 1).reshape(-1)       # integers: any order
        if c.acc:
            want = want + d["g0"][GE:-GE]
        assert np.array_equal(got[GE:-GE].astype(np.float64), want)


@pytest.mark.parametrize("splits", (1, 2, 432, "cancel"))
def test_fwd_reduce(hk, splits):
    """tanhf is held to the 5 ulp the OpenCL profile grants the function, against the fp64 tanh of the restated pre-activation
    (measured: 1.32 ulp at most); everything else is bit-equal to the restatement"""
    cases = [c for c in ru.FWD_CASES if (c.data == "cancel") == (splits == "cancel") and (splits == "cancel" or c.splits == splits)]
    assert cases
    worst = 0.0
    for c in cases:
        d = ru.build_fwd(c)
        dst, part, bias = dev(ru.frame(c.M, c.ld)), dev(d["part"]), dev(d["bias"])
        ok(hk.nsr_test_refine_fwd_reduce(hooks.ptr(part), c.splits, d["split_stride"], d["np"], c.cout, hooks.ptr(bias),
                                         c.act, c.M, hooks.ptr(dst, GR * c.ld + c.ch0), c.ld, hooks.stream()), str(c))
        got = host(dst)
        want, pre = ru.fwd_expected(c, d)
        if c.act != ru.ACT_TANH:
            assert_bits(got, want, f"{c} fwd_reduce")
            if c.data == "cancel":
                blk = d["part"][:, :c.M * d["np"]].reshape(c.splits, c.M, d["np"])[:, :, :c.cout].astype(np.float64)
                v = (blk.sum(0) + d["bias"]).astype(np.float32)                           # the double sum, rounded once
                v = ru.relu_nan(v) if c.act == ru.ACT_RELU else v
                assert_bits(ru.own(got, c.M, c.ch0, c.cout), v, f"{c}: partials that cancel in fp32")
            continue
        o, w = ru.own(got, c.M, c.ch0, c.cout).astype(np.float64), np.tanh(pre.astype(np.float64))
        ulps = np.abs(o - w) / ru.ulp32(w)
        worst = max(worst, float(ulps.max()))
        assert (ulps <= 5).all(), f"{c}: tanhf {ulps.max():.2f} ulp from the fp64 tanh"
        ru.own(got, c.M, c.ch0, c.cout)[:] = ru.own(want, c.M, c.ch0, c.cout)
        assert_bits(got, want, f"{c} fwd_reduce: outside the owned region")
    print(f"refine units, fwd_reduce splits {splits}: tanhf at most {worst:.2f} ulp from the fp64 tanh")
