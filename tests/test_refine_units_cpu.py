"""CPU side of the unit layer under the refinement network's train-mode pair (tests/test_gpu_refine_units.py):

* the fp64 forms of tests/refine_units_ref.py are pinned against torch's own fp64 operations and their autograd, and the
  order-restating fp32 forms against the fp64 forms, so what the device is compared with means what it should;
* the hook library exports the new wrappers, and each refuses null and misaligned pointers before it touches a device;
* SENSITIVITY: every deliberately wrong restatement (``mut=``) changes the expected result of at least one case of the GPU
  tests' own case lists, for every unit it applies to.  No device code is mutated or run.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nerf_sr_amd import _lib, build as nsr_build
from tests import hooks
from tests import refine_units_ref as ru
from tests.conv_ref import im2col_numpy

INV = hooks.NSR_ERR_INVALID_ARG
T64 = dict(dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------------------
# fp64 forms against torch
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", (0.1, 0.0, 1.0))
def test_batchnorm_relu_forms_match_torch_autograd(momentum):
    g = np.random.default_rng(3)
    rows, C = 37, 5
    z, da = g.standard_normal((rows, C)) * 2 + 0.7, g.standard_normal((rows, C))
    gamma, beta = 1 + 0.5 * g.standard_normal(C), 0.3 * g.standard_normal(C)
    rm0, rv0 = g.standard_normal(C), 1 + g.random(C)
    zt = torch.tensor(z.T.reshape(1, C, rows, 1).copy(), requires_grad=True)           # (N, C, H, W) with N H W = rows
    gt, bt = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    rm, rv = torch.tensor(rm0), torch.tensor(rv0)
    a = torch.relu(F.batch_norm(zt, rm, rv, gt, bt, training=True, momentum=momentum, eps=1e-5))
    a.backward(torch.tensor(da.T.reshape(1, C, rows, 1).copy()))
    a64, mean, var, rm64, rv64 = ru.bn_train_fwd64(z, gamma, beta, 1e-5, momentum, rm0, rv0)
    dz64, dg64, db64 = ru.bn_relu_bwd64(z, da, gamma, beta)
    tol = dict(rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(a64, a.detach().numpy().reshape(C, rows).T, **tol)
    np.testing.assert_allclose(rm64, rm.numpy(), **tol)
    np.testing.assert_allclose(rv64, rv.numpy(), **tol)                                   # the UNBIASED variance moves running_var
    np.testing.assert_allclose(dz64, zt.grad.numpy().reshape(C, rows).T, **tol)
    np.testing.assert_allclose(dg64, gt.grad.numpy(), **tol)
    np.testing.assert_allclose(db64, bt.grad.numpy(), **tol)
    # the fp32 chain (reductions -> finishers -> elementwise kernels) computes the same thing, to fp32 accuracy
    z32, da32, g32, b32 = (v.astype(np.float32) for v in (z, da, gamma, beta))
    a64, mean, var, rm64, rv64 = ru.bn_train_fwd64(z32, g32, b32, 1e-5, momentum, rm0, rv0)
    dz64, dg64, db64 = ru.bn_relu_bwd64(z32, da32, g32, b32)
    nparts = ru.reduce_parts(rows)
    mean32, rm32 = ru.fin_mean_f32(ru.col_reduce_f32(0, z32, nparts)[0], rows, momentum, rm0.astype(np.float32))
    stat = np.concatenate([mean32, np.zeros(C, dtype=np.float32)])
    rstd32, rv32 = ru.fin_var_f32(ru.col_reduce_f32(1, z32, nparts, stat)[0], rows, momentum, rv0.astype(np.float32))
    stat[C:] = rstd32
    gg, gb, m = ru.fin_bn_bwd_f32(ru.col_reduce_f32(2, z32, nparts, stat, g32, b32, da32), rows, 0, None, None)
    f32 = dict(rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(mean32, mean, **f32)
    np.testing.assert_allclose(rstd32, 1 / np.sqrt(var + 1e-5), **f32)
    np.testing.assert_allclose(rm32, rm64, **f32)
    np.testing.assert_allclose(rv32, rv64, **f32)
    np.testing.assert_allclose(ru.bn_act_f32(z32, mean32, rstd32, g32, b32), a64, **f32)
    np.testing.assert_allclose(gg, dg64, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(gb, db64, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ru.bn_bwd_f32(z32, da32, stat, g32, b32, m), dz64, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("R", (1, 2, 8))
def test_max_and_route_match_torch_max_autograd(R):
    g = np.random.default_rng(R)
    B, px, C = 2, 5, 6
    src = g.integers(0, 3, size=(B, R, px, C)).astype(np.float32)                        # mostly ties
    gmax = g.standard_normal((B * px, C)).astype(np.float32)
    t = torch.tensor(src, **T64, requires_grad=True)
    v, i = torch.max(t, dim=1)
    v.backward(torch.tensor(gmax.reshape(B, px, C), **T64))
    m, w = ru.max_idx_f32(src)
    assert np.array_equal(m, v.detach().numpy().reshape(B * px, C))
    assert np.array_equal(w, i.numpy().reshape(B * px, C)), "the first maximal index wins"
    assert np.array_equal(ru.route_f32(gmax, w, R, B, px).astype(np.float64), t.grad.numpy())
    # NaN: torch.max propagates it
    src[0, R - 1, 0, 0] = np.nan
    m, w = ru.max_idx_f32(src)
    v, i = torch.max(torch.tensor(src), dim=1)
    assert np.isnan(m[0, 0]) and bool(v[0, 0, 0].isnan()) and w[0, 0] == R - 1 == int(i[0, 0, 0])


@pytest.mark.parametrize("stride,up", ((1, 0), (2, 0), (1, 1)))
@pytest.mark.parametrize("Hs,Ws", ((4, 6), (5, 7)))
def test_col2im_and_weight_gradient_match_conv2d_autograd(Hs, Ws, stride, up):
    g = np.random.default_rng(Hs + stride + up)
    n_img, cin, cout = 2, 4, 3
    Ho, Wo = ru.conv_geometry(Hs, Ws, stride, up)
    kp = ru.pad32(9 * cin)
    x = g.integers(-3, 4, size=(n_img, Hs, Ws, cin)).astype(np.float64)                  # NHWC
    W = g.integers(-3, 4, size=(cout, cin, 3, 3)).astype(np.float64)
    G = g.integers(-3, 4, size=(n_img * Ho * Wo, cout)).astype(np.float64)               # dZ, rows (img, oy, ox)
    xt = torch.tensor(x.transpose(0, 3, 1, 2).copy(), requires_grad=True)
    wt = torch.tensor(W, requires_grad=True)
    inp = F.interpolate(xt, scale_factor=2, mode="nearest") if up else xt
    y = F.conv2d(inp, wt, stride=stride, padding=1)
    assert y.shape == (n_img, cout, Ho, Wo)
    y.backward(torch.tensor(G.reshape(n_img, Ho, Wo, cout).transpose(0, 3, 1, 2).copy()))
    # dcol = dZ W', W' tap-major
    Wt = np.zeros((cout, kp))
    Wt[:, :9 * cin] = W.reshape(cout, cin, 9).transpose(0, 2, 1).reshape(cout, 9 * cin)
    dcol = (G @ Wt).astype(np.float32)
    dcol[:, 9 * cin:] = np.nan
    want = xt.grad.numpy().transpose(0, 2, 3, 1).reshape(-1, cin)
    got = ru.col2im_f32(dcol, cin, n_img, Hs, Ws, stride, up, Ho, Wo)
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(ru.col2im_transpose64(dcol, cin, n_img, Hs, Ws, stride, up, Ho, Wo), want)
    # ... and the weight gradient: dW' = dZ^T col, tap-major (n, tap cin + c) -> (Cout, Cin, 3, 3)
    col = im2col_numpy(x.astype(np.float32), 0, cin, n_img, Hs, Ws, stride, up, Ho, Wo, kp)
    part = np.full((2, 4, kp), np.nan, dtype=np.float32)                                  # two splits of a four-row operand
    half = (n_img * Ho * Wo) // 2
    part[0, :cout], part[1, :cout] = G[:half].T @ col[:half], G[half:].T @ col[half:]
    part[:, :, 9 * cin:] = np.nan
    gw = ru.wgrad_reduce_f32(part, 2, 4 * kp, kp, cin, cout, 0, None)
    assert np.array_equal(gw.reshape(cout, cin, 3, 3).astype(np.float64), wt.grad.numpy())


def test_col2im_is_the_transpose_of_im2col_on_every_case():
    """<col2im(dcol), x> = <dcol, im2col(x)> entry by entry: the gather restatement against the transposition of
    conv_ref.im2col_numpy, exactly (integer data), on the GPU tests' own cases"""
    for c in ru.COL_CASES:
        d = ru.build_col(c)
        got = ru.col2im_f32(d["dcol"], c.cin, c.n_img, c.Hs, c.Ws, c.stride, c.up, d["Ho"], d["Wo"])
        want = ru.col2im_transpose64(d["dcol"], c.cin, c.n_img, c.Hs, c.Ws, c.stride, c.up, d["Ho"], d["Wo"])
        assert np.array_equal(got.astype(np.float64), want), c


def test_tanh_backward_matches_torch_with_the_layout_map():
    c = ru.TANH_CASES[0]
    d = ru.build_tanh(c)
    px = c.H * c.W
    g = np.random.default_rng(0)
    pre = g.standard_normal((c.B, 3, c.H, c.W))
    t = torch.tensor(pre, requires_grad=True)
    out = torch.tanh(t)
    out.backward(torch.tensor(d["g_out"].astype(np.float64).reshape(c.B, 3, c.H, c.W)))
    y_nhwc = out.detach().numpy().transpose(0, 2, 3, 1).reshape(c.B * px, 3)
    want = t.grad.numpy().transpose(0, 2, 3, 1).reshape(c.B * px, 3)
    np.testing.assert_allclose(ru.tanh_bwd64(y_nhwc, d["g_out"]), want, rtol=1e-12, atol=1e-14)
    f = ru.tanh_bwd_f32(y_nhwc.astype(np.float32), d["g_out"])
    np.testing.assert_allclose(f[:, :3], want, rtol=1e-5, atol=1e-6)
    assert not f[:, 3:].any() and not np.signbit(f[:, 3:]).any()
    assert np.array_equal(ru.nhwc3_to_nchw_ref(y_nhwc, c.B, px).reshape(c.B, 3, c.H, c.W), out.detach().numpy())


def test_fwd_reduce_form_sums_in_double():
    d = ru.build_fwd(ru.FWD_CASES[-2])
    c = ru.FWD_CASES[-2]
    pre = ru.fwd_pre_f32(d["part"], c.splits, d["split_stride"], d["np"], c.cout, d["bias"], c.M)
    blk = d["part"][:, :c.M * d["np"]].reshape(c.splits, c.M, d["np"])[:, :, :c.cout].astype(np.float64)
    assert np.array_equal(pre, (blk.sum(0) + d["bias"]).astype(np.float32))             # exact in double: any order


def test_reduce_partitions_as_documented():
    """64-row partitions up to the cap; past it ceil(rows / 256) rows each, a ragged last one and empty ones"""
    assert [ru.reduce_parts(r) for r in (2, 63, 64, 65, 257, 16384, 16448, 20000)] == [1, 1, 1, 2, 5, 256, 256, 256]
    assert ru.rows_per_part(16448, 256) == 65 and 253 * 65 < 16448 <= 254 * 65          # partitions 254 and 255 are empty
    assert ru.rows_per_part(20000, 256) == 79
    lib = hooks.load()
    for r in (1, 2, 63, 64, 65, 257, 16384, 16385, 16448, 20000, 1 << 31):
        assert lib.nsr_test_refine_reduce_parts(r) == ru.reduce_parts(r)


# ------------------------------------------------------------------------------------------------------------------------
# the hook library
# ------------------------------------------------------------------------------------------------------------------------
NEW_HOOKS = [n for n in hooks.SIGNATURES if n.startswith("nsr_test_refine_")]


def test_hook_library_exports_the_refine_train_wrappers():
    lib = hooks.load()
    assert len(NEW_HOOKS) == 16
    out = subprocess.run(["nm", "-D", "--defined-only", nsr_build.TEST_HOOKS_LIB], capture_output=True, text=True, check=True).stdout
    hooked = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_HOOKS) <= hooked
    for n in NEW_HOOKS:
        assert hasattr(lib, n)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    product = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in product if "refine_col_reduce" in s or s.startswith("nsr_test_")], "the launchers stay internal"


A = 4096          # a plausible, 16-byte aligned, never dereferenced address


def _calls():
    """name -> (valid-looking arguments without the stream, indices of the pointers that must not be null,
    {index: misaligned value}); every call below fails a check, so no pointer is ever dereferenced"""
    n = ctypes.c_int()
    return {
        "nsr_test_refine_col_reduce": ([2, A, 8, A, 8, A, A, A, 4, 8, A, ctypes.byref(n)], [1, 3, 5, 6, 7, 10, 11], {1: A + 2, 10: A + 1}),
        "nsr_test_refine_fin_mean": ([A, 1, 8, 4, 0.1, A, A], [0, 5], {0: A + 2, 5: A + 2, 6: A + 2}),
        "nsr_test_refine_fin_var": ([A, 1, 8, 4, 0.1, 1e-5, A, A], [0, 6], {0: A + 2, 6: A + 2, 7: A + 2}),
        "nsr_test_refine_fin_bn_bwd": ([A, 1, 8, 4, 0, A, A, A], [0, 5, 6, 7], {0: A + 2, 5: A + 2, 6: A + 2, 7: A + 2}),
        "nsr_test_refine_fin_bias": ([A, 1, 8, 3, 0, A], [0, 5], {0: A + 2, 5: A + 2}),
        "nsr_test_refine_bn_relu": ([A, A, A, A, 4, 8, A, 8], [0, 1, 2, 3, 6], {0: A + 4, 1: A + 8, 2: A + 4, 3: A + 4, 6: A + 12, 7: 10, 5: 6}),
        "nsr_test_refine_bn_bwd": ([A, A, 8, A, A, A, A, 4, 8, A], [0, 1, 3, 4, 5, 6, 9], {0: A + 4, 1: A + 8, 9: A + 4, 2: 10, 8: 6}),
        "nsr_test_refine_relu_bwd": ([A, A, 4, A], [0, 1, 3], {0: A + 2, 1: A + 1, 3: A + 3}),
        "nsr_test_refine_tanh_bwd": ([A, A, 4, 8, A], [0, 1, 4], {0: A + 2, 1: A + 2, 4: A + 2}),
        "nsr_test_refine_max_idx": ([A, 8, 2, 4, 1, A, 8, A], [0, 5, 7], {0: A + 2, 5: A + 2}),
        "nsr_test_refine_route": ([A, 8, A, 8, 2, 4, 1, A], [0, 2, 7], {0: A + 2, 7: A + 2}),
        "nsr_test_refine_col2im": ([A, 96, 8, 1, 4, 4, 1, 0, 4, 4, 0, A, 8], [0, 11], {0: A + 4, 11: A + 8, 12: 10, 2: 6}),
        "nsr_test_refine_wgrad_reduce": ([A, 1, 1024, 96, 8, 8, 0, A], [0, 7], {0: A + 2, 7: A + 2}),
        "nsr_test_refine_fwd_reduce": ([A, 1, 1024, 32, 8, A, 0, 4, A, 8], [0, 5, 8], {0: A + 2, 5: A + 2, 8: A + 2}),
        "nsr_test_refine_nhwc3_to_nchw": ([A, 4, 1, A], [0, 3], {0: A + 2, 3: A + 2}),
    }


@pytest.mark.parametrize("name", sorted(_calls()))
def test_wrappers_reject_null_and_misaligned_pointers_without_a_device(name):
    lib = hooks.load()
    args, ptrs, bad = _calls()[name]
    fn = getattr(lib, name)
    for i in ptrs:
        a = list(args)
        a[i] = None
        assert fn(*a, None) == INV, (name, "null", i)
    for i, v in bad.items():
        a = list(args)
        a[i] = v
        assert fn(*a, None) == INV, (name, "misaligned", i)


def test_every_wrapper_has_a_rejection_case():
    assert set(_calls()) == set(NEW_HOOKS) - {"nsr_test_refine_reduce_parts"}


# ------------------------------------------------------------------------------------------------------------------------
# sensitivity: the case lists of the GPU tests tell every wrong kernel from the right one
# ------------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    if isinstance(a, dict):
        return any(_differs(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return any(_differs(x, y) for x, y in zip(a, b))
    if a is None or np.isscalar(a):
        return a != b
    return not bool(ru.same_bits(a, b).all())


def _sensitive(cases, build, expected, mut):
    """the cases whose expected result changes under `mut`"""
    hit = []
    for c in cases:
        d = build(c)
        if _differs(expected(c, d), expected(c, d, mut)):
            hit.append(c)
    return hit


SMALL_REDUCE = [c for c in ru.REDUCE_CASES if c.rows <= 257]       # the large cases repeat the small ones' data rules


@pytest.mark.parametrize("unit,cases,build,expected,muts", [
    ("reduce", SMALL_REDUCE, ru.build_reduce, ru.reduce_expected, ("biased_running_var", "mean_wrong_pass", "no_acc", "no_ch0")),
    ("bn_relu", ru.BN_CASES, ru.build_bn, ru.bn_relu_expected, ("no_ch0",)),
    ("bn_bwd", ru.BN_CASES, ru.build_bn, ru.bn_bwd_expected, ("no_ch0",)),
    ("max_idx", ru.MAX_CASES, ru.build_max, ru.max_expected, ("last_winner", "nan_loses", "no_ch0")),
    ("route", ru.MAX_CASES, ru.build_max, ru.route_expected, ("no_ch0",)),
    ("col2im", ru.COL_CASES, ru.build_col, ru.col2im_expected, ("swap_k", "one_up", "no_stride", "no_acc", "no_ch0")),
    ("wgrad_reduce", ru.WGRAD_CASES, ru.build_wgrad, ru.wgrad_expected, ("wgrad_transpose", "no_acc")),
    ("fwd_reduce", ru.FWD_CASES, ru.build_fwd, ru.fwd_expected, ("fwd_sum_f32", "no_ch0")),
], ids=lambda v: v if isinstance(v, str) else None)
def test_case_lists_catch_every_mutation(unit, cases, build, expected, muts):
    for mut in muts:
        assert mut in ru.MUTATIONS
        hit = _sensitive(cases, build, expected, mut)
        assert hit, f"{unit}: no case of the GPU test tells the '{mut}' kernel from the right one"
        if mut == "fwd_sum_f32":
            assert any(c.data == "cancel" for c in hit)
        if mut == "last_winner":
            assert any(c.data == "ties" for c in hit) and any(c.data == "zeros" for c in hit)
        if mut == "nan_loses":
            assert all(c.data == "nan" for c in hit)
        if mut == "no_stride":
            assert all(c.stride == 2 for c in hit) and any(c.Hs % 2 for c in hit)
        if mut == "one_up":
            assert all(c.up for c in hit)


def test_every_mutation_is_applied_somewhere():
    used = {"biased_running_var", "mean_wrong_pass", "no_acc", "no_ch0", "last_winner", "nan_loses", "swap_k", "one_up", "no_stride",
            "wgrad_transpose", "fwd_sum_f32"}
    assert used == set(ru.MUTATIONS)


def test_exact_reduce_cases_are_exact():
    """the integer cases: mean, centred sum of squares and both backward sums are exact in fp32 in ANY order, so the
    order-restating form equals plain fp64 arithmetic"""
    for c in SMALL_REDUCE:
        if c.kind != "int":
            continue
        d = ru.build_reduce(c)
        e = ru.reduce_expected(c, d)
        x = ru.own(d["X"], c.rows, c.ch0, c.C).astype(np.float64)
        da = ru.own(d["DA"], c.rows, c.ch0, c.C).astype(np.float64)
        assert np.array_equal(e["mean"].astype(np.float64), x.mean(0))
        assert np.array_equal(ru.part_sum64(e["part1"][0]), ((x - x.mean(0)) ** 2).sum(0))
        mean, rstd = d["stat2"][:c.C].astype(np.float64), d["stat2"][c.C:].astype(np.float64)
        xhat = (x - mean) * rstd
        dy = np.where(d["gamma"] * xhat + d["beta"] > 0, da, 0.0)
        assert np.array_equal(e["g_beta", 0].astype(np.float64), dy.sum(0))
        assert np.array_equal(e["g_gamma", 0].astype(np.float64), (dy * xhat).sum(0))
        assert np.array_equal(e["g_beta", 1].astype(np.float64), dy.sum(0) + d["g_beta0"])
        assert np.array_equal(e["m"].astype(np.float64), np.concatenate([dy.sum(0), (dy * xhat).sum(0)]) / c.rows)
