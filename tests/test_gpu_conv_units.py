"""Unit layer under the refinement network: ONE convolution at a time through every kernel instantiation gemm_f16x3 can pick
(csrc/nsr_gemm_f16.hip: conv_halo_kernel's eleven reachable shapes and the conv-gather mode of gemm_f16x3_kernel), the
explicit im2col of nsr_refine_conv.h and the packed weight blob (pack_conv_kernel, stream_order_kernel, l0_stream_kernel).

Method: tests/conv_ref.py.  The exact cases feed integer hi planes and INDEPENDENT integer x 2^-8 lo planes, for which the
three-term split product is exact in fp32 in any order; the raw 16-bit output planes must equal the fp64 reference bit for bit
(torch.equal on whole buffers, sentinel surroundings included), so one wrong tap at one block border, one weight slot read
before it was published or one row stored to the wrong image shows.  Every case first asserts the instantiation the dispatch
picks (nsr_test_gemm_f16x3_route): a changed threshold fails here instead of silently moving coverage to another kernel.  The
only tolerance among the exact cases is the tail's: its pre-activation is exact and tanhf is held to 4 ulp of the fp64 tanh,
the figure tests/test_gpu_gemm_units.py::derived_bound uses.

The real-input cases (randn) hold one layer per kernel family to that derived bound and print err / bound (run with -s;
recorded in DESIGN.md), and check the dispatch comment's claim that the halo shapes are bit-identical among themselves.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import hooks
from tests.conv_ref import Case, im2col_numpy
from tests.test_gpu_gemm_units import _ulp32, derived_bound, split_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return hooks.load()


@pytest.fixture(scope="module")
def nsr():
    from nerf_sr_amd import _lib
    return _lib.load()


def launch(hk, c: Case, o: cr.Operands):
    """the case on the device: asserts the route, runs gemm_f16x3, returns the whole output buffers (CPU)"""
    dev = [t.cuda() if t is not None else None for t in (o.A, o.Bh, o.Bl, o.Bs, o.bias)]
    C, Mx = cr.empty_outputs(c)
    C = C.cuda()
    Mx = None if Mx is None else Mx.cuda()
    a = cr.fill_args(c, o, *(hooks.ptr(t) for t in dev), hooks.ptr(C), hooks.ptr(Mx))
    route = cr.route_of(hk, a)
    assert route == c.route, f"{c.name}: dispatch picked {hooks.ROUTE_NAMES.get(route, route)}, the case is built for {hooks.ROUTE_NAMES[c.route]}"
    rc = hk.nsr_test_gemm_f16x3(ctypes.byref(a), hooks.stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{c.name}: gemm_f16x3 returned {rc}"
    return C.cpu(), None if Mx is None else Mx.cpu()


def assert_same(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = tuple(bad[0].tolist())
    lo, hi = bad.min(0).values.tolist(), bad.max(0).values.tolist()
    raise AssertionError(f"{what}: {len(bad)} of {want.numel()} elements differ; first at {first}: got {got[first].item()!r}, want "
                         f"{want[first].item()!r}; index ranges {list(zip(lo, hi))} (planes: [plane, row incl. {cr.GUARD_ROWS} guard rows, column])")


def reference_values(c: Case, o: cr.Operands):
    """fp64 reference of the case, after the exact-regime assertion"""
    cr.assert_exact_regime(o)
    pre = cr.pre_activation(o)
    return pre if c.tail else torch.relu(pre)


def check_exact(hk, c: Case):
    o = cr.build_operands(c)
    v = reference_values(c, o)
    C, Mx = launch(hk, c, o)
    if c.tail:
        check_tail(c, v, C)
        return None
    wantC, wantM = cr.expected_outputs(c, v)
    assert_same(C, wantC, c.name + " output planes")
    if wantM is not None:
        assert_same(Mx, wantM, c.name + " max planes")
    return C, Mx


def check_tail(c: Case, pre, C):
    """fp32 NHWC output: columns < n_valid of the owned rows within 4 ulp of the fp64 tanh of the EXACT pre-activation,
    everything else (guard rows; with ldc = n_valid a store to column n_valid would land in the next row) untouched"""
    assert torch.equal(pre.float().double(), pre)
    want = torch.tanh(pre[:, :c.nv])
    got = C[cr.GUARD_ROWS:cr.GUARD_ROWS + c.M].double()
    err = (got - want).abs()
    tol = 4 * _ulp32(want)
    assert bool((err <= tol).all()), f"{c.name}: tanh output off by up to {float((err / tol).max()):.2f} x (4 ulp)"
    rest = C.clone()
    rest[cr.GUARD_ROWS:cr.GUARD_ROWS + c.M] = cr.SENT32
    assert bool((rest == cr.SENT32).all()), c.name + ": wrote outside its rows"


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------------------------------
# exact cases: every route
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", (16, 32, 48, 128))
def test_half_plain_s1_exact(hk, cin):
    """<4, 2, false, 1>: 1, 2, 3 and 8 channel chunks x (one block with all four borders | 2 x 3 blocks) x (1 | 3 images) x
    (plain | through the x2 upsample)"""
    cases = [c for c in cr.HALF_S1 if c.cin == cin]
    assert len(cases) == 8
    for c in cases:
        check_exact(hk, c)


@pytest.mark.parametrize("c", cr.HALF_S1_WIDE, ids=_ids(cr.HALF_S1_WIDE))
def test_half_plain_s1_column_tiles_exact(hk, c):
    check_exact(hk, c)


@pytest.mark.parametrize("c", cr.HALF_GROUPED_S1, ids=_ids(cr.HALF_GROUPED_S1))
def test_half_grouped_s1_exact(hk, c):
    check_exact(hk, c)


@pytest.mark.parametrize("c", cr.MULTI_S1 + cr.MULTI_S2, ids=_ids(cr.MULTI_S1 + cr.MULTI_S2))
def test_multi_exact(hk, c):
    """eight plain images per block; a batch that is no multiple of eight ends in a block whose missing images are gathered
    clamped and must never be stored: the guard rows behind image n_img - 1 keep the sentinel"""
    check_exact(hk, c)


@pytest.mark.parametrize("c", cr.HALF_S2 + cr.HALF_GROUPED_S2, ids=_ids(cr.HALF_S2 + cr.HALF_GROUPED_S2))
def test_half_s2_exact(hk, c):
    check_exact(hk, c)


@pytest.mark.parametrize("c", cr.BIG, ids=_ids(cr.BIG))
def test_big_tiles_exact(hk, c):
    """the instantiations the dispatch reaches only between 129 and 256 big blocks"""
    check_exact(hk, c)


@pytest.mark.parametrize("c", cr.TAIL, ids=_ids(cr.TAIL))
def test_tail_exact_preactivation(hk, c):
    check_exact(hk, c)


@pytest.mark.parametrize("route,cin,N", cr._STAGED_VARIANTS)
def test_staged_exact(hk, route, cin, N):
    """Bs = null: the staged gather, on shapes no halo block fits (6 x 10, 12 x 20), stride 2 from an odd source, the
    upsample, grouped rows with a ragged last row tile, and n_valid < N (the general epilogue)"""
    cases = [c for c in cr.STAGED if c.route == route]
    assert len(cases) == 6
    for c in cases:
        check_exact(hk, c)


@pytest.mark.parametrize("c", cr.STAGED_WIDE, ids=_ids(cr.STAGED_WIDE))
def test_staged_wide_exact(hk, c):
    check_exact(hk, c)


def test_halo_and_staged_agree_on_exact_case(hk):
    """the same operands through the halo route and, with Bs = null, through the staged route: equal planes (both equal the
    reference)"""
    for c in (cr.HALF_S1[9], cr.HALF_GROUPED_S1[1]):
        assert c.cin == 32
        halo = check_exact(hk, c)
        st = check_exact(hk, Case(c.name + "_staged", hooks.ROUTE_STAGED_K32_FULL, c.cin, c.N, c.n_img, c.Hs, c.Ws, c.stride, c.up,
                                  group=c.group, bs=False, seed=c.seed))
        assert torch.equal(halo[0], st[0])
        if c.group:
            assert torch.equal(halo[1], st[1])


# ------------------------------------------------------------------------------------------------------------------------
# NaN footprint
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,img,y,x", [(cr.HALF_GROUPED_S1[0], 3, 3, 4), (cr.HALF_GROUPED_S1[0], 5, 0, 0), (cr.HALF_S1[8], 0, 15, 15),
                                          (cr.HALF_S1[9], 0, 0, 7)], ids=("grouped_interior", "grouped_corner", "plain_corner", "plain_up_corner"))
@pytest.mark.parametrize("bs", (True, False), ids=("halo", "staged"))
def test_single_nan_poisons_exactly_its_footprint(hk, base, img, y, x, bs):
    """one NaN element in the hi plane of the input: NaN in all N columns, hi and lo, of exactly the outputs whose 3 x 3 window
    covers it (and in the max plane of those pixels); every other output still equals the reference bit for bit.  At an
    image corner the zeroed padding fragments must neither launder the NaN nor spread it."""
    c = base if bs else Case(base.name + "_staged", hooks.ROUTE_STAGED_K32_FULL, base.cin, base.N, base.n_img, base.Hs, base.Ws,
                             base.stride, base.up, group=base.group, bs=False, seed=base.seed)
    assert c.cin == 32 and c.stride == 1
    o = cr.build_operands(c)
    v = reference_values(c, o)
    wantC, wantM = cr.expected_outputs(c, v)
    o.A[0, 1 + img, y, x, o.ch0 + 5] = cr.NAN16
    C, Mx = launch(hk, c, o)
    s = 2 if c.up else 1                                   # source pixel (y, x) = upsampled pixels s y .. s y + s - 1
    hit = torch.zeros(c.n_img, c.Ho, c.Wo, dtype=torch.bool)
    hit[img, max(s * y - 1, 0):s * y + s + 1, max(s * x - 1, 0):s * x + s + 1] = True
    _, co, _, mo = cr.output_geometry(c)
    rows = slice(cr.GUARD_ROWS, cr.GUARD_ROWS + c.M)
    mask = torch.zeros_like(C, dtype=torch.bool)
    mask[:, rows, co:co + c.N] = hit.view(1, -1, 1)
    assert bool(cr.bits_f64(C[mask]).isnan().all()), "an output under the NaN's footprint is not NaN"
    assert_same(torch.where(mask, wantC, C), wantC, c.name + " outputs outside the footprint")
    if c.group:
        mmask = torch.zeros_like(Mx, dtype=torch.bool)
        mhit = hit.view(c.n_img // 8, 8, -1).any(1)
        mmask[:, cr.GUARD_ROWS:cr.GUARD_ROWS + c.M // 8, mo:mo + c.N] = mhit.view(1, -1, 1)
        assert bool(cr.bits_f64(Mx[mmask]).isnan().all()), "the max over a group with a NaN member is not NaN"
        assert_same(torch.where(mmask, wantM, Mx), wantM, c.name + " max planes outside the footprint")


# ------------------------------------------------------------------------------------------------------------------------
# real inputs
# ------------------------------------------------------------------------------------------------------------------------
def real_operands(nsr, c: Case, seed):
    """randn activations (split into planes like a producing epilogue does) and randn / sqrt(K) weights split by nsr_split_weights"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(c.n_img, c.Hs, c.Ws, c.cin, generator=gen)
    w = torch.randn(c.N, c.K, generator=gen) / c.K ** 0.5
    bias = torch.randn(c.N, generator=gen)
    xh, xl = cr.split_planes(x.numpy())
    ah, al = cr.bits_f64(xh), cr.bits_f64(xl)
    hi, lo = split_weights(nsr, w)
    bh, bl = cr.bits_f64(hi), cr.bits_f64(lo)
    ch0 = 16
    ld = ch0 + c.cin + 8
    Bh, Bl, ldbh = cr.build_weights(bh, bl)
    Bs = torch.from_numpy(cr.stream_order(Bh[:, :c.K].numpy(), Bl[:, :c.K].numpy(), c.cin)) if c.bs else None
    o = cr.Operands(c, ah, al, bh, bl, bias, cr.build_planes(ah, al, ld, ch0), ld, ch0, Bh, Bl, ldbh, Bs)
    o.extra["w"] = w
    return o


def first_images(o: cr.Operands, c_small: Case) -> cr.Operands:
    """the operands of the first c_small.n_img images of `o`, same weights (the image behind them serves as the guard image)"""
    n = c_small.n_img
    return cr.Operands(c_small, o.ah[:n], o.al[:n], o.bh, o.bl, o.bias, o.A[:, :n + 2].contiguous(), o.ld, o.ch0, o.Bh, o.Bl, o.ldbh, o.Bs)


@pytest.mark.parametrize("big,n_small,half_route", [(cr.BIG[0], 2, hooks.ROUTE_HALF_S1), (cr.BIG[2], 8, hooks.ROUTE_HALF_GROUPED_S1),
                                                    (cr.BIG[1], 8, hooks.ROUTE_HALF_GROUPED_S1)], ids=("plain_8x2", "grouped_4x4", "grouped_8x2"))
def test_half_and_big_tiles_bit_identical_on_real_inputs(hk, nsr, big, n_small, half_route):
    """csrc/nsr_gemm_f16.hip, dispatch comment: "the halo shapes among themselves are bit-identical (same k-steps, same order per
    output element)" -- what lets a patch set give the same bits whatever batch it arrives in.  One randn layer at a batch
    where the rule picks the big tile and at one where it picks the half tile: the common images (and their max planes) match."""
    o = real_operands(nsr, big, 7)
    Cb, Mb = launch(hk, big, o)
    small = Case(big.name + "_small", half_route, big.cin, big.N, n_small, big.Hs, big.Ws, big.stride, big.up, group=big.group)
    Cs, Ms = launch(hk, small, first_images(o, small))
    rows = slice(cr.GUARD_ROWS, cr.GUARD_ROWS + small.M)
    assert torch.equal(Cs[:, rows], Cb[:, rows])
    assert not bool((Cs[:, rows, 6:6 + big.N] == int(cr.SENT16)).all())
    if big.group:
        mrows = slice(cr.GUARD_ROWS, cr.GUARD_ROWS + small.M // 8)
        assert torch.equal(Ms[:, mrows], Mb[:, mrows])


REAL_CASES = [
    Case("real_half_s1", hooks.ROUTE_HALF_S1, 128, 128, 2, 32, 32),
    Case("real_half_grouped_s1", hooks.ROUTE_HALF_GROUPED_S1, 64, 128, 8, 8, 16, group=8),
    Case("real_multi_s2", hooks.ROUTE_MULTI_S2, 128, 128, 9, 16, 16, 2),
    Case("real_half_s2", hooks.ROUTE_HALF_S2, 128, 128, 2, 64, 32, 2),
    Case("real_staged_k64", hooks.ROUTE_STAGED_K64, 64, 160, 3, 12, 20, bs=False),
    Case("real_staged_k32_grouped", hooks.ROUTE_STAGED_K32_FULL, 32, 128, 8, 6, 10, group=8, bs=False),
    Case("real_tail", hooks.ROUTE_HALO_TAIL, 128, 64, 2, 32, 16, tail=True, n_valid=3),
]


def test_real_inputs_within_derived_bound(hk, nsr):
    """One randn layer per kernel family against the fp64 convolution of the values the planes hold (x = xh + xl) with the fp32
    weights.  Bound: derived_bound with K = 9 cin and eps_products = 2^-21 (the split scheme's dropped lo x lo term and the
    second-rounding residuals, tests/test_gpu_gemm_units.py::test_linear_f16x3_real_inputs_within_derived_bound; the 2^6 weight
    scale and acc_scale = 2^-6 are powers of two and cancel exactly).  Plane outputs add the output split's own error: hi + lo
    represents v to 2^-22 |v| (lo = RNE16(v - hi), |v - hi| <= 2^-11 |v|, one more rounding at 2^-11 relative) or, where lo is
    an fp16 subnormal, to half its spacing, 2^-25."""
    worst = 0.0
    for i, c in enumerate(REAL_CASES):
        o = real_operands(nsr, c, 50 + i)
        x, w = o.ah + o.al, o.extra["w"]
        pre = cr.conv64(x, w, c.stride, c.up) + o.bias.double()
        ref = torch.tanh(pre) if c.tail else torch.relu(pre)
        absprod = cr.conv64(x.abs(), w.abs(), c.stride, c.up)
        atol = derived_bound(absprod, o.bias, c.K, hooks.ACT_TANH if c.tail else hooks.ACT_RELU, ref, eps_products=2.0 ** -21)
        C, Mx = launch(hk, c, o)
        _, co, _, mo = cr.output_geometry(c)
        rows = slice(cr.GUARD_ROWS, cr.GUARD_ROWS + c.M)
        if c.tail:
            got = C[rows].double()
            ref, atol = ref[:, :c.nv], atol[:, :c.nv]
        else:
            got = cr.bits_f64(C[0, rows, co:co + c.N]) + cr.bits_f64(C[1, rows, co:co + c.N])
            atol = atol + 2.0 ** -22 * (ref.abs() + atol) + 2.0 ** -25
        err = (got - ref).abs()
        ratio = float((err / atol).max())
        print(f"conv f16x3 real inputs {c.name} ({hooks.ROUTE_NAMES[c.route]}): max err {float(err.max()):.3e}, max err / bound {ratio:.4f}")
        worst = max(worst, ratio)
        assert bool((err <= atol).all()), (c.name, ratio)
        if c.group:      # the max planes hold the split of the maximum of the values the member planes hold
            gotm = cr.bits_f64(Mx[0, cr.GUARD_ROWS:cr.GUARD_ROWS + c.M // 8, mo:mo + c.N]) + cr.bits_f64(Mx[1, cr.GUARD_ROWS:cr.GUARD_ROWS + c.M // 8, mo:mo + c.N])
            assert torch.equal(gotm, cr.grouped_max(got, c)), c.name + ": max plane is not the maximum of the member planes"
    print(f"conv f16x3 real inputs: largest err / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------------------
# explicit im2col
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchw,cin,ld,ch0,n_img,Hs,Ws,stride,up", [
    (1, 3, 0, 0, 2, 6, 10, 1, 0),          # the first layer: kp = 32, five zero tail columns
    (1, 3, 0, 0, 3, 16, 16, 1, 0),
    (0, 128, 384, 128, 2, 6, 10, 1, 0),    # a slice of a concatenated buffer
    (0, 128, 384, 128, 2, 6, 10, 2, 0),
    (0, 128, 384, 128, 2, 5, 7, 2, 0),     # stride 2 from an odd source
    (0, 128, 384, 128, 2, 6, 10, 1, 1),
    (0, 32, 48, 8, 3, 8, 8, 2, 0),
    (0, 6, 8, 0, 2, 6, 10, 1, 1),          # cin % 4 != 0: the scalar path of the NHWC kernel
])
def test_im2col_exact(hk, nchw, cin, ld, ch0, n_img, Hs, Ws, stride, up):
    gen = torch.Generator().manual_seed(cin + Hs + stride + up)
    Hin, Win = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    Ho, Wo = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    kp = (9 * cin + 31) // 32 * 32
    if nchw:
        src = torch.randn(n_img, cin, Hs, Ws, generator=gen)
        buf, view = src.clone(), src.numpy()
    else:
        buf = torch.full((n_img, Hs, Ws, ld), float("nan"))
        buf[..., ch0:ch0 + cin] = torch.randn(n_img, Hs, Ws, cin, generator=gen)
        view = buf[..., ch0:ch0 + cin].numpy()
    want = torch.from_numpy(im2col_numpy(view, nchw, cin, n_img, Hs, Ws, stride, up, Ho, Wo, kp))
    M = n_img * Ho * Wo
    d = buf.cuda()
    col = torch.full((M + 8, kp), cr.SENT32).cuda()
    rc = hk.nsr_test_im2col(hooks.ptr(d, ch0), nchw, ld, cin, n_img, Hs, Ws, stride, up, Ho, Wo, kp, hooks.ptr(col), hooks.stream())
    torch.cuda.synchronize()
    assert rc == 0
    col = col.cpu()
    assert torch.equal(col[:M], want)
    assert bool((col[M:] == cr.SENT32).all())
    assert bool((want[:, 9 * cin:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------
# packed blob
# ------------------------------------------------------------------------------------------------------------------------
def _pad32(n):
    return (n + 31) // 32 * 32


class Blob:
    """mirror of the blob arithmetic of csrc/nsr_refine.hip: per layer W' (npad x kpad) | b' (npad) | stream-ordered W' (streamed
    layers, same size) | layer 0: its 16-channel stream (npad x 9 x 16 halves x 2 planes)"""

    def __init__(self, noref):
        from nerf_sr_amd import refine
        self.layers = []
        off = 0
        for l, (name, cin, cout, bn) in enumerate(refine.LAYERS):
            if noref:
                cin = refine.NOREF_CIN.get(name, cin)
            relu = l != len(refine.LAYERS) - 1                      # the last layer ends in tanh
            last_tanh = not relu and cout <= 64 and cin % 16 == 0
            kp, np_ = _pad32(9 * cin), (64 if last_tanh else _pad32(cout))
            streamed = kp == 9 * cin and ((cin % 16 == 0 and cout % 128 == 0 and relu) or last_tanh)
            self.layers.append(dict(name=name, cin=cin, cout=cout, bn=bn, kp=kp, np=np_, streamed=streamed, off=off))
            off += np_ * kp * (2 if streamed else 1) + np_ + (np_ * 9 * 16 if l == 0 else 0)
        self.floats = off


@pytest.fixture(scope="module", params=(False, True), ids=("ref", "noref"))
def packed(request):
    """both precisions' blobs of one synthetic state dict, through MaxPoolingModel.load_state_dict = nsr_refine_pack_weights[_noref]"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import refine
    noref = request.param
    sd = refine.make_refine_state_dict(3, not_use_ref=noref)
    blobs = {}
    for prec in ("fp32", "f16x3"):
        net = refine.MaxPoolingModel(precision=prec, not_use_ref=noref).load_state_dict(sd)
        torch.cuda.synchronize()
        blobs[prec] = net.packed.cpu().numpy()
    return Blob(noref), sd, blobs


def _ulps(a, b):
    """distance in fp32 units in the last place (same-sign finite values)"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_packed_blob_fp32_fold_exact(packed):
    """W'[n][tap cin + c] = s_n W[n][c][tap], b' = (b - mean) s + beta, s = gamma / sqrt(var + eps): the same fp32 operation
    sequence in numpy (correctly rounded sqrt and division), bit for bit; padding rows and columns zero"""
    blob, sd, blobs = packed
    p = blobs["fp32"].view(np.float32)
    assert p.size == blob.floats
    worst_w = worst_b = 0
    for L in blob.layers:
        w, b = sd[L["name"] + ".weight"], sd[L["name"] + ".bias"]
        wt = np.ascontiguousarray(w.reshape(L["cout"], L["cin"], 9).transpose(0, 2, 1)).reshape(L["cout"], 9 * L["cin"])
        if L["bn"]:
            gamma, beta = sd[L["bn"] + ".weight"], sd[L["bn"] + ".bias"]
            mean, var = sd[L["bn"] + ".running_mean"], sd[L["bn"] + ".running_var"]
            s = gamma / np.sqrt(var + np.float32(1e-5))
            assert s.dtype == np.float32
            wt = s[:, None] * wt
            b = (b - mean) * s + beta
        W = p[L["off"]:L["off"] + L["np"] * L["kp"]].reshape(L["np"], L["kp"])
        B = p[L["off"] + L["np"] * L["kp"]:L["off"] + L["np"] * L["kp"] + L["np"]]
        assert not W[L["cout"]:].any() and not W[:, 9 * L["cin"]:].any() and not B[L["cout"]:].any(), L["name"] + ": padding is not zero"
        worst_w = max(worst_w, int(_ulps(W[:L["cout"], :9 * L["cin"]], wt).max()))
        worst_b = max(worst_b, int(_ulps(B[:L["cout"]], b).max()))
    print(f"packed blob fp32: W' differs from the numpy sequence by at most {worst_w} ulp, b' by {worst_b} ulp")
    assert worst_w == 0 and worst_b == 0


def test_packed_blob_f16x3_planes_and_streams_exact(packed):
    """NSR_F16X3 blob: the (hi, lo) planes are the RNE split of 64 x the fp32 blob's W' (whatever the root's rounding), the bias
    is the fp32 blob's, the stream-ordered copy is conv_ref.stream_order of the planes (the layout documented in nsr_gemm.h), and
    layer 0's 16-channel stream is the split of 64 w built from the raw weights"""
    blob, sd, blobs = packed
    p32 = blobs["fp32"].view(np.float32)
    h = blobs["f16x3"].view(np.int16)
    assert h.size == 2 * blob.floats
    n_streamed = 0
    for l, L in enumerate(blob.layers):
        nk = L["np"] * L["kp"]
        W = p32[L["off"]:L["off"] + nk]
        hi, lo = cr.split_planes(W * np.float32(64.0))
        base = 2 * L["off"]
        assert np.array_equal(h[base:base + nk], hi), L["name"] + ": hi plane"
        assert np.array_equal(h[base + nk:base + 2 * nk], lo), L["name"] + ": lo plane"
        assert np.array_equal(h[base + 2 * nk:base + 2 * nk + 2 * L["np"]].view(np.float32), p32[L["off"] + nk:L["off"] + nk + L["np"]]), L["name"] + ": bias"
        if L["streamed"]:
            n_streamed += 1
            want = cr.stream_order(hi.reshape(L["np"], L["kp"]), lo.reshape(L["np"], L["kp"]), L["cin"])
            s0 = base + 2 * (nk + L["np"])
            assert np.array_equal(h[s0:s0 + 2 * nk], want), L["name"] + ": stream-ordered copy"
        if l == 0:
            w = sd[L["name"] + ".weight"].reshape(L["cout"], 3, 9)
            w16 = np.zeros((L["np"], 9, 16), dtype=np.float32)
            w16[:L["cout"], :, :3] = w.transpose(0, 2, 1) * np.float32(64.0)
            sh, sl = cr.split_planes(w16.reshape(L["np"], 144))
            s0 = base + 2 * (nk + L["np"])
            assert not L["streamed"]
            assert np.array_equal(h[s0:s0 + 2 * L["np"] * 144], cr.stream_order(sh, sl, 16)), "layer 0: 16-channel stream"
    assert n_streamed == 18
