"""The convolution unit layer without a device: tests/conv_ref.py checked against itself, and the kernel choice of gemm_f16x3
(gemm_f16x3_route through the hook library, host arithmetic only) for every case tests/test_gpu_conv_units.py runs, for the
argument refusals, for the one instantiation no shape can reach and for every layer of the refinement network."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import hooks
from tests.conv_ref import Case
from tests.test_gpu_conv_units import REAL_CASES
from tests.test_gpu_gemm_units import _f32_exact


@pytest.fixture(scope="module")
def hk():
    return hooks.load()


# ------------------------------------------------------------------------------------------------------------------------
# conv_ref against itself
# ------------------------------------------------------------------------------------------------------------------------
SELF_CASES = [cr.HALF_S1[0], cr.HALF_S1[11], cr.HALF_GROUPED_S1[6], cr.MULTI_S2[0], cr.STAGED[2], cr.STAGED[3]]


@pytest.mark.parametrize("c", SELF_CASES, ids=[c.name for c in SELF_CASES])
def test_three_term_reference_is_full_product_minus_lo_lo(c):
    """acc = conv(ah, bh) + conv(ah, bl) + conv(al, bh) = conv(ah + al, bh + bl) - conv(al, bl), all exact in fp64; and the
    dropped term is not nothing: with it the accumulator differs at (nearly) every output"""
    o = cr.build_operands(c)
    full = cr.conv64(o.ah + o.al, o.bh + o.bl, c.stride, c.up)
    lolo = cr.conv64(o.al, o.bl, c.stride, c.up)
    assert torch.equal(cr.accumulator(o), full - lolo)
    assert torch.equal(cr.accumulator(o, four_terms=True), full)
    assert float((lolo != 0).double().mean()) > 0.9


def test_four_term_and_one_term_kernels_cannot_pass():
    """What a kernel that also multiplied lo x lo (or only hi x hi) would store differs from the reference planes: the lo x lo
    term is a multiple of 2^-22 after the scale, which the lo plane of a small output resolves (|v| < 1/2: hi to 2^-12, lo to
    2^-23), and the two cross terms are multiples of 2^-14."""
    c = cr.HALF_S1[0]
    o = cr.build_operands(c)
    want = cr.expected_outputs(c, torch.relu(cr.pre_activation(o)))[0]
    v4 = torch.relu(cr.pre_activation(o, four_terms=True)).float().double()          # as an fp32 epilogue would hold it
    v1 = torch.relu(cr.conv64(o.ah, o.bh, c.stride, c.up) * cr.ACC_SCALE + o.bias.double())
    for v, what in ((v4, "four"), (v1, "one")):
        hi, lo = cr.split_planes(v.float().numpy())
        rows = slice(cr.GUARD_ROWS, cr.GUARD_ROWS + c.M)
        same = np.array_equal(want[0, rows, 6:6 + c.N].numpy(), hi) and np.array_equal(want[1, rows, 6:6 + c.N].numpy(), lo)
        assert not same, f"a {what}-term kernel would pass the exact cases"
        n_diff = int((want[1, rows, 6:6 + c.N].numpy() != lo).sum() + (want[0, rows, 6:6 + c.N].numpy() != hi).sum())
        assert n_diff > 100, (what, n_diff)


@pytest.mark.parametrize("N,cin", [(32, 16), (128, 48), (64, 128)])
def test_stream_order_round_trips(N, cin):
    """the loop form (written from the layout comment of nsr_gemm.h) and the vectorised inverse agree; every element of B
    appears exactly once, at the documented place"""
    K = 9 * cin
    Bh = np.arange(N * K, dtype=np.int32).reshape(N, K)
    Bl = Bh + N * K
    s = cr.stream_order(Bh, Bl, cin)
    assert s.size == 2 * N * K and len(np.unique(s)) == 2 * N * K
    back = cr.stream_order_inverse(s, N, cin)
    assert np.array_equal(back[0], Bh) and np.array_equal(back[1], Bl)
    # spot check against the sentence itself: unit (nb, cc * 9 + tap), plane, lane li + 32 h, half e
    nb, cc, tap, plane, li, h, e = N // 32 - 1, cin // 16 - 1, 7, 1, 13, 1, 5
    flat = ((((nb * (cin // 16) * 9 + cc * 9 + tap) * 2 + plane) * 64) + li + 32 * h) * 8 + e
    assert s[flat] == Bl[32 * nb + li, tap * cin + 16 * cc + 8 * h + e]


def test_planes_builder_poisons_everything_but_the_slice():
    c = cr.HALF_S1[0]
    o = cr.build_operands(c)
    A = o.A.clone()
    A[:, 1:-1, :, :, o.ch0:o.ch0 + c.cin] = cr.NAN16
    assert bool((A == cr.NAN16).all())
    assert float(cr.bits_f64(o.A[0, 1:-1, :, :, o.ch0:o.ch0 + c.cin]).abs().max()) == 3.0
    assert float(cr.bits_f64(o.A[1, 1:-1, :, :, o.ch0:o.ch0 + c.cin]).abs().max()) == 3.0 * cr.LO
    assert bool((o.Bh[:, c.K:] == cr.NAN16).all()) and o.ldbh % 8 == 0 and o.ld % 8 == 0


ALL_CASES = list(cr.EXACT_CASES)


@pytest.mark.parametrize("c", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_every_gpu_case_is_in_the_exact_regime(c):
    """|partial sums| < 2^24 quanta of 2^-8 in any order, and v = act-free 2^-6 acc + bias is its own fp32 rounding"""
    o = cr.build_operands(c)
    cr.assert_exact_regime(o)
    _f32_exact(cr.pre_activation(o))
    assert c.K <= 4608


def test_case_names_unique_and_issue_table_complete():
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    assert {c.cin for c in cr.HALF_S1} == {16, 32, 48, 128} and len(cr.HALF_S1) == 32
    assert {(c.Ho, c.n_img) for c in cr.MULTI_S1} == set(itertools.product((4, 8), (1, 7, 8, 9)))
    assert {(c.Hs, c.Ws, c.Ho, c.Wo) for c in cr.STAGED if c.stride == 2} == {(5, 7, 3, 4)}
    assert {c.M for c in cr.STAGED if c.group} == {480}


# ------------------------------------------------------------------------------------------------------------------------
# the dispatch
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL_CASES + REAL_CASES, ids=[c.name for c in ALL_CASES + REAL_CASES])
def test_every_gpu_case_takes_its_route(hk, c):
    got = cr.route_of(hk, cr.dummy_args(c))
    assert got == c.route, f"{c.name}: {hooks.ROUTE_NAMES.get(got, got)} instead of {hooks.ROUTE_NAMES[c.route]}"


def test_every_route_is_covered_or_accounted_for():
    covered = {c.route for c in ALL_CASES}
    assert covered | set(cr.UNCOVERED_ROUTES) == set(hooks.ROUTE_NAMES)
    assert not covered & set(cr.UNCOVERED_ROUTES)


def _edit(c, **kw):
    a = cr.dummy_args(c)
    for k, v in kw.items():
        obj = a
        *path, leaf = k.split("__")
        for p in path:
            obj = getattr(obj, p)
        setattr(obj, leaf, v)
    return a


def test_route_refusals(hk):
    """gemm_f16x3_route returns NSR_ERR_INVALID_ARG exactly where gemm_f16x3 refuses its arguments (csrc/nsr_gemm_f16.hip)"""
    plain, grouped, tail, staged = cr.HALF_S1[8], cr.HALF_GROUPED_S1[0], cr.TAIL[0], cr.STAGED[0]
    bad = [
        _edit(plain, g__M=-1), _edit(plain, g__N=0), _edit(plain, g__K=0), _edit(plain, g__K=9 * 32 + 8), _edit(plain, g__n_valid=130),
        _edit(plain, Bh=None), _edit(plain, Bl=None), _edit(plain, g__Ct=0x1000), _edit(plain, g__splits=2), _edit(plain, g__a_kmajor=1),
        _edit(plain, g__b_kmajor=1), _edit(plain, ldbh=292), _edit(plain, Bh=0x10000008), _edit(plain, Bl=0x10000004),
        _edit(plain, g__lda=60), _edit(plain, a_plane=12), _edit(plain, Ah=0x10000008),
        _edit(plain, Ah=None),                                   # then fp32 A is expected, and g.A is null
        _edit(plain, Ah=None, g__A=0x10000000, g__lda=58), _edit(plain, Ah=None, g__A=0x10000004),
        _edit(plain, g__ldc=151), _edit(plain, c_plane=33), _edit(plain, g__n_valid=127), _edit(plain, Ch=0x10000002),
        _edit(plain, g__col_sums=0x1000), _edit(plain, g__mask=0x1000),
        _edit(tail, g__C=None),                                   # neither planes nor an fp32 output
        _edit(plain, conv__cin=24, g__K=216), _edit(plain, g__K=9 * 32 + 16),
        _edit(grouped, group=4), _edit(grouped, Mh=None), _edit(grouped, Ch=None, g__C=0x1000), _edit(grouped, g__M=8 * 64 - 4),
        _edit(grouped, ldm=139), _edit(grouped, m_plane=7), _edit(grouped, Mh=0x10000002), _edit(grouped, conv__cin=0),
        # staged tiles: K tiles of 32 inside a tap
        _edit(cr.HALF_S1[16], Bs=None),                          # cin = 48 has no staged kernel
        _edit(Case("x", 0, 16, 128, 2, 6, 10, bs=False)),
    ]
    for i, a in enumerate(bad):
        assert cr.route_of(hk, a) == hooks.NSR_ERR_INVALID_ARG, i
    assert hk.nsr_test_gemm_f16x3_route(None) == hooks.NSR_ERR_INVALID_ARG
    assert cr.route_of(hk, _edit(plain, g__M=0)) == hooks.ROUTE_NONE
    # not refusals: the shape decides -- no stream-ordered copy, or a shape no block fits, goes to the staged tile
    assert cr.route_of(hk, _edit(plain, Bs=None)) == hooks.ROUTE_STAGED_K32_FULL
    assert cr.route_of(hk, _edit(plain, Bs=0x10000008)) == hooks.ROUTE_STAGED_K32_FULL
    assert cr.route_of(hk, _edit(staged, Bs=0x10000000)) == staged.route
    # fp32 A without a gather: the plain split-fp16 linear layer
    lin = _edit(plain, Ah=None, g__A=0x10000000, g__lda=288, conv__cin=0, Ch=None, g__C=0x20000000)
    assert cr.route_of(hk, lin) == hooks.ROUTE_STAGED_F32A


def test_big_4x4_plain_is_unreachable(hk):
    """conv_halo_kernel<4, 4, false, 1> (512 x 128, plain, stride 1) is only chosen for N % 256 != 0, where a plain stride-1 layer
    that fits it (Ho % 32 == 0, Wo % 16 == 0) also fits the half tile (Ho % 16 == 0), which runs as a pair per CU and is
    always taken.  Swept: no shape, batch, width, upsample or stride returns it."""
    seen = set()
    for H, W in itertools.product(range(8, 136, 8), range(8, 136, 8)):
        for n_img, N, (stride, up), cin in itertools.product((1, 2, 3, 8, 33, 129, 130, 255, 256, 257, 1000), (128, 384), ((1, 0), (1, 1), (2, 0)),
                                                           (16, 128)):
            Hs, Ws = (H // 2, W // 2) if up else ((2 * H, 2 * W) if stride == 2 else (H, W))
            r = cr.route_of(hk, cr.dummy_args(Case("sweep", 0, cin, N, n_img, Hs, Ws, stride, up)))
            # (a 16-channel layer no halo block fits has no staged kernel either: refused, K tiles of 32 inside a tap)
            assert (r >= 0 or cin % 32) and r != hooks.ROUTE_BIG44_S1, (H, W, n_img, N, stride, up, cin)
            seen.add(r)
    assert hooks.ROUTE_HALF_S1 in seen and hooks.ROUTE_MULTI_S1 in seen and hooks.ROUTE_HALF_S2 in seen
    # the same sweep on a grouped layer does reach the 512 x 128 tile: the sweep can see what it looks for
    g = {cr.route_of(hk, cr.dummy_args(Case("sweep", 0, 16, 128, n, 64, W, group=8))) for n in (8, 16, 24) for W in range(8, 136, 8)}
    assert hooks.ROUTE_BIG44_GROUPED_S1 in g


# ------------------------------------------------------------------------------------------------------------------------
# the network's own calls
# ------------------------------------------------------------------------------------------------------------------------
def network_calls(noref, B, R, H, W):
    """(layer, cin, cout, n_img, Hs, Ws, stride, up, src ld, dst ld, ldm or 0) of every gemm_f16x3 call of one NSR_F16X3 forward
    (csrc/nsr_refine.hip: encoder on the synthesised patches, encoder on the B R reference patches with the fused max,
    decoder), layer 0 on its 16 padded channels"""
    from nerf_sr_amd import refine
    cins = [refine.NOREF_CIN.get(n, ci) if noref else ci for n, ci, _, _ in refine.LAYERS]
    couts = [co for _, _, co, _ in refine.LAYERS]
    w1, w3, w5, w7 = (512, 1024, 512, 256) if noref else (1024, 1536, 768, 384)
    calls = []

    def conv(l, n_img, Hs, Ws, src_ld, dst_ld, ldm=0, stride=1, up=0):
        calls.append((l, 16 if l == 0 else cins[l], couts[l], n_img, Hs, Ws, stride, up, src_ld, dst_ld, ldm))

    def encoder(n_img, d, mx):
        conv(0, n_img, H, W, 16, 128)
        conv(1, n_img, H, W, 128, d[0], mx[0])
        conv(2, n_img, H, W, d[0], 256, stride=2)
        conv(3, n_img, H // 2, W // 2, 256, d[1], mx[1])
        conv(4, n_img, H // 2, W // 2, d[1], 512, stride=2)
        conv(5, n_img, H // 4, W // 4, 512, d[2], mx[2])
        conv(6, n_img, H // 4, W // 4, d[2], d[3], mx[3], stride=2)

    encoder(B, (w7, w5, w3, w1), (0, 0, 0, 0))
    if not noref:
        encoder(B * R, (128, 256, 512, 512), (w7, w5, w3, w1) if R == 8 else (0, 0, 0, 0))
    h, w = H // 8, W // 8
    conv(7, B, h, w, w1, 512); conv(8, B, h, w, 512, 512); conv(9, B, h, w, 512, w3, up=1)
    conv(10, B, 2 * h, 2 * w, w3, 512); conv(11, B, 2 * h, 2 * w, 512, 512); conv(12, B, 2 * h, 2 * w, 512, w5, up=1)
    conv(13, B, 4 * h, 4 * w, w5, 256); conv(14, B, 4 * h, 4 * w, 256, 256); conv(15, B, 4 * h, 4 * w, 256, w7, up=1)
    conv(16, B, H, W, w7, 128); conv(17, B, H, W, 128, 128); conv(18, B, H, W, 128, 3)
    return calls


@pytest.mark.parametrize("noref", (False, True), ids=("ref", "noref"))
def test_every_network_layer_runs_on_a_covered_route(hk, noref):
    """all 19 layers at 64 x 64 with 8 references, one patch set and refine.py's default tile batch (256, which the entry point
    cuts into 255 + 1: nsr_refine.hip sets_per_pass): the instantiation each call launches is one an exact GPU case covers"""
    covered = {c.route for c in ALL_CASES}
    seen = {}
    for B in (1, 255, 256):
        for (l, cin, cout, n_img, Hs, Ws, stride, up, src_ld, dst_ld, ldm) in network_calls(noref, B, 8, 64, 64):
            last = l == 18
            c = Case(f"layer{l}", 0, cin, 64 if last else cout, n_img, Hs, Ws, stride, up, group=8 if ldm else 0, tail=last,
                     n_valid=3 if last else None)
            a = cr.dummy_args(c)
            a.g.lda, a.g.ldc = src_ld, dst_ld
            a.a_plane = n_img * Hs * Ws * src_ld
            a.c_plane = 0 if last else c.M * dst_ld
            if ldm:
                a.ldm, a.m_plane = ldm, (c.M // 8) * ldm
            r = cr.route_of(hk, a)
            assert r in covered, f"layer {l} at B = {B} ({n_img} images): {hooks.ROUTE_NAMES.get(r, r)} has no exact case"
            seen.setdefault(r, set()).add((l, B))
    # B = 256 is what a caller of the uncut forward would get: the 128-channel layers then sit ON the 32-bit limit and fall to
    # the staged kernel (still a covered route); within the cut no layer of the 64 x 64 network leaves conv_halo_kernel
    halo_only = {r for r, where in seen.items() for (_, B) in where if B in (1, 255)}
    assert max(halo_only) < hooks.ROUTE_STAGED_WIDE, {hooks.ROUTE_NAMES[r] for r in halo_only}
