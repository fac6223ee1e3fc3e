"""Unit layer under the training step's backward chain (csrc/nsr_train_chain.hip): the stream packer and the four chain
instantiations -- chain_bwd_kernel (3 terms), chain_bwd_h_kernel<2>, <1>, <12> -- launched on their own through the test-hook
library (tests/hooks.py, tests/csrc/nsr_test_hooks_chain.hip).  Reference, layouts, error model and the operand builder:
tests/chain_ref.py, itself pinned on the CPU by tests/test_chain_units_cpu.py.

Method (as in tests/test_gpu_gemm_units.py).  The exact cases feed weights that are signed selections times powers of two and
integer inputs times the point's own power of two, so that every true gradient at every layer has at most 11 significant bits
and is a normal fp16 at the point's scale (asserted on the reference, `assert_exact_regime`).  Every product and sum of the
chain is then exact whatever the term count: each decoded panel value times the point's `pscale` must equal the fp64
reference BIT FOR BIT, `gmax` must be the float bits of the reference's maximum, and the four term settings must store the
same bits.  A stale mask word, a sign bit read from the wrong place, a block routed to the wrong rows, a wrong scale of the
all-zero point: each changes at least one stored value.  Every output buffer is filled with NaN or a pattern first; the
regions behind the ten panels, behind pscale and behind gmax[9] must keep it.

The real-valued case holds each setting to the DERIVED elementwise bound of chain_ref.error_bounds (no factor on top); the
largest err / bound per setting and panel is printed (run with -s) and recorded in DESIGN.md.

Points past P inside the last point group(s) get "zeroed everywhere" sign bits: they then carry no gradient, so gmax is the
real points' maximum; what the chain stores for them is unspecified and not looked at.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import chain_ref as cr
from tests import hooks

pytestmark = pytest.mark.gpu

GUARD = 4096                    # bytes / words behind every output region
PAN_FILL = 0x7E                 # 0x7E7E is an fp16 NaN
WORD_FILL = 0x5A5A5A5A
GMAX_GARBAGE = 0x7F7F7F7F       # larger than the bits of any finite gradient: survives unless the launch clears it
STRIDES = ((4, 4), (3, 1))


@pytest.fixture(scope="module")
def hk():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return hooks.load()


class Weights:
    """the 24 state tensors on the device + the host array of their addresses the entry points take"""

    def __init__(self, sd):
        self.t = [torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).cuda() for k in cr.KEYS]
        self.arr = (ctypes.c_void_p * len(self.t))(*[t.data_ptr() for t in self.t])


def run_pack(hk, w, mode, stop_grad):
    """-> device buffer (int32 words: nsr_chain_bwd_packed_bytes + guard, pattern-filled before the call)"""
    nwords = hk.nsr_test_chain_bwd_packed_bytes() // 4
    assert nwords == 2304 * 256 + 768
    buf = torch.full((nwords + GUARD,), WORD_FILL, dtype=torch.int32, device="cuda")
    rc = hk.nsr_test_chain_bwd_pack(w.arr, hooks.ptr(buf), int(stop_grad), mode, hooks.stream())
    assert rc == hooks.NSR_OK, rc
    torch.cuda.synchronize()
    return buf


_cases = {}


def exact(name, stop_grad=False):
    """(sd, masks, d_rgb, d_sigma, reference, device weights) of a case of the table; built and checked once"""
    key = (name, stop_grad)
    if key not in _cases:
        sd, masks, d_rgb, d_sigma = cr.exact_case(**cr.EXACT_CASES[name])
        ref = cr.ref_chain(sd, masks, d_rgb, d_sigma, stop_grad=stop_grad)
        cr.assert_exact_regime(ref, d_sigma, name)
        w = _cases[(name, not stop_grad)][5] if (name, not stop_grad) in _cases else Weights(sd)
        _cases[key] = (sd, masks, d_rgb, d_sigma, ref, w)
    return _cases[key]


def run_chain(hk, packed, masks, d_rgb, d_sigma, mode, strides=(4, 4), gmax_is_zero=0, gmax_fill=GMAX_GARBAGE, pad=True):
    """one launch -> (decoded panels [10] (P, rows) fp16, pscale (10, P) fp32, gmax (10,) uint32); asserts the guards"""
    P = d_rgb.shape[0]
    ng = cr.n_groups(P)
    sgn_np = cr.encode_signs(masks, P, pad=pad)
    assert hk.nsr_test_train_sign_words(P) == sgn_np.size == ng * 34 * 64
    pan_bytes = hk.nsr_test_train_panel_bytes(P)
    assert pan_bytes == 2560 * 64 * ng                                  # twelve panels; the chain owns the first ten
    own = cr.BWD_ROWS * 64 * ng
    sgn = torch.from_numpy(sgn_np.view(np.int32)).cuda()
    dpan = torch.full((pan_bytes + GUARD,), PAN_FILL, dtype=torch.uint8, device="cuda")
    pscale = torch.full((10 * ng * 32 + GUARD,), float("nan"), device="cuda")
    gm = torch.full((10 + GUARD,), gmax_fill, dtype=torch.int32, device="cuda")
    if strides == (4, 4):                                               # as the training step passes them: d_sigma = column 3
        raw = torch.from_numpy(np.concatenate([d_rgb, d_sigma[:, None]], 1).astype(np.float32)).cuda()
        p_rgb, p_sig = hooks.ptr(raw), hooks.ptr(raw, 3)
    else:
        assert strides == (3, 1)
        t_rgb = torch.from_numpy(np.ascontiguousarray(d_rgb, dtype=np.float32)).cuda()
        t_sig = torch.from_numpy(np.ascontiguousarray(d_sigma, dtype=np.float32)).cuda()
        p_rgb, p_sig = hooks.ptr(t_rgb), hooks.ptr(t_sig)
    rc = hk.nsr_test_chain_bwd(hooks.ptr(packed), hooks.ptr(sgn), hooks.ptr(dpan), p_rgb, strides[0], p_sig, strides[1], P,
                               hooks.ptr(gm), hooks.ptr(pscale), mode, gmax_is_zero, hooks.stream())
    assert rc == hooks.NSR_OK, rc
    torch.cuda.synchronize()
    dp, ps, g = dpan.cpu().numpy(), pscale.cpu().numpy(), gm.cpu().numpy().view(np.uint32)
    assert (dp[own:] == PAN_FILL).all(), "bytes behind the ten gradient panels were written"
    assert np.isnan(ps[10 * ng * 32:]).all(), "words behind pscale were written"
    assert (g[10:] == np.uint32(gmax_fill)).all(), "words behind gmax[9] were written"
    return cr.decode_panels(dp[:own], P), ps[:10 * ng * 32].reshape(10, ng * 32)[:, :P].copy(), g[:10].copy()


def mismatches(res, ref):
    """[(panel, point, feature, got, want)] of every real element whose decoded value x pscale is not the reference's bits
    (a NaN left from the fill counts), + (panel, -1, -1, got bits, want bits) where gmax differs"""
    panels, ps, gmax = res
    bad = []
    for panel in range(10):
        with np.errstate(invalid="ignore"):
            got = panels[panel].astype(np.float64) * ps[panel][:, None].astype(np.float64)
        for pt, f in np.argwhere(~(got == ref[panel])):
            bad.append((panel, int(pt), int(f), float(got[pt, f]), float(ref[panel][pt, f])))
        want = int(np.float32(np.abs(ref[panel]).max()).view(np.uint32))
        if int(gmax[panel]) != want:
            bad.append((panel, -1, -1, hex(int(gmax[panel])), hex(want)))
    return bad


def describe(bad):
    """the first mismatches with the coordinates a cause shows in: point group, lane (m, h), block, accumulator register"""
    out = [f"{len(bad)} mismatches"]
    for panel, pt, f, got, want in bad[:12]:
        if pt < 0:
            out.append(f"gmax[{panel}] {got} != {want}")
        else:
            out.append(f"panel {panel} point {pt} (group {pt // 32}, m {pt % 32}, h {(f >> 2) & 1}) feature {f} "
                       f"(block {f // 32}, register {4 * ((f & 31) >> 3) + (f & 3)}): {got!r} != {want!r}")
    return "\n".join(out)


def assert_scales_are_powers_of_two(ps):
    assert np.isfinite(ps).all() and (ps > 0).all(), "a real point's pscale was not written"
    m, _ = np.frexp(ps.astype(np.float64))
    assert (m == 0.5).all(), "a pscale is not a power of two"


def same_bits(a, b):
    return (all(np.array_equal(x.view(np.uint16), y.view(np.uint16)) for x, y in zip(a[0], b[0]))
            and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]))


# ------------------------------------------------------------------------------------------------------------------------
# pack
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stop_grad", (0, 1))
def test_pack_equals_numpy_packer(hk, stop_grad):
    """real-valued weights (every lo piece is live), all four modes: the stream word for word, nothing behind it"""
    sd = cr.real_case(1, 31)[0]
    w = Weights(sd)
    got = {}
    for mode in cr.MODES:
        want = cr.pack_stream(sd, mode, bool(stop_grad))
        buf = run_pack(hk, w, mode, stop_grad).cpu().numpy().view(np.uint32)
        assert want.size == cr.stream_pieces(mode) * 256 + 768
        bad = np.flatnonzero(buf[:want.size] != want)
        assert bad.size == 0, (mode, stop_grad, bad[:8], [(hex(buf[i]), hex(want[i])) for i in bad[:8]])
        assert (buf[want.size:] == WORD_FILL).all(), (mode, "words past the stream's length were written")
        got[mode] = buf
    assert np.array_equal(got[2], got[3])
    if stop_grad:                                        # dir_encoding's g columns are packed as zeros: layer 0 of the stream
        assert not got[3][:256 * 256].any() and not got[1][:128 * 256].any()


def test_pack_exact_case_has_no_lo_and_no_sentinel(hk):
    sd, _, _, _, _, w = exact("P160")
    for mode in cr.MODES:
        buf = run_pack(hk, w, mode, 0).cpu().numpy().view(np.uint32)
        want = cr.pack_stream(sd, mode)
        assert np.array_equal(buf[:want.size], want), mode


# ------------------------------------------------------------------------------------------------------------------------
# exact chain
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cr.EXACT_CASES))
def test_chain_exact_all_terms_all_strides(hk, name):
    """P = 32: one partly filled tile; 128: one 4-wave tile; 160: two tiles, one 8-wave workgroup; 288: the second 8-wave
    workgroup's last four waves repeat the last group; 544: three workgroups"""
    sd, masks, d_rgb, d_sigma, ref, w = exact(name)
    first = None
    for mode in cr.MODES:
        packed = run_pack(hk, w, mode, 0)
        for strides in STRIDES:
            res = run_chain(hk, packed, masks, d_rgb, d_sigma, mode, strides)
            assert_scales_are_powers_of_two(res[1])
            bad = mismatches(res, ref)
            assert not bad, f"{name} terms {mode} strides {strides}: " + describe(bad)
            first = first or res
            assert same_bits(res, first), f"{name}: terms {mode} strides {strides} stores other bits than terms 1"
    # the special points did what they are there for
    panels, ps, _ = first
    assert ps[9][cr.PT_ALL_ZERO] == 1.0 and not any(panels[p][cr.PT_ALL_ZERO].any() for p in range(10))      # S = 1
    assert not panels[9][cr.PT_SIGMA_ONLY].any() and not panels[8][cr.PT_SIGMA_ONLY].any() and panels[7][cr.PT_SIGMA_ONLY].any()
    assert panels[4][cr.PT_DEAD_AT_4].any() and not any(panels[p][cr.PT_DEAD_AT_4].any() for p in range(4))
    assert np.ptp(np.log2(ps[9][:32])) >= 50                            # one wave's points sit at scales 2^50 apart and more


@pytest.mark.parametrize("name", ("P32", "P160", "P288"))
def test_chain_padding_points_do_not_leak(hk, name):
    """sign bits of the points past P all CLEAR instead of all set: those points (copies of the last point's inputs) now carry
    gradients, every real point must still be right, and gmax can only have grown"""
    _, masks, d_rgb, d_sigma, ref, w = exact(name)
    for mode in (3, 12):
        res = run_chain(hk, run_pack(hk, w, mode, 0), masks, d_rgb, d_sigma, mode, pad=False)
        bad = [b for b in mismatches(res, ref) if b[1] >= 0]
        assert not bad, f"{name} terms {mode}: " + describe(bad)
        assert all(int(res[2][p]) >= int(np.float32(np.abs(ref[p]).max()).view(np.uint32)) for p in range(10))


def test_chain_gmax_is_zero(hk):
    _, masks, d_rgb, d_sigma, ref, w = exact("P160")
    for mode in cr.MODES:
        packed = run_pack(hk, w, mode, 0)
        cleared = run_chain(hk, packed, masks, d_rgb, d_sigma, mode, gmax_is_zero=0, gmax_fill=GMAX_GARBAGE)
        assert not mismatches(cleared, ref)                             # 0: pre-filled garbage is cleared
        big = int(np.float32(2.0 ** 100).view(np.uint32))               # 1: a larger value survives the atomicMax
        assert big > int(cleared[2].max())
        kept = run_chain(hk, packed, masks, d_rgb, d_sigma, mode, gmax_is_zero=1, gmax_fill=big)
        assert (kept[2] == big).all() and same_bits((kept[0], kept[1], cleared[2]), cleared)
        zeros = run_chain(hk, packed, masks, d_rgb, d_sigma, mode, gmax_is_zero=1, gmax_fill=0)
        assert same_bits(zeros, cleared)                                # 1 and zeros = the cleared case


def test_chain_stop_grad_exact(hk):
    sd, masks, d_rgb, d_sigma, ref, w = exact("P160", stop_grad=True)
    sigma_only = cr.ref_chain(sd, masks, np.zeros_like(d_rgb), d_sigma)
    assert not ref[8].any() and ref[9].any()
    assert all(np.array_equal(ref[p], sigma_only[p]) for p in range(8))      # the trunk sees the density head's gradient alone
    for mode in cr.MODES:
        res = run_chain(hk, run_pack(hk, w, mode, 1), masks, d_rgb, d_sigma, mode)
        assert_scales_are_powers_of_two(res[1])
        bad = mismatches(res, ref)
        assert not bad, f"stop_grad terms {mode}: " + describe(bad)
        assert not (res[0][8].view(np.uint16) & 0x7FFF).any() and res[2][8] == 0                             # exact zeros


# ------------------------------------------------------------------------------------------------------------------------
# teeth: the device output of one exact case against four deliberately wrong references
# ------------------------------------------------------------------------------------------------------------------------
def test_wrong_references_are_told_apart(hk):
    sd, masks, d_rgb, d_sigma, ref, w = exact("P160")
    res = run_chain(hk, run_pack(hk, w, 12, 0), masks, d_rgb, d_sigma, 12)
    assert not mismatches(res, ref)
    swapped = {p: m[:, np.arange(m.shape[1]) ^ 32] for p, m in masks.items()}       # the two blocks of every pair trade sign bits
    kstep = [cr.act_feature(8 * 5 + j, 0) for j in range(8)]                        # lane half 0's eight features of k-step 5
    wrong = {
        "sign bits of a pair's two blocks swapped": cr.ref_chain(sd, swapped, d_rgb, d_sigma),
        "skip slice at column 62": cr.ref_chain(sd, masks, d_rgb, d_sigma, skip_col0=62),
        "sigma.weight term dropped": cr.ref_chain(sd, masks, d_rgb, d_sigma, drop_sigma=True),
        "one k-step of layer 3 dropped": cr.ref_chain(sd, masks, d_rgb, d_sigma, drop_k=(3, kstep)),
    }
    for what, bad_ref in wrong.items():
        n = len([b for b in mismatches(res, bad_ref) if b[1] >= 0])
        print(f"{what}: {n} elements differ")
        assert n > 0, what


# ------------------------------------------------------------------------------------------------------------------------
# real-valued inputs: the derived elementwise bound
# ------------------------------------------------------------------------------------------------------------------------
_real = {}


def real():
    if not _real:
        sd, masks, d_rgb, d_sigma = cr.real_case(288, 41)
        _real.update(sd=sd, masks=masks, d_rgb=d_rgb, d_sigma=d_sigma, ref=cr.ref_chain(sd, masks, d_rgb, d_sigma), w=Weights(sd))
    return _real


@pytest.mark.parametrize("mode", cr.MODES)
def test_chain_real_inputs_within_derived_bound(hk, mode):
    """|decoded x pscale - fp64 reference| <= chain_ref.error_bounds elementwise, no factor.  The bound is the issue-stated
    recurrence with ONE correction that the CPU file proves without a device (test_half_ulp_of_fp16_is_not_two_to_the_minus_
    twelve, and the `literal` column of test_error_model_bounds_the_emulated_arithmetic): one rounding to fp16 costs up to half
    an ulp = 2^-12 x (the power of two above |x|), not 2^-12 |x| -- a correctly rounded panel 9 reaches 1.98 x the latter.
    Also added, all far below the accumulation term: the dropped lo x lo products of the three-term layers, denormal floors of
    the weight pieces, second-order products of the operand errors.
    Measured on one MI355X (2026-10-19), largest err / bound over the panels: see DESIGN.md."""
    c = real()
    bound = cr.error_bounds(c["sd"], c["masks"], c["d_rgb"], c["d_sigma"], mode, c["ref"])
    literal = cr.error_bounds(c["sd"], c["masks"], c["d_rgb"], c["d_sigma"], mode, c["ref"], literal=True)
    panels, ps, gmax = run_chain(hk, run_pack(hk, c["w"], mode, 0), c["masks"], c["d_rgb"], c["d_sigma"], mode)
    assert_scales_are_powers_of_two(ps)
    worst, fails = 0.0, []
    for panel in range(9, -1, -1):
        got = panels[panel].astype(np.float64) * ps[panel][:, None].astype(np.float64)
        assert np.isfinite(got).all(), panel
        err = np.abs(got - c["ref"][panel])
        nz = bound[panel] > 0
        ratio, lit = float((err[nz] / bound[panel][nz]).max()), float((err[nz] / literal[panel][nz]).max())
        print(f"chain terms {mode:2d} panel {panel}: max err / bound {ratio:.4f}   (with 2^-12 |x| per fp16 rounding: {lit:.4f})")
        worst = max(worst, ratio)
        if not (err <= bound[panel]).all():
            fails.append((panel, ratio))
        # gmax: the panel's largest true magnitude as the kernel saw it, i.e. within the bound of the reference's
        assert abs(float(gmax[panel:panel + 1].view(np.float32)[0]) - np.abs(c["ref"][panel]).max()) <= bound[panel].max()
    print(f"chain terms {mode:2d}: largest err / bound {worst:.4f}")
    assert not fails, fails
