"""NSR_F16X3_GEMM_BWD (include/nsr_train.h: the layer-by-layer training pair with its gradient products on the split-fp16 MFMA)
without a GPU: the value and its Python mirror, the size functions (the saved state is f16x3_gemm's, the workspace grows by a
tail for this value only, every older value sizes what it sized before), the rejections with fake pointers (the codes
f16x3_gemm returns), the 'f16x3' mapping, and the numpy restatement of the two kernels (tests/train_bwd_ref.py) against the
fp64 product."""
import ctypes
import os
import re
import warnings
from ctypes import c_void_p

import numpy as np
import pytest

from nerf_sr_amd import _lib

from . import train_bwd_ref as ref

INVALID, UNSUPPORTED, WORKSPACE, OK = -1, -2, -4, 0
FP32, GEMM, BWD = _lib.NSR_FP32, _lib.NSR_F16X3_GEMM, 24
A = _lib.NsrArch
ARCHS = (dict(D=8, W=256, skips=1 << 4, deg_pos=10, deg_dir=4, no_dir=0), dict(D=6, W=192, skips=(1 << 1) | (1 << 3), deg_pos=10, deg_dir=4, no_dir=0),
         dict(D=4, W=128, skips=0, deg_pos=10, deg_dir=4, no_dir=0), dict(D=3, W=100, skips=1 << 1, deg_pos=5, deg_dir=2, no_dir=1))


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except Exception as e:  # noqa: BLE001
        pytest.fail(f"libnsr.so not built: {e}")


def test_value_and_mirror():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsr_train.h")).read()
    assert int(re.search(r"#define NSR_F16X3_GEMM_BWD (\d+)", hdr).group(1)) == 24 == _lib.TRAIN_PRECISIONS["f16x3_gemm_bwd"]
    assert _lib.NSR_F16X3_GEMM_BWD == 24 and 23 not in _lib.TRAIN_PRECISIONS.values()
    from nerf_sr_amd import train
    assert "f16x3_gemm_bwd" in train.ARCH_PRECISIONS


def test_23_sizes_nothing_and_the_saved_state_is_f16x3_gemms(lib):
    assert lib.nsr_train_workspace_bytes_for(23, 2048, 64, 64) == 0 and lib.nsr_train_saved_bytes(23, 64, 64, 64, 0) == 0
    assert lib.nsr_version() == 131
    for kw in ARCHS:
        a = A(**kw)
        for R, chunk in ((32, 0), (96, 0), (96, 32), (2048, 512)):
            want = lib.nsr_train_arch_saved_bytes(ctypes.byref(a), GEMM, R, 64, 64, chunk)
            assert want > 0 and lib.nsr_train_arch_saved_bytes(ctypes.byref(a), BWD, R, 64, 64, chunk) == want, (kw, R, chunk)
            assert lib.nsr_train_arch_saved_bytes_e(ctypes.byref(a), 0, BWD, R, 64, 64, chunk) == want
    for R in (32, 96, 2048):
        assert lib.nsr_train_saved_bytes(BWD, R, 64, 64, 0) == lib.nsr_train_saved_bytes(GEMM, R, 64, 64, 0) > 0


def _a64(n):
    return (n + 63) // 64 * 64


def _tail_floats(kw):
    """The tail of this value's workspace, from the header comment: per network the transposed split halves of every matrix an
    input gradient reads (hi + lo = one float per element, in 256-byte granules), then 64 range words."""
    r32 = lambda n: (n + 31) // 32 * 32
    D, W, skips = kw["D"], kw["W"], kw["skips"]
    Kx, Wp, Hp = r32(3 + 6 * kw["deg_pos"]), r32(W), r32(W // 2)
    Dp = 0 if kw["no_dir"] else r32(3 + 6 * kw["deg_dir"])
    kin = lambda l: Kx if l == 0 else (Kx + Wp if (skips >> l) & 1 else Wp)
    per_net = sum(_a64(Wp * kin(l)) for l in range(D)) + _a64((Wp + 32) * Wp) + _a64(Hp * (Wp + Dp)) + _a64(32 * Hp)
    return 2 * per_net + 64


# nsr_train_workspace_bytes_for / nsr_train_arch_workspace_bytes[_r] of the parent commit (computed by its library) for the
# precisions it knew: (function, precision, descriptor index or None, ray_chunk) -> bytes at 64 + 64 samples
PARENT_SIZES = {('nsr_train_arch_workspace_bytes', 0, 0, 32): 137337600,
 ('nsr_train_arch_workspace_bytes', 0, 0, 96): 240559872,
 ('nsr_train_arch_workspace_bytes', 0, 0, 2048): 3388838912,
 ('nsr_train_arch_workspace_bytes', 0, 1, 32): 86161408,
 ('nsr_train_arch_workspace_bytes', 0, 1, 96): 154764288,
 ('nsr_train_arch_workspace_bytes', 0, 1, 2048): 2247151872,
 ('nsr_train_arch_workspace_bytes', 0, 2, 32): 36263168,
 ('nsr_train_arch_workspace_bytes', 0, 2, 96): 74440960,
 ('nsr_train_arch_workspace_bytes', 0, 2, 2048): 1238863360,
 ('nsr_train_arch_workspace_bytes', 0, 3, 32): 42345216,
 ('nsr_train_arch_workspace_bytes', 0, 3, 96): 75280128,
 ('nsr_train_arch_workspace_bytes', 0, 3, 2048): 1079794688,
 ('nsr_train_arch_workspace_bytes', 18, 0, 32): 142187264,
 ('nsr_train_arch_workspace_bytes', 18, 0, 96): 245409536,
 ('nsr_train_arch_workspace_bytes', 18, 0, 2048): 3393688576,
 ('nsr_train_arch_workspace_bytes', 18, 1, 32): 88471552,
 ('nsr_train_arch_workspace_bytes', 18, 1, 96): 157074432,
 ('nsr_train_arch_workspace_bytes', 18, 1, 2048): 2249462016,
 ('nsr_train_arch_workspace_bytes', 18, 2, 32): 36984064,
 ('nsr_train_arch_workspace_bytes', 18, 2, 96): 75161856,
 ('nsr_train_arch_workspace_bytes', 18, 2, 2048): 1239584256,
 ('nsr_train_arch_workspace_bytes', 18, 3, 32): 42984192,
 ('nsr_train_arch_workspace_bytes', 18, 3, 96): 75919104,
 ('nsr_train_arch_workspace_bytes', 18, 3, 2048): 1080433664,
 ('nsr_train_arch_workspace_bytes_r', 0, 0, 32): 140008192,
 ('nsr_train_arch_workspace_bytes_r', 0, 0, 96): 248571648,
 ('nsr_train_arch_workspace_bytes_r', 0, 0, 2048): 3559756800,
 ('nsr_train_arch_workspace_bytes_r', 0, 1, 32): 89880576,
 ('nsr_train_arch_workspace_bytes_r', 0, 1, 96): 165921792,
 ('nsr_train_arch_workspace_bytes_r', 0, 1, 2048): 2485178624,
 ('nsr_train_arch_workspace_bytes_r', 0, 2, 32): 37885184,
 ('nsr_train_arch_workspace_bytes_r', 0, 2, 96): 79307008,
 ('nsr_train_arch_workspace_bytes_r', 0, 2, 2048): 1342672384,
 ('nsr_train_arch_workspace_bytes_r', 0, 3, 32): 44491520,
 ('nsr_train_arch_workspace_bytes_r', 0, 3, 96): 81719040,
 ('nsr_train_arch_workspace_bytes_r', 0, 3, 2048): 1217158144,
 ('nsr_train_arch_workspace_bytes_r', 18, 0, 32): 144857856,
 ('nsr_train_arch_workspace_bytes_r', 18, 0, 96): 253421312,
 ('nsr_train_arch_workspace_bytes_r', 18, 0, 2048): 3564606464,
 ('nsr_train_arch_workspace_bytes_r', 18, 1, 32): 92190720,
 ('nsr_train_arch_workspace_bytes_r', 18, 1, 96): 168231936,
 ('nsr_train_arch_workspace_bytes_r', 18, 1, 2048): 2487488768,
 ('nsr_train_arch_workspace_bytes_r', 18, 2, 32): 38606080,
 ('nsr_train_arch_workspace_bytes_r', 18, 2, 96): 80027904,
 ('nsr_train_arch_workspace_bytes_r', 18, 2, 2048): 1343393280,
 ('nsr_train_arch_workspace_bytes_r', 18, 3, 32): 45130496,
 ('nsr_train_arch_workspace_bytes_r', 18, 3, 96): 82358016,
 ('nsr_train_arch_workspace_bytes_r', 18, 3, 2048): 1217797120,
 ('nsr_train_workspace_bytes_for', 0, None, 32): 142187264,
 ('nsr_train_workspace_bytes_for', 0, None, 96): 245409536,
 ('nsr_train_workspace_bytes_for', 0, None, 2048): 3393688576,
 ('nsr_train_workspace_bytes_for', 2, None, 32): 83136768,
 ('nsr_train_workspace_bytes_for', 2, None, 96): 228892928,
 ('nsr_train_workspace_bytes_for', 2, None, 2048): 3731785728,
 ('nsr_train_workspace_bytes_for', 18, None, 32): 142187264,
 ('nsr_train_workspace_bytes_for', 18, None, 96): 245409536,
 ('nsr_train_workspace_bytes_for', 18, None, 2048): 3393688576,
 ('nsr_train_workspace_bytes_for', 19, None, 32): 83136768,
 ('nsr_train_workspace_bytes_for', 19, None, 96): 228892928,
 ('nsr_train_workspace_bytes_for', 19, None, 2048): 3731785728,
 ('nsr_train_workspace_bytes_for', 20, None, 32): 83136768,
 ('nsr_train_workspace_bytes_for', 20, None, 96): 228892928,
 ('nsr_train_workspace_bytes_for', 20, None, 2048): 3731785728,
 ('nsr_train_workspace_bytes_for', 21, None, 32): 83136768,
 ('nsr_train_workspace_bytes_for', 21, None, 96): 228892928,
 ('nsr_train_workspace_bytes_for', 21, None, 2048): 3731785728,
 ('nsr_train_workspace_bytes_for', 22, None, 32): 83136768,
 ('nsr_train_workspace_bytes_for', 22, None, 96): 228892928,
 ('nsr_train_workspace_bytes_for', 22, None, 2048): 3731785728,
 ('nsr_train_workspace_bytes_r', 0, None, 32): 142187264,
 ('nsr_train_workspace_bytes_r', 0, None, 96): 245409536,
 ('nsr_train_workspace_bytes_r', 0, None, 2048): 3393688576,
 ('nsr_train_workspace_bytes_r', 2, None, 32): 83529984,
 ('nsr_train_workspace_bytes_r', 2, None, 96): 229482752,
 ('nsr_train_workspace_bytes_r', 2, None, 2048): 3738372096,
 ('nsr_train_workspace_bytes_r', 18, None, 32): 142187264,
 ('nsr_train_workspace_bytes_r', 18, None, 96): 245409536,
 ('nsr_train_workspace_bytes_r', 18, None, 2048): 3393688576,
 ('nsr_train_workspace_bytes_r', 19, None, 32): 83529984,
 ('nsr_train_workspace_bytes_r', 19, None, 96): 229482752,
 ('nsr_train_workspace_bytes_r', 19, None, 2048): 3738372096,
 ('nsr_train_workspace_bytes_r', 20, None, 32): 83529984,
 ('nsr_train_workspace_bytes_r', 20, None, 96): 229482752,
 ('nsr_train_workspace_bytes_r', 20, None, 2048): 3738372096,
 ('nsr_train_workspace_bytes_r', 21, None, 32): 83529984,
 ('nsr_train_workspace_bytes_r', 21, None, 96): 229482752,
 ('nsr_train_workspace_bytes_r', 21, None, 2048): 3738372096,
 ('nsr_train_workspace_bytes_r', 22, None, 32): 83529984,
 ('nsr_train_workspace_bytes_r', 22, None, 96): 229482752,
 ('nsr_train_workspace_bytes_r', 22, None, 2048): 3738372096}


def test_workspace_grows_for_this_value_only(lib):
    for i, kw in enumerate(ARCHS):
        a = A(**kw)
        for chunk in (32, 96, 2048):
            g = lib.nsr_train_arch_workspace_bytes(ctypes.byref(a), GEMM, chunk, 64, 64)
            b = lib.nsr_train_arch_workspace_bytes(ctypes.byref(a), BWD, chunk, 64, 64)
            assert g > 0 and b == g + 4 * _tail_floats(kw), (kw, chunk, g, b)
            assert lib.nsr_train_arch_workspace_bytes_e(ctypes.byref(a), 0, BWD, chunk, 64, 64) == b
            gr = lib.nsr_train_arch_workspace_bytes_r(ctypes.byref(a), 0, GEMM, chunk, 64, 64)
            assert lib.nsr_train_arch_workspace_bytes_r(ctypes.byref(a), 0, BWD, chunk, 64, 64) == gr + 4 * _tail_floats(kw)
    for chunk in (32, 2048):
        g = lib.nsr_train_workspace_bytes_for(GEMM, chunk, 64, 64)
        assert lib.nsr_train_workspace_bytes_for(BWD, chunk, 64, 64) == g + 4 * _tail_floats(ARCHS[0])
        assert lib.nsr_train_workspace_bytes_for(FP32, chunk, 64, 64) == g
        assert lib.nsr_train_workspace_bytes(chunk, 64, 64) >= lib.nsr_train_workspace_bytes_for(BWD, chunk, 64, 64)
        assert lib.nsr_train_workspace_bytes_r(BWD, chunk, 64, 64) == lib.nsr_train_workspace_bytes_for(BWD, chunk, 64, 64)


# nsr_train_workspace_bytes (the precision-agnostic union) of the parent commit: ray_chunk -> bytes at 64 + 64 samples
PARENT_UNION = {32: 225124864, 96: 473707008, 2048: 7112792320}


def test_the_union_grows_by_exactly_the_tail(lib):
    """nsr_train_workspace_bytes suffices whatever runs, so it includes the new precision's tail: the parent's answer plus the
    default network's tail, no more."""
    for chunk, was in PARENT_UNION.items():
        assert lib.nsr_train_workspace_bytes(chunk, 64, 64) == was + 4 * _tail_floats(ARCHS[0]), chunk
    assert 4 * _tail_floats(ARCHS[0]) == 4849920


def test_every_older_value_sizes_what_the_parent_sized(lib):
    """PARENT_SIZES: what the parent commit's library answered."""
    assert len(PARENT_SIZES) >= 40
    for (fn, prec, i, chunk), want in PARENT_SIZES.items():
        if i is None:
            got = getattr(lib, fn)(prec, chunk, 64, 64)
        elif fn.endswith("_r"):
            got = getattr(lib, fn)(ctypes.byref(A(**ARCHS[i])), 0, prec, chunk, 64, 64)
        else:
            got = getattr(lib, fn)(ctypes.byref(A(**ARCHS[i])), prec, chunk, 64, 64)
        assert got == want, (fn, prec, i, chunk, got, want)


def _fwd(lib, arch, **kw):
    one = c_void_p(256)
    n = lib.nsr_arch_n_tensors(ctypes.byref(arch))
    pn = (c_void_p * n)(*[one] * n)
    outs = (c_void_p * 8)(*[one] * 8)
    a = dict(wc=pn, wf=pn, rays=one, stride=8, R=64, nc=64, ni=64, flags=0, prec=BWD, chunk=0, outs=outs, ws=one, ws_bytes=1 << 40,
             saved=one, saved_bytes=1 << 40)
    a.update(kw)
    return lib.nsr_train_arch_forward(ctypes.byref(arch), a["wc"], a["wf"], a["rays"], a["stride"], a["R"], a["nc"], a["ni"], a["flags"],
                                      0, None, None, None, None, 0.0, a["prec"], a["chunk"], a["outs"], a["ws"], a["ws_bytes"],
                                      a["saved"], a["saved_bytes"], None)


def test_rejections_have_f16x3_gemms_codes(lib):
    """Fake pointers that are never dereferenced: every mistake gets the code the same call returns under f16x3_gemm."""
    one, null = c_void_p(256), c_void_p(0)
    a = A(**ARCHS[1])
    cases = [dict(), dict(wc=None), dict(outs=None), dict(rays=null), dict(stride=9), dict(R=-1), dict(ws=null), dict(saved=c_void_p(16)),
             dict(nc=1), dict(ni=0), dict(R=3, nc=40, ni=24), dict(flags=32), dict(flags=_lib.NSR_TRAIN_GAMMA_CORRECT | _lib.NSR_TRAIN_COLOR_NONE),
             dict(ws_bytes=1024), dict(saved_bytes=1024), dict(R=0)]
    for kw in cases:
        assert _fwd(lib, a, **kw) == _fwd(lib, a, prec=GEMM, **kw), kw
    assert _fwd(lib, a, ws_bytes=1024) == WORKSPACE and _fwd(lib, a, prec=23) == UNSUPPORTED
    need = lib.nsr_train_arch_workspace_bytes(ctypes.byref(a), BWD, 64, 64, 64)
    assert _fwd(lib, a, ws_bytes=need - 1) == WORKSPACE
    assert _fwd(lib, a, ws_bytes=need, saved_bytes=1024) == WORKSPACE          # the workspace suffices: the next check answers
    # the default pair and the fused step: accepted like f16x3_gemm (the workspace check is the last before any launch)
    p24 = (c_void_p * 24)(*[one] * 24)
    outs = (c_void_p * 8)(*[one] * 8)
    for prec in (GEMM, BWD):
        assert lib.nsr_train_forward(p24, p24, one, 8, 64, 64, 64, 0, 0, None, None, None, None, 0.0, prec, 0, outs, one, 1024, one,
                                     1 << 40, None) == WORKSPACE
        assert lib.nsr_train_loss_and_grads(p24, p24, p24, p24, one, 8, 64, 1, one, 64, 64, 0, 0, None, None, None, None, 0.0, 1.0, 1.0,
                                            prec, 0, outs, one, one, one, one, 1024, None) == WORKSPACE
    assert lib.nsr_train_forward(p24, p24, one, 8, 64, 64, 64, 0, 0, None, None, None, None, 0.0, 23, 0, outs, one, 1024, one,
                                 1 << 40, None) == UNSUPPORTED


def test_f16x3_still_maps_to_f16x3_gemm_with_one_warning():
    from nerf_sr_amd import train
    arch = train.normalize_arch(dict(D=5, W=96, skips=[2], deg_pos=7, deg_dir=3))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert train.arch_precision(arch, "f16x3") == "f16x3_gemm"
        assert train.arch_precision(arch, "f16x3") == "f16x3_gemm"
    assert len([x for x in w if issubclass(x.category, RuntimeWarning)]) == 1
    assert train.arch_precision(arch, "f16x3_gemm_bwd") == "f16x3_gemm_bwd" and train.embed_precision(1, "f16x3_gemm_bwd") == "f16x3_gemm_bwd"
    with pytest.raises(ValueError):
        train.arch_precision(arch, "f16x3_bwd3")


# ---- the restatement against the fp64 product -------------------------------------------------------------------------------
def test_range_exponent():
    assert ref.range_exp(0.0) == 0 and ref.range_exp(float("nan")) == 0
    for v in (1.0, 1.5, 3e-7, 2.0 ** -40, 12345.0, 2.0 ** 13, 2.0 ** 14 - 1):
        s = v * 2.0 ** ref.range_exp(v)
        assert 2.0 ** 13 <= s < 2.0 ** 14, (v, s)
    assert ref.range_exp(2.0 ** -120) == 100 and ref.range_exp(float("inf")) == -100


def test_restatement_agrees_with_fp64_to_the_promised_accuracy():
    """Per product the three terms drop lo lo and two roundings of lo: ~2^-21 |a| |b|; each of the 3 K / 16 fp32 additions adds
    at most 2^-24 of the running magnitude.  Rows of gradients 2^-30 apart are each held to that RELATIVE accuracy."""
    rng = np.random.default_rng(5)
    P, K, N = 70, 96, 64
    dy = (rng.standard_normal((P, K)) * np.exp2(rng.integers(-30, 0, (P, 1)))).astype(np.float32)
    w = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
    mask = rng.standard_normal((P, N)).astype(np.float32)
    got = ref.dgrad(dy, w, mask).astype(np.float64)
    exact = np.where(mask > 0, dy.astype(np.float64) @ w.astype(np.float64), 0.0)
    bound = (2.0 ** -21 + (3 * K / 16) * 2.0 ** -24) * (np.abs(dy).astype(np.float64) @ np.abs(w).astype(np.float64)) + 1e-45
    assert (np.abs(got - exact) <= bound).all(), float((np.abs(got - exact) / bound).max())
    assert (got[mask <= 0] == 0).all()
    # the weight gradient: one scale per matrix; slices of a ragged P
    P, M, N = 1100, 32, 64
    dy = (rng.standard_normal((P, M)) * 3e-7).astype(np.float32)
    x = np.maximum(rng.standard_normal((P, N)), 0).astype(np.float32)
    sp = ref.n_splits(P)
    assert sp == 3 and ref.slice_len(P, sp) == 384
    part = ref.wgrad(dy, x, sp).astype(np.float64)
    L = ref.slice_len(P, sp)
    for z in range(sp):
        a, b = dy[z * L:(z + 1) * L].astype(np.float64), x[z * L:(z + 1) * L].astype(np.float64)
        bound = (2.0 ** -21 + (3 * L / 16) * 2.0 ** -24) * (np.abs(a).T @ np.abs(b)) + 1e-45
        assert (np.abs(part[z] - a.T @ b) <= bound).all(), z
    # powers of two pass through both exactly
    for k in (-16, 8):
        assert np.array_equal(ref.dgrad(dy[:40, :32] * np.float32(2.0 ** k), w[:32], None), ref.dgrad(dy[:40, :32], w[:32], None) * np.float32(2.0 ** k))
        assert np.array_equal(ref.wgrad(dy * np.float32(2.0 ** k), x, sp), ref.wgrad(dy, x, sp) * np.float32(2.0 ** k))
