"""The launchers of the refinement network's split-fp16 training precision, each ALONE on exact inputs
(csrc/nsr_refine_train_work.h: refine_conv_f16x3, refine_flip_pack, refine_dgrad_f16x3, refine_fold2x2, and the range word of
the kernels that write dZ), reached through tests/csrc/nsr_test_hooks_refine_mixed.hip.  Inputs are small integers (dZ: integers
x 2^-30, so the range word is exercised), every sum is below 2^24: the results must EQUAL tests/refine_mixed_ref.py's numpy
forms bit for bit.  Outputs are compared as whole NaN-framed buffers: destination slices with ch0 != 0 and ld > C carry NaN
where nothing may be written, sources carry NaN where nothing may be read."""
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from . import hooks
from . import refine_mixed_ref as ref

pytestmark = pytest.mark.gpu

SIGNATURES = {
    "nsr_test_refine_conv_f16x3": [c_void_p, c_int64] + [c_int] * 6 + [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p],
    "nsr_test_refine_flip_pack": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "nsr_test_refine_dgrad_f16x3": [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p],
    "nsr_test_refine_fold2x2": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p],
    "nsr_test_refine_bn_bwd_range": [c_void_p, c_void_p, c_int64] + [c_void_p] * 4 + [c_int64, c_int, c_void_p, c_void_p, c_void_p],
    "nsr_test_refine_tanh_bwd_range": [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    lib = hooks.load()
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = c_int, args
    return lib


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def framed(rows, ld):
    return torch.full((rows, ld), float("nan"), dtype=torch.float32, device="cuda")


def in_slice(x2d, ld, ch0):
    """(rows, C) values in channels [ch0, ch0 + C) of a NaN buffer with row stride ld"""
    buf = framed(x2d.shape[0], ld)
    buf[:, ch0:ch0 + x2d.shape[1]] = dev(x2d)
    return buf


def same(got, want):
    return np.array_equal(got.cpu().numpy(), np.asarray(want, dtype=np.float32), equal_nan=True)


def expect_slice(want2d, ld, ch0):
    out = np.full((want2d.shape[0], ld), np.nan, dtype=np.float32)
    out[:, ch0:ch0 + want2d.shape[1]] = want2d
    return out


def packed_forward(w, bias, np_):
    """pack_conv_kernel's f16x3 layout of a raw weight: [hi (np x 9 cin)] [lo] halves, np bias floats (integers: lo = 0)"""
    cout, cin = w.shape[:2]
    m = np.zeros((np_, 9, cin))
    m[:cout] = 64.0 * w.transpose(0, 2, 3, 1).reshape(cout, 9, cin)
    hi = m.reshape(-1).astype(np.float16)
    assert np.array_equal(hi.astype(np.float64), m.reshape(-1))
    b = np.zeros(np_, dtype=np.float32)
    b[:cout] = bias
    return torch.from_numpy(np.concatenate([hi.view(np.uint8), np.zeros(hi.size * 2, np.uint8), b.view(np.uint8)])).cuda()


def flip_packed(lib, w, np_):
    cout, cin = w.shape[:2]
    dst = torch.zeros(2 * cin * 9 * np_, dtype=torch.float16, device="cuda")
    assert lib.nsr_test_refine_flip_pack(hooks.ptr(dev(w)), cin, cout, np_, hooks.ptr(dst), hooks.stream()) == 0
    return dst


def max_bits(t):
    return t.abs().max().reshape(1).view(torch.int32)


@pytest.mark.parametrize("case", ref.FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_site_convolution(lib, case):
    H, W, n, cin, cout, stride, up = case
    x, w, b = ref.fwd_inputs(case)
    want = ref.conv_fwd(x, w, stride, up, b)
    np_ = ref.pad32(cout)
    src = in_slice(x.reshape(-1, cin), cin + 128, 128)
    ld, ch0 = (cout + 64, 32) if cout >= 32 else (8, 4)
    dst = framed(want.shape[0] * want.shape[1] * want.shape[2], ld)
    rc = lib.nsr_test_refine_conv_f16x3(hooks.ptr(src, 128), cin + 128, cin, n, H, W, stride, up, hooks.ptr(packed_forward(w, b, np_)), np_,
                                        cout, hooks.ACT_NONE, hooks.ptr(dst, ch0), ld, hooks.stream())
    assert rc == 0
    assert same(dst, expect_slice(want.reshape(-1, cout), ld, ch0))


@pytest.mark.parametrize("cin,cout", ref.PACK_CASES)
def test_flipped_pack(lib, cin, cout):
    w, np_ = ref.weights(cin, cout), ref.pad32(cout)
    got = flip_packed(lib, w, np_).cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:cin * 9 * np_].reshape(cin, 9 * np_), ref.flip_pack(w, np_))
    assert not got[cin * 9 * np_:].any()                                   # integers x 64: the lo halves are zero


@pytest.mark.parametrize("case", ref.DGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_input_gradient(lib, case):
    """pack -> implicit convolution of dZ (-> 2 x 2 fold behind the upsample) into a slice of a wider gradient buffer"""
    H, W, n, cin, cout, up = case
    dz, w = ref.dgrad_inputs(case)
    np_ = dz.shape[-1]
    r = 2 if up else 1
    dzd = dev(dz * ref.DZ_UNIT)
    bits = max_bits(dzd)
    bw = flip_packed(lib, w, np_)
    ld, ch0 = cin + 256, 128
    dst = framed(n * H * W, ld)
    if up:
        scratch = framed(n * 4 * H * W, cin)
        assert lib.nsr_test_refine_dgrad_f16x3(hooks.ptr(dzd), np_, hooks.ptr(bw), cin, n, r * H, r * W, hooks.ptr(bits), hooks.ptr(scratch),
                                               cin, hooks.stream()) == 0
        assert same(scratch, (ref.dgrad(dz, w) * ref.DZ_UNIT).reshape(-1, cin))
        assert lib.nsr_test_refine_fold2x2(hooks.ptr(scratch), cin, n, H, W, hooks.ptr(dst, ch0), ld, hooks.stream()) == 0
    else:
        assert lib.nsr_test_refine_dgrad_f16x3(hooks.ptr(dzd), np_, hooks.ptr(bw), cin, n, H, W, hooks.ptr(bits), hooks.ptr(dst, ch0), ld,
                                               hooks.stream()) == 0
    assert same(dst, expect_slice((ref.dgrad_expected(case) * ref.DZ_UNIT).reshape(-1, cin), ld, ch0))


@pytest.mark.parametrize("Hs,Ws,n,C", ref.FOLD_CASES)
def test_fold(lib, Hs, Ws, n, C):
    g = ref.ints(np.random.default_rng(5), (n, 2 * Hs, 2 * Ws, C), 1 << 20)
    ld, ch0 = C + 128, 64
    dst = framed(n * Hs * Ws, ld)
    assert lib.nsr_test_refine_fold2x2(hooks.ptr(dev(g)), C, n, Hs, Ws, hooks.ptr(dst, ch0), ld, hooks.stream()) == 0
    assert same(dst, expect_slice(ref.fold2x2(g).reshape(-1, C), ld, ch0))


def test_range_word_scales_and_zero(lib):
    """dZ x 2^-16 and x 2^8 give the gradient x 2^-16 / 2^8 exactly (the power of two follows the word); a zero word with a
    zero dZ gives exact zeros; a word from a larger maximum than dZ holds (another chunk's) changes nothing on exact inputs."""
    case = (8, 8, 3, 128, 128, 0)
    H, W, n, cin, cout, _ = case
    dz, w = ref.dgrad_inputs(case)
    bw = flip_packed(lib, w, dz.shape[-1])
    want = ref.dgrad(dz, w).reshape(-1, cin)
    for scale, word_scale in ((1.0, 1.0), (2.0 ** -16, 1.0), (2.0 ** 8, 1.0), (1.0, 4.0), (0.0, 0.0)):
        dzd = dev(dz * ref.DZ_UNIT * scale)
        bits = max_bits(dzd * word_scale) if word_scale else torch.zeros(1, dtype=torch.int32, device="cuda")
        dst = framed(n * H * W, cin)
        assert lib.nsr_test_refine_dgrad_f16x3(hooks.ptr(dzd), dz.shape[-1], hooks.ptr(bw), cin, n, H, W, hooks.ptr(bits), hooks.ptr(dst),
                                               cin, hooks.stream()) == 0
        assert same(dst, want * ref.DZ_UNIT * scale), (scale, word_scale)


def test_dz_writers_leave_the_range_word(lib):
    """bn_bwd and tanh_bwd with a range word: dZ as without one, the word = float bits of max |dZ| (raised from what was there)"""
    rng = np.random.default_rng(9)
    rows, C = 333, 128
    z, da = dev(rng.standard_normal((rows, C))), dev(rng.standard_normal((rows, C)) * 1e-6)
    stat = dev(np.concatenate([rng.standard_normal(C) * 0.1, 1.0 + rng.random(C)]))
    gamma, beta, m = dev(1.0 + rng.random(C)), dev(rng.standard_normal(C) * 0.1), dev(rng.standard_normal(2 * C) * 1e-7)
    dz0, dz1 = framed(rows, C), framed(rows, C)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.nsr_test_refine_bn_bwd(hooks.ptr(z), hooks.ptr(da), C, hooks.ptr(stat), hooks.ptr(gamma), hooks.ptr(beta), hooks.ptr(m),
                                      rows, C, hooks.ptr(dz0), hooks.stream()) == 0
    assert lib.nsr_test_refine_bn_bwd_range(hooks.ptr(z), hooks.ptr(da), C, hooks.ptr(stat), hooks.ptr(gamma), hooks.ptr(beta), hooks.ptr(m),
                                            rows, C, hooks.ptr(dz1), hooks.ptr(word), hooks.stream()) == 0
    assert torch.equal(dz0, dz1) and torch.equal(word, max_bits(dz0))
    px, B = 37, 3
    y, go = dev(np.tanh(rng.standard_normal((B * px, 3)))), dev(rng.standard_normal((B, 3, px)) * 1e-5)
    t0, t1 = framed(B * px, 32), framed(B * px, 32)
    big = torch.tensor([1.0], device="cuda").view(torch.int32)              # already above every |dZ|: stays
    for w_, want in ((torch.zeros(1, dtype=torch.int32, device="cuda"), None), (big.clone(), big)):
        assert lib.nsr_test_refine_tanh_bwd(hooks.ptr(y), hooks.ptr(go), px, B * px, hooks.ptr(t0), hooks.stream()) == 0
        assert lib.nsr_test_refine_tanh_bwd_range(hooks.ptr(y), hooks.ptr(go), px, B * px, hooks.ptr(t1), hooks.ptr(w_), hooks.stream()) == 0
        assert torch.equal(t0, t1) and torch.equal(w_, max_bits(t0) if want is None else want)
