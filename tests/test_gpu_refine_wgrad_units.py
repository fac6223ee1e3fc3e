"""The launcher of the refinement network's implicit split-fp16 weight gradient ALONE on exact inputs
(csrc/nsr_refine_train_work.h: refine_wgrad_f16x3 -- kernel and slice-order reduce), reached through
tests/csrc/nsr_test_hooks_refine_wgrad.hip.  Activations are integers in [-8, 8], dZ integers x 2^-30 with the range word set to
the bits of max |dZ|, every sum is below 2^24: the result must EQUAL tests/refine_wgrad_ref.py's numpy form bit for bit.  The
gradient is compared as a whole NaN-framed buffer; the input is a slice (ch0 != 0, ld > C) of a NaN buffer, so nothing outside
it may be read; a gradient that is stored (acc = 0) starts NaN-filled."""
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from . import hooks
from . import refine_wgrad_ref as ref

pytestmark = pytest.mark.gpu

FRAME = 64
SIGNATURES = {
    "nsr_test_refine_wgrad_f16x3": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int64] + [c_int] * 6 + [c_void_p, c_void_p, c_int64, c_int,
                                            c_void_p, c_int64, c_void_p]),
    "nsr_test_refine_wgrad_slice_len": (c_int64, [c_int, c_int, c_int64]),
}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    lib = hooks.load()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def in_slice(x2d, ld, ch0):
    buf = torch.full((x2d.shape[0], ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, ch0:ch0 + x2d.shape[1]] = dev(x2d)
    return buf


def max_bits(t):
    return t.abs().max().reshape(1).view(torch.int32)


def run(lib, c, dz, x, g0=None, bits=None, scale=1.0):
    """one call on dz (units of 2^-30) x scale; returns the whole framed gradient buffer and the expected frame maker"""
    Ho, Wo = ref.out_extent(c)
    np_ = dz.shape[-1]
    dzd = dev(dz * (ref.DZ_UNIT * scale))
    assert np.array_equal(dzd.cpu().numpy().astype(np.float64), dz * (ref.DZ_UNIT * scale))
    bits = max_bits(dzd) if bits is None else bits
    ld, ch0 = c.cin + 256, 128
    src = in_slice(x.reshape(-1, c.cin), ld, ch0)
    n_w = c.cout * c.cin * 9
    n_slices = -(-(c.n * Ho * Wo) // ref.used_slice_len(c))
    part = torch.full(((c.part_slices or n_slices) * n_w,), float("nan"), dtype=torch.float32, device="cuda")
    g = torch.full((n_w + 2 * FRAME,), float("nan"), dtype=torch.float32, device="cuda")
    if g0 is not None:
        g[FRAME:FRAME + n_w] = dev(g0.reshape(-1) * (ref.DZ_UNIT * scale))
    rc = lib.nsr_test_refine_wgrad_f16x3(hooks.ptr(dzd), np_, c.cout, hooks.ptr(src, ch0), ld, c.cin, c.n, c.H, c.W, c.stride, c.up,
                                         hooks.ptr(bits), hooks.ptr(part), part.numel(), 1 if g0 is not None else 0, hooks.ptr(g, FRAME),
                                         c.slice_len, hooks.stream())
    assert rc == 0
    return g


def framed(want):
    out = np.full(want.size + 2 * FRAME, np.nan, dtype=np.float32)
    out[FRAME:FRAME + want.size] = want.reshape(-1)
    return out


def same(got, want):
    return np.array_equal(got.cpu().numpy(), want, equal_nan=True)


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_weight_gradient(lib, case):
    dz, x, g0 = ref.inputs(case)
    got = run(lib, case, dz, x, g0 if case.acc else None)
    want = ref.expected(case) * ref.DZ_UNIT
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert same(got, framed(want))


def test_slice_length_is_the_reference_function(lib):
    for cin, cout, k in ((128, 128, 6), (128, 128, 1152), (128, 128, 1 << 20), (1536, 512, 8192), (128, 3, 131072), (512, 512, 65536),
                         (256, 128, 96), (1024, 512, 2048)):
        assert lib.nsr_test_refine_wgrad_slice_len(cin, cout, k) == ref.slice_len(cin, cout, k)


def test_range_word_scales_zero_and_repeat(lib):
    """dZ x 2^-16 and x 2^8 give the gradient x 2^-16 / 2^8 exactly (the power of two follows the word); a word from a larger
    maximum than this dZ holds changes nothing on exact inputs; a zero word with a zero dZ gives exact zeros over a NaN-filled
    gradient; two identical calls give equal bits."""
    case = ref.CASES[8]                                                          # 16 x 24 x 3: 4.5 slices of the product's own length
    dz, x, _ = ref.inputs(case)
    want = ref.wgrad(dz, x, case.stride, case.up, case.cout) * ref.DZ_UNIT
    for scale, word_scale in ((1.0, 1.0), (2.0 ** -16, 1.0), (2.0 ** 8, 1.0), (1.0, 4.0)):
        bits = max_bits(dev(dz * (ref.DZ_UNIT * scale * word_scale)))
        assert same(run(lib, case, dz, x, bits=bits, scale=scale), framed(want * scale)), (scale, word_scale)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = run(lib, case, np.zeros_like(dz), x, bits=zero)
    assert same(got, framed(np.zeros_like(want)))
    assert not np.signbit(got.cpu().numpy()[FRAME:-FRAME]).any()
    wide = ref.CASES[-2]
    dzw, xw, _ = ref.inputs(wide)
    a, b = run(lib, wide, dzw, xw), run(lib, wide, dzw, xw)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
