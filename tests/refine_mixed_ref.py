"""Numpy forms of what the four launchers of the refinement network's split-fp16 training precision compute
(csrc/nsr_refine_train_work.h: refine_conv_f16x3, refine_flip_pack, refine_dgrad_f16x3, refine_fold2x2), on EXACT inputs:
activations that are integers in [-8, 8], weights that are integers in [-3, 3], dZ integers x 2^-30, every sum below 2^24 --
so the kernels' results are exact and the comparison is bit for bit.  float64 matrix products of such integers are exact.

The case lists of tests/test_gpu_refine_mixed_units.py live here, so that tests/test_refine_train_mixed_cpu.py can check on the
CPU that each deliberately wrong form (`wrong=`) changes the expected result of at least one of those very cases, and the
right forms against torch fp64."""
import numpy as np

DZ_UNIT = 2.0 ** -30

# (H, W, n_img, cin, cout, stride, up): the forward site convolution.  Images of 2 x 3, 8 x 8, 8 x 16, 16 x 24; 1 and 3 images;
# M = 6, 192, 24 ... are no multiples of the 128-row tile, 3 x 16 x 24 = 1152 is; stride 2 and the x2 upsample as the layers have
FWD_CASES = [
    (2, 3, 1, 128, 128, 1, 0), (2, 3, 3, 128, 3, 1, 1), (8, 8, 3, 128, 128, 1, 0), (8, 8, 1, 256, 128, 2, 0),
    (8, 16, 1, 256, 128, 1, 1), (8, 16, 3, 128, 3, 1, 0), (16, 24, 3, 128, 128, 1, 0), (16, 24, 1, 128, 128, 2, 0),
    (16, 24, 1, 256, 128, 1, 0),
]
# (H, W, n_img, cin, cout, up): the input gradient; H x W is the SOURCE (the gradient's) extent, dZ is (2 H x 2 W with up)
DGRAD_CASES = [
    (2, 3, 1, 128, 128, 0), (2, 3, 3, 256, 128, 1), (8, 8, 3, 128, 3, 0), (8, 8, 1, 128, 128, 1), (8, 16, 3, 256, 128, 0),
    (8, 16, 1, 128, 3, 1), (16, 24, 1, 128, 128, 0), (16, 24, 3, 128, 3, 0), (16, 24, 1, 256, 128, 0),
]
# (Hs, Ws, n_img, C): the 2 x 2 fold alone
FOLD_CASES = [(2, 3, 1, 128), (8, 8, 3, 256), (8, 16, 1, 128), (16, 24, 3, 128)]
# (cin, cout): the flipped pack alone
PACK_CASES = [(128, 128), (256, 128), (128, 3)]


def pad32(n):
    return (n + 31) & ~31


def ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


def weights(cin, cout):
    """(cout, cin, 3, 3) integers in [-3, 3] that differ from tap to tap and between (n, c) and (c, n): a missing flip or a
    swapped transpose changes them"""
    n, c, ky, kx = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(3), np.arange(3), indexing="ij")
    return ((n * 5 + c * 3 + (ky * 3 + kx) * (1 + n % 3) + (n * c) % 7) % 7 - 3).astype(np.float64)


def upsample2(x):
    """nearest x2 of (n, H, W, C)"""
    return x.repeat(2, axis=1).repeat(2, axis=2)


def conv_fwd(x, w, stride=1, up=0, bias=None, wrong=""):
    """x (n, Hs, Ws, cin), w (cout, cin, 3, 3) -> (n, Ho, Wo, cout): 3 x 3 / pad 1 behind the optional nearest x2 upsample.
    wrong = "no_upsample": the convolution runs on the source and its OUTPUT is upsampled instead."""
    if up and wrong != "no_upsample":
        x = upsample2(x)
    n, H, W, cin = x.shape
    cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = np.zeros((n, H + 2, W + 2, cin))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((n, Ho, Wo, cout))
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H:stride, kx:kx + W:stride][:, :Ho, :Wo] @ w[:, :, ky, kx].T
    if bias is not None:
        out += bias
    if up and wrong == "no_upsample":
        out = upsample2(out)
    return out


def dgrad(dz, w, wrong=""):
    """dz (n, H, W, >= cout) [the columns past cout are padding and must not matter], w (cout, cin, 3, 3) ->
    dx[(img, y, x)][c] = sum over (ky, kx, n) of dz[(img, y + 1 - ky, x + 1 - kx)][n] w[n][c][ky][kx]   (n, H, W, cin).
    wrong = "no_flip": the taps are not mirrored; "swap": w[c][n] for w[n][c] (square weights only)."""
    n, H, W, _ = dz.shape
    cout, cin = w.shape[:2]
    dzp = np.zeros((n, H + 2, W + 2, cout))
    dzp[:, 1:-1, 1:-1] = dz[..., :cout]
    dx = np.zeros((n, H, W, cin))
    for ky in range(3):
        for kx in range(3):
            ty, tx = (ky, kx) if wrong == "no_flip" else (2 - ky, 2 - kx)
            m = w[:, :, ky, kx]
            dx += dzp[:, ty:ty + H, tx:tx + W] @ (m.T if wrong == "swap" and cin == cout else m)
    return dx


def fold2x2(g, wrong=""):
    """(n, 2 Hs, 2 Ws, C) -> (n, Hs, Ws, C): the nearest x2 upsample backwards.  wrong = "one_pixel": one of the four."""
    if wrong == "one_pixel":
        return g[:, 0::2, 0::2].copy()
    return ((g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + g[:, 1::2, 0::2]) + g[:, 1::2, 1::2]


def flip_pack(w, np_):
    """(cin, 9 np) matrix B'[c][((2 - ky) * 3 + (2 - kx)) np + n] = 64 w[n][c][ky][kx], zero for n >= cout"""
    cout, cin = w.shape[:2]
    b = np.zeros((cin, 9, np_))
    for ky in range(3):
        for kx in range(3):
            b[:, (2 - ky) * 3 + (2 - kx), :cout] = 64.0 * w[:, :, ky, kx].T
    return b.reshape(cin, 9 * np_)


def range_exponent(max_abs):
    """the power of two refine_dgrad_kernel multiplies dZ by: max |dZ| -> [2^13, 2^14); 0 for max = 0"""
    if not max_abs > 0:
        return 0
    e = int(np.float32(max_abs).view(np.uint32) >> 23) - 127
    return int(np.clip(13 - e, -100, 100))


def fwd_inputs(case, seed=0):
    H, W, n, cin, cout, stride, up = case
    rng = np.random.default_rng(1000 + seed)
    return ints(rng, (n, H, W, cin), 8), weights(cin, cout), ints(rng, (cout,), 8)


def fwd_expected(case, wrong=""):
    x, w, b = fwd_inputs(case)
    return conv_fwd(x, w, case[5], case[6], b, wrong)


def dgrad_inputs(case, seed=0):
    H, W, n, cin, cout, up = case
    rng = np.random.default_rng(2000 + seed)
    r = 2 if up else 1
    return ints(rng, (n, r * H, r * W, pad32(cout)), 8), weights(cin, cout)      # padding columns of dZ filled too


def dgrad_expected(case, wrong=""):
    """in units of 2^-30 (wrong = "scaled": the range scale is not removed)"""
    dz, w = dgrad_inputs(case)
    g = dgrad(dz, w, wrong)
    if case[5]:
        g = fold2x2(g, wrong)
    if wrong == "scaled":
        g = g * 2.0 ** range_exponent(np.abs(dz[..., :]).max() * DZ_UNIT)
    return g
