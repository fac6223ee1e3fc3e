"""Numpy form of what the refinement network's implicit split-fp16 weight gradient computes
(csrc/nsr_refine_wgrad_f16.hip, launcher refine_wgrad_f16x3 of csrc/nsr_refine_train_work.h):

    dW[n][c][ky][kx] = sum over the output pixels (b, y, x) of dZ[b, y, x][n] X[b, s y + ky - 1, s x + kx - 1][c]

with zero padding and X read through the nearest x2 upsample where the site has one -- on EXACT inputs: activations that are
integers in [-8, 8], dZ integers x 2^-30, every sum below 2^24, so that the kernel's result is exact and the comparison is bit for
bit.  Two cases carry values of more than 11 bits in ONE operand (u 2^11 + v): their fp16 (hi, lo) split has a non-zero lo half,
so a dropped cross term shows, while lo x lo (which the kernel drops by design) stays zero.

The case list of tests/test_gpu_refine_wgrad_units.py lives here, so that tests/test_refine_wgrad_cpu.py can check on the CPU
that each deliberately wrong form (`wrong=`) changes the expected result of at least one of those very cases, and the right
form against torch fp64."""
from collections import namedtuple

import numpy as np

from .refine_mixed_ref import DZ_UNIT, ints, pad32, range_exponent, upsample2

# H x W: the SOURCE extent (before the optional upsample); slice_len: 0 = the product's own (slice_len() below), otherwise the
# override of the test hook; part_slices: slices the partial buffer of the call holds (0: all of them -- one pass);
# acc: the call adds to a known gradient; wide: "" / "dz" / "x" -- the operand with values of more than 11 bits
Case = namedtuple("Case", "H W n cin cout stride up slice_len part_slices acc wide")
CASES = [
    Case(2, 3, 1, 128, 128, 1, 0, 0, 0, 0, ""),        # K = 6: less than one K tile of 32
    Case(2, 3, 3, 256, 128, 1, 1, 0, 0, 1, ""),        # upsample, K = 72, two column tiles per tap
    Case(8, 8, 3, 128, 3, 1, 0, 0, 0, 0, ""),          # D.conv9's shape: 3 of the tile's 128 rows stored
    Case(8, 8, 1, 128, 128, 2, 0, 0, 0, 0, ""),        # stride 2
    Case(5, 7, 1, 128, 128, 2, 0, 0, 0, 0, ""),        # stride 2 on odd extents (Ho x Wo = 3 x 4)
    Case(5, 7, 3, 128, 128, 1, 0, 32, 0, 0, ""),       # K = 105: slices 32, 32, 32, 9 -- ends inside a slice and inside a K tile
    Case(8, 16, 3, 256, 128, 2, 0, 32, 0, 1, ""),      # stride 2, K = 96: three whole slices, accumulating (the encoder's 2nd call)
    Case(8, 16, 1, 128, 128, 1, 1, 96, 0, 0, ""),      # upsample, K = 512: five slices of 96 and one of 32
    Case(16, 24, 3, 128, 128, 1, 0, 0, 0, 0, ""),      # K = 1152 at the product's own slice length (256): 4.5 slices
    Case(16, 24, 1, 128, 3, 1, 0, 64, 4, 1, ""),       # six slices in passes of four (the partial buffer holds four)
    Case(16, 24, 1, 256, 128, 2, 0, 0, 0, 0, ""),      # stride 2, K = 96
    Case(8, 8, 3, 128, 128, 1, 0, 0, 0, 0, "dz"),      # dZ = u 2^11 + v: its lo half x the input's hi half
    Case(8, 8, 3, 128, 128, 1, 0, 0, 0, 0, "x"),       # input = u 2^11 + v: dZ's hi half x its lo half
]
WRONG_FORMS = ["no_tap", "no_stride", "no_upsample", "swap", "clamp", "scaled", "no_acc", "drop_last_slice", "drop_hilo", "drop_lohi"]


def case_id(c):
    return "x".join(str(v) for v in c if v != "") + (f"-wide_{c.wide}" if c.wide else "")


def out_extent(c):
    r = 2 if c.up else 1
    return (r * c.H - 1) // c.stride + 1, (r * c.W - 1) // c.stride + 1


def slice_len(cin, cout, K):
    """refine_wgrad_slice_len: pixels per slice, a function of the shape alone"""
    tiles = 9 * (cin // 128) * ((cout + 127) // 128)
    want = (2048 + tiles - 1) // tiles
    n = ((K + want - 1) // want + 31) // 32 * 32
    return min(max(n, 256), 4096)


def split16(v):
    """fp16 (hi, lo) halves of float64 values, as the kernel's staging makes them (both in float64)"""
    hi = v.astype(np.float16).astype(np.float64)
    lo = (v - hi).astype(np.float16).astype(np.float64)
    return hi, lo


def wgrad(dz, x, stride, up, cout, wrong="", slice_px=0):
    """dz (n, Ho, Wo, >= cout) [columns past cout are padding and must not matter], x (n, Hs, Ws, cin) -> (cout, cin, 3, 3).
    wrong: "no_tap" -- every tap reads the centre; "no_stride" -- the input is read at stride 1; "no_upsample" -- the source is
    read as the top-left corner of the upsampled extent; "swap" -- dW[c][n] for dW[n][c] (square cases); "clamp" -- the border
    repeats instead of zero padding; "drop_last_slice" -- the pixels behind the last whole slice of `slice_px` are left out;
    "drop_hilo" / "drop_lohi" -- the product without dZ_hi x X_lo / dZ_lo x X_hi of the fp16 split (dZ at the kernel's scale)."""
    n, Ho, Wo, _ = dz.shape
    cin = x.shape[-1]
    if up:
        if wrong == "no_upsample":
            big = np.zeros((n, 2 * x.shape[1], 2 * x.shape[2], cin))
            big[:, :x.shape[1], :x.shape[2]] = x
            x = big
        else:
            x = upsample2(x)
    H, W = x.shape[1:3]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge" if wrong == "clamp" else "constant")
    z = dz[..., :cout].reshape(-1, cout)
    K = z.shape[0]
    if wrong == "drop_last_slice" and K % slice_px:
        z = z.copy()
        z[K // slice_px * slice_px:] = 0.0
    s = 2.0 ** range_exponent(np.abs(dz).max() * DZ_UNIT) * DZ_UNIT     # dz is in units of 2^-30: the kernel's scaled operand
    zh, zl = split16(z * s)
    dw = np.zeros((cout, cin, 3, 3))
    for ky in range(3):
        for kx in range(3):
            ty, tx = (1, 1) if wrong == "no_tap" else (ky, kx)
            st = 1 if wrong == "no_stride" else stride
            p = xp[:, ty:ty + H:st, tx:tx + W:st][:, :Ho, :Wo].reshape(-1, cin)
            t = z.T @ p
            if wrong in ("drop_hilo", "drop_lohi"):
                ph, pl = split16(p)
                t = t - (zh.T @ pl if wrong == "drop_hilo" else zl.T @ ph) / s
            dw[:, :, ky, kx] = t
    if wrong == "swap" and cin == cout:
        dw = dw.transpose(1, 0, 2, 3).copy()
    return dw


def inputs(c, seed=0):
    """dz (n, Ho, Wo, pad32(cout)) in units of 2^-30 with the padding columns filled too, x (n, H, W, cin), the gradient the call
    adds to (cout, cin, 3, 3), in units of 2^-30"""
    rng = np.random.default_rng(3000 + seed)
    Ho, Wo = out_extent(c)
    dz, x = ints(rng, (c.n, Ho, Wo, pad32(c.cout)), 8), ints(rng, (c.n, c.H, c.W, c.cin), 8)
    if c.wide == "dz":
        dz = dz + 2048.0 * ints(rng, dz.shape, 3)
    if c.wide == "x":
        x = x + 2048.0 * ints(rng, x.shape, 3)
    g0 = ints(rng, (c.cout, c.cin, 3, 3), 1 << 10)
    return dz, x, g0


def used_slice_len(c):
    Ho, Wo = out_extent(c)
    return c.slice_len or slice_len(c.cin, c.cout, c.n * Ho * Wo)


def expected(c, wrong=""):
    """what the call leaves in the gradient, in units of 2^-30"""
    dz, x, g0 = inputs(c)
    g = wgrad(dz, x, c.stride, c.up, c.cout, wrong, used_slice_len(c))
    if wrong == "scaled":
        g = g * 2.0 ** range_exponent(np.abs(dz).max() * DZ_UNIT)
    if c.acc and wrong != "no_acc":
        g = g + g0
    return g
