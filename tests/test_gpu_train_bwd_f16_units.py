"""The two kernels of csrc/nsr_train_bwd_f16.hip (precision NSR_F16X3_GEMM_BWD) alone, through tests/csrc/nsr_test_hooks_train_bwd.hip,
on EXACT inputs: small integers times powers of two, chosen so that every hi / lo half, every product and every partial sum is
exact in the kernels' arithmetic.  The result must equal int64 numpy bit for bit; a wrong fragment map, k order, transpose or
scale changes every output (every element of both operands is a different-looking nonzero integer).  Small integers have
zero lo halves; the `lo_planes` tests give ONE operand 12-bit integers (hi = the value rounded to 11 bits, lo = +-1 unit or 0),
so that the lo hi and hi lo terms and the lo planes' fragment maps are inside the bit-exact comparison too (with one wide
operand lo lo = 0: the three terms are the whole product).

One random case per kernel goes against the numpy restatement (tests/train_bwd_ref.py, checked against fp64 on the CPU) at the
accuracy the arithmetic promises."""
import ctypes
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from . import hooks
from . import train_bwd_ref as ref

pytestmark = pytest.mark.gpu

SIGS = {
    "nsr_test_split_f16_t": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "nsr_test_absmax_bits": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "nsr_test_dgrad_f16x3": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                     c_int, c_void_p, c_void_p, c_void_p]),
    "nsr_test_bwd_f16_slice_len": (c_int64, [c_int64, c_int]),
    "nsr_test_n_splits": (c_int, [c_int64]),
    "nsr_test_wgrad_f16x3": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_int, c_int64,
                                     c_void_p]),
}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    h = hooks.load()
    for name, (res, args) in SIGS.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    return h


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def ints(rng, shape, lo=-7, hi=7):
    """integers in [lo, hi] without zeros"""
    v = rng.integers(lo, hi, shape)
    return np.where(v == 0, hi, v).astype(np.int64)


def wide(rng, shape):
    """12-bit integers of either sign, 2048 <= |v| <= 4095: as fp16 (hi, lo) halves hi = v rounded to 11 bits and lo = v - hi is
    -1, 0 or +1 of v's unit: half the elements have a non-zero lo half"""
    return (rng.integers(2048, 4096, shape) * rng.choice([-1, 1], shape)).astype(np.int64)


class Dgrad:
    """dx = (dy w[:, c0 : c0 + N]) * [mask > 0] through split_f16_t + dgrad_f16x3; every buffer wider than it needs to be"""

    def __init__(self, lib, w_int, c0=0, N=None, wscale=2.0 ** -9):
        self.lib, self.K, self.cols = lib, w_int.shape[0], w_int.shape[1]
        self.N = self.cols - c0 if N is None else N
        self.c0, self.wscale = c0, wscale
        self.w = dev(w_int.astype(np.float64) * wscale)                           # (K, cols): the nn.Linear layout, K rows
        self.halves = torch.zeros(2 * self.K * self.cols, dtype=torch.int16, device="cuda")
        assert lib.nsr_test_split_f16_t(hooks.ptr(self.w), self.K, self.cols, self.cols, hooks.ptr(self.halves), hooks.stream()) == 0

    def run(self, dy, mask=None, mask_c0=0, col_tiles=False, out_max=False, pad=4):
        P = dy.shape[0]
        lddy, lddx = self.K + pad, self.N + 2 * pad
        a = torch.full((P, lddy), 77.0, device="cuda")
        a[:, :self.K] = dy
        dx = torch.full((P, lddx), float("nan"), device="cuda")
        tiles = torch.full(((P + 127) // 128, self.N), float("nan"), device="cuda") if col_tiles else None
        word = torch.zeros(1, dtype=torch.int32, device="cuda") if out_max else None
        rc = self.lib.nsr_test_dgrad_f16x3(hooks.ptr(a), lddy, self.K, hooks.ptr(self.halves, self.c0 * self.K), self.K * self.cols, self.K,
                                           hooks.ptr(mask, mask_c0) if mask is not None else None, mask.shape[1] if mask is not None else 0,
                                           hooks.ptr(dx), lddx, P, self.N, hooks.ptr(tiles), hooks.ptr(word), hooks.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert torch.isnan(dx[:, self.N:]).all()                                   # nothing behind the N columns
        return dx[:, :self.N].cpu().numpy(), None if tiles is None else tiles.cpu().numpy(), None if word is None else int(word.item())


def exact_dgrad(dy_int, dy_scale, w_int, wscale, c0, N, mask=None):
    """int64 product, scaled by the (power-of-two) scales of the rows and of the weights"""
    prod = dy_int @ w_int[:, c0:c0 + N]
    out = prod.astype(np.float64) * np.asarray(dy_scale, np.float64).reshape(-1, 1) * wscale
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)          # representable: the comparison is exact
    if mask is not None:
        out = np.where(mask > 0, out, 0.0)
    return out.astype(np.float32)


@pytest.mark.parametrize("K,N", [(32, 32), (96, 96), (224, 160), (288, 256), (32, 256), (288, 32)])
@pytest.mark.parametrize("P", [1, 33, 129, 257])
def test_dgrad_exact(lib, K, N, P):
    """Below, at and across the 128 tile in K, N and P; a mask with its own row stride and a column offset; a weight column
    offset (a skip layer's h columns); col_tiles = the column sums per 128-row tile; the range word = max |dx|."""
    rng = np.random.default_rng(K * 1000 + N + P)
    c0 = 32
    w_int = ints(rng, (K, c0 + N + 32))
    dy_int = ints(rng, (P, K), -15, 15)
    row_e = rng.integers(-30, -10, P)                                              # every row its own magnitude
    dy = dy_int.astype(np.float64) * np.exp2(row_e)[:, None]
    mask_np = rng.integers(-1, 2, (P, N + 40)).astype(np.float32)
    d = Dgrad(lib, w_int, c0, N)
    got, tiles, word = d.run(dev(dy), dev(mask_np), 8, col_tiles=True, out_max=True)
    want = exact_dgrad(dy_int, np.exp2(row_e), w_int, d.wscale, c0, N, mask_np[:, 8:8 + N])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the sums of at most 128 values 2^e x integer stay exact in fp32 when the rows share a scale; here they do not, so sum in the
    # kernel's order is not specified beyond "fp32": compare against the fp64 sum at fp32 accuracy of the largest term
    for t in range(tiles.shape[0]):
        rows = want[128 * t:128 * (t + 1)].astype(np.float64)
        assert np.allclose(tiles[t], rows.sum(0), rtol=0, atol=2.0 ** -20 * np.abs(rows).sum(0).max() + 1e-30)
    assert word == int(np.abs(want).max().view(np.uint32))
    # without mask / tiles / word: the plain product
    got2, _, _ = d.run(dev(dy))
    assert np.array_equal(got2, exact_dgrad(dy_int, np.exp2(row_e), w_int, d.wscale, c0, N))


@pytest.mark.parametrize("side", ["dy", "w"])
@pytest.mark.parametrize("K,N,P", [(96, 160, 33), (288, 96, 257)])
def test_dgrad_exact_lo_planes(lib, side, K, N, P):
    """One operand 12 bits wide: its lo plane is non-zero and meets the other's hi plane (`dy`: the lo hi term, `w`: hi lo).
    |sum| <= 288 x 4095 x 7 < 2^24 units: every partial sum is exact whatever the order."""
    rng = np.random.default_rng(K + N + P + len(side))
    c0 = 32
    w_int = wide(rng, (K, c0 + N)) if side == "w" else ints(rng, (K, c0 + N))
    dy_int = wide(rng, (P, K)) if side == "dy" else ints(rng, (P, K))
    assert (np.abs(dy_int) if side == "dy" else np.abs(w_int)).max() >= 2048 and ((dy_int if side == "dy" else w_int) % 2 != 0).mean() > 0.3
    row_e = rng.integers(-30, -10, P)
    mask_np = rng.integers(-1, 2, (P, N)).astype(np.float32)
    d = Dgrad(lib, w_int, c0, N)
    got, _, word = d.run(dev(dy_int.astype(np.float64) * np.exp2(row_e)[:, None]), dev(mask_np), out_max=True)
    want = exact_dgrad(dy_int, np.exp2(row_e), w_int, d.wscale, c0, N, mask_np)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert word == int(np.abs(want).max().view(np.uint32))


def test_dgrad_col_tiles_exact_when_rows_share_a_scale(lib):
    rng = np.random.default_rng(3)
    K, N, P = 96, 160, 300
    w_int, dy_int = ints(rng, (K, N)), ints(rng, (P, K), -15, 15)
    d = Dgrad(lib, w_int)
    got, tiles, _ = d.run(dev(dy_int * 2.0 ** -20), col_tiles=True)
    want = exact_dgrad(dy_int, np.full(P, 2.0 ** -20), w_int, d.wscale, 0, N)
    assert np.array_equal(got, want)
    for t in range(3):
        assert np.array_equal(tiles[t], want[128 * t:128 * (t + 1)].astype(np.float64).sum(0).astype(np.float32))


def test_dgrad_zero_matrix_and_mixed_magnitudes(lib):
    rng = np.random.default_rng(4)
    K, N, P = 96, 96, 130
    w_int = ints(rng, (K, N))
    d = Dgrad(lib, w_int)
    got, tiles, word = d.run(torch.zeros(P, K, device="cuda"), col_tiles=True, out_max=True)
    assert (got == 0).all() and (tiles == 0).all() and word == 0
    # rows of 2^-40 next to rows of 2^0 in one tile: each exact
    dy_int = ints(rng, (P, K), -15, 15)
    scale = np.where(np.arange(P) % 2 == 0, 2.0 ** -40, 1.0)
    got, _, _ = d.run(dev(dy_int * scale[:, None]))
    assert np.array_equal(got, exact_dgrad(dy_int, scale, w_int, d.wscale, 0, N))
    # a zero row among them stays zero; non-finite values stay in their row
    dy = dy_int * scale[:, None]
    dy[5] = 0
    dy[7, 3] = np.inf
    got, _, _ = d.run(dev(dy))
    assert (got[5] == 0).all() and not np.isfinite(got[7]).all()
    keep = np.ones(P, bool)
    keep[[5, 7]] = False
    assert np.array_equal(got[keep], exact_dgrad(dy_int, scale, w_int, d.wscale, 0, N)[keep])


def test_dgrad_row_locality(lib):
    """A row's bits are the same computed alone, at another position, or among other tile mates (random data: no exactness)."""
    rng = np.random.default_rng(6)
    K, N, P = 224, 160, 200
    w = (rng.standard_normal((K, N)) * 0.05)
    d = Dgrad(lib, np.zeros((K, N), np.int64))
    d.w = dev(w)
    assert lib.nsr_test_split_f16_t(hooks.ptr(d.w), K, N, N, hooks.ptr(d.halves), hooks.stream()) == 0
    dy = (rng.standard_normal((P, K)) * np.exp2(rng.integers(-30, 0, (P, 1)))).astype(np.float32)
    mask = rng.standard_normal((P, N)).astype(np.float32)
    full, _, _ = d.run(dev(dy), dev(mask))
    for r in (0, 77, 131, 199):
        alone, _, _ = d.run(dev(dy[r:r + 1]), dev(mask[r:r + 1]))
        assert np.array_equal(alone[0].view(np.uint32), full[r].view(np.uint32)), r
    perm = rng.permutation(P)
    moved, _, _ = d.run(dev(dy[perm]), dev(mask[perm]))
    assert np.array_equal(moved.view(np.uint32), full[perm].view(np.uint32))
    others = dy.copy()
    others[1::2] *= 1e6                                                            # other tile mates, much larger
    mixed, _, _ = d.run(dev(others), dev(mask))
    assert np.array_equal(mixed[0::2].view(np.uint32), full[0::2].view(np.uint32))
    # ... and the restatement holds it to the promised accuracy
    want = ref.dgrad(dy, w.astype(np.float32), mask)
    bound = (2.0 ** -20 + (3 * K / 16) * 2.0 ** -23) * (np.abs(dy).astype(np.float64) @ np.abs(w)) + 1e-45
    assert (np.abs(full.astype(np.float64) - want) <= bound).all()


# ---- weight gradient --------------------------------------------------------------------------------------------------------
def run_wgrad(lib, dy, x, M, N, splits, dy_c0=0, x_c0=0):
    """dy (P, >= dy_c0 + M), x (P, >= x_c0 + N) device tensors -> (splits, M, N) slices; the range word from absmax_bits"""
    P = dy.shape[0]
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.nsr_test_absmax_bits(hooks.ptr(dy), dy.shape[1], P, dy_c0, M, hooks.ptr(word), hooks.stream()) == 0
    stride = M * N + 64
    part = torch.full((splits, stride), float("nan"), device="cuda")
    rc = lib.nsr_test_wgrad_f16x3(hooks.ptr(dy, dy_c0), dy.shape[1], M, hooks.ptr(x, x_c0), x.shape[1], N, P, hooks.ptr(word),
                                  hooks.ptr(part), splits, stride, hooks.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.isnan(part[:, M * N:]).all()
    return part[:, :M * N].reshape(splits, M, N).cpu().numpy(), int(word.item())


@pytest.mark.parametrize("M,N", [(32, 32), (32, 96), (96, 64), (224, 288)])
@pytest.mark.parametrize("P", [100, 900, 1100, 1568])
def test_wgrad_exact(lib, M, N, P):
    """1, 2, 3 and 4 slices (n_splits(P)) with a ragged last slice and a ragged last K tile; row strides larger than the widths
    and column offsets in both operands; each slice = the int64 sum over its points; x 2^-16 and x 2^8 scale exactly."""
    rng = np.random.default_rng(M * 1000 + N + P)
    splits = lib.nsr_test_n_splits(P)
    assert splits == ref.n_splits(P) == {100: 1, 900: 2, 1100: 3, 1568: 4}[P]
    L = lib.nsr_test_bwd_f16_slice_len(P, splits)
    assert L == ref.slice_len(P, splits) and L % 32 == 0 and (splits - 1) * L < P <= splits * L
    dy_int, x_int = ints(rng, (P, M + 36), -3, 3), ints(rng, (P, N + 8), -3, 3)
    want = np.stack([dy_int[z * L:(z + 1) * L, 4:4 + M].T @ x_int[z * L:(z + 1) * L, 8:8 + N] for z in range(splits)])
    assert np.abs(want).max() < 2 ** 24
    x = dev(x_int * 2.0 ** -3)
    for k in (-22, -22 - 16, -22 + 8):
        got, word = run_wgrad(lib, dev(dy_int * 2.0 ** k), x, M, N, splits, 4, 8)
        assert word == int(np.float32(3 * 2.0 ** k).view(np.uint32))
        assert np.array_equal(got, (want * 2.0 ** (k - 3)).astype(np.float32)), k


@pytest.mark.parametrize("side", ["dy", "x"])
@pytest.mark.parametrize("M,N,P", [(96, 64, 100), (224, 160, 900)])
def test_wgrad_exact_lo_planes(lib, side, M, N, P):
    """One operand 12 bits wide (see test_dgrad_exact_lo_planes); a slice holds at most 480 points: |sum| <= 480 x 4095 x 3 < 2^24."""
    rng = np.random.default_rng(M + N + P + len(side))
    splits = lib.nsr_test_n_splits(P)
    L = lib.nsr_test_bwd_f16_slice_len(P, splits)
    dy_int = wide(rng, (P, M + 4)) if side == "dy" else ints(rng, (P, M + 4), -3, 3)
    x_int = wide(rng, (P, N + 8)) if side == "x" else ints(rng, (P, N + 8), -3, 3)
    want = np.stack([dy_int[z * L:(z + 1) * L, 4:4 + M].T @ x_int[z * L:(z + 1) * L, 8:8 + N] for z in range(splits)])
    assert np.abs(want).max() < 2 ** 24 and L <= 480
    kx = -12 if side == "x" else -3                                   # x in [0.5, 1) or small multiples of 2^-3: inside fp16 as it is
    for k in (-30, -30 + 8):
        got, word = run_wgrad(lib, dev(dy_int * 2.0 ** k), dev(x_int * 2.0 ** kx), M, N, splits, 4, 8)
        assert word == int(np.float32(np.abs(dy_int[:, 4:4 + M]).max() * 2.0 ** k).view(np.uint32))
        assert np.array_equal(got, (want * 2.0 ** (k + kx)).astype(np.float32)), k


def test_wgrad_zero_and_restatement(lib):
    rng = np.random.default_rng(8)
    P, M, N = 1100, 96, 160
    x = np.maximum(rng.standard_normal((P, N)), 0).astype(np.float32)
    got, word = run_wgrad(lib, torch.zeros(P, M, device="cuda"), dev(x), M, N, 3)
    assert (got == 0).all() and word == 0
    dy = (rng.standard_normal((P, M)) * 3e-7).astype(np.float32)
    got, _ = run_wgrad(lib, dev(dy), dev(x), M, N, 3)
    again, _ = run_wgrad(lib, dev(dy), dev(x), M, N, 3)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    L = ref.slice_len(P, 3)
    for z in range(3):
        a, b = dy[z * L:(z + 1) * L].astype(np.float64), x[z * L:(z + 1) * L].astype(np.float64)
        bound = (2.0 ** -20 + (3 * L / 16) * 2.0 ** -23) * (np.abs(a).T @ np.abs(b)) + 1e-45
        assert (np.abs(got[z] - a.T @ b) <= bound).all(), z
    want = ref.wgrad(dy, x, 3)
    assert np.abs(got - want).max() <= 2.0 ** -18 * np.abs(want).max()
