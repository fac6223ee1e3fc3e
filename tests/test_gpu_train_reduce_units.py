"""Unit layer between the matrix products and the gradient tensors, part 1: the reduction and placement kernels of the
layer-by-layer path (csrc/nsr_train_gemm.hip: place_kernel, scatter_heads_kernel, colsum_few_kernel, tilesum_partial_kernel,
sum_finish_kernel, reduce_place_kernel) and the head streams of the chain path (csrc/nsr_train_wgrad.hip:
panel_wsums_kernel<128, 3> and <256, 1>), each launched on its own through the product's launcher (csrc/nsr_train_work.h; hooks:
tests/csrc/nsr_test_hooks_reduce.hip).  Reference, inputs and the exact regime: tests/train_reduce_ref.py, pinned on the CPU by
tests/test_train_reduce_cpu.py; the device side and the house rules (guards, whole-buffer comparison): tests/train_reduce_gpu.py.

All inputs but the two real-valued panel cases are integers for which no sum rounds: every comparison is bit for bit.

Which case reaches which branch:
  place          (1, 1) one thread; (258, 63) and (128, 283) several blocks with a partial last one; both transposes; r0, c0,
                 col0 non-zero, src_ld > cols; -0.0 and a NaN payload inside the rectangle (a copy of bits)
  scatter_heads  P = 1, 31, 33 (8 threads per point: a partial block), 257 (more than one block); ldg 32 (rows touch), 64, 288
  colsum         cols 1..4 (5 is refused); P = 1, 255, 256, 257 around one block's rows; 65,536 = the last row of the first sweep
                 of 256 x 256 threads, 65,537 = the first row of the second; ld 288 with col0 256; accumulate 0 / 1; the
                 cancellation column 2^25, 1 x 255, -2^25 needs the double accumulator
  tile_sums      n_tiles 1, 3 (row phases without work), 63, 64 (one tile per slice), 65 (two per slice: slices 33.. are empty
                 and must contribute 0 -- the scratch is NaN beforehand), 257 (five per slice: all four row phases and a second
                 turn of phase 0); N 32 (half a column group), 64, 96, 288; n_bias N, N - 30, 3 and 0 (= N)
  reduce_place   splits 1, 3 (tail only), 4, 8 (no tail), 5, 9 (both), 256; dst_ld 283 / dc0 256 and dst_ld 319 / dc0 63; pr0,
                 pc0 non-zero, p_ld > cols; 258 x 63 = several blocks; scale 2^-7; accumulate 0 / 1
  panel_wsums    P 32 (one slice), 96, 160, 4,096 (one point group per slice), 32,800 (1,025 groups: two per slice, the last group
                 alone, slices 513..1,023 empty and written as zeros); NW = 1 reads column 3 at stride 4
"""
import numpy as np
import pytest

from tests import hooks
from tests import train_reduce_gpu as dv
from tests import train_reduce_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    return dv.load()


def test_place_copies_bits(hk):
    for c in rr.place_cases():
        got = dv.run_place(hk, c)
        dv.assert_bits(got, rr.place(c), c.name)
        assert (rr.bits(got) == rr.NEG_ZERO_BITS).any() and (c.rows * c.cols == 1 or (rr.bits(got) == rr.NAN_BITS).any()), c.name


def test_scatter_heads_copies_bits(hk):
    for c in rr.scatter_cases():
        drgb, gsig = dv.run_scatter_heads(hk, c)
        want = rr.scatter_heads(c)
        dv.assert_bits(drgb, want[0], c.name + " drgb")
        dv.assert_bits(gsig, want[1], c.name + " gsig")
        if c.ldg > 32:       # columns 32 .. ldg of every gsig row keep what they held
            dv.assert_bits(gsig.reshape(c.P, c.ldg)[:, 32:], c.gsig0.reshape(c.P, c.ldg)[:, 32:], c.name + " gsig columns 32..")
        assert (rr.bits(drgb) == rr.NEG_ZERO_BITS).any() and (rr.bits(gsig) == rr.NAN_BITS).any(), c.name


def test_colsum_exact(hk):
    for c in rr.colsum_cases():
        got = dv.run_colsum(hk, c)
        dv.assert_bits(got, rr.colsum(c), c.name)
        if "cancel" in c.name:
            assert got[0] == (c.dst0[0] if c.accumulate else 0.0) + 255.0


def test_colsum_refuses_five_columns(hk):
    c = rr.colsum_case(257, 32, 0, 4, 1)
    c.cols = 5
    dv.assert_bits(dv.run_colsum(hk, c, expect=hooks.NSR_ERR_INVALID_ARG), c.dst0, c.name + ": a refused call wrote dst")


def test_tile_sums_exact(hk):
    for c in rr.tile_sums_cases():
        got = dv.run_tile_sums(hk, c)
        dv.assert_bits(got, rr.tile_sums(c), c.name)
        nb = c.n_bias or c.N
        dv.assert_bits(got[nb:], c.dst0[nb:], c.name + ": columns n_bias .. N")
        if "cancel" in c.name:
            assert got[0] == (c.dst0[0] if c.accumulate else 0.0) + 255.0


def test_reduce_place_exact(hk):
    for c in rr.reduce_place_cases():
        dv.assert_bits(dv.run_reduce_place(hk, c), rr.reduce_place(c), c.name)


@pytest.mark.parametrize("R,NW", rr.PANEL_KINDS)
def test_panel_wsums_exact(hk, R, NW):
    for P in rr.PANEL_P:
        c = rr.panel_case(R, NW, P)
        slices, got = dv.run_panel_wsums(hk, c)
        want = rr.panel_wsums(c)
        dv.assert_bits(got, want, c.name)
        dv.assert_bits(got.astype(np.float64).sum(0), want.sum(0), c.name + ": the total over the slices")
        if P == 32800:
            assert slices == 1024 and want[:513].any(1).all() and not got[513:].any(), c.name


def test_panel_wsums_refuses_other_instantiations(hk):
    c = rr.panel_case(128, 3, 96)
    for R, NW in ((128, 1), (256, 3), (64, 1), (128, 4)):
        dv.run_panel_wsums(hk, c, R=R, NW=NW, expect=hooks.NSR_ERR_UNSUPPORTED)


@pytest.mark.parametrize("R,NW", rr.PANEL_KINDS)
def test_panel_wsums_real_inputs_within_derived_bound(hk, R, NW):
    """randn values (fp16) and weights (fp32).  Per thread one fused multiply-add per point of its slice -- one rounding each --
    then five shuffle additions: |partial - ref64| <= gamma(n + 5) sum |v w| with u = 2^-24 and n = the points of the slice, no
    factor on top.  Two launches give identical bits (no atomics, a fixed order).
    The largest err / bound is printed (run with -s); the measured figures are in DESIGN.md."""
    P = 32800
    c = rr.panel_case(R, NW, P, real=True)
    slices, got = dv.run_panel_wsums(hk, c)
    _, again = dv.run_panel_wsums(hk, c)
    dv.assert_bits(got, again, c.name + ": second launch")
    ref, mag = rr.panel_wsums(c), rr.panel_wsums_abs(c)
    hs, per = rr.slice_plan(P)
    points = np.clip(P // 32 - per * np.arange(hs), 0, per) * 32
    bound = np.array([rr.gamma(n + 5) if n else 0.0 for n in points])[:, None] * mag
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{c.name}: max err {float(err.max()):.3e}, largest err / bound {worst:.4f}")
    assert (err <= bound).all(), (c.name, worst)
    assert not got[points == 0].any()


def test_wrong_references_are_told_apart(hk):
    dv.check_teeth(hk, ("place", "scatter_heads", "colsum", "tile_sums", "reduce_place", "panel_wsums"))
