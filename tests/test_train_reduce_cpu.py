"""Pins tests/train_reduce_ref.py -- the reference of the gradient reduction and placement kernels -- without a GPU: every
function against an independent formulation (Python loops over exact integers / ``math.fsum``), the column map of the encoding
panels against the encoders' own register maps, the product table of ``chain_weight_grads`` against the nn.Linear shapes, the
exact regime of every input set the GPU tests use, and the teeth of every entry of ``WRONG``."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import train_reduce_ref as rr
from tests.panel_layout import dircol, enc_row, pecol

f32, f64 = np.float32, np.float64


def _fin(d0, terms, scale, acc):
    """float32(dst0 + float32(sum * scale)) from exact rational arithmetic"""
    s = sum((Fraction(float(t)) for t in terms), Fraction(0)) * Fraction(float(scale))
    assert Fraction(float(f32(float(s)))) == s
    tot = (Fraction(float(d0)) if acc else Fraction(0)) + s
    assert Fraction(float(f32(float(tot)))) == tot
    return f32(float(tot))


def test_finish_states_the_two_roundings():
    d0, s = np.array([4.0, 3.0], f32), np.array([2.0 ** 25 + 8.0, 0.5])
    assert rr.finish(d0, s, 0.5, 1).tolist() == [2.0 ** 24 + 8.0, 3.25] and rr.finish(d0, s, 0.5, 0).tolist() == [2.0 ** 24 + 4.0, 0.25]
    d0 = np.array([1.0, 3.0], f32)
    with pytest.raises(AssertionError):
        rr.finish(d0, np.array([2.0 ** 24 + 1.0, 0.0]), 1.0, 0)            # sum * scale is no fp32 number
    with pytest.raises(AssertionError):
        rr.finish(d0, np.array([2.0 ** 24, 0.0]), 1.0, 1)                  # dst0 + sum is none
    assert rr.finish(d0, np.array([2.0 ** 24, 0.0]), 1.0, 1, exact=False).tolist() == [2.0 ** 24, 3.0]


def test_place_and_scatter_against_loops():
    for c in (rr.place_case(3, 16, 0), rr.place_case(3, 16, 1), rr.place_case(1, 1, 1), rr.place_case(5, 3, 0)):
        want = rr.bits(c.dst0).copy()
        src = rr.bits(c.src)
        for i in range(c.rows):
            for j in range(c.cols):
                at = (c.r0 + j) * c.dst_ld + c.c0 + i if c.transpose else (c.r0 + i) * c.dst_ld + c.c0 + j
                want[at] = src[i * c.src_ld + c.col0 + j]
        got = rr.bits(rr.place(c))
        assert np.array_equal(got, want), c.name
        assert (got == rr.NEG_ZERO_BITS).any() and (c.rows * c.cols == 1 or (got == rr.NAN_BITS).any()), c.name
        assert (got != rr.bits(c.dst0)).sum() == c.rows * c.cols            # values 1000.. never equal the source's -99..99
    for c in (rr.scatter_case(1, 32), rr.scatter_case(33, 64), rr.scatter_case(31, 288)):
        drgb, gsig, d4 = rr.bits(c.drgb0).copy(), rr.bits(c.gsig0).copy(), rr.bits(c.d4)
        for p in range(c.P):
            drgb[p * 32:p * 32 + 32] = [d4[4 * p], d4[4 * p + 1], d4[4 * p + 2]] + [0] * 29
            gsig[p * c.ldg:p * c.ldg + 32] = [d4[4 * p + 3]] + [0] * 31
        got = rr.scatter_heads(c)
        assert np.array_equal(rr.bits(got[0]), drgb) and np.array_equal(rr.bits(got[1]), gsig), c.name
        assert (drgb == rr.NEG_ZERO_BITS).any() and (gsig == rr.NAN_BITS).any()


def test_sums_against_exact_rationals():
    for c in (rr.colsum_case(257, 288, 256, 3, 1), rr.colsum_case(1, 32, 0, 4, 0), rr.colsum_case(257, 32, 0, 2, 1, cancel=True)):
        want = c.dst0.copy()
        for k in range(c.cols):
            want[k] = _fin(c.dst0[k], [c.src[r * c.ld + c.col0 + k] for r in range(c.P)], 1.0, c.accumulate)
        assert np.array_equal(rr.bits(rr.colsum(c)), rr.bits(want)), c.name
    c = rr.colsum_case(257, 32, 0, 2, 0, cancel=True)
    assert rr.colsum(c)[0] == 255.0 and math.fsum(c.src.reshape(257, 32)[:, 0].tolist()) == 255.0
    for c in (rr.tile_sums_case(65, 96, 66, 1), rr.tile_sums_case(3, 32, 0, 0), rr.tile_sums_case(257, 96, 66, 1, cancel=True)):
        nb = c.n_bias or c.N
        want = c.dst0.copy()
        for k in range(nb):
            want[k] = _fin(c.dst0[k], c.tiles[:, k].tolist(), 1.0, c.accumulate)
        assert np.array_equal(rr.bits(rr.tile_sums(c)), rr.bits(want)), c.name
    for c in (rr.reduce_place_case(9, 3, 27, 283, 256, 2.0 ** -7, 1), rr.reduce_place_case(4, 2, 256, 319, 63, 1.0, 0)):
        want = c.dst0.copy()
        for i in range(c.rows):
            for j in range(c.cols):
                terms = [c.partial[z * c.stride + (c.pr0 + i) * c.p_ld + c.pc0 + j] for z in range(c.splits)]
                want[i * c.dst_ld + c.dc0 + j] = _fin(c.dst0[i * c.dst_ld + c.dc0 + j], terms, c.scale, c.accumulate)
        assert np.array_equal(rr.bits(rr.reduce_place(c)), rr.bits(want)), c.name


def test_tile_slices_plan():
    for n in (1, 3, 63, 64, 65, 257):
        s = rr.tile_slices(n)
        assert len(s) == 64 and s[0][0] == 0 and all(a[1] == b[0] or b[0] == b[1] == n for a, b in zip(s, s[1:]))
        assert sorted(t for lo, hi in s for t in range(lo, hi)) == list(range(n))
    assert rr.tile_slices(65)[32] == (64, 65) and rr.tile_slices(65)[33] == (65, 65)       # per = 2: slices 33.. are empty
    assert rr.tile_slices(64)[63] == (63, 64)


def test_slice_plan_and_panel_wsums_against_integers():
    assert [rr.slice_plan(P) for P in (0, 32, 96, 160, 4096, 32768, 32800)] == \
        [(1, 0), (1, 1), (3, 1), (5, 1), (128, 1), (1024, 1), (1024, 2)]
    for (R, NW), P in ((k, P) for k in rr.PANEL_KINDS for P in (96, 160)):
        c = rr.panel_case(R, NW, P)
        hs, per = rr.slice_plan(P)
        m, w = c.mat.astype(np.int64), c.w.astype(np.int64)
        assert np.array_equal(m.astype(np.float16), c.mat)
        want = np.zeros((hs, NW * R), np.int64)
        for p in range(P):
            for k in range(NW):
                want[p // 32 // per, k * R:(k + 1) * R] += w[p, k] * m[p]
        assert np.array_equal(rr.panel_wsums(c), want.astype(f64)), c.name
    c = rr.panel_case(128, 3, 32800)                     # 1,025 groups: slices of two, the last point group alone in slice 512
    got = rr.panel_wsums(c)
    assert got.shape == (1024, 384) and got[:513].any(1).all() and not got[513:].any()
    assert np.array_equal(got[512, :128], c.w[32768:, 0].astype(f64) @ c.mat[32768:].astype(f64))


def test_panel_matrix_is_one_to_one_within_a_group():
    for R in (128, 256):
        m = rr.panel_matrix(64, R)
        assert float(np.abs(m).max()) <= 2046 and np.array_equal(m, np.round(m))
        assert len(np.unique(m[:32])) == min(32 * R, 4093) and not np.array_equal(m[:32], m[32:])


def test_enc_panel_row_is_the_inverse_of_the_encoders_register_maps():
    for enc, cols, n_regs, col_of in ((1, 63, 32, pecol), (2, 27, 16, dircol)):
        written = {enc_row(t, h): col_of(t, h) for t in range(n_regs) for h in (0, 1) if col_of(t, h) is not None}
        assert sorted(written.values()) == list(range(cols))              # the encoders write every column once
        rows = [rr.enc_panel_row(enc, j) for j in range(cols)]
        assert len(set(rows)) == cols and set(rows) == set(written)       # injective, onto the rows the encoders write
        assert all(written[r] == j for j, r in enumerate(rows))
    assert [rr.enc_panel_row(0, j) for j in range(256)] == list(range(256))


def test_finish_job_against_exact_rationals():
    for q in (rr.finish_case(0, 3, 63, 21, 1, 1), rr.finish_case(0, 2, 27, 9, 0, 2), rr.finish_case(0, 2, 256, 7, 1, 0),
              rr.finish_case(1, 128, 1, 9, 1), rr.finish_case(1, 5, 1, 70, 0, scale=2.0 ** -3), rr.finish_case(2, 1, 1, 65, 1),
              rr.finish_case(2, 4, 1, 63, 0)):
        p = q.partial[q.p_off:]
        want = q.dst0.copy()
        if q.kind == 0:
            inv = {pecol(t, h): enc_row(t, h) for t in range(32) for h in (0, 1)} if q.enc_rows == 1 else \
                  {dircol(t, h): enc_row(t, h) for t in range(16) for h in (0, 1)} if q.enc_rows == 2 else {j: j for j in range(256)}
            for i in range(q.rows):
                for j in range(q.cols):
                    at = i * q.dst_ld + q.dc0 + j
                    want[at] = _fin(q.dst0[at], [p[z * q.stride + i * q.p_ld + inv[j]] for z in range(q.splits)], q.scale, q.accumulate)
        else:
            for i in range(q.rows):
                step = q.rows if q.kind == 1 else q.stride
                want[i] = _fin(q.dst0[i], [p[z * step + i] for z in range(q.splits)], q.scale if q.kind == 1 else 1.0, q.accumulate)
        assert np.array_equal(rr.bits(rr.finish_ref(q)), rr.bits(want)), q.name
        assert not np.isnan(want).any()


def test_product_table_covers_every_element_once():
    count = [np.zeros(int(np.prod(s)), np.int64) for s in rr.TENSOR_SHAPES]
    assert len(rr.PRODUCTS) == 12 and len(rr.TENSOR_SHAPES) == 24
    per_tensor = {}
    for q in rr.PRODUCTS:
        shape = rr.TENSOR_SHAPES[q.tensor]
        assert (q.rows, q.dst_ld) == shape and q.dc0 + q.cols <= q.dst_ld
        assert rr.PANEL_ROWS[q.a] == q.rows and q.a <= 9 and rr.PANEL_ROWS[q.b] == (q.cols if q.enc == 0 else 64)
        i, j = np.ogrid[:q.rows, :q.cols]
        count[q.tensor][i * q.dst_ld + q.dc0 + j] += 1
        per_tensor[q.tensor] = per_tensor.get(q.tensor, 0) + 1
        if q.bias is not None:
            assert rr.TENSOR_SHAPES[q.bias] == (q.rows,)
            count[q.bias] += 1
    for t in (20, 21, 22, 23):                          # the two heads: a stream over a panel, the per-ray sums
        count[t] += 1
    assert all((k == 1).all() for k in count)
    assert {t for t, n in per_tensor.items() if n == 2} == {0 * 2 + 8, 18} and per_tensor[0] == 1
    # launch order = the tile shapes tests/hooks.py::STEP_JOBS lists
    assert [(q.rows, q.cols if q.enc == 0 else 64) for q in rr.PRODUCTS] == \
        [(128, 256), (128, 64)] + [(256, 256)] * 5 + [(256, 64)] + [(256, 256)] * 3 + [(256, 64)]


def test_chain_weight_grads_against_the_linear_layers():
    """independent formulation: un-permute the encoding panels with the encoders' own maps, build every nn.Linear input, take
    (gradient)^T (input) in exact integers (quanta of 2^-3)"""
    c = rr.chain_case(160, 5, 1)
    rr.assert_chain_exact(c)
    q8 = [np.round(a * 8).astype(np.int64) for a in c.A]
    assert all(np.array_equal(q / 8.0, a) for q, a in zip(q8, c.A))
    B = [b.astype(np.int64) for b in c.B]
    pe, de = np.zeros((c.P, 63), np.int64), np.zeros((c.P, 27), np.int64)
    for t in range(32):
        for h in (0, 1):
            if pecol(t, h) is not None:
                pe[:, pecol(t, h)] = B[10][:, enc_row(t, h)]
            if t < 16 and dircol(t, h) is not None:
                de[:, dircol(t, h)] = B[11][:, enc_row(t, h)]
    inputs = [pe] + [B[L - 2] for L in range(2, 5)] + [np.concatenate([pe, B[3]], 1)] + [B[L - 2] for L in range(6, 9)]
    want = [None] * 24
    for L in range(1, 9):
        want[2 * (L - 1)], want[2 * (L - 1) + 1] = q8[L - 1].T @ inputs[L - 1], q8[L - 1].sum(0)
    want[16], want[17] = q8[8].T @ B[7], q8[8].sum(0)
    want[18], want[19] = q8[9].T @ np.concatenate([B[8], de], 1), q8[9].sum(0)
    d4, bp = c.d4.astype(np.int64) * 8, c.bias_part.astype(np.int64) * 8
    want[20], want[21] = d4[:, 3:].T @ B[7], bp[:, 3:].sum(0)
    want[22], want[23] = d4[:, :3].T @ B[9], bp[:, :3].sum(0)
    got = rr.chain_weight_grads(c)
    for t in range(24):
        assert want[t].shape == rr.TENSOR_SHAPES[t]
        w = (c.g0[t].astype(f64) * 8 + want[t].reshape(-1)) / 8.0
        assert np.array_equal(got[t].astype(f64), w), t
    c.acc = 0
    got = rr.chain_weight_grads(c)
    assert all(np.array_equal(got[t].astype(f64), want[t].reshape(-1) / 8.0) for t in range(24))


def test_every_input_set_is_in_the_exact_regime():
    """every right reference asserts `finish`'s two roundings round nothing; the fp32 partial sums of panel_wsums and of the
    fp16 products stay below 2^24 quanta"""
    for c in rr.colsum_cases():
        rr.colsum(c)
        assert np.isnan(c.src).sum() == c.P * (c.ld - c.cols)
    for c in rr.tile_sums_cases():
        rr.tile_sums(c)
    for c in rr.reduce_place_cases():
        rr.reduce_place(c)
    for c in rr.panel_cases():
        assert float(rr.panel_wsums_abs(c).max()) < 2.0 ** 24, c.name
        assert float(np.abs(rr.panel_wsums(c)).sum(0).max()) < 2.0 ** 24, c.name     # the head's finish job carries the total
    for q in rr.finish_cases() + rr.mixed_jobs(33):
        assert not np.isnan(rr.finish_ref(q)).any(), q.name
    for (P, n_rays) in rr.CHAIN_SHAPES:
        first = rr.chain_case(P, n_rays, 0)
        rr.assert_chain_exact(first)
        second = rr.chain_case(P, n_rays, 1, g0=rr.chain_weight_grads(first), seed=1)
        rr.assert_chain_exact(second)
        rr.chain_weight_grads(second)


def test_case_lists_reach_every_branch():
    assert {c.P for c in rr.colsum_cases()} >= {1, 255, 256, 257, 65536, 65537} and {c.cols for c in rr.colsum_cases()} == {1, 2, 3, 4}
    assert {c.n_tiles for c in rr.tile_sums_cases()} == {1, 3, 63, 64, 65, 257}
    assert {c.splits for c in rr.reduce_place_cases()} == {1, 3, 4, 5, 8, 9, 256}
    fin = rr.finish_cases()
    assert {(q.enc_rows, q.cols) for q in fin if q.kind == 0 and q.rows == 3} == {(0, 256), (1, 63), (2, 27)}
    assert {q.splits for q in fin if q.kind == 0 and q.rows == 3} == {1, 7, 8, 9, 21}
    assert {(q.rows, q.splits) for q in fin if q.kind == 1 and q.splits > 64} == {(r, s) for r in (1, 384, 1025) for s in (65, 1024)}
    assert {(q.rows, q.splits) for q in fin if q.kind == 2} == {(r, s) for r in (1, 2, 3, 4) for s in (1, 63, 64, 65, 5000)}
    assert all({q.accumulate for q in fin if q.kind == k} == {0, 1} for k in (0, 1, 2))
    mixed = rr.mixed_jobs()
    assert len(mixed) == 32 and {q.kind for q in mixed} == {0, 1, 2}


@pytest.mark.parametrize("entry", rr.WRONG, ids=[f"{k}: {what} ({case})" for k, what, case, _ in rr.WRONG])
def test_every_wrong_reference_differs(entry):
    kernel, what, case, wrong = entry
    c = rr.TEETH_CASES[case]()
    assert rr.differs(rr.RIGHT[kernel](c), wrong(c)), f"{kernel}: '{what}' gives the right result on '{case}'"


def test_wrong_list_holds_the_variants_the_kernels_can_fall_into():
    have = {(k, what) for k, what, _, _ in rr.WRONG}
    assert have >= {("panel_wsums", "point index without the swizzle"), ("panel_wsums", "4 h and 8 (e >> 2) row terms exchanged"),
                    ("panel_wsums", "last slice dropped"), ("tile_sums", "last slice dropped"),
                    ("finish_jobs", "identity instead of enc_panel_row"), ("finish_jobs", "splits % 8 tail dropped"),
                    ("reduce_place", "splits % 4 tail dropped"), ("colsum", "fp32 accumulation"), ("tile_sums", "fp32 accumulation"),
                    ("colsum", "rows from 65,536 on dropped"), ("tile_sums", "row phase 3 dropped"), ("tile_sums", "n_bias taken as N")}
    assert all(any(k == kernel and what == "accumulate ignored" for k, what, _, _ in rr.WRONG)
               for kernel in ("colsum", "tile_sums", "reduce_place", "finish_jobs"))
    assert {k for k, _, _, _ in rr.WRONG} == set(rr.RIGHT)
