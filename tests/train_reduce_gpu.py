"""Device side of the unit layer over the gradient reduction and placement kernels: uploads a case of
tests/train_reduce_ref.py, launches ONE launcher through the test-hook library (tests/csrc/nsr_test_hooks_reduce.hip) and
returns what it wrote.  Shared by tests/test_gpu_train_reduce_units.py, test_gpu_train_finish_jobs.py and
test_gpu_chain_weight_grads.py.

House rules (tests/test_gpu_train_heads.py): every buffer a launcher writes -- outputs and scratch -- has GUARD NaN elements
behind it that must survive; outputs start from the case's ``dst0`` (distinct integers), so the comparison of the WHOLE buffer
with the reference's also proves that cells outside the written region kept their bits; a refused call leaves every bit."""
import ctypes

import numpy as np
import torch

from tests import hooks
from tests import train_reduce_ref as rr

GUARD = 1024                     # elements behind every written buffer
f32 = np.float32


def load():
    if not torch.cuda.is_available():
        import pytest
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return hooks.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def up(a):
    """flat fp32 host array -> device buffer with the guard behind it"""
    a = np.ascontiguousarray(a, dtype=f32).reshape(-1)
    return dev(np.concatenate([a, np.full(GUARD, np.nan, f32)]))


def nan_buf(n):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")


def down(t, what=""):
    """the buffer without its guard, which must still be NaN"""
    a = t.cpu().numpy()
    assert np.isnan(a[-GUARD:]).all(), f"{what}: floats behind the buffer were written"
    return a[:-GUARD].copy()


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == f32 and want.dtype == f32:
        same = rr.bits(got) == rr.bits(want)
    else:
        same = got.astype(np.float64) == want.astype(np.float64)
    if not same.all():
        bad = np.flatnonzero(~same.reshape(-1))
        i = bad[0]
        raise AssertionError(f"{what}: {bad.size} of {same.size} elements differ, first at {i} (last at {bad[-1]}): got "
                             f"{got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def sync(rc, expect=hooks.NSR_OK):
    torch.cuda.synchronize()
    assert rc == expect, f"return code {rc}, expected {expect}"


# ---- nsr_train_gemm.hip ---------------------------------------------------------------------------------------------------
def run_place(hk, c):
    dst, src = up(c.dst0), dev(c.src)
    sync(hk.nsr_test_place(hooks.ptr(dst), c.dst_ld, c.r0, c.c0, hooks.ptr(src), c.src_ld, c.rows, c.cols, c.col0, c.transpose,
                           hooks.stream()))
    return down(dst, c.name)


def run_scatter_heads(hk, c):
    drgb, gsig, d4 = up(c.drgb0), up(c.gsig0), dev(c.d4)
    sync(hk.nsr_test_scatter_heads(hooks.ptr(d4), c.P, hooks.ptr(drgb), hooks.ptr(gsig), c.ldg, hooks.stream()))
    return down(drgb, c.name), down(gsig, c.name)


def run_colsum(hk, c, expect=hooks.NSR_OK):
    dst, src, scratch = up(c.dst0), dev(c.src), nan_buf(256 * 4 * 2)       # kSumBlocks x 4 doubles
    sync(hk.nsr_test_colsum(hooks.ptr(src), c.ld, c.P, c.col0, c.cols, hooks.ptr(dst), c.accumulate, hooks.ptr(scratch),
                            hooks.stream()), expect)
    s = down(scratch, c.name + " scratch")
    if expect != hooks.NSR_OK:
        assert np.isnan(s).all(), c.name + ": a refused call wrote its scratch"
    return down(dst, c.name)


def run_tile_sums(hk, c):
    # the tile sums, then the launcher's scratch of 64 x N doubles: NaN, so a slice nobody writes poisons the sum
    buf = up(np.concatenate([c.tiles.reshape(-1), np.full(64 * c.N * 2, np.nan, f32)]))
    dst = up(c.dst0)
    sync(hk.nsr_test_tile_sums(hooks.ptr(buf), c.n_tiles, c.N, c.n_bias, hooks.ptr(dst), c.accumulate, hooks.stream()))
    tiles = down(buf, c.name + " col_tiles")[:c.tiles.size]
    assert_bits(tiles, c.tiles.reshape(-1), c.name + ": the tile sums themselves")
    return down(dst, c.name)


def run_reduce_place(hk, c):
    dst, part = up(c.dst0), dev(c.partial)
    sync(hk.nsr_test_reduce_place(hooks.ptr(dst), c.dst_ld, c.dc0, c.rows, c.cols, hooks.ptr(part), c.splits, c.p_ld, c.pr0, c.pc0,
                                  c.accumulate, c.scale, c.stride, hooks.stream()))
    return down(dst, c.name)


# ---- nsr_train_wgrad.hip --------------------------------------------------------------------------------------------------
def pack_into(hk, buf, byte_off, mat16, rows):
    """(P, rows) fp16 -> the panel at byte_off of the int16 device buffer `buf`, groups 64 * rows bytes apart"""
    src = dev(np.ascontiguousarray(mat16, dtype=np.float16).view(np.int16))
    rc = hk.nsr_test_pack_panel(hooks.ptr(src), rows, mat16.shape[0], rows, buf.data_ptr() + byte_off, 64 * rows, hooks.stream())
    sync(rc)


def run_panel_wsums(hk, c, R=None, NW=None, expect=hooks.NSR_OK):
    """-> (slices, partial (slices, NW * R) fp32); every slice must have been written"""
    panel = torch.full((c.P // 32 * 32 * c.R + 64,), 0x7e00, dtype=torch.int16, device="cuda")       # fp16 NaN behind the panel
    pack_into(hk, panel, 0, c.mat, c.R)
    w4 = dev(c.w4)
    hs, _ = rr.slice_plan(c.P)
    part = nan_buf(hs * c.NW * c.R)
    slices = ctypes.c_int(-1)
    rc = hk.nsr_test_panel_wsums(c.R if R is None else R, c.NW if NW is None else NW, hooks.ptr(panel), c.P, hooks.ptr(w4, c.w_col), 4,
                                 hooks.ptr(part), ctypes.byref(slices), hooks.stream())
    sync(rc, expect)
    out = down(part, c.name)
    if expect != hooks.NSR_OK:
        assert np.isnan(out).all() and slices.value == -1, c.name + ": a refused call wrote"
        return None, None
    assert slices.value == hs, (c.name, slices.value, hs)
    assert not np.isnan(out).any(), c.name + ": a slice of the partial was not written"
    return slices.value, out.reshape(hs, c.NW * c.R)


def run_finish_jobs(hk, qs, expect=hooks.NSR_OK, n=None):
    """ONE launch of the jobs `qs` (tests/train_reduce_ref.py finish_case), each on buffers of its own -> their dst arrays"""
    jobs = (hooks.FinishJob * max(len(qs), 1))()
    keep = []
    for j, q in zip(jobs, qs):
        dst, part = up(q.dst0), dev(q.partial)
        keep.append((dst, part))
        j.dst, j.partial, j.stride = hooks.ptr(dst), hooks.ptr(part, q.p_off), q.stride
        j.kind, j.dst_ld, j.dc0, j.rows, j.cols, j.splits, j.p_ld = q.kind, q.dst_ld, q.dc0, q.rows, q.cols, q.splits, q.p_ld
        j.accumulate, j.enc_rows, j.scale = q.accumulate, q.enc_rows, q.scale
    sync(hk.nsr_test_finish_jobs(jobs, len(qs) if n is None else n, hooks.stream()), expect)
    out = [down(dst, q.name) for (dst, _), q in zip(keep, qs)]
    if expect != hooks.NSR_OK:
        for got, q in zip(out, qs):
            assert_bits(got, q.dst0, q.name + ": a refused call wrote")
    return out


ROWS_BEFORE = [256 * p for p in range(10)] + [2304 + 128, 2304 + 192, 2304 + 256]       # csrc/nsr_panels.h


def run_chain_weight_grads(hk, c):
    """-> the 24 tensors.  Both panel sets are laid out as the product carves them: n_groups = the point groups of P rounded up
    to 128 points, panel p at ROWS_BEFORE[p] * 64 * n_groups bytes, the padding groups zero; the two encoding slots of the
    gradient set, which no product reads, hold fp16 NaN"""
    P = c.P
    n_groups = -(-P // 128) * 4
    halves = ROWS_BEFORE[12] * 32 * n_groups
    zpan = torch.zeros(halves + 64, dtype=torch.int16, device="cuda")
    dpan = torch.zeros(halves + 64, dtype=torch.int16, device="cuda")
    dpan[ROWS_BEFORE[10] * 32 * n_groups:] = 0x7e00
    zpan[halves:] = 0x7e00
    for p in range(12):
        pack_into(hk, zpan, ROWS_BEFORE[p] * 64 * n_groups, c.B[p], rr.PANEL_ROWS[p])
    for p in range(10):
        pack_into(hk, dpan, ROWS_BEFORE[p] * 64 * n_groups, c.stored[p], rr.PANEL_ROWS[p])
    pscale = np.ones((10, n_groups * 32), f32)
    for p in range(10):
        pscale[p, :P] = c.ps[p]
    gmax = np.zeros(16, f32)
    gmax[:10] = c.amax
    sizes = (ctypes.c_int64 * 2)()
    assert hk.nsr_test_chain_weight_grads_scratch(P, sizes) == hooks.NSR_OK
    slots, row_part = nan_buf(int(sizes[0])), nan_buf(int(sizes[1]))
    g = [up(t) for t in c.g0]
    gp = (ctypes.c_void_p * 24)(*[hooks.ptr(t) for t in g])
    ins = [dev(gmax.view(np.int32)), dev(pscale), dev(c.d4), dev(c.bias_part)]
    rc = hk.nsr_test_chain_weight_grads(hooks.ptr(dpan), hooks.ptr(zpan), hooks.ptr(ins[0]), hooks.ptr(ins[1]), hooks.ptr(ins[2]),
                                        hooks.ptr(ins[3]), hooks.ptr(slots), hooks.ptr(row_part), P, c.n_rays, gp, c.acc,
                                        hooks.stream())
    sync(rc)
    down(slots, c.name + " slots")
    down(row_part, c.name + " row_part")
    return [down(t, f"{c.name} tensor {i}") for i, t in enumerate(g)]


RUN = {"place": run_place, "scatter_heads": run_scatter_heads, "colsum": run_colsum, "tile_sums": run_tile_sums,
       "reduce_place": run_reduce_place, "panel_wsums": lambda hk, c: run_panel_wsums(hk, c)[1],
       "finish_jobs": lambda hk, q: run_finish_jobs(hk, [q])[0], "chain_weight_grads": run_chain_weight_grads}


def check_teeth(hk, kernels):
    """ONE device output per teeth case of the given kernels: it equals the right reference and differs from every WRONG one"""
    outputs = {}
    n = 0
    for kernel, what, case, wrong in rr.WRONG:
        if kernel not in kernels:
            continue
        if case not in outputs:
            c = rr.TEETH_CASES[case]()
            outputs[case] = (c, RUN[kernel](hk, c))
            right = rr.RIGHT[kernel](c)
            got = outputs[case][1]
            for g, r in zip(got, right) if isinstance(right, (tuple, list)) else ((got, right),):
                assert_bits(g, r, f"{kernel} on '{case}'")
        c, got = outputs[case]
        assert rr.differs(got, wrong(c)), f"{kernel}: the device output on '{case}' also equals the reference with '{what}'"
        n += 1
    assert n >= len(kernels)
    return n
