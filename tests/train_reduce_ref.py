"""Reference of the gradient reduction and placement kernels of the training step, in plain numpy (fp64 / exact integers), and
the inputs their unit tests run on.

The kernels (csrc/nsr_train_gemm.hip: place, scatter_heads, colsum, tile_sums, reduce_place; csrc/nsr_train_wgrad.hip:
panel_wsums, finish_jobs, chain_weight_grads) sum in double and store ``float32(dst0 + float32(sum * scale))`` -- ``0 +``
without accumulate.  ``finish`` below is that statement; every function here is "gather the terms, sum them in fp64, finish".

Exact regime.  All exact-input cases hold small integers (times powers of two).  Where fp32 carries a value -- the operands, a
partial sum of ``panel_wsums`` or of the fp16 products, ``sum * scale``, ``dst0 + sum`` -- it is an integer number of quanta
below 2^24, so no rounding happens anywhere, the order of a sum is immaterial and the device must agree BIT FOR BIT.  ``finish``
asserts its part of that condition on every call (``exact=True``); ``assert_exact_products`` is the condition of the products
(the same as ``_assert_exact_regime`` of tests/test_gpu_gemm_units.py).  One deliberate exception: the cancellation column
``2^25, 1 x k, -2^25``.  Its terms are fp32 numbers and its exact sum k is one, but the partial sums are not: a double
accumulator returns k, an fp32 accumulator does not.

A case is a ``SimpleNamespace`` of the launcher's arguments and host arrays; the GPU tests upload it, the functions here take it.
``WRONG`` lists deliberately wrong variants of the references, each with the case on which it must differ from the right one
(tests/test_train_reduce_cpu.py) and from the device (the GPU tests' teeth).
"""
import itertools
from types import SimpleNamespace as C

import numpy as np

from tests.panel_layout import enc_row

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                   # fp32 unit roundoff
NAN_BITS = 0x7FC12345            # a quiet NaN with a payload
NEG_ZERO_BITS = 0x80000000
MAX_FINISH_JOBS = 32


def gamma(n):
    return n * U / (1.0 - n * U)


def finish(dst0, s64, scale=1.0, accumulate=0, exact=True):
    """float32(dst0 + float32(sum * scale)), elementwise; exact: both roundings are asserted to round nothing"""
    s64 = np.asarray(s64, f64)
    add64 = s64 * f64(scale)
    add = add64.astype(f32)
    base = np.asarray(dst0, f32) if accumulate else np.zeros(add.shape, f32)
    out = base + add                                  # one fp32 addition
    assert out.dtype == f32
    if exact:
        assert np.array_equal(add.astype(f64), add64), "left the exact regime: sum * scale is not an fp32 number"
        assert np.array_equal(out.astype(f64), base.astype(f64) + add64), "left the exact regime: dst0 + sum * scale"
    return out


def assert_exact_products(a_abs, b_abs, quantum=1.0, what=""):
    """max_ij sum_p |a_pi| |b_pj| < 2^24 quanta: every partial sum of a^T b, in any order, is exact in fp32"""
    worst = float((np.asarray(a_abs, f64).T @ np.asarray(b_abs, f64)).max()) / quantum
    assert worst < 2.0 ** 24, f"{what}: left the exact regime (max sum |a||b| = {worst:.3g} quanta)"


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _ints(rng, shape, lo=-4, hi=4):
    return rng.randint(lo, hi + 1, size=shape).astype(f32)


def _special(rng, a):
    """plants -0.0 and a NaN with a payload into a float32 array (a copy of bits must keep both)"""
    a = np.ascontiguousarray(a, dtype=f32)
    flat = a.reshape(-1).view(np.uint32)
    flat[rng.randint(0, flat.size)] = NEG_ZERO_BITS
    if flat.size > 1:
        flat[rng.randint(0, flat.size)] = NAN_BITS
        flat[0], flat[-1] = NEG_ZERO_BITS, NAN_BITS
    return a


# ------------------------------------------------------------------------------------------------------------------------
# nsr_train_gemm.hip
# ------------------------------------------------------------------------------------------------------------------------
def place(c, transpose=None, col0=None):
    """dst[(r0 + i) * dst_ld + c0 + j] = src[i * src_ld + col0 + j] (transpose: dst[(r0 + j) * dst_ld + c0 + i]): bits"""
    transpose = c.transpose if transpose is None else transpose
    col0 = c.col0 if col0 is None else col0
    out = bits(c.dst0).copy()
    i, j = np.ogrid[:c.rows, :c.cols]
    v = bits(c.src)[i * c.src_ld + col0 + j]
    if transpose:
        out[(c.r0 + j) * c.dst_ld + c.c0 + i] = v
    else:
        out[(c.r0 + i) * c.dst_ld + c.c0 + j] = v
    return out.view(f32)


def scatter_heads(c, sigma_col=None):
    """drgb row p = [d4[p][0..2] | 29 zeros], gsig[p * ldg .. + 32) = [d4[p][3] | 31 zeros]: bits; -> (drgb, gsig)"""
    drgb, gsig = bits(c.drgb0).copy(), bits(c.gsig0).copy()
    d4 = bits(c.d4).reshape(c.P, 4)
    p = np.arange(c.P)[:, None]
    k = np.arange(32)[None, :]
    drgb[p * 32 + k] = 0
    gsig[p * c.ldg + k] = 0
    drgb[p * 32 + np.arange(3)[None, :]] = d4[:, :3]
    if sigma_col is None:
        gsig[p[:, 0] * c.ldg] = d4[:, 3]
    else:                                             # wrong: d sigma left where d4 has it
        drgb[p[:, 0] * 32 + sigma_col] = d4[:, 3]
    return drgb.view(f32), gsig.view(f32)


def colsum(c, rows=None, fp32=False, accumulate=None, exact=True):
    """dst[k] (+)= sum over the P rows of src[r * ld + col0 + k], k < cols"""
    r = np.arange(c.P if rows is None else rows)[:, None]
    vals = c.src[r * c.ld + c.col0 + np.arange(c.cols)[None, :]]
    s = np.add.accumulate(vals, axis=0, dtype=f32)[-1] if fp32 else vals.astype(f64).sum(0)
    out = c.dst0.copy()
    out[:c.cols] = finish(c.dst0[:c.cols], s, 1.0, c.accumulate if accumulate is None else accumulate, exact and not fp32)
    return out


def tile_slices(n_tiles, slices=64):
    """the row tiles [lo, hi) of each of the 64 slices of tilesum_partial_kernel (later slices may be empty)"""
    per = -(-n_tiles // slices)
    return [(min(per * z, n_tiles), min(per * z + per, n_tiles)) for z in range(slices)]


def tile_sums(c, fp32=False, accumulate=None, n_bias=None, keep=None, exact=True):
    """dst[k] (+)= sum over the n_tiles rows of tiles[t][k], k < n_bias (0: N); keep: a mask of the tiles that count"""
    nb = c.n_bias if n_bias is None else n_bias
    nb = nb if nb > 0 else c.N
    t = c.tiles[:, :nb] if keep is None else c.tiles[keep, :nb]
    s = np.add.accumulate(t, axis=0, dtype=f32)[-1] if fp32 else t.astype(f64).sum(0)
    out = c.dst0.copy()
    out[:nb] = finish(c.dst0[:nb], s, 1.0, c.accumulate if accumulate is None else accumulate, exact and not fp32 and keep is None)
    return out


def reduce_place(c, splits=None, accumulate=None, scale=None, pc0=None, exact=True):
    """dst[i * dst_ld + dc0 + j] (+)= scale * sum_z partial[z * stride + (pr0 + i) * p_ld + pc0 + j]"""
    splits = c.splits if splits is None else splits
    i, j = np.ogrid[:c.rows, :c.cols]
    src = (c.pr0 + i) * c.p_ld + (c.pc0 if pc0 is None else pc0) + j
    s = c.partial[np.arange(splits)[:, None, None] * c.stride + src[None]].astype(f64).sum(0)
    d = i * c.dst_ld + c.dc0 + j
    out = c.dst0.copy()
    out[d] = finish(c.dst0[d], s, c.scale if scale is None else scale, c.accumulate if accumulate is None else accumulate, exact)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# nsr_train_wgrad.hip
# ------------------------------------------------------------------------------------------------------------------------
def slice_plan(P):
    """(slices, point groups per slice) of panel_wsums: up to 1,024 slices; from P / 32 = 1,025 on, later slices are empty"""
    n_pg = P // 32
    hs = min(max(n_pg, 1), 1024)
    return hs, -(-n_pg // hs)


def panel_wsums(c, w_point=None, row_of=None, drop_last=False):
    """partial[z][k * R + row] = sum over the points p of slice z of w[p][k] * mat[p][row], fp64 (slices, NW * R).
    w_point / row_of: the wrong variants' maps (point, row) -> point whose weight is used, row -> row it is stored at"""
    hs, per = slice_plan(c.P)
    n = (c.P // 32) * 32
    span = per * 32
    W = np.zeros((hs * span, c.NW), f64)
    V = np.zeros((hs * span, c.R), f64)
    V[:n] = c.mat[:n].astype(f64)
    w = c.w[:n].astype(f64)
    if w_point is None:
        W[:n] = w
        out = np.einsum("zpk,zpr->zkr", W.reshape(hs, span, c.NW), V.reshape(hs, span, c.R))
    else:                                             # the weight's point depends on the row
        src = w_point(np.arange(n)[:, None], np.arange(c.R)[None, :])        # (n, R)
        out = np.zeros((hs, c.NW, c.R), f64)
        for k in range(c.NW):
            prod = np.zeros((hs * span, c.R), f64)
            prod[:n] = w[src, k] * V[:n]
            out[:, k] = prod.reshape(hs, span, c.R).sum(1)
    if row_of is not None:
        moved = np.zeros_like(out)
        moved[:, :, row_of(np.arange(c.R))] = out
        out = moved
    if drop_last:
        out[(c.P // 32 - 1) // per] = 0.0             # the last slice that holds a point group
    return out.reshape(hs, c.NW * c.R)


def panel_wsums_abs(c):
    """sum over the slice of |w| |v|: the magnitude the fp32 partial sums live under (exact regime, error bound)"""
    a = C(**vars(c))
    a.mat, a.w = np.abs(c.mat.astype(f64)), np.abs(c.w)
    return panel_wsums(a)


def enc_panel_row(enc_rows, j):
    """the panel row of column j of the encoded position (1: 63 columns) / direction (2: 27), csrc/nsr_train_wgrad.hip"""
    if enc_rows == 0:
        return j
    per = 30 if enc_rows == 1 else 12
    if j < 2:
        t, h = j, 0
    elif j == 2:
        t, h = 0, 1
    else:
        t, h = (j - 3) % per + 2, (j - 3) // per
    return enc_row(t, h)


def finish_job(q, dst0, partial, splits=None, accumulate=None, enc_rows=None, exact=True):
    """one job of finish_jobs on its own dst (a copy is returned) and partial (flat)"""
    splits = q.splits if splits is None else splits
    acc = q.accumulate if accumulate is None else accumulate
    z = np.arange(splits)
    out = dst0.copy()
    if q.kind == 0:
        enc = q.enc_rows if enc_rows is None else enc_rows
        col = np.array([enc_panel_row(enc, j) for j in range(q.cols)], dtype=np.int64)
        i, j = np.ogrid[:q.rows, :q.cols]
        s = partial[z[:, None, None] * q.stride + (i * q.p_ld + col[j])[None]].astype(f64).sum(0)
        d = i * q.dst_ld + q.dc0 + j
        out[d] = finish(dst0[d], s, q.scale, acc, exact)
    elif q.kind == 1:
        s = partial[z[:, None] * q.rows + np.arange(q.rows)[None, :]].astype(f64).sum(0)
        out[:q.rows] = finish(dst0[:q.rows], s, q.scale, acc, exact)
    else:                                             # kind 2 takes no scale
        s = partial[z[:, None] * q.stride + np.arange(q.rows)[None, :]].astype(f64).sum(0)
        out[:q.rows] = finish(dst0[:q.rows], s, 1.0, acc, exact)
    return out


# the 24 tensors of the default network (state_dict order): layer i (1..8) weight 2 (i - 1), bias 2 (i - 1) + 1, then
# xyz_encoding_final 16 / 17, dir_encoding 18 / 19, sigma 20 / 21, rgb 22 / 23
TENSOR_SHAPES = [s for L in range(1, 9) for s in ((256, 63 if L == 1 else (319 if L == 5 else 256)), (256,))] + \
                [(256, 256), (256,), (128, 283), (128,), (1, 256), (1,), (3, 128), (3,)]
PANEL_ROWS = [256] * 9 + [128, 64, 64]              # forward panels 0..11; the gradient panels are 0..9
# The twelve products of chain_weight_grads, in launch order: tensor[:, dc0 : dc0 + cols] = (gradient panel a)^T (forward panel
# b)[:, enc_panel_row(enc, .)]; `bias`: the tensor that gets the row sums of gradient panel a (None: none)
PRODUCTS = [C(a=9, b=8, tensor=18, dst_ld=283, dc0=0, rows=128, cols=256, enc=0, bias=19),
            C(a=9, b=11, tensor=18, dst_ld=283, dc0=256, rows=128, cols=27, enc=2, bias=None),
            C(a=8, b=7, tensor=16, dst_ld=256, dc0=0, rows=256, cols=256, enc=0, bias=17)]
for _L in range(8, 0, -1):
    if _L > 1:
        PRODUCTS.append(C(a=_L - 1, b=_L - 2, tensor=2 * (_L - 1), dst_ld=319 if _L == 5 else 256, dc0=63 if _L == 5 else 0,
                          rows=256, cols=256, enc=0, bias=2 * (_L - 1) + 1))
    if _L in (1, 5):
        PRODUCTS.append(C(a=_L - 1, b=10, tensor=2 * (_L - 1), dst_ld=63 if _L == 1 else 319, dc0=0, rows=256, cols=63, enc=1,
                          bias=1 if _L == 1 else None))


def chain_weight_grads(c, products=None, enc_identity=False):
    """the 24 gradient tensors (flat fp32) from the true gradients A[0..9] (P, rows) = stored integers x pscale, the forward
    panels B[0..11] (P, rows), d4 (P, 4) and bias_part (n_rays, 4); c.g0 / c.acc: what the tensors held"""
    out = [g.copy() for g in c.g0]

    def put(t, idx, s):
        out[t][idx] = finish(c.g0[t][idx], s, 1.0, c.acc)

    for q in (PRODUCTS if products is None else products):
        col = [enc_panel_row(0 if enc_identity else q.enc, j) for j in range(q.cols)]
        s = c.A[q.a].T @ c.B[q.b][:, col]
        i, j = np.ogrid[:q.rows, :q.cols]
        put(q.tensor, i * q.dst_ld + q.dc0 + j, s)
        if q.bias is not None:
            put(q.bias, np.arange(q.rows), c.A[q.a].sum(0))
    d4, bp = c.d4.astype(f64), c.bias_part.astype(f64)
    put(22, np.arange(3 * 128), (d4[:, :3].T @ c.B[9]).reshape(-1))
    put(23, np.arange(3), bp[:, :3].sum(0))
    put(20, np.arange(256), d4[:, 3] @ c.B[7])
    put(21, np.arange(1), bp[:, 3:].sum(0))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the cases of the unit tests
# ------------------------------------------------------------------------------------------------------------------------
def place_case(rows, cols, transpose, seed=0):
    rng = np.random.RandomState(1000 + seed + 7 * rows + cols + transpose)
    r0, c0, col0 = 2, 3, 5
    src_ld = col0 + cols + 3
    out_r, out_c = (cols, rows) if transpose else (rows, cols)
    dst_ld = c0 + out_c + 4
    src = _ints(rng, rows * src_ld, -99, 99)
    inside = bits(src).reshape(rows, src_ld)[:, col0:col0 + cols]            # a view: the rectangle the call copies
    inside[0, 0] = NEG_ZERO_BITS
    inside[rows // 2, cols // 2] = NAN_BITS if rows * cols > 1 else NEG_ZERO_BITS
    dst0 = _ints(rng, (r0 + out_r + 2) * dst_ld, 1000, 1999)
    return C(name=f"place {rows}x{cols} t{transpose}", rows=rows, cols=cols, transpose=transpose, r0=r0, c0=c0, col0=col0,
             src_ld=src_ld, dst_ld=dst_ld, src=src, dst0=dst0)


def place_cases():
    return [place_case(r, k, t) for (r, k) in ((1, 1), (3, 16), (258, 63), (128, 283)) for t in (0, 1)]


def scatter_case(P, ldg):
    rng = np.random.RandomState(2000 + P + ldg)
    return C(name=f"scatter_heads P={P} ldg={ldg}", P=P, ldg=ldg, d4=_special(rng, _ints(rng, P * 4, -99, 99)),
             drgb0=_ints(rng, P * 32, 1000, 1999), gsig0=_ints(rng, P * ldg, 2000, 2999))


def scatter_cases():
    return [scatter_case(P, ldg) for P in (1, 31, 33, 257) for ldg in (32, 64, 288)]


def _cancel_column(n):
    col = np.ones(n, f32)
    col[0], col[-1] = 2.0 ** 25, -2.0 ** 25
    return col


def colsum_case(P, ld, col0, cols, accumulate, cancel=False):
    rng = np.random.RandomState(3000 + P % 1000 + ld + col0 + 10 * cols + accumulate)
    src = np.full(P * ld, np.nan, f32)               # every column the call does not own is poison
    vals = _ints(rng, (P, cols))
    if cancel:
        vals[:, 0] = _cancel_column(P)
    src.reshape(P, ld)[:, col0:col0 + cols] = vals
    return C(name=f"colsum P={P} ld={ld} col0={col0} cols={cols} acc={accumulate}" + (" cancel" if cancel else ""), P=P, ld=ld,
             col0=col0, cols=cols, accumulate=accumulate, src=src, dst0=_ints(rng, 8, -50, 50))


def colsum_cases():
    out = [colsum_case(P, ld, col0, cols, acc) for P in (1, 255, 256, 257) for (ld, col0) in ((32, 0), (288, 0), (288, 256))
           for cols in (1, 2, 3, 4) for acc in (0, 1)]
    out += [colsum_case(P, 32, 4 * acc, cols, acc) for P in (65536, 65537) for (cols, acc) in ((4, 1), (1, 0))]
    out += [colsum_case(257, 32, 0, 2, acc, cancel=True) for acc in (0, 1)]
    return out


def tile_sums_case(n_tiles, N, n_bias, accumulate, cancel=False):
    rng = np.random.RandomState(4000 + n_tiles + N + n_bias + accumulate)
    tiles = _ints(rng, (n_tiles, N))
    if cancel:
        tiles[:, 0] = _cancel_column(n_tiles)
    return C(name=f"tile_sums n_tiles={n_tiles} N={N} n_bias={n_bias} acc={accumulate}" + (" cancel" if cancel else ""),
             n_tiles=n_tiles, N=N, n_bias=n_bias, accumulate=accumulate, tiles=tiles, dst0=_ints(rng, N, -50, 50))


def tile_sums_cases():
    out = [tile_sums_case(nt, N, nb, acc) for nt in (1, 3, 63, 64, 65, 257) for N in (32, 64, 96, 288) for nb in (N, N - 30, 3)
           for acc in (0, 1)]
    out += [tile_sums_case(65, 96, 0, 1)]            # n_bias = 0 stands for N
    out += [tile_sums_case(257, 96, 66, acc, cancel=True) for acc in (0, 1)]
    return out


def reduce_place_case(splits, rows, cols, dst_ld, dc0, scale, accumulate):
    rng = np.random.RandomState(5000 + splits + rows + cols + dc0 + accumulate)
    pr0, pc0 = 2, 3
    p_ld = pc0 + cols + 2
    stride = (pr0 + rows + 1) * p_ld + 5
    partial = np.full(splits * stride, np.nan, f32)
    tile = partial.reshape(splits, stride)[:, :(pr0 + rows + 1) * p_ld].reshape(splits, pr0 + rows + 1, p_ld)
    assert np.shares_memory(tile, partial)
    tile[:, pr0:pr0 + rows, pc0:pc0 + cols] = _ints(rng, (splits, rows, cols)) * f32(1.0 / scale)
    # dst0 in quanta of `scale` x the stored integers = whole numbers again
    return C(name=f"reduce_place splits={splits} {rows}x{cols} dst_ld={dst_ld} dc0={dc0} scale={scale} acc={accumulate}",
             splits=splits, rows=rows, cols=cols, dst_ld=dst_ld, dc0=dc0, p_ld=p_ld, pr0=pr0, pc0=pc0, accumulate=accumulate,
             scale=scale, stride=stride, partial=partial, dst0=_ints(rng, (rows + 1) * dst_ld, 3000, 3999))


REDUCE_RECTS = ((3, 27, 283, 256), (2, 256, 319, 63), (258, 63, 63, 0))      # rows, cols, dst_ld, dc0


def reduce_place_cases():
    return [reduce_place_case(sp, r, k, ld, dc0, scale, acc) for sp in (1, 3, 4, 5, 8, 9, 256) for (r, k, ld, dc0) in REDUCE_RECTS
            for scale in (1.0, 2.0 ** -7) for acc in (0, 1) if not (sp == 256 and r == 258 and scale == 1.0)]


def panel_matrix(P, R):
    """(P, R) fp16 integers in -2046 .. 2046 (exact in fp16): within a point group (point, row) -> value is one-to-one up to the
    4,093 values there are; the group index shifts the pattern"""
    p, r = np.arange(P, dtype=np.int64)[:, None], np.arange(R, dtype=np.int64)[None, :]
    return (((R * (p % 32) + r + 17 * (p // 32)) % 4093) - 2046).astype(np.float16)


def panel_case(R, NW, P, real=False):
    rng = np.random.RandomState(6000 + R + P)
    if real:
        mat, w4 = rng.standard_normal((P, R)).astype(np.float16), rng.standard_normal((P, 4)).astype(f32)
    else:
        mat, w4 = panel_matrix(P, R), _ints(rng, (P, 4))
    col = 0 if NW == 3 else 3                        # the product reads d4[:, 0..2] or d4[:, 3], row stride 4
    return C(name=f"panel_wsums<{R}, {NW}> P={P}" + (" real" if real else ""), R=R, NW=NW, P=P, mat=mat, w4=w4, w_col=col,
             w=w4[:, col:col + NW])


PANEL_KINDS = ((128, 3), (256, 1))
PANEL_P = (32, 96, 160, 4096, 32800)


def panel_cases():
    return [panel_case(R, NW, P) for (R, NW) in PANEL_KINDS for P in PANEL_P]


def finish_case(kind, rows, cols, splits, accumulate, enc_rows=0, scale=1.0, seed=0):
    """a job and its buffers: q (the job's scalars), dst0, partial (flat; NaN wherever the job must not read)"""
    rng = np.random.RandomState(7000 + 31 * kind + rows + cols + splits + accumulate + enc_rows + seed)
    q = C(kind=kind, rows=rows, cols=cols, splits=splits, accumulate=accumulate, enc_rows=enc_rows, scale=scale, dst_ld=0, dc0=0,
          p_ld=0, stride=0, p_off=0)
    vals = f32(1.0 / scale)
    if kind == 0:
        q.p_ld = 256 if enc_rows == 0 else 64
        q.dc0, q.dst_ld = 5, 5 + cols + 3
        q.stride = rows * q.p_ld + 7
        partial = np.full(splits * q.stride, np.nan, f32)
        tile = partial.reshape(splits, q.stride)[:, :rows * q.p_ld].reshape(splits, rows, q.p_ld)
        assert np.shares_memory(tile, partial)
        used = [enc_panel_row(enc_rows, j) for j in range(cols)]
        tile[:, :, used] = _ints(rng, (splits, rows, cols)) * vals
        dst0 = _ints(rng, rows * q.dst_ld + 3, 3000, 3999)
    elif kind == 1:
        partial = _ints(rng, splits * rows) * vals
        dst0 = _ints(rng, rows + 3, 3000, 3999)
    else:
        q.stride = 4
        q.p_off = 3 if rows == 1 else 0               # the density head's bias reads column 3 of the per-ray rows
        partial = np.full(splits * 4, np.nan, f32)
        partial.reshape(splits, 4)[:, q.p_off:q.p_off + rows] = _ints(rng, (splits, rows))
        dst0 = _ints(rng, rows + 3, 3000, 3999)
    q.name = f"finish kind={kind} {rows}x{cols} splits={splits} acc={accumulate} enc={enc_rows} scale={scale}"
    q.dst0, q.partial = dst0, partial
    return q


def finish_ref(q, **kw):
    return finish_job(q, q.dst0, q.partial[q.p_off:], **kw)


def finish_cases():
    out = [finish_case(0, 3, cols, sp, acc, enc) for (enc, cols) in ((0, 256), (1, 63), (2, 27)) for sp in (1, 7, 8, 9, 21)
           for acc in (0, 1)]
    out += [finish_case(0, 256, 256, 1, 1)]                                   # the grid's last thread owns the last element
    out += [finish_case(1, rows, 1, sp, acc) for rows in (1, 128, 256) for (sp, acc) in ((1, 0), (9, 1), (64, 1))]
    out += [finish_case(1, rows, 1, sp, int(sp == 65), scale=2.0 ** -3) for rows in (1, 384, 1025) for sp in (65, 1024)]
    out += [finish_case(2, rows, 1, sp, (rows + sp) & 1) for rows in (1, 2, 3, 4) for sp in (1, 63, 64, 65, 5000)]
    return out


def mixed_jobs(n=MAX_FINISH_JOBS):
    """n jobs of all kinds and paths for one launch"""
    pool = [finish_case(0, 3, 63, 9, 1, 1, seed=1), finish_case(1, 384, 1, 65, 0, scale=2.0 ** -3, seed=1),
            finish_case(2, 3, 1, 65, 1, seed=1), finish_case(0, 5, 256, 8, 0, 0, seed=1), finish_case(1, 128, 1, 7, 1, seed=1),
            finish_case(2, 1, 1, 5000, 0, seed=1), finish_case(0, 2, 27, 21, 1, 2, seed=1), finish_case(1, 1025, 1, 70, 1, seed=1)]
    return [finish_case(q.kind, q.rows, q.cols, q.splits, q.accumulate, q.enc_rows, q.scale, seed=100 + i)
            for i, q in zip(range(n), itertools.cycle(pool))]


CHAIN_SHAPES = ((128, 2), (160, 5), (4128, 129))     # (P, n_rays)
CHAIN_SPREAD = 3                                      # pscale = 2^-3 .. 2^3


def chain_case(P, n_rays, acc, g0=None, seed=0):
    """stored (ints, fp16-exact) and true (x pscale) gradient panels, forward panels, d4, bias_part; the panels' points are padded
    to a multiple of 128 with zeros by the test, as the product leaves them.  amax of panel a = its largest true magnitude."""
    rng = np.random.RandomState(8000 + P + 13 * acc + seed)
    stored = [_ints(rng, (P, PANEL_ROWS[a])) for a in range(10)]
    ps = [np.exp2(rng.randint(-CHAIN_SPREAD, CHAIN_SPREAD + 1, size=P)).astype(f32) for _ in range(10)]
    A = [s.astype(f64) * p.astype(f64)[:, None] for s, p in zip(stored, ps)]
    B = [_ints(rng, (P, rows)).astype(f64) for rows in PANEL_ROWS]
    c = C(name=f"chain_weight_grads P={P} rays={n_rays} acc={acc}", P=P, n_rays=n_rays, acc=acc, stored=stored, ps=ps, A=A, B=B,
          amax=[f32(np.abs(a).max()) for a in A], d4=_ints(rng, (P, 4)), bias_part=_ints(rng, (n_rays, 4), -40, 40))
    c.g0 = g0 if g0 is not None else [_ints(rng, int(np.prod(s)), 5000, 5999) for s in TENSOR_SHAPES]
    return c


def assert_chain_exact(c):
    """the fp16 products' condition (tests/test_gpu_gemm_units.py, run_wgrad), for every product, its row sums and the two
    head streams; quanta of the smallest scale"""
    quantum = 2.0 ** -CHAIN_SPREAD
    for q in PRODUCTS:
        assert_exact_products(np.abs(c.A[q.a]), np.abs(c.B[q.b]), quantum, f"product {q.a} x {q.b}")
        assert float(np.abs(c.A[q.a]).sum(0).max()) / quantum < 2.0 ** 24
        top, nz = float(np.abs(c.A[q.a]).max()), np.abs(c.A[q.a])[c.A[q.a] != 0]
        assert top > 0 and float(nz.min()) / top * 2.0 ** 13 >= 2.0 ** -14     # every element a normal fp16 number after the rescale
    assert_exact_products(np.abs(c.d4[:, :3]), np.abs(c.B[9]), 1.0, "rgb head")
    assert_exact_products(np.abs(c.d4[:, 3:]), np.abs(c.B[7]), 1.0, "sigma head")


# ------------------------------------------------------------------------------------------------------------------------
# deliberately wrong references: (kernel, what is wrong, the case it shows on, the wrong function of that case)
# ------------------------------------------------------------------------------------------------------------------------
def _swap_bits_2_3(row):
    return (row & ~12) | ((row & 4) << 1) | ((row & 8) >> 1)


def _last_tile_slice_dropped(c):
    lo = [s for s in tile_slices(c.n_tiles) if s[0] < s[1]][-1][0]
    return np.arange(c.n_tiles) < lo


def _phase3_dropped(c):
    keep = np.ones(c.n_tiles, bool)
    for lo, hi in tile_slices(c.n_tiles):
        keep[lo + 3:hi:4] = False
    return keep


def _layer5_halves_swapped():
    out = []
    for q in PRODUCTS:
        q = C(**vars(q))
        if q.tensor == 8:
            q.dc0 = 256 if q.enc == 1 else 0          # [h | pe] instead of [pe | h]
        out.append(q)
    return out


TEETH_CASES = {
    "place": lambda: place_case(3, 16, 1),
    "scatter_heads": lambda: scatter_case(33, 64),
    "colsum cancel": lambda: colsum_case(257, 32, 0, 2, 1, cancel=True),
    "colsum long": lambda: colsum_case(65537, 32, 4, 4, 1),
    "tile_sums": lambda: tile_sums_case(257, 96, 66, 1, cancel=True),
    "reduce_place": lambda: reduce_place_case(9, 3, 27, 283, 256, 2.0 ** -7, 1),
    "panel_wsums 128": lambda: panel_case(128, 3, 160),
    "panel_wsums 256": lambda: panel_case(256, 1, 160),
    "finish_jobs": lambda: finish_case(0, 3, 63, 21, 1, 1),
    "chain_weight_grads": lambda: chain_case(160, 5, 1),
}
RIGHT = {"place": place, "scatter_heads": scatter_heads, "colsum": colsum, "tile_sums": tile_sums, "reduce_place": reduce_place,
         "panel_wsums": panel_wsums, "finish_jobs": finish_ref, "chain_weight_grads": chain_weight_grads}
# the point whose weight meets the data of (point p, row r) without the `^ 8 (U & 1)` of the slot index: odd units (rows with bit
# 4 set) pair slot sl with point sl >> 1 instead of (sl ^ 8) >> 1
_NO_SWIZZLE = dict(w_point=lambda p, r: np.where((r & 16) != 0, p ^ 4, p))
WRONG = [
    ("place", "transpose ignored", "place", lambda c: place(c, transpose=0)),
    ("place", "col0 ignored", "place", lambda c: place(c, col0=0)),
    ("scatter_heads", "d sigma left in column 3 of drgb", "scatter_heads", lambda c: scatter_heads(c, sigma_col=3)),
    ("colsum", "fp32 accumulation", "colsum cancel", lambda c: colsum(c, fp32=True)),
    ("colsum", "accumulate ignored", "colsum cancel", lambda c: colsum(c, accumulate=0)),
    ("colsum", "rows from 65,536 on dropped", "colsum long", lambda c: colsum(c, rows=65536)),
    ("tile_sums", "fp32 accumulation", "tile_sums", lambda c: tile_sums(c, fp32=True)),
    ("tile_sums", "accumulate ignored", "tile_sums", lambda c: tile_sums(c, accumulate=0)),
    ("tile_sums", "last slice dropped", "tile_sums", lambda c: tile_sums(c, keep=_last_tile_slice_dropped(c))),
    ("tile_sums", "row phase 3 dropped", "tile_sums", lambda c: tile_sums(c, keep=_phase3_dropped(c))),
    ("tile_sums", "n_bias taken as N", "tile_sums", lambda c: tile_sums(c, n_bias=c.N)),
    ("reduce_place", "splits % 4 tail dropped", "reduce_place", lambda c: reduce_place(c, splits=c.splits & ~3)),
    ("reduce_place", "accumulate ignored", "reduce_place", lambda c: reduce_place(c, accumulate=0)),
    ("reduce_place", "scale ignored", "reduce_place", lambda c: reduce_place(c, scale=1.0, exact=False)),
    ("panel_wsums", "point index without the swizzle", "panel_wsums 128", lambda c: panel_wsums(c, **_NO_SWIZZLE)),
    ("panel_wsums", "4 h and 8 (e >> 2) row terms exchanged", "panel_wsums 128", lambda c: panel_wsums(c, row_of=_swap_bits_2_3)),
    ("panel_wsums", "last slice dropped", "panel_wsums 128", lambda c: panel_wsums(c, drop_last=True)),
    ("panel_wsums", "point index without the swizzle", "panel_wsums 256", lambda c: panel_wsums(c, **_NO_SWIZZLE)),
    ("panel_wsums", "4 h and 8 (e >> 2) row terms exchanged", "panel_wsums 256", lambda c: panel_wsums(c, row_of=_swap_bits_2_3)),
    ("panel_wsums", "last slice dropped", "panel_wsums 256", lambda c: panel_wsums(c, drop_last=True)),
    ("finish_jobs", "identity instead of enc_panel_row", "finish_jobs", lambda c: finish_ref(c, enc_rows=0, exact=False)),
    ("finish_jobs", "splits % 8 tail dropped", "finish_jobs", lambda c: finish_ref(c, splits=c.splits & ~7)),
    ("finish_jobs", "accumulate ignored", "finish_jobs", lambda c: finish_ref(c, accumulate=0)),
    ("chain_weight_grads", "identity instead of enc_panel_row", "chain_weight_grads", lambda c: chain_weight_grads(c, enc_identity=True)),
    ("chain_weight_grads", "layer 5 as [h | pe]", "chain_weight_grads", lambda c: chain_weight_grads(c, products=_layer5_halves_swapped())),
]


def differs(a, b):
    """do two reference results (an array, or a tuple / list of arrays) differ in at least one element's bits?"""
    if isinstance(a, (tuple, list)):
        return any(differs(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == f32 and b.dtype == f32:
        return not np.array_equal(bits(a), bits(b))
    return not np.array_equal(a.astype(f64), b.astype(f64))
