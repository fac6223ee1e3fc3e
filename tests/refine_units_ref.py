"""Plain numpy restatements of the small kernels of the refinement network's train-mode pair (csrc/nsr_refine_train.hip; their
launchers: csrc/nsr_refine_train_work.h), the case lists of tests/test_gpu_refine_units.py and the data of every case.

Two forms per operation where that makes sense:

* the ORDER-RESTATING fp32 form (``*_f32``): the same operations in the same order with one rounding each (the unit is compiled
  with -ffp-contract=off and numpy's float32 arithmetic rounds every operation once).  A per-channel reduction is four row
  lanes striding by 4 inside a partition of ceil(rows / nparts) rows, combined as ((s0 + s1) + s2) + s3, then the partitions in
  order in double.  The device result must equal it bit for bit on any input; only sqrtf and tanhf are left to a bound.
* the fp64 MATHEMATICAL form (``*64``): what the operation means.  tests/test_refine_units_cpu.py pins these against torch's
  fp64 autograd.

``mut=`` turns a restatement into a deliberately WRONG kernel (one name per mistake the unit tests must notice); the CPU file
asserts that every one of them changes the expected result of at least one case of the unit it applies to.  Nothing here is
ever run on a device.

Buffers: an output is a NaN-filled frame, ``GR`` guard rows (``GE`` guard elements for vectors) before and after the owned
region and, where the kernel takes a row stride, ``ld`` > C columns of which it owns [ch0, ch0 + C); an input with a stride is
laid out the same way with NaN in what the kernel must not read.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

F32 = np.float32
NAN = F32(np.nan)
GR, GE = 2, 4
EPS = F32(1e-5)
MAX_PARTS = 256
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 3
TINY = F32(np.float32(1.401298464324817e-45))     # the smallest positive fp32

MUTATIONS = ("swap_k", "one_up", "no_stride", "last_winner", "nan_loses", "biased_running_var", "mean_wrong_pass", "no_acc",
             "no_ch0", "wgrad_transpose", "fwd_sum_f32")


def same_bits(a, b):
    """elementwise: the same bit pattern, or both NaN (a NaN's payload is not part of any contract here)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b


def frame(rows, ld):
    return np.full((rows + 2 * GR, ld), NAN, dtype=F32)


def vec_frame(n):
    return np.full(n + 2 * GE, NAN, dtype=F32)


def own(buf, rows, ch0, C, mut=None):
    """the owned region of a frame (a view)"""
    c0 = 0 if mut == "no_ch0" else ch0
    return buf[GR:GR + rows, c0:c0 + C]


def relu_nan(x):
    """nsr_relu_nan: x <= 0 -> +0, NaN stays NaN"""
    return np.where(x <= 0, F32(0), x).astype(F32)


def bn_act_f32(z, mean, rstd, g, b):
    with np.errstate(invalid="ignore"):
        return relu_nan((((z - mean) * rstd) * g + b).astype(F32))


# ------------------------------------------------------------------------------------------------------------------------
# per-channel reductions and their finishers
# ------------------------------------------------------------------------------------------------------------------------
def reduce_parts(rows):
    return min(MAX_PARTS, (rows + 63) // 64)


def rows_per_part(rows, nparts):
    return -(-rows // nparts)


def reduce_terms_f32(mode, x, stat=None, gamma=None, beta=None, da=None, mut=None):
    """the fp32 terms the kernel adds, per row and channel: [t] (modes 0, 1) or [dy, dy xhat] (mode 2)"""
    x = x.astype(F32, copy=False)
    C = x.shape[1]
    with np.errstate(invalid="ignore"):
        if mode == 0:
            return [x]
        mean = stat[:C]
        if mode == 1:
            if mut == "mean_wrong_pass":
                return [x * x]
            d = x - mean
            return [d * d]
        rstd = stat[C:2 * C]
        dy = np.where(bn_act_f32(x, mean, rstd, gamma, beta) > 0, da, F32(0)).astype(F32)
        return [dy, dy * ((x - mean) * rstd)]


def lanes_sum_f32(t, nparts):
    """(rows, C) terms -> (nparts, C): four lanes striding by 4 inside each partition, sequential fp32, ((s0+s1)+s2)+s3"""
    rows, C = t.shape
    rpp = rows_per_part(rows, nparts)
    r0 = np.arange(nparts, dtype=np.int64) * rpp
    r1 = np.minimum(r0 + rpp, rows)
    s = np.zeros((nparts, 4, C), dtype=F32)
    lane = np.arange(4)
    with np.errstate(invalid="ignore"):
        for k in range(-(-rpp // 4)):
            r = r0[:, None] + lane[None, :] + 4 * k                      # (nparts, 4)
            ok = r < r1[:, None]
            v = np.where(ok[:, :, None], t[np.where(ok, r, 0)], F32(0))
            # a lane that has run out adds nothing (the kernel's loop has ended): keep its sum, -0.0 and NaN included
            s = np.where(ok[:, :, None], s + v, s)
        return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def col_reduce_f32(mode, x, nparts, stat=None, gamma=None, beta=None, da=None, mut=None):
    """part (1 or 2, nparts, C) as col_reduce_kernel<mode> leaves it"""
    return np.stack([lanes_sum_f32(t, nparts) for t in reduce_terms_f32(mode, x, stat, gamma, beta, da, mut)])


def part_sum64(part):
    """(nparts, C) -> the partitions added in order in double"""
    s = np.zeros(part.shape[1], dtype=np.float64)
    for p in range(part.shape[0]):
        s = s + part[p].astype(np.float64)
    return s


def momentum_f32(run, new, momentum):
    m = F32(momentum)
    return ((F32(1) - m) * run + m * new).astype(F32)


def fin_mean_f32(part, rows, momentum=0.0, run_mean=None):
    mean = (part_sum64(part) / float(rows)).astype(F32)
    return mean, (None if run_mean is None else momentum_f32(run_mean, mean, momentum))


def fin_var_f32(part, rows, momentum=0.0, run_var=None, eps=EPS, mut=None, mean=None):
    """(rstd with numpy's correctly rounded sqrt, running_var').  The device's sqrtf is held to a bound, not to these bits."""
    ss = part_sum64(part)
    var = (ss / float(rows)).astype(F32)
    if mut == "mean_wrong_pass":               # the mean taken off after the sum of the RAW squares
        var = (var - mean * mean).astype(F32)
    rstd = (F32(1) / np.sqrt((var + F32(eps)).astype(F32))).astype(F32)
    if run_var is None:
        return rstd, None
    unbiased = var if mut == "biased_running_var" else (ss / float(rows - 1)).astype(F32)
    return rstd, momentum_f32(run_var, unbiased, momentum)


def fin_bn_bwd_f32(part, rows, acc, g_gamma, g_beta, mut=None):
    """(g_gamma', g_beta', m (2 C))"""
    s1, s2 = part_sum64(part[0]), part_sum64(part[1])
    keep = acc and mut != "no_acc"
    zero = np.zeros_like(s1, dtype=F32)
    gb = ((g_beta if keep else zero) + s1.astype(F32)).astype(F32)
    gg = ((g_gamma if keep else zero) + s2.astype(F32)).astype(F32)
    return gg, gb, np.concatenate([(s1 / float(rows)).astype(F32), (s2 / float(rows)).astype(F32)])


def fin_bias_f32(part, n_valid, acc, g_bias, mut=None):
    """elements [0, n_valid) of the bias gradient; the rest of g_bias stays"""
    out = g_bias.copy()
    s = part_sum64(part).astype(F32)[:n_valid]
    out[:n_valid] = ((g_bias[:n_valid] if (acc and mut != "no_acc") else F32(0)) + s).astype(F32)
    return out


# fp64 mathematical forms
def bn_train_fwd64(z, gamma, beta, eps=1e-5, momentum=0.1, run_mean=None, run_var=None):
    """BatchNorm (train) + ReLU over the rows of (rows, C): (a, mean, biased var, running_mean', running_var')"""
    z = z.astype(np.float64)
    n = z.shape[0]
    mean = z.mean(0)
    ss = ((z - mean) ** 2).sum(0)
    var = ss / n
    a = np.maximum(gamma * (z - mean) / np.sqrt(var + eps) + beta, 0.0)
    rm = None if run_mean is None else (1 - momentum) * run_mean + momentum * mean
    rv = None if run_var is None else (1 - momentum) * run_var + momentum * ss / (n - 1)
    return a, mean, var, rm, rv


def bn_relu_bwd64(z, da, gamma, beta, eps=1e-5):
    """(dZ, d gamma, d beta) of a = relu(gamma xhat + beta) with batch statistics"""
    z, da = z.astype(np.float64), da.astype(np.float64)
    n = z.shape[0]
    mean = z.mean(0)
    rstd = 1.0 / np.sqrt(((z - mean) ** 2).mean(0) + eps)
    xhat = (z - mean) * rstd
    dy = np.where(gamma * xhat + beta > 0, da, 0.0)
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    return gamma * rstd * (dy - dbeta / n - xhat * dgamma / n), dgamma, dbeta


def sum_bound(abs_terms_sum, rows, nparts, extra_roundings=0):
    """first-order bound of a fixed-order fp32 sum against its fp64 value: a lane adds ceil(rpp / 4) terms (one rounding
    each at most), three more roundings combine the lanes; the partitions are added in double"""
    return (-(-rows_per_part(rows, nparts) // 4) + 3 + extra_roundings) * 2.0 ** -24 * abs_terms_sum


ReduceCase = namedtuple("ReduceCase", "rows C n_valid kind ld ch0 seed")


def _reduce_cases():
    out, seed = [], 0
    shapes = [(r, C) for r in (2, 8, 63, 64, 65, 257) for C in (8, 64)]
    shapes += [(257, 32), (257, 128), (257, 512), (16384, 8), (16384, 128), (16448, 8), (16448, 32), (16448, 128), (20000, 8), (20000, 512)]
    for rows, C in shapes:
        seed += 1
        nv = 3 if C == 32 else C
        ld, ch0 = (384, 128) if C == 128 else (C + 12, 8)
        out.append(ReduceCase(rows, C, nv, "real", ld, ch0, seed))
        if rows & (rows - 1) == 0:
            out.append(ReduceCase(rows, C, nv, "int", ld, ch0, 100 + seed))
    return out


REDUCE_CASES = _reduce_cases()


def build_reduce(c: ReduceCase):
    """x and dA in NaN frames (ld, ch0), gamma, beta and the numpy-made stat of mode 2, prefilled gradients and running stats"""
    g = np.random.default_rng(c.seed)
    rows, C = c.rows, c.C
    d = {}
    if c.kind == "int":
        # mirrored halves: the mean of a channel is the integer k, so the centred squares and every sum are exact in fp32
        k = g.integers(-1, 3, size=C)
        half = g.integers(-3, 4, size=(rows // 2, C))
        x = np.concatenate([half, 2 * k - half]).astype(F32)
        da = g.integers(-3, 4, size=(rows, C)).astype(F32)
        gamma = g.choice(np.array([1, 2, -1], dtype=F32), size=C)
        beta = g.integers(-1, 2, size=C).astype(F32)
        stat2 = np.concatenate([k.astype(F32), np.full(C, 0.5, dtype=F32)])      # mode 2: rstd a power of two
        pre = g.integers(-4, 5, size=(3, C)).astype(F32)
    else:
        x = (g.standard_normal((rows, C)) * (1 + np.arange(C) % 3) + (np.arange(C) % 5 - 1.5)).astype(F32)
        da = g.standard_normal((rows, C)).astype(F32)
        gamma = (1 + 0.5 * g.standard_normal(C)).astype(F32)
        beta = (0.3 * g.standard_normal(C)).astype(F32)
        x64 = x.astype(np.float64)
        stat2 = np.concatenate([x64.mean(0), 1 / np.sqrt(x64.var(0) + 1e-5)]).astype(F32)
        pre = g.standard_normal((3, C)).astype(F32)
    X, DA = frame(rows, c.ld), frame(rows, c.ld)
    own(X, rows, c.ch0, C)[:] = x
    own(DA, rows, c.ch0, C)[:] = da
    d.update(X=X, DA=DA, gamma=gamma, beta=beta, stat2=stat2, g_gamma0=pre[0], g_beta0=pre[1], g_bias0=pre[2],
             run_mean0=(pre[0] * F32(0.5)).astype(F32), run_var0=np.abs(pre[1]) + F32(1))
    return d


def reduce_expected(c: ReduceCase, d, mut=None):
    """every output of the reduction chain of one case, each kernel fed by the restatement of the one before"""
    rows, C = c.rows, c.C
    x, da = own(d["X"], rows, c.ch0, C, mut), own(d["DA"], rows, c.ch0, C, mut)
    nparts = reduce_parts(rows)
    e = {"nparts": nparts}
    e["part0"] = col_reduce_f32(0, x, nparts)
    e["mean"] = fin_mean_f32(e["part0"][0], rows)[0]
    e["run_mean"] = {m: fin_mean_f32(e["part0"][0], rows, m, d["run_mean0"])[1] for m in (0.1, 0.0, 1.0)}
    stat1 = np.concatenate([e["mean"], np.zeros(C, dtype=F32)])
    e["part1"] = col_reduce_f32(1, x, nparts, stat1, mut=mut)
    e["rstd"] = fin_var_f32(e["part1"][0], rows, mut=mut, mean=e["mean"])[0]
    e["run_var"] = {m: fin_var_f32(e["part1"][0], rows, m, d["run_var0"], mut=mut, mean=e["mean"])[1] for m in (0.1, 0.0, 1.0)}
    e["part2"] = col_reduce_f32(2, x, nparts, d["stat2"], d["gamma"], d["beta"], da)
    for acc in (0, 1):
        e["g_gamma", acc], e["g_beta", acc], e["m"] = fin_bn_bwd_f32(e["part2"], rows, acc, d["g_gamma0"], d["g_beta0"], mut)
        e["g_bias", acc] = fin_bias_f32(e["part0"][0], c.n_valid, acc, d["g_bias0"], mut)
    return e


# ------------------------------------------------------------------------------------------------------------------------
# bn_relu / bn_bwd / relu_bwd
# ------------------------------------------------------------------------------------------------------------------------
BnCase = namedtuple("BnCase", "rows C ld ch0 seed")
BN_CASES = [BnCase(r, C, 384 if C == 128 else C + 12, 128 if C == 128 else 8, 10 * r + C) for r in (1, 63, 257) for C in (8, 128)]


def build_bn(c: BnCase):
    g = np.random.default_rng(c.seed)
    rows, C = c.rows, c.C
    z = g.standard_normal((rows, C)).astype(F32)
    mean = (0.2 * g.standard_normal(C)).astype(F32)
    rstd = (0.5 + g.random(C)).astype(F32)
    gamma = (1 + 0.5 * g.standard_normal(C)).astype(F32)
    beta = (0.3 * g.standard_normal(C)).astype(F32)
    # row 0, channels 0..7: activations that are exactly +0, -0 -> +0, the smallest positive fp32, its negative, NaN, exactly 0
    # through the affine map, one rounding step above and one below 0
    mean[:8], rstd[:8], gamma[:8] = 0, 1, 1
    beta[:8] = [0, 0, 0, 0, 1, 1, 1, 0]
    z[0, :8] = [0.0, TINY, -TINY, np.nan, -1.0, np.nextafter(F32(-1), F32(0)), np.nextafter(F32(-1), F32(-2)), -0.0]
    if rows > 2:
        z[rows // 2, C - 1] = np.nan
    da = g.standard_normal((rows, C)).astype(F32)
    m = (0.1 * g.standard_normal(2 * C)).astype(F32)
    DA = frame(rows, c.ld)
    own(DA, rows, c.ch0, C)[:] = da
    return dict(z=z, stat=np.concatenate([mean, rstd]), gamma=gamma, beta=beta, m=m, DA=DA)


def bn_relu_expected(c: BnCase, d, mut=None):
    out = frame(c.rows, c.ld)
    C = c.C
    own(out, c.rows, c.ch0, C, mut)[:] = bn_act_f32(d["z"], d["stat"][:C], d["stat"][C:], d["gamma"], d["beta"])
    return out


def bn_bwd_f32(z, da, stat, gamma, beta, m):
    C = z.shape[1]
    mean, rstd = stat[:C], stat[C:]
    with np.errstate(invalid="ignore"):
        dy = np.where(bn_act_f32(z, mean, rstd, gamma, beta) > 0, da, F32(0)).astype(F32)
        xhat = (z - mean) * rstd
        return ((gamma * rstd) * ((dy - m[:C]) - xhat * m[C:])).astype(F32)


def bn_bwd_expected(c: BnCase, d, mut=None):
    out = frame(c.rows, c.C)
    out[GR:GR + c.rows] = bn_bwd_f32(d["z"], own(d["DA"], c.rows, c.ch0, c.C, mut), d["stat"], d["gamma"], d["beta"], d["m"])
    return out


def relu_bwd_expected(c: BnCase, d, mut=None):
    """a = the bn_relu output of the case (dense), dA dense"""
    a = bn_act_f32(d["z"], d["stat"][:c.C], d["stat"][c.C:], d["gamma"], d["beta"])
    da = np.ascontiguousarray(own(d["DA"], c.rows, c.ch0, c.C))
    out = frame(c.rows, c.C)
    with np.errstate(invalid="ignore"):
        out[GR:GR + c.rows] = np.where(a > 0, da, F32(0))
    return a, da, out


# ------------------------------------------------------------------------------------------------------------------------
# tanh_bwd, nhwc3_to_nchw
# ------------------------------------------------------------------------------------------------------------------------
TanhCase = namedtuple("TanhCase", "B H W seed")
TANH_CASES = [TanhCase(2, 3, 5, 1), TanhCase(2, 16, 24, 2)]


def build_tanh(c: TanhCase):
    g = np.random.default_rng(c.seed)
    px = c.H * c.W
    y = np.tanh(g.standard_normal((c.B * px, 3))).astype(F32)
    y[0] = [1.0, -1.0, 0.0]
    return dict(y=y, g_out=g.standard_normal((c.B, 3, px)).astype(F32))


def tanh_bwd_f32(y, g_out):
    """y (B px, 3) NHWC, g_out (B, 3, px) NCHW -> (B px, 32): columns 0..2 g (1 - t t), the rest +0"""
    B, _, px = g_out.shape
    out = np.zeros((B * px, 32), dtype=F32)
    g = g_out.transpose(0, 2, 1).reshape(B * px, 3)          # the NCHW -> NHWC index map
    out[:, :3] = g * (F32(1) - y * y)
    return out


def tanh_bwd64(y, g_out):
    B, _, px = g_out.shape
    y = y.astype(np.float64)
    return g_out.astype(np.float64).transpose(0, 2, 1).reshape(B * px, 3) * (1 - y * y)


def tanh_bwd_expected(c: TanhCase, d):
    out = frame(c.B * c.H * c.W, 32)
    out[GR:-GR] = tanh_bwd_f32(d["y"], d["g_out"])
    return out


def nhwc3_to_nchw_ref(src, B, px):
    return np.ascontiguousarray(src.reshape(B, px, 3).transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------------------
# max over the references and its routing
# ------------------------------------------------------------------------------------------------------------------------
WIN_SENT = 0xAB
MaxCase = namedtuple("MaxCase", "R C px B data ld ch0 seed")


def _max_cases():
    out, seed = [], 0
    for R in (1, 2, 8, 255):
        for C, px, B in ((8, 4, 1), (8, 15, 3), (128, 4, 3), (128, 15, 1)):
            for data in ("random", "ties", "nan", "zeros"):
                if R == 255 and C == 128 and data in ("nan", "zeros"):
                    continue                                  # the large shape once per tie rule is enough
                seed += 1
                ld, ch0 = (384, 256) if C == 128 else (C + 12, 8)
                out.append(MaxCase(R, C, px, B, data, ld, ch0, seed))
    return out


MAX_CASES = _max_cases()


def build_max(c: MaxCase):
    g = np.random.default_rng(c.seed)
    n = c.B * c.px
    if c.data == "random":
        src = g.standard_normal((c.B, c.R, c.px, c.C)).astype(F32)
    elif c.data == "ties":
        src = g.integers(0, 3, size=(c.B, c.R, c.px, c.C)).astype(F32)      # three values: most entries tie
    elif c.data == "zeros":
        src = np.array([0.0, -0.0, -0.0, -1.0], dtype=F32)[g.integers(0, 4, size=(c.B, c.R, c.px, c.C))]   # -0.0 against +0.0
    else:
        src = g.standard_normal((c.B, c.R, c.px, c.C)).astype(F32)
        # one NaN at reference r = (px + c) % R in every third column, a second one behind it in every sixth
        b, p, ch = np.meshgrid(np.arange(c.B), np.arange(c.px), np.arange(c.C), indexing="ij")
        r = (p + ch) % c.R
        one = ch % 3 == 0
        src[b[one], r[one], p[one], ch[one]] = np.nan
        two = (ch % 6 == 0) & (r + 1 < c.R)
        src[b[two], r[two] + 1, p[two], ch[two]] = np.nan
        big = (ch % 3 == 0) & (r > 0)
        src[b[big], 0, p[big], ch[big]] = 1e30        # a large finite value in front of the NaN must not keep the maximum
    G = frame(n, c.ld)
    own(G, n, c.ch0, c.C)[:] = g.standard_normal((n, c.C)).astype(F32)
    return dict(src=src, G=G)


def max_idx_f32(src, mut=None):
    """src (B, R, px, C) -> (max (B px, C), win uint8 (B px, C)): the FIRST r that reaches the maximum; a NaN wins and stays"""
    B, R, px, C = src.shape
    m = src[:, 0].copy()
    w = np.zeros(m.shape, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for r in range(1, R):
            t = src[:, r]
            if mut == "last_winner":
                take = ~np.isnan(m) & (np.isnan(t) | (t >= m))
            elif mut == "nan_loses":
                take = (t > m) | (np.isnan(m) & ~np.isnan(t))
            else:
                take = ~np.isnan(m) & (np.isnan(t) | (t > m))
            m = np.where(take, t, m)
            w = np.where(take, np.uint8(r), w)
    return m.reshape(B * px, C), w.reshape(B * px, C)


def max_expected(c: MaxCase, d, mut=None):
    n = c.B * c.px
    m, w = max_idx_f32(d["src"], mut)
    dst = frame(n, c.ld)
    own(dst, n, c.ch0, c.C, mut)[:] = m
    win = np.full(n * c.C + 2 * GE, WIN_SENT, dtype=np.uint8)
    win[GE:-GE] = w.reshape(-1)
    return dst, win


def route_f32(g_max, win, R, B, px):
    """g_max (B px, C), win (B px, C) -> g_fc (B, R, px, C): the gradient at the winner, +0 elsewhere"""
    C = g_max.shape[1]
    g = g_max.reshape(B, 1, px, C)
    hit = win.reshape(B, 1, px, C) == np.arange(R, dtype=np.uint8).reshape(1, R, 1, 1)
    return np.where(hit, g, F32(0)).astype(F32)


def route_expected(c: MaxCase, d, mut=None):
    n = c.B * c.px
    _, w = max_idx_f32(d["src"])
    out = frame(c.B * c.R * c.px, c.C)
    out[GR:-GR] = route_f32(own(d["G"], n, c.ch0, c.C, mut), w, c.R, c.B, c.px).reshape(-1, c.C)
    return w, out


# ------------------------------------------------------------------------------------------------------------------------
# col2im
# ------------------------------------------------------------------------------------------------------------------------
ColCase = namedtuple("ColCase", "Hs Ws stride up cin n_img acc ld ch0 seed")


def _col_cases():
    out, seed = [], 0
    for Hs, Ws in ((2, 2), (4, 6), (5, 7), (8, 8)):
        for stride, up in ((1, 0), (2, 0), (1, 1)):
            for cin, n_img, acc, strided in ((4, 1, 0, 0), (8, 3, 1, 1), (128, 1, 1, 0), (128, 3, 0, 1), (8, 1, 0, 1), (4, 3, 1, 0)):
                if cin == 128 and (Hs, Ws) == (8, 8) and n_img == 3:
                    n_img = 2
                seed += 1
                ld, ch0 = ((384, 128) if cin == 128 else (cin + 12, 8)) if strided else (cin, 0)
                out.append(ColCase(Hs, Ws, stride, up, cin, n_img, acc, ld, ch0, seed))
    return out


COL_CASES = _col_cases()


def conv_geometry(Hs, Ws, stride, up):
    Hin, Win = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    return (Hin - 1) // stride + 1, (Win - 1) // stride + 1


def pad32(n):
    return (n + 31) // 32 * 32


def build_col(c: ColCase, real=False):
    g = np.random.default_rng(c.seed)
    Ho, Wo = conv_geometry(c.Hs, c.Ws, c.stride, c.up)
    kp = pad32(9 * c.cin)
    M = c.n_img * Ho * Wo
    dcol = np.full((M, kp), NAN, dtype=F32)                 # the padding columns [9 cin, kp) are never read
    dcol[:, :9 * c.cin] = g.standard_normal((M, 9 * c.cin)) if real else g.integers(-3, 4, size=(M, 9 * c.cin))
    n = c.n_img * c.Hs * c.Ws
    dst0 = frame(n, c.ld)
    own(dst0, n, c.ch0, c.cin)[:] = g.standard_normal((n, c.cin)) if real else g.integers(-3, 4, size=(n, c.cin))
    if not c.acc:
        own(dst0, n, c.ch0, c.cin)[:] = NAN                 # a store must not read what it overwrites
    return dict(dcol=dcol, dst0=dst0, Ho=Ho, Wo=Wo, kp=kp)


def col2im_f32(dcol, cin, n_img, Hs, Ws, stride, up, Ho, Wo, mut=None):
    """gather form in the kernel's order (dy, dx, ky, kx), sequential fp32: (n_img Hs Ws, cin)"""
    img, sy, sx = np.meshgrid(np.arange(n_img), np.arange(Hs), np.arange(Ws), indexing="ij")
    s = np.zeros((n_img, Hs, Ws, cin), dtype=F32)
    rep = 2 if (up and mut != "one_up") else 1
    for dy in range(rep):
        for dx in range(rep):
            iy, ix = (2 * sy + dy, 2 * sx + dx) if up else (sy, sx)
            for ky in range(3):
                ty = iy + 1 - ky
                oky = (ty >= 0) & (ty // stride < Ho)
                if mut != "no_stride":
                    oky &= ty % stride == 0
                for kx in range(3):
                    tx = ix + 1 - kx
                    ok = oky & (tx >= 0) & (tx // stride < Wo)
                    if mut != "no_stride":
                        ok &= tx % stride == 0
                    m = (img * Ho + ty // stride) * Wo + tx // stride
                    tap = kx * 3 + ky if mut == "swap_k" else ky * 3 + kx
                    v = dcol[np.where(ok, m, 0), tap * cin:(tap + 1) * cin]
                    s = np.where(ok[..., None], s + v, s)
    return s.reshape(n_img * Hs * Ws, cin)


def col2im_expected(c: ColCase, d, mut=None):
    n = c.n_img * c.Hs * c.Ws
    s = col2im_f32(d["dcol"], c.cin, c.n_img, c.Hs, c.Ws, c.stride, c.up, d["Ho"], d["Wo"], mut)
    out = d["dst0"].copy()
    o = own(out, n, c.ch0, c.cin, mut)
    o[:] = (s + o).astype(F32) if (c.acc and mut != "no_acc") else s
    return out


def col2im_transpose64(dcol, cin, n_img, Hs, Ws, stride, up, Ho, Wo):
    """the transpose of conv_ref.im2col_numpy, entry by entry, in double: every column of dcol is added to the source element
    im2col copied there (found by pushing element numbers through im2col itself)"""
    from tests.conv_ref import im2col_numpy
    ids = np.arange(1, n_img * Hs * Ws * cin + 1, dtype=F32).reshape(n_img, Hs, Ws, cin)      # < 2^24: exact in fp32
    assert ids.size < 2 ** 24
    kp = dcol.shape[1]
    where = im2col_numpy(ids, 0, cin, n_img, Hs, Ws, stride, up, Ho, Wo, kp).astype(np.int64)
    live = where > 0
    out = np.bincount(where[live] - 1, weights=dcol[live].astype(np.float64), minlength=ids.size)
    return out.reshape(n_img * Hs * Ws, cin)


# ------------------------------------------------------------------------------------------------------------------------
# wgrad_reduce, fwd_reduce
# ------------------------------------------------------------------------------------------------------------------------
WgradCase = namedtuple("WgradCase", "cin cout rows splits acc seed")
WGRAD_CASES = [WgradCase(cin, cout, 4 if cout < 4 else cout, s, acc, 7 * i + s + acc)
               for i, (cin, cout) in enumerate(((3, 128), (128, 3), (8, 8), (64, 32))) for s in (1, 3, 64) for acc in (0, 1)]


def build_wgrad(c: WgradCase):
    g = np.random.default_rng(c.seed)
    kp = pad32(9 * c.cin)
    stride = c.rows * kp + 64                                # larger than the used block: NaN between the splits
    part = np.full((c.splits, stride), NAN, dtype=F32)
    blk = np.full((c.splits, c.rows, kp), NAN, dtype=F32)   # padding columns and the operand's rows >= cout: never read
    blk[:, :c.cout, :9 * c.cin] = g.integers(-3, 4, size=(c.splits, c.cout, 9 * c.cin))
    part[:, :c.rows * kp] = blk.reshape(c.splits, -1)
    g0 = vec_frame(c.cout * c.cin * 9)
    g0[GE:-GE] = g.integers(-3, 4, size=c.cout * c.cin * 9) if c.acc else NAN
    return dict(part=part, g0=g0, kp=kp, split_stride=stride)


def wgrad_reduce_f32(part, splits, split_stride, kp, cin, cout, acc, g0, mut=None):
    """tap-major (n, tap cin + c) -> (Cout, Cin, 3, 3), the splits added in order in fp32 onto g0 (acc) or 0"""
    flat = part.reshape(-1)
    n, ch, tap = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(9), indexing="ij")
    col = ch * 9 + tap if mut == "wgrad_transpose" else tap * cin + ch
    s = g0.reshape(cout, cin, 9).copy() if (acc and mut != "no_acc") else np.zeros((cout, cin, 9), dtype=F32)
    for z in range(splits):
        s = (s + flat[z * split_stride + n * kp + col]).astype(F32)
    return s.reshape(-1)


def wgrad_expected(c: WgradCase, d, mut=None):
    out = d["g0"].copy()
    out[GE:-GE] = wgrad_reduce_f32(d["part"], c.splits, d["split_stride"], d["kp"], c.cin, c.cout, c.acc, d["g0"][GE:-GE], mut)
    return out


FwdCase = namedtuple("FwdCase", "splits cout M act data ld ch0 seed")


def _fwd_cases():
    out, seed = [], 0
    for splits in (1, 2, 432):
        for cout in (3, 8, 128):
            for M in (1, 255, 257):
                if splits == 432 and cout == 128 and M != 255:
                    continue
                for act in (ACT_NONE, ACT_RELU, ACT_TANH):
                    seed += 1
                    ld, ch0 = (384, 128) if cout == 128 else (cout + 9, 5)
                    out.append(FwdCase(splits, cout, M, act, "real", ld, ch0, seed))
    # partials that cancel in fp32 but not in double
    out.append(FwdCase(4, 8, 255, ACT_NONE, "cancel", 17, 5, 900))
    out.append(FwdCase(432, 3, 257, ACT_RELU, "cancel", 12, 5, 901))
    return out


FWD_CASES = _fwd_cases()


def build_fwd(c: FwdCase):
    g = np.random.default_rng(c.seed)
    np_ = pad32(c.cout)
    stride = c.M * np_ + 32
    part = np.full((c.splits, stride), NAN, dtype=F32)
    blk = np.full((c.splits, c.M, np_), NAN, dtype=F32)      # columns [cout, np) are never read
    if c.data == "cancel":
        pat = np.array([2.0 ** 24, 1.0, -2.0 ** 24, 1.0, 3.0, 2.0 ** 25, -2.0 ** 25, 0.5], dtype=F32)
        idx = (np.arange(c.splits)[:, None, None] + np.arange(c.M)[None, :, None] * 0 + np.arange(c.cout)[None, None, :]) % len(pat)
        blk[:, :, :c.cout] = pat[idx]
        bias = g.integers(-2, 3, size=c.cout).astype(F32)
    else:
        blk[:, :, :c.cout] = g.standard_normal((c.splits, c.M, c.cout)) / np.sqrt(c.splits)
        bias = g.standard_normal(c.cout).astype(F32)
        if c.act == ACT_RELU and c.M > 1:
            blk[0, 1, 0] = np.nan                             # NaN through nsr_relu_nan
    part[:, :c.M * np_] = blk.reshape(c.splits, -1)
    return dict(part=part, bias=bias, np=np_, split_stride=stride)


def fwd_pre_f32(part, splits, split_stride, np_, cout, bias, M, mut=None):
    """the partials added in order in double, + bias in double, rounded once"""
    flat = part.reshape(-1)
    m, n = np.meshgrid(np.arange(M), np.arange(cout), indexing="ij")
    acc_t = F32 if mut == "fwd_sum_f32" else np.float64
    s = np.zeros((M, cout), dtype=acc_t)
    with np.errstate(invalid="ignore"):
        for z in range(splits):
            s = (s + flat[z * split_stride + m * np_ + n].astype(acc_t)).astype(acc_t)
        return (s.astype(np.float64) + bias.astype(np.float64)).astype(F32)


def fwd_expected(c: FwdCase, d, mut=None):
    """(frame with the pre-activation or its ReLU -- for tanh the caller compares against tanh of the pre-activation --, pre)"""
    pre = fwd_pre_f32(d["part"], c.splits, d["split_stride"], d["np"], c.cout, d["bias"], c.M, mut)
    out = frame(c.M, c.ld)
    v = relu_nan(pre) if c.act == ACT_RELU else (np.tanh(pre.astype(np.float64)).astype(F32) if c.act == ACT_TANH else pre)
    own(out, c.M, c.ch0, c.cout, mut)[:] = v
    return out, pre


def ulp32(x):
    """the spacing of fp32 at |x| (float64 array)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.maximum(2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -126))) - 23), 2.0 ** -149)
