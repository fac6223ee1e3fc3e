"""Restatements, error model and test inputs of the unit layer over the ray-side forward stages: sample_kernel, sr_mean_kernel,
unflatten_kernel (csrc/nsr_rays.hip), composite_kernel<K> (csrc/nsr_render.hip, csrc/nsr_composite.h) and resample_kernel
(csrc/nsr_render.hip).  Every restatement follows its kernel operation by operation in np.float32 (np.float64 where the kernel
holds a double), so that the device's outputs can be asked for in every bit.  Pinned on the CPU by
tests/test_ray_stages_cpu.py (against torch, the oracle and the committed fixtures); used on the device by
tests/test_gpu_ray_stages.py.

Two things make bit equality possible where a libm call or a summation order would seem to forbid it:
  the alpha probe    composite_ray's only inexact calls are expf and the softplus logf / expf, all inside alpha.  A 2-sample
                     ray z = (0, delta_k), sigma = (sigma_k, 0) has weights[0] = fl(alpha_k * 1) = the device's alpha_k exactly
                     (T_0 = 1), so one extra launch yields every alpha of a case, and everything behind alpha is IEEE
                     arithmetic in a fixed order (emulate_composite);
  exact sums         the resampler's two fp64 sums (normaliser, cdf) are exact for finite weights in [0, 1] and Nc <= 256
                     (sums_are_exact), so the lane-strided / butterfly / Hillis-Steele orders cannot show and the restatement
                     may sum in any order.
`wrong=`: deliberately wrong variants, used by the sensitivity tests only."""
import numpy as np

from tests import train_heads_ref as hr

f32 = np.float32
WHITE, SOFTPLUS = hr.WHITE, hr.SOFTPLUS
NSR_OK, NSR_ERR_INVALID_ARG, NSR_ERR_UNSUPPORTED = 0, -1, -2
EPS = f32(1e-5)

SAMPLER_WRONG = ("two_rounding_linspace", "midpoint_form")
COMPOSITE_WRONG = ("T_inclusive", "last_delta_from_z", "eps_dropped", "lane_boundary_delta", "sequential_sum", "sequential_product",
                   "white_dropped")
RESAMPLE_WRONG = ("searchsorted_left", "snap_le", "pdf_shifted", "carry_dropped", "normaliser_fp32")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ------------------------------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------------------------------
def linspace01(n, two_rounding=False):
    """nsr_linspace01(i, n) for i = 0..n-1: step = fl(1 / (n - 1)); fl(step i) below n // 2, and above it the SINGLE rounding
    fl(1 - step (n-1-i)) of a fused multiply-subtract.  step (n-1-i) is a 24-bit by 10-bit product and 1 minus it spans under
    40 bits: both are exact in fp64, so one cast to fp32 is the fma's rounding.  two_rounding: fl(1 - fl(step (n-1-i))), the
    form the kernel held before."""
    if n == 1:
        return np.zeros(1, dtype=f32)
    assert n <= 1 << 20
    step = f32(1.0) / f32(n - 1)
    i = np.arange(n)
    lower = step * i.astype(f32)
    back = (n - 1 - i).astype(f32)
    if two_rounding:
        upper = f32(1.0) - step * back
    else:
        upper = (1.0 - np.float64(step) * back.astype(np.float64)).astype(f32)
    return np.where(i < n // 2, lower, upper).astype(f32)


def coarse_z(near, far, t, lindisp):
    """nsr_coarse_z: near, far (R, 1), t (N,) -> (R, N), fp32 operation by operation"""
    one = f32(1.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if lindisp:
            a = (one / near) * (one - t)
            b = (one / far) * t
            return (one / (a + b)).astype(f32)
        return (near * (one - t) + far * t).astype(f32)


def sample_numpy(rays, N, lindisp, u=None, wrong=None):
    """sample_kernel: rays (R, >= 8) fp32 [o, d, near, far, ...] -> z (R, N), pts (R, N, 3).  u: None (deterministic) or (R, N)."""
    assert wrong is None or wrong in SAMPLER_WRONG
    rays = np.asarray(rays, dtype=f32)
    R = rays.shape[0]
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    t = linspace01(N, two_rounding=wrong == "two_rounding_linspace")
    z = coarse_z(near, far, t[None, :], lindisp)
    assert z.shape == (R, N) and z.dtype == f32
    if u is not None:
        u = np.asarray(u, dtype=f32).reshape(R, N)
        lower, upper = z.copy(), z.copy()
        if N > 1:
            mid = f32(0.5) * (z[:, :-1] + z[:, 1:])
            lower[:, 1:] = mid
            upper[:, :-1] = mid
        with np.errstate(invalid="ignore", over="ignore"):
            z = lower + u * (upper if wrong == "midpoint_form" else (upper - lower))
    with np.errstate(invalid="ignore", over="ignore"):
        pts = o[:, None, :] + z[:, :, None] * d[:, None, :]
    assert z.dtype == f32 and pts.dtype == f32
    return z, pts


def sampler_rays(R, stride, seed=0, near_eq_far=False):
    """R ray rows of `stride` floats; columns behind the eight the sampler reads are NaN"""
    rng = np.random.default_rng(100 + 10 * R + stride + seed)
    rays = np.full((R, stride), np.nan, dtype=f32)
    rays[:, 0:3] = rng.uniform(-2, 2, (R, 3))
    rays[:, 3:6] = rng.standard_normal((R, 3))
    rays[:, 6] = rng.uniform(0.05, 2.5, R)
    rays[:, 7] = rays[:, 6] if near_eq_far else rays[:, 6] + rng.uniform(0.5, 5.0, R).astype(f32)
    return rays


def sampler_u(R, N, seed=0):
    """u with the planted 0 and the largest fp32 below 1 at both ends of the first ray, random elsewhere"""
    rng = np.random.default_rng(7 + 1000 * N + R + seed)
    u = rng.random((R, N)).astype(f32)
    below1 = np.nextafter(f32(1.0), f32(0.0))
    u = np.minimum(u, below1)
    flat = u.reshape(-1)
    flat[0] = 0.0
    flat[-1] = below1
    if flat.size > 2:
        flat[1] = below1
        flat[-2] = 0.0
    return u


# edge_cases.npz: does the restatement reproduce the stored depths in every bit?  (tests/test_ray_stages_cpu.py measures it)
EDGE_FIXTURE_BIT_EQUAL = {"z_coarse_rand": True, "z_coarse_lindisp": True}
SAMPLER_N = (1, 2, 3, 64, 65, 257)
SAMPLER_R = (1, 5)


# ------------------------------------------------------------------------------------------------------------------------
# compositor
# ------------------------------------------------------------------------------------------------------------------------
def lanes_K(N):
    """samples per lane of the instantiation nsr_composite launches for N samples"""
    K = (N + 63) // 64
    return K if K <= 4 else 8


def composite_deltas(z, wrong=None):
    """delta_k of composite_ray, fp32: fl(z_{k+1} - z_k), 1e10f at the last sample.  z (R, N)"""
    z = np.asarray(z, dtype=f32)
    R, N = z.shape
    delta = np.full((R, N), 1e10, dtype=f32)
    delta[:, :-1] = z[:, 1:] - z[:, :-1]
    if wrong == "last_delta_from_z" and N > 1:
        delta[:, -1] = delta[:, -2]
    if wrong == "lane_boundary_delta":
        K = lanes_K(N)
        last_in_lane = np.arange(K - 1, N - 1, K)          # the neighbour is taken inside the lane: the lane's own last z again
        delta[:, last_in_lane] = 0.0
    return delta


def probe_inputs(sigma, z):
    """The alpha probe of a case (sigma, z: (R, N) fp32): R N rays of 2 samples, z = (0, delta_k), sigma = (sigma_k, 0), colour 0.5.
    delta_k = fl(delta_k - 0) survives the probe's own subtraction unchanged, so weights[:, 0] of nsr_composite on these rays
    (same flag word) is alpha_k of the case, bit for bit."""
    sigma = np.asarray(sigma, dtype=f32)
    P = sigma.size
    pz = np.zeros((P, 2), dtype=f32)
    pz[:, 1] = composite_deltas(z).reshape(-1)
    ps = np.zeros((P, 2), dtype=f32)
    ps[:, 0] = sigma.reshape(-1)
    return np.full((P, 2, 3), 0.5, dtype=f32), ps, pz


def alpha_libm(sigma, z, flags, wrong=None):
    """alpha with libm's exp / log rounded to fp32 standing in for the device's expf / logf: the CPU file's stand-in for the probe"""
    sigma = np.asarray(sigma, dtype=f32)
    delta = composite_deltas(z, wrong)
    with np.errstate(over="ignore", under="ignore"):
        if flags & SOFTPLUS:
            dens = np.log((f32(1.0) + hr._expf(sigma - f32(1.0))).astype(np.float64)).astype(f32)
        else:
            dens = np.maximum(sigma, f32(0.0))
        return (f32(1.0) - hr._expf(-delta * dens)).astype(f32)


def _butterfly(v):
    """wave_sum: v (R, 64) fp32 -> lane 0's value after the xor butterfly 32, 16, .., 1"""
    v = v.copy()
    lanes = np.arange(64)
    o = 32
    while o:
        v = (v + v[:, lanes ^ o]).astype(f32)
        o >>= 1
    return v[:, 0]


def _scan_mul(v):
    """wave_scan_mul_d: v (R, 64) fp64 -> inclusive products, Hillis-Steele: lane l takes lane l - o for o = 1, 2, .., 32"""
    v = v.copy()
    o = 1
    while o < 64:
        t = v.copy()
        v[:, o:] = v[:, o:] * t[:, :-o]
        o <<= 1
    return v


def emulate_composite(rgb, sigma, z, flags, alpha, wrong=None):
    """composite_ray<K> behind alpha, in the kernel's order.  rgb (R, N, >= 3), sigma, z, alpha (R, N) fp32; sigma enters through
    alpha alone and is taken for its shape.  -> comp_rgb (R, 3), depth (R,), opacity (R,), weights (R, N), all fp32.
      lane l owns samples l K .. l K + K - 1 (K = lanes_K(N)); samples k >= N: alpha = 0, f = 1, no contribution
      f = fl(fl(1 - a) + 1e-10f); lane-local running product in fp64; inclusive Hillis-Steele product scan of the lane totals;
      T_k = fp32(excl_lane * pl[i - 1]) (i > 0), fp32(excl_lane) (i = 0), T_0 = 1;  w = fl(a T)
      per lane, in sample order: acc = fl(acc + fl(w c)) for r, g, b, z and acc = fl(acc + w); xor butterfly; white term"""
    assert wrong is None or wrong in COMPOSITE_WRONG
    alpha = np.asarray(alpha, dtype=f32)
    R, N = alpha.shape
    rgb = np.asarray(rgb, dtype=f32).reshape(R, N, -1)[:, :, :3]
    z = np.asarray(z, dtype=f32).reshape(R, N)
    K = lanes_K(N)
    P = 64 * K
    a = np.zeros((R, P), dtype=f32)
    a[:, :N] = alpha
    valid = (np.arange(P) < N)[None, :]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        f = (f32(1.0) - a) if wrong == "eps_dropped" else ((f32(1.0) - a) + f32(1e-10))
        f = np.where(valid, f, f32(1.0)).astype(f32)
        fd = f.astype(np.float64).reshape(R, 64, K)
        pl = np.empty((R, 64, K))
        run = np.ones((R, 64))
        for i in range(K):
            run = run * fd[:, :, i]
            pl[:, :, i] = run
        if wrong == "sequential_product":
            incl = np.empty((R, 64))
            acc = np.ones(R)
            for lane in range(64):
                acc = acc * run[:, lane]
                incl[:, lane] = acc
        else:
            incl = _scan_mul(run)
        excl = np.ones((R, 64))
        excl[:, 1:] = incl[:, :-1]
        Td = np.empty((R, 64, K))
        Td[:, :, 0] = excl
        for i in range(1, K):
            Td[:, :, i] = excl * pl[:, :, i - 1]
        if wrong == "T_inclusive":
            Td = excl[:, :, None] * pl
        T = Td.astype(f32).reshape(R, P)
        if wrong != "T_inclusive":
            T[:, 0] = 1.0
        w = (a * T).astype(f32)
        cols = np.zeros((R, P, 5), dtype=f32)                 # r, g, b, z, 1 per sample
        cols[:, :N, :3] = rgb
        cols[:, :N, 3] = z
        terms = np.empty((R, P, 5), dtype=f32)
        terms[:, :, :4] = w[:, :, None] * cols[:, :, :4]
        terms[:, :, 4] = w
        terms = np.where(valid[:, :, None], terms, f32(0.0)).astype(f32).reshape(R, 64, K, 5)
        sums = np.empty((R, 5), dtype=f32)
        for c in range(5):
            if wrong == "sequential_sum":
                acc = np.zeros(R, dtype=f32)
                flat = terms[:, :, :, c].reshape(R, P)
                for k in range(N):
                    acc = (acc + flat[:, k]).astype(f32)
                sums[:, c] = acc
                continue
            acc = np.zeros((R, 64), dtype=f32)
            for i in range(K):
                acc = (acc + terms[:, :, i, c]).astype(f32)
            sums[:, c] = _butterfly(acc)
        comp = sums[:, :3].copy()
        if (flags & WHITE) and wrong != "white_dropped":
            bg = (f32(1.0) - sums[:, 4]).astype(f32)
            comp = (comp + bg[:, None]).astype(f32)
    out = comp, sums[:, 3].copy(), sums[:, 4].copy(), np.ascontiguousarray(w[:, :N])
    assert all(o.dtype == f32 for o in out)
    return out


def composite_output_bounds(rgb, sigma, z, flags):
    """fp64 values and derived bounds of the four outputs: dict name -> (value, bound), by train_heads_ref's rules.
    weights: forward_bounds' (w, Ew).  A sum over the ray (colour c: terms fl(w c); depth: fl(w z); opacity: w): the terms' own
    bounds, plus one rounding per addition a term passes through -- at most K in its lane and 6 in the butterfly, each of a
    partial sum that the absolute sum of the terms bounds: (K + 6) u sum(|term| + E_term).  White: bg = fl(1 - opacity), then one
    more addition per channel."""
    sigma = np.asarray(sigma, dtype=np.float64)
    R, N = sigma.shape
    rgb = np.asarray(rgb, dtype=np.float64).reshape(R, N, -1)[:, :, :3]
    z = np.asarray(z, dtype=np.float64).reshape(R, N)
    fw = hr.forward_bounds(sigma, z, flags)
    w, Ew = fw["w"], fw["Ew"]
    depth_adds = lanes_K(N) + 6

    def total(v, E):
        return v.sum(1), E.sum(1) + depth_adds * hr.U * (np.abs(v) + E).sum(1) + hr.TINY

    out = {"weights": (w, Ew), "alpha": (fw["alpha"], fw["Ea"])}
    out["opacity"] = total(w, Ew)
    out["depth"] = total(*hr._mul(w, Ew, z, 0.0))
    comp, Ecomp = np.empty((R, 3)), np.empty((R, 3))
    for c in range(3):
        v, E = total(*hr._mul(w, Ew, rgb[:, :, c], 0.0))
        if flags & WHITE:
            bg, Ebg = hr._add(1.0, 0.0, -out["opacity"][0], out["opacity"][1])
            v, E = hr._add(v, E, bg, Ebg)
        comp[:, c], Ecomp[:, c] = v, E
    out["comp_rgb"] = (comp, Ecomp)
    return out


COMPOSITE_N = (1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 448, 511, 512)
COMPOSITE_R = (1, 4, 5, 9)
COMPOSITE_FLAGS = (0, WHITE, SOFTPLUS, WHITE | SOFTPLUS)


def composite_inputs(R, N):
    """composite_case(R, N) of train_heads_ref as (rgb4 (R, N, 4) with NaN in column 3, sigma (R, N), z (R, N))"""
    c = hr.composite_case(R, N) if N >= 2 else _one_sample_case(R)
    return c["rgb4"].reshape(R, N, 4), c["sigma"].reshape(R, N), c["z"].reshape(R, N)


def _one_sample_case(R):
    """N = 1 (composite_case plants at k = 1.. and needs N >= 2): one sample per ray, its density by the ray's kind"""
    rng = np.random.default_rng(10 * R + 1)
    sigma = np.array([1e-11, -0.0, 80.0, 0.0, 0.7], dtype=f32)[np.arange(R) % 5]
    rgb4 = np.full((R, 1, 4), np.nan, dtype=f32)
    rgb4[:, :, :3] = rng.uniform(0.02, 0.98, (R, 1, 3))
    return dict(rgb4=rgb4, sigma=sigma, z=(2.0 + rng.uniform(0, 1, (R, 1))).astype(f32))


PRODUCT_ORDER_SEED, PRODUCT_ORDER_BATCH, PRODUCT_ORDER_ROW = 295, 16384, 9761


def product_order_case():
    """One ray of 64 samples (K = 1) on which the ORDER of the fp64 transmittance product shows in fp32: the Hillis-Steele
    association and the sequential one differ in the last bits of a double, which moves T only where the product sits within
    ~2^-53 of a fp32 rounding boundary -- about one ray of 64 samples in a million.  Found by a search over batches of this
    generator with libm's exp supplying alpha (row PRODUCT_ORDER_ROW of the batch of seed PRODUCT_ORDER_SEED: T_40 differs);
    tests/test_ray_stages_cpu.py::test_composite_wrong_restatements_show holds it.  The device runs the same inputs, whatever
    its expf makes of them.  -> rgb4 (1, 64, 4), sigma (1, 64), z (1, 64)"""
    rng = np.random.default_rng(PRODUCT_ORDER_SEED)
    B, N, row = PRODUCT_ORDER_BATCH, 64, PRODUCT_ORDER_ROW
    z = (2.0 + np.cumsum(rng.uniform(0.2, 1.8, (B, N)) * (4.0 / N), 1)).astype(f32)[row:row + 1]
    sigma = rng.uniform(0.0, 1.5, (B, N)).astype(f32)[row:row + 1]
    rgb4 = np.full((1, N, 4), np.nan, dtype=f32)
    rgb4[:, :, :3] = np.random.default_rng(PRODUCT_ORDER_ROW).uniform(0.02, 0.98, (1, N, 3))
    return rgb4, np.ascontiguousarray(sigma), np.ascontiguousarray(z)


# ------------------------------------------------------------------------------------------------------------------------
# resampler
# ------------------------------------------------------------------------------------------------------------------------
def sums_are_exact(terms):
    """True when EVERY partial sum of these non-negative fp32 / fp64 numbers, in any order, is exact in fp64: all terms are
    multiples of one power of two 2^q, and their total stays below 2^(q + 53).  terms: (..., n), checked per leading index."""
    t = np.asarray(terms, dtype=np.float64)
    if not (np.isfinite(t).all() and (t >= 0).all()):
        return False
    pos = np.where(t > 0, t, 1.0)
    _, e = np.frexp(pos)                                       # pos = m 2^e, m in [0.5, 1): a 24-bit (fp32) or 53-bit m
    mant_bits = 24 if np.asarray(terms).dtype == np.float32 else 53
    q = np.where(t > 0, e - mant_bits, np.iinfo(np.int64).max).min(-1)      # every term is a multiple of 2^q
    total = t.sum(-1)                                          # within a factor (1 + n 2^-53) of the true total
    return bool((total * 1.0000001 < np.ldexp(1.0, q + 53)).all())


def resample_cdf(z, w, wrong=None):
    """bins (R, Nc - 1), cdf (R, Nc - 1) = [0, cumsum(pdf)] of resample_kernel, and whether both sums met sums_are_exact"""
    z, w = np.asarray(z, dtype=f32), np.asarray(w, dtype=f32)
    R, Nc = z.shape
    nb = Nc - 2
    bins = (f32(0.5) * (z[:, :-1] + z[:, 1:])).astype(f32)
    t = ((w[:, :-2] if wrong == "pdf_shifted" else w[:, 1:-1]) + EPS).astype(f32)
    if wrong == "normaliser_fp32":
        wsum = np.zeros(R, dtype=f32)
        for j in range(nb):
            wsum = (wsum + t[:, j]).astype(f32)
    else:
        wsum = t.astype(np.float64).sum(1).astype(f32)          # exact in fp64 (sums_are_exact), rounded once
    pdf = (t / wsum[:, None]).astype(f32)
    run = np.cumsum(pdf.astype(np.float64), 1)
    if wrong == "carry_dropped":
        for seg in range(64, nb, 64):
            run[:, seg:seg + 64] = np.cumsum(pdf[:, seg:seg + 64].astype(np.float64), 1)
    cdf = np.zeros((R, Nc - 1), dtype=f32)
    cdf[:, 1:] = run.astype(f32)
    return bins, cdf, sums_are_exact(t) and sums_are_exact(pdf)


def resample_numpy(z, w, Ni, u=None, rays=None, wrong=None, require_exact=True):
    """resample_kernel: z, w (R, Nc) fp32, u None (nsr_linspace01(j, Ni)) or (R, Ni) -> z_out (R, Nc + Ni) and, with rays
    (R, >= 8), pts (R, Nc + Ni, 3) else None.
      bins = fl(0.5 fl(z_k + z_k+1)); t = fl(w + 1e-5f) over w[:, 1:-1]; wsum = fp32(fp64 sum); pdf = fl(t / wsum);
      cdf = [0, fp32(fp64 prefix sums)]; lo = searchsorted(cdf[0 .. Nc-2], u, right); below = max(lo - 1, 0), above = min(lo, Nc - 2);
      denom = fl(cdf[above] - cdf[below]), < 1e-5f -> 1; z_new = fl(bb + fl(fl(fl(u - cb) / denom) fl(ba - bb)));
      stable merge of [z, z_new] (ties: position); pts = fl(o + fl(v d))."""
    assert wrong is None or wrong in RESAMPLE_WRONG
    z, w = np.asarray(z, dtype=f32), np.asarray(w, dtype=f32)
    R, Nc = z.shape
    nb = Nc - 2
    assert nb >= 1
    bins, cdf, exact = resample_cdf(z, w, wrong)
    assert exact or not require_exact, "a partial sum of the normaliser or of the cdf is not exact in fp64"
    if u is None:
        u = np.broadcast_to(linspace01(Ni)[None, :], (R, Ni))
    u = np.asarray(u, dtype=f32).reshape(R, Ni)
    side = "left" if wrong == "searchsorted_left" else "right"
    lo = np.stack([np.searchsorted(cdf[r], u[r], side=side) for r in range(R)])
    below, above = np.maximum(lo - 1, 0), np.minimum(lo, nb)
    cb, ca = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    bb, ba = np.take_along_axis(bins, below, 1), np.take_along_axis(bins, above, 1)
    denom = (ca - cb).astype(f32)
    denom = np.where((denom <= EPS) if wrong == "snap_le" else (denom < EPS), f32(1.0), denom).astype(f32)
    z_new = (bb + ((u - cb) / denom) * (ba - bb)).astype(f32)
    val = np.concatenate([z, z_new], 1)
    order = np.argsort(val, axis=1, kind="stable")
    z_out = np.take_along_axis(val, order, 1)
    pts = None
    if rays is not None:
        rays = np.asarray(rays, dtype=f32)
        pts = (rays[:, None, 0:3] + z_out[:, :, None] * rays[:, None, 3:6]).astype(f32)
    assert z_out.dtype == f32
    return z_out, pts


RESAMPLE_NC = (3, 4, 64, 65, 66, 67, 130, 256)
RESAMPLE_NI = (1, 2, 63, 64, 65, 256)
RESAMPLE_R = (1, 4, 5)
(RS_ZERO, RS_ONE_HOT, RS_HOT_FIRST, RS_HOT_LAST, RS_TINY, RS_TIES, RS_RANDOM, RS_PEAKED, RS_ON_SNAP) = range(9)
RS_KINDS = 9


def _on_snap_weight(nb):
    """x with fp32(sum of fl(x + 1e-5f) and nb - 1 terms 1e-5f) == 1: the zero-weight bins' pdf is then 1e-5f itself"""
    x = f32(1.0 - nb * 1e-5)
    for _ in range(64):
        total = f32(np.float64((x + EPS).astype(f32)) + (nb - 1) * np.float64(EPS))
        if total == f32(1.0):
            return x
        x = np.nextafter(x, f32(0.0) if total > 1 else f32(2.0))
    raise AssertionError(nb)


def resample_case(R, Nc, seed=0):
    """z, w (R, Nc) fp32, weights in [0, 1].  Ray r is of kind (r + seed) % 9:
      0 all-zero weights; 1 one-hot in the middle; 2 one-hot at the first interior bin (k = 1); 3 one-hot at the last (k = Nc - 2);
      4 every weight 1e-9; 5 repeated coarse depths (runs of equal z: zero-width bins, many ties) under random weights;
      6 random weights; 7 a compositor-like profile (a narrow peak over a floor of 2e-4);
      8 exactly ON the snap (Nc >= 4): one weight chosen so that the normaliser is 1.0f, every other interior weight 0, whose bins
        then have denom = fl(1e-5f / 1) = 1e-5f: not below the threshold, so not snapped.
    The outer weights k = 0 and k = Nc - 1, which the pdf must not read, are 1 / 0.75 on every ray."""
    rng = np.random.default_rng(1000 * Nc + 10 * R + seed)
    z = (2.0 + np.cumsum(rng.uniform(0.2, 1.8, (R, Nc)) * (4.0 / Nc), 1)).astype(f32)
    w = np.zeros((R, Nc), dtype=f32)
    for r in range(R):
        kind = (r + seed) % RS_KINDS
        if kind == RS_ONE_HOT:
            w[r, Nc // 2] = 1.0
        elif kind == RS_HOT_FIRST:
            w[r, 1] = 1.0
        elif kind == RS_HOT_LAST:
            w[r, Nc - 2] = 1.0
        elif kind == RS_TINY:
            w[r] = 1e-9
        elif kind == RS_TIES:
            z[r] = z[r, (np.arange(Nc) // 3) * 3]              # runs of three equal depths
            w[r] = rng.random(Nc) * 0.1
        elif kind == RS_RANDOM:
            w[r] = rng.random(Nc)
        elif kind == RS_PEAKED:
            c = rng.integers(0, Nc)
            w[r] = np.maximum(np.exp(-0.5 * ((np.arange(Nc) - c) / 1.5) ** 2) * 0.6, 2e-4)
        elif kind == RS_ON_SNAP and Nc >= 4:
            w[r, 2] = _on_snap_weight(Nc - 2)
        w[r, 0], w[r, Nc - 1] = 1.0, 0.75
    assert (w >= 0).all() and (w <= 1).all()
    return z, w


def resample_u(z, w, Ni, seed=0):
    """u (R, Ni) with the planted entries: 0, 1, values equal to cdf entries (the first, a middle and the last one), the
    fp32 just above the last cdf entry and 5e-6 (inside the first bin of the ray that sits on the snap); random elsewhere.  Slots are filled as far as Ni reaches, in that order, rotated by ray so
    that every kind of entry appears at Ni = 1 and 2 as well."""
    _, cdf, _ = resample_cdf(z, w)
    R, n = cdf.shape
    rng = np.random.default_rng(31 + Ni + 100 * n + seed)
    u = rng.random((R, Ni)).astype(f32)
    for r in range(R):
        last = cdf[r, -1]
        planted = [f32(0.0), f32(1.0), cdf[r, 1], f32(5e-6), cdf[r, n // 2], last, np.nextafter(last, f32(2.0))]
        k = (r + Ni) % len(planted)
        planted = planted[k:] + planted[:k]
        slots = rng.permutation(Ni)[:len(planted)]
        for s, v in zip(slots, planted):
            u[r, s] = v
    return u


# ------------------------------------------------------------------------------------------------------------------------
# s^2 mean and un-flatten
# ------------------------------------------------------------------------------------------------------------------------
def sr_mean_numpy(hr_, n_lr, s2, c):
    """sr_mean_kernel: left-to-right fp32 sum over the s2 rows of each LR pixel, one division by fl(s2)"""
    x = np.asarray(hr_, dtype=f32).reshape(n_lr, s2, c)
    acc = np.zeros((n_lr, c), dtype=f32)
    for k in range(s2):
        acc = (acc + x[:, k, :]).astype(f32)
    return (acc / f32(s2)).astype(f32)


def sr_mean_data(n_lr, s2, c, seed=0):
    """values of mixed sign over ten binades: any other summation order changes the rounded sum on most pixels"""
    rng = np.random.default_rng(3 + n_lr + 10 * s2 + c + seed)
    return (rng.standard_normal((n_lr * s2, c)) * np.exp2(rng.integers(-5, 5, (n_lr * s2, c)))).astype(f32)


def unflatten_numpy(x, H, W, s, c):
    """unflatten_kernel as an index permutation: out[py, px, ch] = x[((py // s) (W // s) + px // s) s^2 + (py % s) s + px % s, ch]"""
    x = np.asarray(x).reshape(-1, c)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    src = ((py // s) * (W // s) + px // s) * (s * s) + (py % s) * s + (px % s)
    return x[src.reshape(-1)].reshape(H, W, c)
