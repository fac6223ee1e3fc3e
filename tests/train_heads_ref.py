"""Reference, error model, fp32 emulation and test inputs of the unit layer over what feeds the network's backward
(csrc/nsr_train.hip: composite_bwd_kernel, lr_loss_kernel, loss_finish_kernel, sigma_noise_kernel, gamma_points_kernel).
Plain numpy fp64 over the fp32 inputs as given.  Pinned on the CPU by tests/test_train_heads_cpu.py (against torch.autograd in
float64 and against an fp32 emulation of the kernel's arithmetic); used on the device by tests/test_gpu_train_heads.py.
"""
import numpy as np

WHITE, SOFTPLUS, GAMMA, COLOR_NONE = 1, 2, 4, 8       # NSR_WHITE_BKGD, NSR_SIGMA_SOFTPLUS, NSR_TRAIN_GAMMA_CORRECT, NSR_TRAIN_COLOR_NONE
U = 2.0 ** -24                                        # unit roundoff of fp32
TINY = 2.0 ** -149                                    # smallest fp32 denormal: absolute error of an operation that underflows
# what the project grants one expf / logf / powf call (tests/test_gpu_gemm_units.py::derived_bound): ulps of the function value
TRANSCENDENTAL_ULPS = 4
F_EPS = 1e-10                                         # the reference's 1e-10 in f = 1 - alpha + 1e-10
LAST_DELTA = 1e10
DOUBLE_OPS_SLACK = 2.0 ** -53                         # one fp64 rounding

WRONG = ("suffix_inclusive", "T_inclusive", "last_delta_from_z", "mask_ge", "white_dropped")


def ulp32(v):
    """ulp of fp32 at |v| (v fp64): 2^(e - 24) with |v| in [2^(e-1), 2^e), 2^-149 below the normal range"""
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** -126))
    return np.ldexp(1.0, e - 24)


def _rays(rgb4, sigma, z, g_comp):
    g_comp = np.asarray(g_comp, dtype=np.float64).reshape(-1, 3)
    R = g_comp.shape[0]
    sigma = np.asarray(sigma, dtype=np.float64).reshape(R, -1)
    N = sigma.shape[1]
    return (R, N, np.asarray(rgb4, dtype=np.float64).reshape(R, N, -1)[:, :, :3], sigma, np.asarray(z, dtype=np.float64).reshape(R, N),
            g_comp)


def _opt(a, shape):
    return None if a is None else np.asarray(a, dtype=np.float64).reshape(shape)


def head_of(flags):
    return 1 if flags & GAMMA else (2 if flags & COLOR_NONE else 0)


def ref_composite_bwd(rgb4, sigma, z, g_comp, flags, g_depth=None, g_opacity=None, g_weights=None, *, wrong=None):
    """d4 (P, 4) = (d rgb_pre 0..2, d sigma) and bias_part (R, 4) = its sums per ray, fp64.

    The operation as csrc/nsr_train.hip states it: delta_k = z_{k+1} - z_k, delta_{N-1} = 1e10; density relu(sigma) or
    log(1 + exp(sigma - 1)); e_k = exp(-delta_k density_k), alpha_k = 1 - e_k, f_k = 1 - alpha_k + 1e-10 (evaluated as
    e_k + 1e-10, the same number without fp64's cancellation at alpha -> 1), T_k = prod_{j<k} f_j, w_k = alpha_k T_k;
      gw_k = g_comp . rgb_k - [white] sum(g_comp) + g_depth z_k + g_opacity + g_weights_k
      dL/dalpha_k = gw_k T_k - (sum_{i>k} gw_i w_i) / f_k
      dL/dsigma_k = dL/dalpha_k delta_k e_k m_k, m = [sigma > 0] or sigmoid(sigma - 1);   dL/drgb_k = g_comp w_k
    and through the colour head from the colour y it produced: y (1 - y) (sigmoid), y (1 - y^2.2) / 2.2 (gamma-corrected
    sigmoid), 1 (none).  `wrong`: one of WRONG, the deliberately wrong variants of the teeth tests."""
    assert wrong is None or wrong in WRONG
    R, N, rgb, sigma, z, g_comp = _rays(rgb4, sigma, z, g_comp)
    delta = np.empty((R, N))
    delta[:, :-1] = z[:, 1:] - z[:, :-1]
    delta[:, -1] = (z[:, -1] - z[:, -2]) if wrong == "last_delta_from_z" else LAST_DELTA
    soft = bool(flags & SOFTPLUS)
    dens = np.log1p(np.exp(sigma - 1.0)) if soft else np.maximum(sigma, 0.0)
    e = np.exp(-delta * dens)
    alpha = -np.expm1(-delta * dens)
    f = e + F_EPS
    T = np.ones((R, N))
    for k in range(1, N):
        T[:, k] = T[:, k - 1] * f[:, k - 1]
    if wrong == "T_inclusive":
        T = T * f
    w = alpha * T
    gw = rgb @ g_comp[:, :, None]
    gw = gw[:, :, 0]
    if (flags & WHITE) and wrong != "white_dropped":
        gw = gw - g_comp.sum(1)[:, None]
    g_depth, g_opacity, g_weights = _opt(g_depth, (R,)), _opt(g_opacity, (R,)), _opt(g_weights, (R, N))
    if g_depth is not None:
        gw = gw + g_depth[:, None] * z
    if g_opacity is not None:
        gw = gw + g_opacity[:, None]
    if g_weights is not None:
        gw = gw + g_weights
    gww = gw * w
    suffix = np.zeros((R, N))
    for k in range(N - 2, -1, -1):
        suffix[:, k] = suffix[:, k + 1] + gww[:, k + 1]
    if wrong == "suffix_inclusive":
        suffix = suffix + gww
    d_alpha = gw * T - suffix / f
    if soft:
        mask = 1.0 / (1.0 + np.exp(1.0 - sigma))
    else:
        mask = ((sigma >= 0.0) if wrong == "mask_ge" else (sigma > 0.0)).astype(np.float64)
    d_sigma = d_alpha * delta * e * mask
    d_rgb = g_comp[:, None, :] * w[:, :, None]
    head = head_of(flags)
    if head == 0:
        d_rgb = d_rgb * rgb * (1.0 - rgb)
    elif head == 1:
        d_rgb = d_rgb * rgb * (1.0 - rgb ** 2.2) / 2.2
    d4 = np.concatenate([d_rgb, d_sigma[:, :, None]], 2)
    return d4.reshape(R * N, 4), d4.sum(1)


# ------------------------------------------------------------------------------------------------------------------------
# error model
# ------------------------------------------------------------------------------------------------------------------------
def _rnd(v, E):
    """error bound after ONE fp32 rounding of a result whose unrounded value is within E of v"""
    return E + U * (np.abs(v) + E) + TINY


def _mul(a, Ea, b, Eb):
    """(value, error bound) of one rounded fp32 product of two quantities known to Ea, Eb"""
    return a * b, _rnd(a * b, np.abs(a) * Eb + np.abs(b) * Ea + Ea * Eb)


def _add(a, Ea, b, Eb):
    return a + b, _rnd(a + b, Ea + Eb)


def _exp_neg(x, Ex):
    """expf(-x^) for x^ within Ex of x >= 0: the argument's error moves the value inside [exp(-x - Ex), exp(-x + Ex)] (no
    overflow whatever Ex), the call itself is granted TRANSCENDENTAL_ULPS ulps of its value"""
    v = np.exp(-x)
    hi, lo = np.exp(-np.maximum(x - Ex, 0.0)), np.exp(-(x + Ex))
    E = np.maximum(hi - v, v - lo)
    return v, E + TRANSCENDENTAL_ULPS * ulp32(v + E)


def _exp(t, Et):
    v = np.exp(t)
    E = v * np.expm1(Et)
    return v, E + TRANSCENDENTAL_ULPS * ulp32(v + E)


def forward_bounds(sigma, z, flags):
    """The forward part of error_bounds on its own (sigma, z: (R, N), the fp32 inputs as given): every intermediate of the
    compositing forward as (fp64 value, bound on a correct fp32 implementation's distance from it), by the rules error_bounds
    states, in the kernels' order (csrc/nsr_composite.h states the same chain as csrc/nsr_train.hip):
      delta, E_delta; x = delta density, Ex; e = exp(-x), Ee; alpha, Ea; f, Ef, f_lo; T, ET; w = alpha T, Ew.
    Shared by error_bounds below and by the forward compositor's unit tests (tests/ray_stages_ref.py)."""
    sigma, z = np.asarray(sigma, dtype=np.float64), np.asarray(z, dtype=np.float64)
    R, N = sigma.shape
    soft = bool(flags & SOFTPLUS)
    zero = np.zeros((R, N))
    delta = np.empty((R, N))
    delta[:, :-1] = z[:, 1:] - z[:, :-1]
    delta[:, -1] = LAST_DELTA
    E_delta = U * np.abs(delta) + TINY
    E_delta[:, -1] = 0.0
    if soft:
        t, Et = sigma - 1.0, U * np.abs(sigma - 1.0)
        v1, E1 = _exp(t, Et)
        p, Ep = _add(1.0, 0.0, v1, E1)
        dens = np.log1p(v1)
        E_dens = Ep / (p - Ep)
        E_dens = E_dens + TRANSCENDENTAL_ULPS * ulp32(dens + E_dens)
    else:
        dens, E_dens = np.maximum(sigma, 0.0), zero
    x, Ex = _mul(delta, E_delta, dens, E_dens)
    e, Ee = _exp_neg(x, Ex)
    alpha = -np.expm1(-x)
    Ea = _rnd(alpha, Ee)
    E_s1 = _rnd(e, Ea)
    f = e + F_EPS
    Ef = _rnd(f, E_s1 + U * F_EPS)
    f_lo = np.maximum(f - Ef, F_EPS * (1.0 - 2.0 * U))
    # T: fp64 product of the fp32 factors, rounded once
    Td, E_Td = np.ones((R, N)), np.zeros((R, N))
    for k in range(1, N):
        a, Ea_, b, Eb_ = Td[:, k - 1], E_Td[:, k - 1], f[:, k - 1], Ef[:, k - 1]
        Td[:, k] = a * b
        E_Td[:, k] = a * Eb_ + b * Ea_ + Ea_ * Eb_ + 2.0 * DOUBLE_OPS_SLACK * a * b
    T, ET = Td, _rnd(Td, E_Td)
    ET[:, 0] = 0.0
    w, Ew = _mul(alpha, Ea, T, ET)
    return dict(delta=delta, E_delta=E_delta, dens=dens, E_dens=E_dens, x=x, Ex=Ex, e=e, Ee=Ee, alpha=alpha, Ea=Ea, f=f, Ef=Ef,
                f_lo=f_lo, T=T, ET=ET, w=w, Ew=Ew)


def error_bounds(rgb4, sigma, z, g_comp, flags, g_depth=None, g_opacity=None, g_weights=None):
    """Elementwise bounds (P, 4) on |d4 of composite_bwd_kernel - ref_composite_bwd|, and (R, 4) on bias_part.  Derived, not
    fitted: a running error analysis of the arithmetic csrc/nsr_train.hip states, carried out on the reference's own values.

    Every intermediate carries (value v, bound E >= |v^ - v|) where v^ is what a correct fp32 implementation holds.  Rules,
    u = 2^-24:
      one fp32 operation on operands known to Ea, Eb: the exact operation's propagated error (product: |a| Eb + |b| Ea + Ea Eb;
        sum: Ea + Eb) and then one rounding, u (|v| + E) (+ 2^-149 should it underflow);
      expf / logf / powf: the argument's error through the function, plus TRANSCENDENTAL_ULPS ulps of the function value;
      the inputs (rgb, sigma, z, upstream gradients) are exact: both sides read the same fp32 numbers.
    Applied in the kernel's order:
      delta = fl(z' - z) (exact 1e10 at the last sample); density = relu (exact) or logf(fl(1 + expf(fl(sigma - 1))));
      x = fl(delta density); e = expf(-x); alpha = fl(1 - e);  f = fl(fl(1 - alpha) + 1e-10).
        The roundings of alpha and f ARE the absorption of e < 2^-24 and of 1e-10: up to u ABSOLUTE each, however small f
        itself is (delta sigma ~ 20: f^ = 1e-10, f = 2.2e-9).  Everything below therefore carries absolute errors.
      T_k = fl(prod_{j<k} f_j), the product held in fp64: product rule per factor, one fp32 rounding at the end;
      w = fl(alpha T);  gw = the fp32 sum, term by term, of the three rounded products, the white term, g_depth z, g_opacity,
        g_weights (3 to 6 terms, one rounding per addition);
      dL/dalpha = fl32(gw T - S / f), S = sum_{i>k} gw_i w_i in fp64.  S and f are NOT treated as independent: every w_i of the
        suffix holds f_k as a factor of its T_i, so S / f_k = sum_{i>k} gw_i alpha_i Q_ki (1 + d)(1 + d'), Q_ki = prod_{j<i,
        j != k} f_j, |d|, |d'| <= u (the roundings of T_i and w_i) -- the same f^_k cancels exactly.  Q's error follows the
        product rule over its own factors.  What does NOT cancel is the fp64 rounding of the kernel's S = total - prefix
        (absolute, (N + 16) 2^-53 sum |gw w|), which is divided by f^_k >= max(f_k - E_f, 1e-10 (1 - 2u)).
      d sigma = fl(fl(dL/dalpha delta) e) [x the mask: exact under relu; under softplus fl(1 / fl(1 + expf(fl(1 - sigma)))), one
        more expf, and a correctly rounded division];
      d rgb_pre = fl(g_comp w) through the head: fl(fl(g y) fl(1 - y)), or with powf(y, 2.2f) (its exponent is 2.2 (1 + d):
        relative 2.2 u |ln y| more) and the constant 1 / 2.2f (relative 2 u).
    bias_part: the sum of its points' bounds plus N fp32 additions of values bounded by |ref| + bound.
    Nothing measured on a device enters."""
    R, N, rgb, sigma, z, g_comp = _rays(rgb4, sigma, z, g_comp)
    g_depth, g_opacity, g_weights = _opt(g_depth, (R,)), _opt(g_opacity, (R,)), _opt(g_weights, (R, N))
    soft = bool(flags & SOFTPLUS)
    fw = forward_bounds(sigma, z, flags)
    delta, E_delta, e, Ee, alpha, Ea, f, Ef, f_lo = (fw[k] for k in ("delta", "E_delta", "e", "Ee", "alpha", "Ea", "f", "Ef", "f_lo"))
    T, ET, w, Ew = fw["T"], fw["ET"], fw["w"], fw["Ew"]
    # gw
    gw, Egw = _mul(g_comp[:, None, 0], 0.0, rgb[:, :, 0], 0.0)
    for c in (1, 2):
        pc, Epc = _mul(g_comp[:, None, c], 0.0, rgb[:, :, c], 0.0)
        gw, Egw = _add(gw, Egw, pc, Epc)
    if flags & WHITE:
        wt, Ewt = _add(g_comp[:, 0], 0.0, g_comp[:, 1], 0.0)
        wt, Ewt = _add(wt, Ewt, g_comp[:, 2], 0.0)
        gw, Egw = _add(gw, Egw, -wt[:, None], Ewt[:, None])
    else:
        gw, Egw = _add(gw, Egw, 0.0, 0.0)                         # the kernel subtracts its 0.0f all the same: exact, bounded anyway
    if g_depth is not None:
        pz, Epz = _mul(g_depth[:, None], 0.0, z, 0.0)
        gw, Egw = _add(gw, Egw, pz, Epz)
    if g_opacity is not None:
        gw, Egw = _add(gw, Egw, g_opacity[:, None], 0.0)
    if g_weights is not None:
        gw, Egw = _add(gw, Egw, g_weights, 0.0)
    # dL/dalpha = gw T - sum_{i>k} gw_i alpha_i Q_ki
    A = gw * T
    EA = np.abs(gw) * ET + np.abs(T) * Egw + ET * Egw
    ga, Ega = gw * alpha, np.abs(gw) * Ea + np.abs(alpha) * Egw + Ea * Egw          # exact product of the two held values
    Q, EQ = np.ones((R, N)), np.zeros((R, N))                                        # per k: Q_ki at the running i
    B, EB = np.zeros((R, N)), np.zeros((R, N))
    ks = np.arange(N)
    for i in range(N):
        live = (ks < i)[None, :]                                                     # samples k < i take sample i into their suffix
        v = ga[:, i:i + 1] * Q
        Ev = np.abs(ga[:, i:i + 1]) * EQ + Q * Ega[:, i:i + 1] + EQ * Ega[:, i:i + 1]
        Ev = Ev + (2.0 * U + U * U) * (np.abs(v) + Ev) + 2.0 * TINY / f_lo
        B = B + np.where(live, v, 0.0)
        EB = EB + np.where(live, Ev, 0.0)
        # Q_k,i+1 = Q_ki f_i for every k but k == i
        fi, Efi = f[:, i:i + 1], Ef[:, i:i + 1]
        step = (ks != i)[None, :]
        EQ = np.where(step, Q * Efi + fi * EQ + EQ * Efi + 2.0 * DOUBLE_OPS_SLACK * Q * fi, EQ)
        Q = np.where(step, Q * fi, Q)
    gww_abs = (np.abs(gw) + Egw) * (np.abs(w) + Ew)
    cancel = (N + 16) * DOUBLE_OPS_SLACK * gww_abs.sum(1, keepdims=True) / f_lo
    d_alpha = A - B
    E_da = _rnd(d_alpha, EA + EB + cancel)
    # d sigma
    v, Ev = _mul(d_alpha, E_da, delta, E_delta)
    v, Ev = _mul(v, Ev, e, Ee)
    if soft:
        t, Et = 1.0 - sigma, U * np.abs(1.0 - sigma)
        v1, E1 = _exp(t, Et)
        q, Eq = _add(1.0, 0.0, v1, E1)
        sg = 1.0 / q
        Esg = _rnd(sg, Eq / (q * (q - Eq)))
        v, Ev = _mul(v, Ev, sg, Esg)
    else:
        Ev = np.where(sigma > 0.0, Ev, 0.0)                       # a masked sample stores the constant 0
    bound = np.empty((R, N, 4))
    bound[:, :, 3] = Ev
    # d rgb_pre
    head = head_of(flags)
    for c in range(3):
        y = rgb[:, :, c]
        g, Eg = _mul(g_comp[:, None, c], 0.0, w, Ew)
        if head == 0:
            g, Eg = _mul(g, Eg, y, 0.0)
            g, Eg = _mul(g, Eg, 1.0 - y, U * np.abs(1.0 - y))
        elif head == 1:
            g, Eg = _mul(g, Eg, y, 0.0)
            pw = y ** 2.2
            Epw = pw * 2.2 * U * np.abs(np.log(np.maximum(y, 1e-300)))
            Epw = Epw + TRANSCENDENTAL_ULPS * ulp32(pw + Epw)
            g, Eg = _mul(g, Eg, 1.0 - pw, _rnd(1.0 - pw, Epw))
            g, Eg = _mul(g, Eg, 1.0 / 2.2, 2.0 * U / 2.2)
        bound[:, :, c] = Eg
    ref = ref_composite_bwd(rgb4, sigma, z, g_comp, flags, g_depth, g_opacity, g_weights)[0].reshape(R, N, 4)
    bias = bound.sum(1) + N * U * (np.abs(ref) + bound).sum(1)
    return bound.reshape(R * N, 4), bias


# ------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernel's arithmetic (CPU check that the bound is reachable by a correct implementation)
# ------------------------------------------------------------------------------------------------------------------------
f32 = np.float32


def _expf(x):
    """libm exp rounded to fp32"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(x.astype(np.float64)).astype(f32)


def emulate_composite_bwd(rgb4, sigma, z, g_comp, flags, g_depth=None, g_opacity=None, g_weights=None):
    """composite_bwd_kernel operation by operation in np.float32 (fp64 where the kernel holds fp64), vectorised over the rays
    instead of spread over lanes -> d4 (P, 4) fp32"""
    g_comp = np.asarray(g_comp, dtype=f32).reshape(-1, 3)
    R = g_comp.shape[0]
    sigma = np.asarray(sigma, dtype=f32).reshape(R, -1)
    N = sigma.shape[1]
    rgb, z = np.asarray(rgb4, dtype=f32).reshape(R, N, -1), np.asarray(z, dtype=f32).reshape(R, N)
    soft = bool(flags & SOFTPLUS)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        delta = np.full((R, N), 1e10, dtype=f32)
        delta[:, :-1] = z[:, 1:] - z[:, :-1]
        dens = np.log((f32(1.0) + _expf(sigma - f32(1.0))).astype(np.float64)).astype(f32) if soft else np.maximum(sigma, f32(0.0))
        e = _expf(-delta * dens)
        alpha = f32(1.0) - e
        f = (f32(1.0) - alpha) + f32(1e-10)
        Td = np.ones((R, N))
        for k in range(1, N):
            Td[:, k] = Td[:, k - 1] * f[:, k - 1].astype(np.float64)
        T = Td.astype(f32)
        w = alpha * T
        gc = [g_comp[:, None, c] for c in range(3)]
        white_term = ((gc[0] + gc[1]) + gc[2]) if flags & WHITE else f32(0.0)
        gw = ((gc[0] * rgb[:, :, 0] + gc[1] * rgb[:, :, 1]) + gc[2] * rgb[:, :, 2]) - white_term
        if g_depth is not None:
            gw = gw + np.asarray(g_depth, dtype=f32).reshape(R, 1) * z
        if g_opacity is not None:
            gw = gw + np.asarray(g_opacity, dtype=f32).reshape(R, 1)
        if g_weights is not None:
            gw = gw + np.asarray(g_weights, dtype=f32).reshape(R, N)
        gww = gw.astype(np.float64) * w.astype(np.float64)
        pre = np.cumsum(gww, 1)
        suffix = pre[:, -1:] - pre
        d_alpha = (gw.astype(np.float64) * T.astype(np.float64) - suffix / f.astype(np.float64)).astype(f32)
        if soft:
            d_sigma = d_alpha * delta * e * (f32(1.0) / (f32(1.0) + _expf(f32(1.0) - sigma)))
        else:
            d_sigma = np.where(sigma > 0, d_alpha * delta * e, f32(0.0))
        head = head_of(flags)
        out = np.empty((R, N, 4), dtype=f32)
        for c in range(3):
            g, y = gc[c] * w, rgb[:, :, c]
            if head == 0:
                g = g * y * (f32(1.0) - y)
            elif head == 1:
                pw = np.power(y.astype(np.float64), float(f32(2.2))).astype(f32)
                g = g * y * (f32(1.0) - pw) * (f32(1.0) / f32(2.2))
            out[:, :, c] = g
        out[:, :, 3] = d_sigma
    assert out.dtype == f32
    return out.reshape(R * N, 4)


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
RAY_PLAIN_LAST_TINY, RAY_TRANSPARENT, RAY_OPAQUE_AT_0, RAY_OPAQUE_MID = 0, 1, 2, 3       # ray r of a case is of kind r % 5 (4: random)


def ray_kind(r):
    return r % 5


def composite_case(R, N, seed=0):
    """fp32 inputs of R rays x N samples with the planted samples.  Ray r is of kind r % 5:
      0  no opaque sample: sigma < 0 at k = 1, +0 at k = 2, -0 at k = 3 (where these are not the last sample), and a LAST sample
         with sigma = 1e-11: delta = 1e10 makes delta sigma = 0.1, e = 0.905, d sigma of order 1e10 dL/dalpha
      1  all transparent: every sigma <= 0 (negative, +0 and -0 mixed)
      2  opaque at k = 0: sigma_0 = 80 across a gap of 2.0 in z (delta sigma = 160 > 104: e = 0 in fp32, f = 1e-10)
      3  sigma < 0 / +0 / -0 as kind 0, delta sigma = 20 at k = N / 2 (sigma = 40 across a gap of 0.5: e = 2e-9 < 2^-24 is
         absorbed into alpha = 1, f^ = 1e-10 against f = 2.2e-9), two opaque samples in a row at k = 3 N / 4 and the next one,
         and a LAST sample with sigma = -0.5   (N >= 12; below that only the last sample is planted)
      4  random, a quarter of the densities negative
    The planted densities stay below 89 so that the softplus option's expf(sigma - 1) is finite: the same inputs serve both
    density modes.  z: strictly increasing from 2, uneven steps.  Column 3 of rgb4 is NaN: the kernel must not read it.
    -> dict of fp32 arrays: rgb4 (P, 4), sigma (P,), z (P,), g_comp (R, 3), g_depth (R,), g_opacity (R,), g_weights (R, N)"""
    rng = np.random.default_rng(1000 * N + 10 * R + seed)
    steps = rng.uniform(0.2, 1.8, (R, N)) * (4.0 / N)
    sigma = rng.uniform(0.0, 1.5, (R, N))
    neg = rng.random((R, N)) < 0.25
    sigma[neg] = -rng.uniform(0.1, 2.0, (R, N))[neg]
    for r in range(R):
        kind = ray_kind(r)
        if kind in (RAY_PLAIN_LAST_TINY, RAY_OPAQUE_MID):
            for k, v in ((1, -0.75), (2, 0.0), (3, -0.0)):
                if k < N - 1:
                    sigma[r, k] = v
            sigma[r, 0] = 0.9
            sigma[r, N - 1] = 1e-11 if kind == RAY_PLAIN_LAST_TINY else -0.5
            if kind == RAY_OPAQUE_MID and N >= 12:
                k20, kop = N // 2, (3 * N) // 4
                sigma[r, k20], steps[r, k20 + 1] = 40.0, 0.5
                sigma[r, kop], steps[r, kop + 1] = 80.0, 2.0
                sigma[r, kop + 1], steps[r, kop + 2] = 80.0, 2.0
        elif kind == RAY_TRANSPARENT:
            sigma[r] = -np.abs(sigma[r])
            sigma[r, ::3] = 0.0
            sigma[r, 1::3] = -0.0
        elif kind == RAY_OPAQUE_AT_0:
            sigma[r, 0], steps[r, 1] = 80.0, 2.0
    z = (2.0 + np.cumsum(steps, 1)).astype(f32)
    assert (np.diff(z, axis=1) > 0).all()
    rgb4 = np.full((R, N, 4), np.nan, dtype=f32)
    rgb4[:, :, :3] = rng.uniform(0.02, 0.98, (R, N, 3))
    return dict(rgb4=rgb4.reshape(R * N, 4), sigma=sigma.astype(f32).reshape(R * N), z=z.reshape(R * N),
                g_comp=rng.standard_normal((R, 3)).astype(f32), g_depth=(0.3 * rng.standard_normal(R)).astype(f32),
                g_opacity=rng.standard_normal(R).astype(f32), g_weights=rng.standard_normal((R, N)).astype(f32))


# the shapes of the unit layer: every K = 1..4 (N <= 64 K) at its first, a middle and its last N; R: a part-filled block of 4
# waves, a full one, three blocks
ALL_N = (2, 3, 63, 64, 65, 100, 128, 129, 192, 193, 255, 256)
SHAPES = [(5, N) for N in ALL_N] + [(R, N) for R in (1, 3, 4, 9) for N in (65, 193)]
FLAG_SETS = (0, WHITE, SOFTPLUS, GAMMA, COLOR_NONE, WHITE | SOFTPLUS, WHITE | GAMMA, WHITE | COLOR_NONE)
# upstream-gradient subsets: names of the case's arrays passed non-null.  g_opacity / g_weights select the FULL instantiation
UPSTREAM_PLAIN = ((), ("g_depth",))
UPSTREAM_FULL = (("g_opacity",), ("g_weights",), ("g_opacity", "g_weights"), ("g_depth", "g_opacity", "g_weights"))


def option_sets():
    """(flags, upstream subset) of the real-valued cases: every flag set without and with g_depth; the FULL instantiation's
    four subsets under the plain options and under the white + gamma pair, and one of them under every other flag set"""
    out = [(fl, up) for fl in FLAG_SETS for up in UPSTREAM_PLAIN]
    out += [(fl, up) for fl in (0, WHITE | GAMMA) for up in UPSTREAM_FULL]
    out += [(fl, UPSTREAM_FULL[i % 4]) for i, fl in enumerate(FLAG_SETS) if fl not in (0, WHITE | GAMMA)]
    return out


def upstream(case, names):
    return {n: (case[n] if n in names else None) for n in ("g_depth", "g_opacity", "g_weights")}


def flag_name(flags):
    return "+".join(n for b, n in ((WHITE, "white"), (SOFTPLUS, "softplus"), (GAMMA, "gamma"), (COLOR_NONE, "none")) if flags & b) or "plain"


# ------------------------------------------------------------------------------------------------------------------------
# loss head
# ------------------------------------------------------------------------------------------------------------------------
def block_tree(v):
    """lr_loss_kernel's / loss_finish_kernel's reduction of 256 per-thread values per block (v: (nblk, 256) fp64): partner at
    distance 128, 64, .., 1"""
    v = np.array(v, dtype=np.float64)
    o = 128
    while o:
        v[:, :o] = v[:, :o] + v[:, o:2 * o]
        o >>= 1
    return v[:, 0].copy()


def ref_lr_loss(comp, target, s2, scale, lam, lam_var, lam_dvar, far, depth):
    """lr (n_lr, 3), g_comp (n_lr s2, 3), g_depth (n_lr s2,) or None (depth None), block_sums (3, nblk): squared errors, colour
    variances, depth variances per block of 256 LR pixels.

    fp64 in the kernel's operation order.  With float32 inputs the three steps the kernel makes in fp32 are made in fp32 (they
    define the operation: the mean is the fp32 left-to-right sum and one division, the residual one fp32 subtraction,
    depth / far one fp32 division, and the colour gradient is the fp32 sum of its two rounded parts when lam_var != 0), so that
    the results are the kernel's bit for bit; with float64 inputs everything is fp64 (the CPU file's comparison with autograd).
    lam, lam_var, lam_dvar, far, scale: python floats holding the fp32 / fp64 values the kernel receives."""
    comp = np.asarray(comp)
    single = comp.dtype == np.float32
    ft = f32 if single else np.float64
    rnd = (lambda a: np.asarray(a, dtype=np.float64).astype(f32).astype(np.float64)) if single else (lambda a: a)
    comp = comp.reshape(-1, s2, 3)
    n_lr = comp.shape[0]
    target = np.asarray(target, dtype=ft).reshape(n_lr, 3)
    acc = np.zeros((n_lr, 3), dtype=ft)
    for k in range(s2):
        acc = acc + comp[:, k, :]
    lr = acc / ft(s2)
    d = (lr - target).astype(np.float64)
    sq = np.zeros(n_lr)
    for c in range(3):
        sq = sq + d[:, c] * d[:, c]
    gc = rnd(2.0 * lam * d * scale / float(s2))
    g_comp = np.empty((n_lr, s2, 3))
    var_rgb = np.zeros(n_lr)
    if lam_var != 0.0:
        for c in range(3):
            ss = np.zeros(n_lr)
            for k in range(s2):
                e = comp[:, k, c].astype(np.float64) - lr[:, c].astype(np.float64)
                ss = ss + e * e
                part = rnd(2.0 * lam_var * e / float(s2 - 1))
                g_comp[:, k, c] = rnd(gc[:, c] + part)
            var_rgb = var_rgb + ss / float(s2 - 1)
    else:
        g_comp[:] = gc[:, None, :]
    g_depth, var_d = None, np.zeros(n_lr)
    if depth is not None:
        g_depth = np.zeros((n_lr, s2))
        if lam_dvar != 0.0:
            dn = (np.asarray(depth, dtype=ft).reshape(n_lr, s2) / ft(far)).astype(np.float64)
            m = np.zeros(n_lr)
            for k in range(s2):
                m = m + dn[:, k]
            m = m / float(s2)
            ss = np.zeros(n_lr)
            for k in range(s2):
                e = dn[:, k] - m
                ss = ss + e * e
                g_depth[:, k] = rnd(2.0 * lam_dvar * e / (float(s2 - 1) * far))
            var_d = ss / float(s2 - 1)
        g_depth = g_depth.reshape(-1)
    nblk = (n_lr + 255) // 256
    sums = np.zeros((3, nblk * 256))
    sums[0, :n_lr], sums[1, :n_lr], sums[2, :n_lr] = sq, var_rgb, var_d
    block_sums = np.stack([block_tree(s.reshape(nblk, 256)) for s in sums])
    return lr.astype(np.float64), g_comp.reshape(-1, 3), g_depth, block_sums


def ref_loss_finish(block_sums, n, scale, lam, slot, carry, lam_var, lam_dvar):
    """-> (carry after the call (6 fp64 words, a copy), losses[slot] as fp32, (var_losses[slot], var_losses[2 + slot]) as fp32).
    block_sums: the 3 n fp64 words at layout [q n + block]; thread t sums blocks t, t + 256, .. in order, then the tree."""
    block_sums = np.asarray(block_sums, dtype=np.float64).reshape(3, n)
    carry = np.array(carry, dtype=np.float64)
    tot = []
    for q in range(3):
        per_thread = np.zeros(256)
        for i in range(n):
            per_thread[i % 256] = per_thread[i % 256] + block_sums[q, i]
        tot.append(block_tree(per_thread[None, :])[0])
    carry[slot] += tot[0]
    carry[2 + slot] += tot[1]
    carry[4 + slot] += tot[2]
    return carry, f32(lam * carry[slot] * scale), (f32(lam_var * carry[2 + slot]), f32(lam_dvar * carry[4 + slot]))
