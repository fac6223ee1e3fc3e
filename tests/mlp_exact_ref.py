"""Exact-input cases for the default 8 x 256 network's inference kernels, and their reference (numpy only, no device).

Every case is a 24-tensor state_dict plus (P, 90) input rows whose operands and partial sums are all exactly representable
in the precision under test, so that a kernel must return the exact result in every bit (tests/test_gpu_mlp_exact.py); the
cases themselves are checked on the CPU (tests/test_mlp_exact_cpu.py).

Numbers.  Every tensor and every activation is an int64 array ``n`` with one power-of-two exponent ``e``: value = n * 2^e
("dyadic"; e = 0 for the integer cases).  The reference (``forward``) runs the network in that arithmetic, following the
contract of ``oracle.nerf_oracle.mlp_forward`` (colour activation "none") without sharing code with it.

Families.
  A  the whole network sparse: m nonzero weights (+-1) per row at seed-dependent positions, small integer biases and
     inputs.  Sees routing between layers, the skip concatenation, block order, the re-split between layers, signs and
     bias rows.  Sparse: it does not touch every element of a tensor.
  B  one tensor T (and its bias) dense with nonzero small integers; every other trunk layer a non-negative routing layer
     that keeps T's inputs and outputs observable, both heads dense +-1.  Sees every single element of T.  ``observability``
     measures that on the CPU.
  C  one tensor T (and its bias) "wide": dense odd n * 2^-12 with |n| < 2^12, values that need both halves of the split-fp16
     operand pair, on inputs of at most 11 significant bits, every other layer routing.  Sees a lost a_hi * w_lo term or a
     truncated bias (fp32 and f16x3 only: the single-16-bit formats cannot carry such a weight).
  Ray cases are A and B restricted to what the in-kernel encoding makes exact: see ``ray_case``.

Preconditions (``precondition``), one function per precision, written from the operand formats documented in include/nsr.h
and the headers of csrc/nsr_mlp_f16.hip and csrc/nsr_mlp_h1.hip.  They are sufficient conditions: somewhat stricter than
the formats where that keeps them simple, never looser.
"""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np

from nerf_sr_amd.weights import STATE_DICT_SPEC

POS, DIR, WIDTH = 63, 27, 256
LAYERS = tuple(f"xyz_encoding_{i}.0" for i in range(1, 9)) + ("xyz_encoding_final", "dir_encoding.0", "sigma", "rgb.0")
TRUNK = LAYERS[:8]
SKIP = "xyz_encoding_5.0"
PRECISIONS = ("fp32", "f16x3", "f16", "bf16")
P_ROWS = 333                     # two 128-point tiles and a 77-row tail (one 256-point tile and a tail for the 16-bit kernel)
F16X3_LIMIT = 1023.75            # include/nsr.h: weights (nsr_pack_weights) and hidden activations (NSR_FLAG_ACTIVATION_RANGE)
ACC_LIMIT = 1 << 24              # fp32 accumulation is exact in any order below this many units


# ---------------------------------------------------------------------------------------------------------------------
# dyadic helpers
# ---------------------------------------------------------------------------------------------------------------------
def _bits(n):
    """Significant bits of every element of an integer array (0 for 0): bit length minus trailing zeros."""
    a = np.abs(np.asarray(n, dtype=np.int64))
    nz = a != 0
    safe = np.where(nz, a, 1)
    top = np.frexp(safe.astype(np.float64))[1]
    low = np.frexp((safe & -safe).astype(np.float64))[1] - 1
    return np.where(nz, top - low, 0)


def sigbits(n) -> int:
    b = _bits(n)
    return int(b.max()) if b.size else 0


def _lsb_exp(n, e) -> int:
    """Exponent of the smallest nonzero bit any element of n * 2^e has (e itself if n is all zero)."""
    a = np.abs(np.asarray(n, dtype=np.int64))
    a = a[a != 0]
    if a.size == 0:
        return e
    return e + int((np.frexp((a & -a).astype(np.float64))[1] - 1).min())


def _to_float(n, e, dtype=np.float64):
    return np.ldexp(np.asarray(n, dtype=np.float64), e).astype(dtype)


def _cat(a, ea, b, eb):
    e = min(ea, eb)
    return np.concatenate([a * (1 << (ea - e)), b * (1 << (eb - e))], 1), e


def _rne(x, bits):
    """Round float64 values to ``bits`` significant bits, ties to even (exponent range not modelled)."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)


# ---------------------------------------------------------------------------------------------------------------------
# the case and the reference
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One exact case.  sd / exp: key -> int64 array / exponent; x (P, 90) int64 with exponent x_exp."""

    def __init__(self, name, family, sd, exp, x, x_exp, precisions, tensor=None, seed=0, no_dir=False, params=None):
        self.name, self.family, self.tensor, self.seed, self.no_dir = name, family, tensor, seed, no_dir
        self.sd, self.exp, self.x, self.x_exp = sd, exp, x, x_exp
        self.precisions = tuple(precisions)
        self.params = params or {}
        self.rays = self.z = None

    def state_dict(self, dtype=np.float32):
        """The float image of the weights (exact: ``precondition`` checks every value against the format)."""
        return OrderedDict((k, _to_float(self.sd[k], self.exp[k], dtype)) for k in STATE_DICT_SPEC)

    def rows(self, dtype=np.float32):
        return _to_float(self.x, self.x_exp, dtype)

    @functools.lru_cache(maxsize=None)
    def _forward(self):
        return forward(self.sd, self.exp, self.x, self.x_exp)

    def forward(self, sigma_only=False):
        """(out float64 (P, 4) = [rgb, sigma] or -- sigma_only: the density head sits before the colour branch -- (P, 1), trace)."""
        out, trace = self._forward()
        return (out[:, 3:4], trace) if sigma_only else (out, trace)

    def __repr__(self):
        return f"Case({self.name})"


def forward(sd, exp, x, x_exp, sigma_only=False):
    """The default network in exact dyadic arithmetic, colour activation "none"; a (128, 256) dir_encoding weight is the
    no_dir network.  Returns (out as float64 -- exact, every integer involved is far below 2^53 --, trace); trace[layer] holds
    the layer's input ``a`` and pre-activation ``z`` as int64 with their exponents ``ea`` / ``ez``."""
    trace = OrderedDict()

    def lin(key, a, ea):
        w, ew = sd[key + ".weight"], exp[key + ".weight"]
        b, eb = sd[key + ".bias"], exp[key + ".bias"]
        e = min(ea + ew, eb)
        z = (a @ w.T) * (1 << (ea + ew - e)) + b * (1 << (eb - e))
        trace[key] = {"a": a, "ea": ea, "z": z, "ez": e}
        return z, e

    pe, de = x[:, :POS], x[:, POS:]
    h, eh = pe, x_exp
    for key in TRUNK:
        if key == SKIP:
            h, eh = _cat(pe, x_exp, h, eh)
        z, eh = lin(key, h, eh)
        h = np.maximum(z, 0)
    sigma, es = lin("sigma", h, eh)
    if sigma_only:
        return _to_float(sigma, es), trace
    g, eg = lin("xyz_encoding_final", h, eh)
    if sd["dir_encoding.0.weight"].shape[1] != WIDTH:
        g, eg = _cat(g, eg, de, x_exp)
    c, ec = lin("dir_encoding.0", g, eg)
    rgb, er = lin("rgb.0", np.maximum(c, 0), ec)
    return np.concatenate([_to_float(rgb, er), _to_float(sigma, es)], 1), trace


# ---------------------------------------------------------------------------------------------------------------------
# preconditions
# ---------------------------------------------------------------------------------------------------------------------
def _acc_units(terms, b, eb):
    """Largest sum |w| |a| + |b| over the outputs, in units of the products' (or the bias's, if finer) least significant
    bit.  terms: [(a, ea, w, ew), ...] summed into one accumulator.  Below 2^24 every partial sum, in any order, is an
    integer number of units below 2^24: exact in fp32."""
    e = min([ea + ew for _, ea, _, ew in terms] + [eb])
    tot = np.abs(b).astype(np.float64) * 2.0 ** (eb - e)
    for a, ea, w, ew in terms:
        tot = tot + (np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T) * 2.0 ** (ea + ew - e)
    return int(tot.max())


def _peak(n, e):
    return float(np.abs(n).max()) * 2.0 ** e if np.size(n) else 0.0


def _product_bits(a, w):
    """max over the columns of min(widest activation, widest weight) of that column: at most 11 means that in every
    product one factor has an empty lo half, so hi*hi + hi*lo + lo*hi is the whole product (there is no lo*lo)."""
    return int(np.minimum(_bits(a).max(0), _bits(w).max(0)).max())


def _fold(case):
    """The folded dir_encoding the f16x3 kernel multiplies (include/nsr.h, nsr_pack_weights): W' = W_dir[:, :256] W_final,
    b' = W_dir[:, :256] b_final + b_dir, then the direction columns of W_dir; as ((W, e), (b, e), (W_de, e) or None)."""
    sd, ex = case.sd, case.exp
    wd, ed = sd["dir_encoding.0.weight"], ex["dir_encoding.0.weight"]
    wf, ef = sd["xyz_encoding_final.weight"], ex["xyz_encoding_final.weight"]
    bf, ebf = sd["xyz_encoding_final.bias"], ex["xyz_encoding_final.bias"]
    bd, ebd = sd["dir_encoding.0.bias"], ex["dir_encoding.0.bias"]
    wp = wd[:, :WIDTH] @ wf
    e1 = ed + ebf
    eb = min(e1, ebd)
    bp = (wd[:, :WIDTH] @ bf) * (1 << (e1 - eb)) + bd * (1 << (ebd - eb))
    wde = (wd[:, WIDTH:], ed) if wd.shape[1] > WIDTH else None
    return (wp, ed + ef), (bp, eb), wde


def _check(rep, name, value, ok):
    rep[name] = value
    if not ok:
        rep.setdefault("failed", []).append(name)


def precondition_fp32(case):
    """fp32 MFMA (csrc/nsr_mlp.hip: "exact fp32 products, fp32 accumulation", heads as fp32 dot products): every weight,
    bias, input and activation fits 24 significant bits; every accumulator stays below 2^24 units."""
    _, tr = case.forward()
    rep = {}
    wb = max(sigbits(case.sd[k]) for k in STATE_DICT_SPEC)
    ab = max(max(sigbits(t["a"]), sigbits(t["z"])) for t in tr.values())
    acc = max(_acc_units([(t["a"], t["ea"], case.sd[k + ".weight"], case.exp[k + ".weight"])], case.sd[k + ".bias"], case.exp[k + ".bias"])
              for k, t in tr.items())
    _check(rep, "weight_bits", wb, wb <= 24)
    _check(rep, "activation_bits", ab, ab <= 24)
    _check(rep, "acc_units_log2", float(np.log2(max(acc, 1))), acc < ACC_LIMIT)
    rep["peak_hidden"] = max(_peak(tr[k]["z"], tr[k]["ez"]) for k in TRUNK)
    return rep


def precondition_f16x3(case):
    """Split fp16 (include/nsr.h NSR_F16X3; header of csrc/nsr_mlp_f16.hip): a value is carried as an fp16 (hi, lo) pair,
    22 significant bits, weights x 2^6; products are hi*hi + hi*lo + lo*hi.  dir_encoding is multiplied in its folded form,
    xyz_encoding_final's output never exists; the colour head is an fp32 dot product on dir_encoding's fp32 output."""
    _, tr = case.forward()
    rep = {}
    (wp, ewp), (bp, ebp), wde = _fold(case)
    h8, e8 = tr["sigma"]["a"], tr["sigma"]["ea"]
    # operands of the matrix pipe: every layer but the colour head, dir_encoding as [W' | W_dir[:, 256:]] on [h8 | de]
    if wde is not None:
        de = case.x[:, POS:]
        wfold, ewf = _cat(wp, ewp, wde[0], wde[1])       # two column groups with their own exponents ...
        afold = np.concatenate([h8, de], 1)              # ... against their own inputs: only bit counts are taken of these
        fold_terms = [(h8, e8, wp, ewp), (de, case.x_exp, wde[0], wde[1])]
    else:
        wfold, ewf, afold = wp, ewp, h8
        fold_terms = [(h8, e8, wp, ewp)]
    pipe = [(k, tr[k]["a"], tr[k]["ea"], case.sd[k + ".weight"], case.exp[k + ".weight"]) for k in TRUNK + ("sigma",)]
    w_peak = max([_peak(w, ew) for _, _, _, w, ew in pipe] + [_peak(wp, ewp)] + ([_peak(*wde)] if wde else []))
    w_bits = max([sigbits(w) for _, _, _, w, _ in pipe] + [sigbits(wfold)])
    w_lsb = min([_lsb_exp(w, ew) for _, _, _, w, ew in pipe] + [_lsb_exp(wp, ewp)] + ([_lsb_exp(*wde)] if wde else []))
    a_peak = max([_peak(a, ea) for _, a, ea, _, _ in pipe] + [_peak(case.x, case.x_exp)])
    a_bits = max([sigbits(a) for _, a, _, _, _ in pipe] + [sigbits(case.x)])
    a_lsb = min([_lsb_exp(a, ea) for _, a, ea, _, _ in pipe] + [_lsb_exp(case.x, case.x_exp)])
    prod = max([_product_bits(a, w) for _, a, _, w, _ in pipe] + [_product_bits(afold, wfold)])
    b_bits = max([sigbits(case.sd[k + ".bias"]) for k in TRUNK + ("sigma", "rgb.0")] + [sigbits(bp)])
    acc = max([_acc_units([(a, ea, w, ew)], case.sd[k + ".bias"], case.exp[k + ".bias"]) for k, a, ea, w, ew in pipe]
              + [_acc_units(fold_terms, bp, ebp)]
              + [_acc_units([(tr["rgb.0"]["a"], tr["rgb.0"]["ea"], case.sd["rgb.0.weight"], case.exp["rgb.0.weight"])],
                            case.sd["rgb.0.bias"], case.exp["rgb.0.bias"])])
    c_bits = max(sigbits(tr["rgb.0"]["a"]), sigbits(case.sd["rgb.0.weight"]))          # fp32 head
    _check(rep, "weight_peak", w_peak, w_peak < F16X3_LIMIT)
    _check(rep, "weight_bits", w_bits, w_bits <= 22)
    _check(rep, "weight_lsb_log2", w_lsb, w_lsb + 6 >= -24)      # 2^6 w as fp16: nothing below the subnormal floor
    _check(rep, "activation_peak", a_peak, a_peak < F16X3_LIMIT)
    _check(rep, "activation_bits", a_bits, a_bits <= 22)
    _check(rep, "activation_lsb_log2", a_lsb, a_lsb >= -24)
    _check(rep, "product_bits", prod, prod <= 11)
    _check(rep, "bias_bits", b_bits, b_bits <= 22)
    _check(rep, "head_bits", c_bits, c_bits <= 24)
    _check(rep, "acc_units_log2", float(np.log2(max(acc, 1))), acc < ACC_LIMIT)
    rep["peak_hidden"] = max(_peak(tr[k]["z"], tr[k]["ez"]) for k in TRUNK)
    return rep


def _precondition_h1(case, bits, peak_limit):
    """One 16-bit operand per value (header of csrc/nsr_mlp_h1.hip): weights and everything that feeds a matrix product --
    the inputs, the outputs of L1..L8 and of xyz_encoding_final -- are rounded to the format; a bias is an accumulator
    initialised from a (hi, lo) pair of the format; the density is read off the fp32 accumulator; dir_encoding's output and
    the colour head (weights, bias, dot product) stay fp32."""
    _, tr = case.forward()
    rep = {}
    pipe = [k for k in LAYERS if k != "rgb.0"]
    w_bits = max(sigbits(case.sd[k + ".weight"]) for k in pipe)
    a_bits = max(sigbits(tr[k]["a"]) for k in pipe)
    peak = max(max(_peak(case.sd[k + ".weight"], case.exp[k + ".weight"]), _peak(tr[k]["a"], tr[k]["ea"])) for k in pipe)
    lsb = min(min(_lsb_exp(case.sd[k + ".weight"], case.exp[k + ".weight"]), _lsb_exp(tr[k]["a"], tr[k]["ea"])) for k in pipe)
    bias_ok = True
    for k in pipe:
        b = _to_float(case.sd[k + ".bias"], case.exp[k + ".bias"])
        hi = _rne(b, bits)
        bias_ok &= bool(np.array_equal(hi + _rne(b - hi, bits), b))
    head_bits = max(sigbits(tr["rgb.0"]["a"]), sigbits(case.sd["rgb.0.weight"]), sigbits(case.sd["rgb.0.bias"]),
                    sigbits(tr["sigma"]["z"]))
    acc = max(_acc_units([(t["a"], t["ea"], case.sd[k + ".weight"], case.exp[k + ".weight"])], case.sd[k + ".bias"], case.exp[k + ".bias"])
              for k, t in tr.items())
    _check(rep, "weight_bits", w_bits, w_bits <= bits)
    _check(rep, "activation_bits", a_bits, a_bits <= bits)
    _check(rep, "operand_peak", peak, peak <= peak_limit)
    _check(rep, "operand_lsb_log2", lsb, lsb >= (-24 if bits == 11 else -126))
    _check(rep, "bias_pairs_exact", bias_ok, bias_ok)
    _check(rep, "head_bits", head_bits, head_bits <= 24)
    _check(rep, "acc_units_log2", float(np.log2(max(acc, 1))), acc < ACC_LIMIT)
    rep["peak_hidden"] = max(_peak(tr[k]["z"], tr[k]["ez"]) for k in TRUNK)
    return rep


def precondition_f16(case):
    return _precondition_h1(case, 11, 65504.0)


def precondition_bf16(case):
    return _precondition_h1(case, 8, 3.0e38)


_PRE = {"fp32": precondition_fp32, "f16x3": precondition_f16x3, "f16": precondition_f16, "bf16": precondition_bf16}


def precondition(case, precision):
    """The report of ``precision``'s precondition on ``case``: named peaks, plus "failed" (a list) if any is violated."""
    return _PRE[precision](case)


# ---------------------------------------------------------------------------------------------------------------------
# numpy emulation of the split-fp16 arithmetic (for the CPU test: what a lost term would do to a case)
# ---------------------------------------------------------------------------------------------------------------------
def _split(v):
    hi = _rne(v, 11)
    return hi, _rne(v - hi, 11)


def emulate_f16x3(case, drop=None):
    """The f16x3 kernel's arithmetic in float64 (every product and sum below is exact there): operands split into 11-bit
    (hi, lo) pairs, products hi*hi + hi*lo + lo*hi, dir_encoding folded, fp32 colour head.  drop = (layer, "w_lo") leaves the
    a_hi * w_lo term of that layer out, (layer, "a_lo") the a_lo * w_hi term; for xyz_encoding_final and dir_encoding the
    layer is the folded product.  Returns the (P, 4) output."""
    sd = case.state_dict(np.float64)
    x = case.rows(np.float64)

    def prod(a, w, keys):
        ah, al = _split(a)
        wh, wl = _split(w)
        t = ah @ wh.T
        if not (drop and drop[0] in keys and drop[1] == "w_lo"):
            t = t + ah @ wl.T
        if not (drop and drop[0] in keys and drop[1] == "a_lo"):
            t = t + al @ wh.T
        return t

    pe, de = x[:, :POS], x[:, POS:]
    h = pe
    for key in TRUNK:
        if key == SKIP:
            h = np.concatenate([pe, h], 1)
        h = np.maximum(prod(h, sd[key + ".weight"], (key,)) + sd[key + ".bias"], 0.0)
    sigma = prod(h, sd["sigma.weight"], ("sigma",)) + sd["sigma.bias"]
    wd = sd["dir_encoding.0.weight"]
    wp = (wd[:, :WIDTH] @ sd["xyz_encoding_final.weight"]).astype(np.float32).astype(np.float64)
    bp = (wd[:, :WIDTH] @ sd["xyz_encoding_final.bias"] + sd["dir_encoding.0.bias"]).astype(np.float32).astype(np.float64)
    if wd.shape[1] > WIDTH:
        wp, h = np.concatenate([wp, wd[:, WIDTH:]], 1), np.concatenate([h, de], 1)
    c = np.maximum(prod(h, wp, ("xyz_encoding_final", "dir_encoding.0")) + bp, 0.0)
    wr = sd["rgb.0.weight"]
    if drop and drop[0] == "rgb.0" and drop[1] == "w_lo":
        wr = _split(wr)[0]
    return np.concatenate([c @ wr.T + sd["rgb.0.bias"], sigma], 1)


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def _allowed_cols(key, rays, no_dir=False):
    """The weight columns a case may use: all of them, or -- ray cases -- all but the sin / cos columns of the encodings."""
    n_in = STATE_DICT_SPEC[key + ".weight"][1]
    if key == "dir_encoding.0" and no_dir:
        return np.arange(WIDTH)
    if not rays:
        return np.arange(n_in)
    if key == "xyz_encoding_1.0":
        return np.arange(3)
    if key == SKIP:
        return np.concatenate([np.arange(3), np.arange(POS, POS + WIDTH)])
    if key == "dir_encoding.0":
        return np.concatenate([np.arange(WIDTH), np.arange(WIDTH, WIDTH + 3)])
    return np.arange(n_in)


def _n_in(key, no_dir):
    return WIDTH if (key == "dir_encoding.0" and no_dir) else STATE_DICT_SPEC[key + ".weight"][1]


def _sparse(rng, key, m, cols, no_dir):
    n_out = STATE_DICT_SPEC[key + ".weight"][0]
    w = np.zeros((n_out, _n_in(key, no_dir)), dtype=np.int64)
    k = min(m, len(cols))
    pos = np.argsort(rng.random((n_out, len(cols))), 1)[:, :k]
    w[np.arange(n_out)[:, None], cols[pos]] = rng.choice([-1, 1], size=(n_out, k))
    return w


def _routing(rng, key, cols, no_dir):
    """Non-negative routing layer: ceil(in / out) ones per row, every allowed input column read by some row."""
    n_out = STATE_DICT_SPEC[key + ".weight"][0]
    w = np.zeros((n_out, _n_in(key, no_dir)), dtype=np.int64)
    k = -(-len(cols) // n_out)
    deal = np.concatenate([rng.permutation(cols) for _ in range(-(-n_out * k // len(cols)))])[:n_out * k]
    w[np.tile(np.arange(n_out), k), deal] = 1
    return w


def _dense(rng, shape, amp, cols=None):
    """Dense nonzero integers of magnitude 1 .. amp.  Each row gets as many + as - signs, at random places: the inputs of a
    routing network are non-negative with a common mean, and a row whose weights sum far below zero would be dead on every
    row of the batch -- invisible to the outputs."""
    n = shape[-1]
    signs = np.where(np.arange(n) % 2 == 0, 1, -1) * np.ones(shape, dtype=np.int64)
    signs = rng.permuted(signs.reshape(-1, n), axis=1).reshape(shape)
    v = rng.integers(1, amp + 1, size=shape) * signs
    if cols is not None:
        keep = np.zeros(n, dtype=bool)
        keep[cols] = True
        v = v * keep
    return v.astype(np.int64)


def _inputs(rng, P, lo, hi, frac_bits):
    """(P, 90) inputs: integers in [lo, hi], plus -- frac_bits > 0 -- a fraction k 2^-frac_bits, so that an input (and what the
    network makes of it) needs the lo half of a split operand.  Returns (int64 array, exponent)."""
    x = rng.integers(lo, hi + 1, size=(P, POS + DIR)).astype(np.int64)
    if frac_bits:
        x = x * (1 << frac_bits) + rng.integers(-(1 << (frac_bits - 1)) + 1, 1 << (frac_bits - 1), size=x.shape)
    return x, -frac_bits


#: Family A per configuration: nonzeros per row (the largest the narrowest precision of the configuration allows on every
#: seed tried), input range, fraction bits of the inputs, the precisions it is valid at, and four seeds -- the first four
#: whose case is not degenerate; "binds": the precision whose precondition limits m (max |out| > 100; tests/test_mlp_exact_cpu.py), nothing about a kernel enters the choice
FAMILY_A = OrderedDict([
    ("m3", {"binds": "bf16", "m": 3, "x": (-3, 3), "frac_bits": 0, "precisions": ("fp32", "f16x3", "f16", "bf16"), "seeds": (2, 3, 4, 5)}),
    ("m6", {"binds": "f16x3", "m": 6, "x": (-2, 2), "frac_bits": 0, "precisions": ("fp32", "f16x3", "f16"), "seeds": (0, 1, 2, 3)}),
    ("m6d", {"binds": "f16x3", "m": 6, "x": (-2, 2), "frac_bits": 10, "precisions": ("fp32", "f16x3"), "seeds": (0, 1, 2, 3)}),
    ("m24", {"binds": "fp32", "m": 24, "x": (-2, 2), "frac_bits": 0, "precisions": ("fp32",), "seeds": (0, 1, 2, 3)}),
])


@functools.lru_cache(maxsize=None)
def family_a(config, seed, P=P_ROWS, no_dir=False, rays=False):
    cfg = FAMILY_A[config]
    rng = _rng(1, list(FAMILY_A).index(config), seed, int(no_dir), int(rays))
    sd, exp = OrderedDict(), {}
    for key in LAYERS:
        sd[key + ".weight"] = _sparse(rng, key, cfg["m"], _allowed_cols(key, rays, no_dir), no_dir)
        sd[key + ".bias"] = rng.integers(-1, 2, size=STATE_DICT_SPEC[key + ".bias"]).astype(np.int64)
        exp[key + ".weight"] = exp[key + ".bias"] = 0
    x, xe = _inputs(rng, P, cfg["x"][0], cfg["x"][1], cfg["frac_bits"])
    name = f"A-{config}-s{seed}" + ("-nodir" if no_dir else "") + ("-rays" if rays else "")
    return Case(name, "A", sd, exp, x, xe, cfg["precisions"], seed=seed, no_dir=no_dir, params=dict(cfg, weights="+-1", biases="[-1, 1]"))


#: Family B per configuration: amplitude of the dense tensor, input range, the lifting first-layer bias, routing biases
FAMILY_B = OrderedDict([
    ("narrow", {"amp": 1, "x": (-1, 0), "lift": 1, "route_bias": 0, "precisions": ("fp32", "f16x3", "f16", "bf16")}),
    ("wide", {"amp": 3, "x": (-2, 2), "lift": 2, "route_bias": 0, "precisions": ("fp32", "f16x3", "f16")}),
])


def _one_tensor_network(rng, tensor, dense_w, dense_b, lift, route_bias, rays):
    """Family B / C skeleton: ``tensor`` dense (made by the two callables), the other trunk layers routing, dense +-1 heads."""
    sd, exp = OrderedDict(), {}
    for key in LAYERS:
        shape = STATE_DICT_SPEC[key + ".weight"]
        cols = _allowed_cols(key, rays)
        exp[key + ".weight"] = exp[key + ".bias"] = 0
        if key == tensor:
            sd[key + ".weight"], sd[key + ".bias"] = dense_w(shape, cols), dense_b((shape[0],))
        elif key in ("sigma", "rgb.0"):
            sd[key + ".weight"], sd[key + ".bias"] = _dense(rng, shape, 1), rng.integers(-1, 2, size=(shape[0],)).astype(np.int64)
        else:
            sd[key + ".weight"] = _routing(rng, key, cols, False)
            # every raw input a routing row reads (all of L1; the pe part of the skip layer, the direction part of
            # dir_encoding) is lifted to >= 0 by the bias, so that no routing neuron is dead on every row
            raw = {"xyz_encoding_1.0": slice(0, POS), SKIP: slice(0, POS), "dir_encoding.0": slice(WIDTH, WIDTH + DIR)}.get(key)
            sd[key + ".bias"] = rng.integers(0, route_bias + 1, size=(shape[0],)).astype(np.int64) if key != "xyz_encoding_1.0" \
                else np.zeros((shape[0],), dtype=np.int64)
            if raw is not None:
                sd[key + ".bias"] = sd[key + ".bias"] + lift * sd[key + ".weight"][:, raw].sum(1)
    return sd, exp


@functools.lru_cache(maxsize=None)
def family_b(config, tensor, seed, P=P_ROWS, rays=False):
    cfg = FAMILY_B[config]
    rng = _rng(2, list(FAMILY_B).index(config), LAYERS.index(tensor), seed, int(rays))
    sd, exp = _one_tensor_network(rng, tensor, lambda s, cols: _dense(rng, s, cfg["amp"], cols if rays else None),
                                  lambda s: _dense(rng, s, cfg["amp"]), cfg["lift"], cfg["route_bias"], rays)
    x, xe = _inputs(rng, P, cfg["x"][0], cfg["x"][1], 0)
    name = f"B-{config}-{tensor}-s{seed}" + ("-rays" if rays else "")
    return Case(name, "B", sd, exp, x, xe, cfg["precisions"], tensor=tensor, seed=seed, params=dict(cfg))


C_FRAC, C_BITS = 12, 12          # Family C: T = odd n 2^-12, |n| < 2^12: up to 12 significant bits, |w| < 1.  One bit more and
                                 # the dense +-1 density head, summing 256 such activations, leaves the 2^24 accumulation budget


@functools.lru_cache(maxsize=None)
def family_c(tensor, seed=0, P=P_ROWS):
    rng = _rng(3, LAYERS.index(tensor), seed)

    def wide(shape, cols=None):
        n = rng.integers(0, 1 << (C_BITS - 1), size=shape) | (1 << (C_BITS - 1)) | 1      # first and last bit always in use
        return (n * rng.choice([-1, 1], size=shape)).astype(np.int64)

    sd, exp = _one_tensor_network(rng, tensor, wide, wide, 1, 0, False)
    exp[tensor + ".weight"] = exp[tensor + ".bias"] = -C_FRAC
    x, xe = _inputs(rng, P, -1, 0, 0)
    return Case(f"C-{tensor}-s{seed}", "C", sd, exp, x, xe, ("fp32", "f16x3"), tensor=tensor, seed=seed,
                params={"weights": "odd n 2^-12, |n| < 2^12", "inputs": "{-1, 0}", "lift": 1})


# ---------------------------------------------------------------------------------------------------------------------
# ray cases
# ---------------------------------------------------------------------------------------------------------------------
def ray_case(base, R, N, z_set, seed=0, at_origin=False):
    """``base`` (a case built with rays=True: zero weights on every sin / cos column of L1, of the skip layer's pe part and
    of dir_encoding's direction part) on R rays x N samples whose points o + z d are exact: integer origins, direction
    components in {-1, 0, 1}, z from ``z_set`` nondecreasing along the ray.  The in-kernel encoding is exact on the three
    un-encoded coordinates of each block only, so the reference rows carry xyz and d there and zeros elsewhere.
    at_origin: every ray is o = d = 0 and ``base`` is a full case (rays=False) instead: nsr_sincos returns exactly (0, 1) at
    argument 0 (k = 0, r = 0, both polynomials collapse to their constant term), so the rows are the encoding of 0 -- sin
    columns 0, cos columns 1 -- and the cos-column weights take part."""
    rng = _rng(4, seed, R, N)
    zs = np.asarray(z_set, dtype=np.float64)
    q = int(round(-np.log2(np.min(np.diff(np.unique(np.concatenate([[0.0], zs])))))))        # z = k 2^-q
    z = np.sort(rng.choice(zs, size=(R, N)), 1)
    if at_origin:
        o, d = np.zeros((R, 3), dtype=np.int64), np.zeros((R, 3), dtype=np.int64)
    else:
        o, d = rng.integers(-2, 3, size=(R, 3)), rng.integers(-1, 2, size=(R, 3))
    zi = np.rint(z * (1 << q)).astype(np.int64)
    xyz = o[:, None, :] * (1 << q) + zi[:, :, None] * d[:, None, :]
    x = np.zeros((R * N, POS + DIR), dtype=np.int64)
    x[:, :3] = xyz.reshape(-1, 3)
    x[:, POS:POS + 3] = np.repeat(d, N, 0) * (1 << q)
    if at_origin:
        for f in range(10):
            x[:, 6 + 6 * f:9 + 6 * f] = 1 << q
        for f in range(4):
            x[:, POS + 6 + 6 * f:POS + 9 + 6 * f] = 1 << q
    case = Case(f"{base.name}-R{R}xN{N}" + ("-origin" if at_origin else ""), base.family, base.sd, base.exp, x, -q, base.precisions,
                tensor=base.tensor, seed=base.seed, params=dict(base.params, z_set=list(map(float, z_set))))
    near, far = np.full((R, 1), 2.0), np.full((R, 1), 6.0)
    case.rays = np.concatenate([o, d, near, far], 1).astype(np.float32)
    case.z = z.astype(np.float32)
    return case


Z_QUARTERS = tuple(0.25 * k for k in range(13))     # 0 .. 3 in steps of 1/4
Z_INTEGERS = (0.0, 1.0, 2.0, 3.0)                   # the single-16-bit formats: no room for fraction bits


# ---------------------------------------------------------------------------------------------------------------------
# Family B: which elements of T can the outputs see?
# ---------------------------------------------------------------------------------------------------------------------
def observability(case, tensor=None):
    """Element (o, i) of ``tensor`` (default: case.tensor) counts as observed when on some row input i of the tensor is
    nonzero and pre-activation o has a nonzero path to an output: the ReLU-masked product of |W| downstream.  Returns
    (observed (out, in) bool, observed bias (out,) bool)."""
    tensor = tensor or case.tensor
    _, tr = case.forward()
    sd = case.sd
    live = lambda k: (tr[k]["z"] > 0).astype(np.float64)
    absw = lambda k: np.abs(sd[k + ".weight"]).astype(np.float64)
    P = case.x.shape[0]
    g = {"rgb.0": np.ones((P, 3)), "sigma": np.ones((P, 1))}
    g["dir_encoding.0"] = (g["rgb.0"] @ absw("rgb.0")) * live("dir_encoding.0")
    g["xyz_encoding_final"] = (g["dir_encoding.0"] @ absw("dir_encoding.0"))[:, :WIDTH]
    gh = g["xyz_encoding_final"] @ absw("xyz_encoding_final") + g["sigma"] @ absw("sigma")
    for key in reversed(TRUNK):
        g[key] = gh * live(key)
        gh = g[key] @ absw(key)
        if key == SKIP:
            gh = gh[:, POS:]
    path = (g[tensor] > 0).astype(np.float64)
    used = (tr[tensor]["a"] != 0).astype(np.float64)
    return (path.T @ used) > 0, path.sum(0) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the lists both test files run
# ---------------------------------------------------------------------------------------------------------------------
B_SEEDS = (0,)                   # observability reaches the Family B condition with one seed per tensor (at most four allowed)


def row_cases(precision):
    """Every (P_ROWS, 90) case valid at ``precision``: Family A (every configuration x four seeds, plus one no_dir network
    per configuration), B (every tensor), C (every tensor; fp32 and f16x3)."""
    out = []
    for cfg, d in FAMILY_A.items():
        if precision in d["precisions"]:
            out += [family_a(cfg, s) for s in d["seeds"]] + [family_a(cfg, d["seeds"][0], no_dir=True)]
    for cfg, d in FAMILY_B.items():
        if precision in d["precisions"]:
            out += [family_b(cfg, t, s) for t in LAYERS for s in B_SEEDS]
    if precision in ("fp32", "f16x3"):
        out += [family_c(t) for t in LAYERS]
    return out


def all_row_cases():
    seen = OrderedDict()
    for p in PRECISIONS:
        for c in row_cases(p):
            seen[c.name] = c
    return list(seen.values())


#: ray cases per precision: Family A configuration, Family B configuration, the z set (the points' fraction bits come out
#: of the operand budget: bf16's 8 bits leave none, nor do f16's 11 at m = 6)
RAY = {"fp32": ("m6", "wide", Z_QUARTERS), "f16x3": ("m6", "wide", Z_QUARTERS), "f16": ("m6", "narrow", Z_INTEGERS),
       "bf16": ("m3", "narrow", Z_INTEGERS)}
RAY_B_N128 = ("xyz_encoding_1.0", SKIP, "xyz_encoding_8.0", "dir_encoding.0")


@functools.lru_cache(maxsize=None)
def ray_cases(precision):
    """5 rays x 64 samples (f16x3: one group of four rays plus a one-ray tail, two 32-sample windows): Family A (two seeds),
    Family B (every tensor), one case with every ray at the origin; f16x3 also 2 rays x 128 samples."""
    cfg_a, cfg_b, zs = RAY[precision]
    seeds = FAMILY_A[cfg_a]["seeds"]
    out = [ray_case(family_a(cfg_a, s, rays=True), 5, 64, zs, seed=s) for s in seeds[:2]]
    out += [ray_case(family_b(cfg_b, t, 0, rays=True), 5, 64, zs) for t in LAYERS]
    out.append(ray_case(family_a(cfg_a, seeds[0]), 5, 64, zs, at_origin=True))
    if precision == "f16x3":
        out.append(ray_case(family_a(cfg_a, seeds[0], rays=True), 2, 128, zs, seed=7))
        out += [ray_case(family_b(cfg_b, t, 0, rays=True), 2, 128, zs, seed=7) for t in RAY_B_N128]
    return tuple(out)
