"""CPU reference of the backward chain (csrc/nsr_train_chain.hip) for tests/test_gpu_chain_units.py and
tests/test_chain_units_cpu.py: numpy only, no device.

Everything is written from the documented contracts -- the header comment of nsr_train_chain.hip (what the chain computes, the
per-point power-of-two scales), "Training panels" and "Sign panels" in nsr_f16x3_core.h, nsr_panels.h -- and is pinned on the
CPU against things that do not share its code: the panel decoder against a thread-by-thread restatement of the test writer
pack_panel_kernel, the fp64 chain against torch.autograd through oracle/nerf_oracle.py::mlp_forward, the error model against an
emulation of the three arithmetics (tests/test_chain_units_cpu.py).

Conventions.  A gradient is a (P, rows) array, row = sample point, column = feature.  Panels 0..7 = d(pre-activation) of trunk
layers 1..8, 8 = d(output of xyz_encoding_final) (no ReLU), 9 = d(pre-activation of dir_encoding) (128 features).  `masks[p]`
(p = 0..7, 9) is a boolean (P, rows) array, True = "the ReLU zeroed this pre-activation" (the sign panels' bit).  Chain layer
lam = 0..8 consumes panel 9 - lam (lam = 0: panel 9) and produces panel 8 - lam.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from nerf_sr_amd.weights import STATE_DICT_SPEC, make_state_dict

KEYS = list(STATE_DICT_SPEC)              # the 24 state tensors in state_dict order = the chain's pointer array
PANEL_ROWS = (256,) * 9 + (128,)          # gradient panels 0..9
MASK_PANELS = (0, 1, 2, 3, 4, 5, 6, 7, 9)
BWD_ROWS = 2432                           # rows of the ten gradient panels together; a full (forward) panel set has 2560
SIGN_PAIRS = 34
MODES = (1, 2, 3, 12)
SENTINEL = np.float32(1.0e30)             # what the chain must never read: 64 x it is inf in fp16 and poisons a whole panel
U32 = 2.0 ** -24


def n_groups(P):
    return (P + 127) // 128 * 4


def nt_of(mode, lam):
    """MFMA terms of chain layer lam: 12 = two on the six layers nearest the output, one on the three below"""
    return (2 if lam < 6 else 1) if mode == 12 else mode


def act_feature(t, h):
    """feature held in half t (0..127: eight per k-step) of lane half h of an operand register set (nsr_mlp_layout.h)"""
    return 32 * (t >> 4) + (t & 3) + 8 * ((t & 15) >> 2) + 4 * h


# ------------------------------------------------------------------------------------------------------------------------
# training panels: decoder (and its inverse)
# ------------------------------------------------------------------------------------------------------------------------
def _panel_view(buf_u16, P, panel):
    ng, rows = n_groups(P), PANEL_ROWS[panel]
    first = 256 * panel * 32 * ng                      # panel_rows_before * 64 bytes * n_groups, in halves
    return buf_u16[first:first + rows * 32 * ng].reshape(ng, rows // 32, 2, 64, 8)   # [group][block][unit][slot][half]


def _unit_slots(u, h):
    m = np.arange(32)
    return (2 * m + h) ^ (8 * u)


def decode_panels(buf_u8, P):
    """bytes of a gradient panel set -> ten (P, rows) float16 arrays.  A block of 32 features is two 1 KiB units; lane (m, h)
    of unit u sits in 16-byte slot (2m + h) ^ 8u and holds features 16u + 4h + {0..3}, then 16u + 8 + 4h + {0..3}."""
    buf = np.ascontiguousarray(buf_u8).view(np.uint16)
    out = []
    for panel in range(10):
        a = _panel_view(buf, P, panel)
        ng, nblk = a.shape[:2]
        o = np.empty((ng, 32, nblk, 32), np.uint16)    # [group][m][block][feature in block]
        for u in range(2):
            for h in range(2):
                x = a[:, :, u, _unit_slots(u, h), :]   # (ng, nblk, 32 m, 8)
                for jj in range(2):
                    f0 = 16 * u + 8 * jj + 4 * h
                    o[:, :, :, f0:f0 + 4] = x[..., 4 * jj:4 * jj + 4].transpose(0, 2, 1, 3)
        out.append(o.reshape(ng * 32, nblk * 32)[:P].view(np.float16).copy())
    return out


def encode_panels(panels, P, fill=0x7E7E):
    """inverse of decode_panels: ten (P, rows) float16 arrays -> bytes of the panel set (padding points = `fill` halves)"""
    ng = n_groups(P)
    buf = np.full(BWD_ROWS * 32 * ng, fill, np.uint16)
    for panel in range(10):
        a = _panel_view(buf, P, panel)
        nblk = a.shape[1]
        src = np.full((ng * 32, nblk * 32), fill, np.uint16)
        src[:P] = np.ascontiguousarray(panels[panel]).view(np.uint16)
        s = src.reshape(ng, 32, nblk, 32)
        for u in range(2):
            for h in range(2):
                x = np.empty((ng, nblk, 32, 8), np.uint16)
                for jj in range(2):
                    f0 = 16 * u + 8 * jj + 4 * h
                    x[..., 4 * jj:4 * jj + 4] = s[:, :, :, f0:f0 + 4].transpose(0, 2, 1, 3)
                a[:, :, u, _unit_slots(u, h), :] = x
    return buf.view(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------
# sign panels: encoder (and its inverse)
# ------------------------------------------------------------------------------------------------------------------------
def _pair0(panel):
    return 32 if panel == 9 else 4 * panel


def encode_signs(masks, P, pad=True):
    """masks -> sign words.  Per point group 34 pair blocks of 64 dwords, panel p from pair 4p (panel 9: 32); lane (m, h) = dword
    m + 32h; register r of block nb = feature 32 nb + 8 (r >> 2) + (r & 3) + 4h goes to bit 31 - r (nb even) or 15 - r (nb odd)
    of the pair's dword.  Points past P get `pad` (True: everything zeroed, so they carry no gradient)."""
    ng = n_groups(P)
    words = np.zeros((ng, SIGN_PAIRS, 64), np.uint32)
    wgt = (1 << (15 - np.arange(16))).astype(np.uint32)
    for panel in MASK_PANELS:
        rows = PANEL_ROWS[panel]
        m = np.full((ng * 32, rows), bool(pad))
        m[:P] = masks[panel]
        # feature = 32 nb + 8 rhi + 4 h + rlo  ->  [group][m][nb][rhi][h][rlo] -> [group][nb][h][m][r = 4 rhi + rlo]
        b = m.reshape(ng, 32, rows // 32, 4, 2, 4).transpose(0, 2, 4, 1, 3, 5).reshape(ng, rows // 32, 64, 16)
        hw = (b.astype(np.uint32) * wgt).sum(-1, dtype=np.uint32)                  # (ng, nb, lane)
        words[:, _pair0(panel):_pair0(panel) + rows // 64] = (hw[:, 0::2] << 16) | hw[:, 1::2]
    return words.reshape(-1)


def decode_signs(words, P):
    ng = n_groups(P)
    w = np.asarray(words, np.uint32).reshape(ng, SIGN_PAIRS, 64)
    out = {}
    for panel in MASK_PANELS:
        rows = PANEL_ROWS[panel]
        pw = w[:, _pair0(panel):_pair0(panel) + rows // 64]
        hw = np.stack([pw >> 16, pw & 0xFFFF], 2).reshape(ng, rows // 32, 64)       # (ng, nb, lane)
        bits = ((hw[..., None] >> (15 - np.arange(16))) & 1).astype(bool)           # (ng, nb, lane, r)
        b = bits.reshape(ng, rows // 32, 2, 32, 4, 4).transpose(0, 3, 1, 4, 2, 5)   # [group][m][nb][rhi][h][rlo]
        out[panel] = b.reshape(ng * 32, rows)[:P].copy()
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the nine matrices of the chain and the stream packer
# ------------------------------------------------------------------------------------------------------------------------
def layer_mats(sd, stop_grad=False, skip_col0=63):
    """[M_0 .. M_8], M_lam (K, 256) with (input gradient) @ M_lam = output gradient before the mask: the first 256 columns of
    dir_encoding's weight (zeros under stop_grad: its input is detached), xyz_encoding_final's weight, then trunk layers
    8..2, the skip layer (5) without the 63 columns of the encoded position in front of its h4 columns."""
    dirw = np.asarray(sd["dir_encoding.0.weight"])[:, :256]
    mats = [np.zeros_like(dirw) if stop_grad else dirw, np.asarray(sd["xyz_encoding_final.weight"])]
    for l in range(8, 1, -1):
        W = np.asarray(sd[f"xyz_encoding_{l}.0.weight"])
        mats.append(W[:, skip_col0:skip_col0 + 256] if l == 5 else W)
    return mats


def split_f16(x32):
    """fp32 -> (hi, lo) fp16, both rounded to nearest even: hi = f16(x), lo = f16(x - hi)"""
    hi = x32.astype(np.float16)
    return hi, (x32 - hi.astype(np.float32)).astype(np.float16)


def stream_pieces(mode):
    return {1: 1152, 2: 2304, 3: 2304, 12: 1536 + 384}[mode]


def pack_stream(sd, mode, stop_grad=False):
    """the transposed weight stream as 32-bit words: per layer eight chunks (one 32-feature output block nb each) of 16 k-steps,
    per k-step a hi piece and -- where the layer runs on two or three terms -- a lo piece behind it.  A piece is 64 lanes x 8
    halves: lane (i, h) = i + 32h, half j = 64 W[k = act_feature(8 s + j, h)][column 32 nb + i] (the 128-row dir_encoding
    layer zero-padded to 16 k-steps).  Behind the stream 768 fp32 words: rgb.weight as [feature][4] (fourth = 0), sigma.weight."""
    s_, h_, j_ = np.meshgrid(np.arange(16), np.arange(2), np.arange(8), indexing="ij")
    kidx = act_feature(8 * s_ + j_, h_)                                            # (s, h, j)
    out = []
    for lam, M in enumerate(layer_mats(sd, stop_grad)):
        X = np.zeros((256, 256), np.float32)
        X[:M.shape[0]] = np.float32(64.0) * M.astype(np.float32)
        parts = split_f16(X)[:2 if nt_of(mode, lam) > 1 else 1]
        # [s][h][j][nb][i] -> [nb][s][part][h][i][j]
        pcs = np.stack([p[kidx].reshape(16, 2, 8, 8, 32).transpose(3, 0, 1, 4, 2) for p in parts], 2)
        out.append(np.ascontiguousarray(pcs).view(np.uint16).reshape(-1))
    halves = np.concatenate(out)
    words = halves[0::2].astype(np.uint32) | (halves[1::2].astype(np.uint32) << 16)
    assert words.size == stream_pieces(mode) * 256
    aux = np.zeros((128, 4), np.float32)
    aux[:, :3] = np.asarray(sd["rgb.0.weight"], np.float32).T
    return np.concatenate([words, aux.reshape(-1).view(np.uint32), np.asarray(sd["sigma.weight"], np.float32).reshape(-1).view(np.uint32)])


# ------------------------------------------------------------------------------------------------------------------------
# fp64 reference chain
# ------------------------------------------------------------------------------------------------------------------------
def ref_chain(sd, masks, d_rgb, d_sigma, stop_grad=False, skip_col0=63, drop_sigma=False, drop_k=None):
    """the ten panels' true gradients in float64.  The last three arguments make deliberately WRONG references (the teeth test):
    the skip slice taken elsewhere, the density head's term left out, input features drop_k = (lam, [features]) of one layer
    left out."""
    f8 = np.float64
    M = [m.astype(f8) for m in layer_mats(sd, stop_grad, skip_col0)]
    keep = {p: ~np.asarray(masks[p], bool) for p in MASK_PANELS}
    d_rgb, d_sigma = np.asarray(d_rgb, f8), np.asarray(d_sigma, f8).reshape(-1)
    wsig = np.asarray(sd["sigma.weight"], f8).reshape(-1)
    g = [None] * 10
    g[9] = (d_rgb @ np.asarray(sd["rgb.0.weight"], f8)) * keep[9]                # dzc = (Wrgb^T d_rgb) * m9
    g[8] = g[9] @ M[0]                                                           # dg = Wdir[:, :256]^T dzc
    rank1 = 0.0 if drop_sigma else d_sigma[:, None] * wsig[None, :]
    g[7] = (g[8] @ M[1] + rank1) * keep[7]                                       # dz8 = (Wfinal^T dg + wsigma d_sigma) * m7
    for lam in range(2, 9):                                                      # dz_{l-1} = (W_l^T dz_l) * m_{l-2}, l = 10 - lam
        src = g[9 - lam]
        if drop_k is not None and drop_k[0] == lam:
            src = src.copy()
            src[:, list(drop_k[1])] = 0.0
        g[8 - lam] = (src @ M[lam]) * keep[8 - lam]
    return g


# ------------------------------------------------------------------------------------------------------------------------
# per-point scales, as documented: the prologue brings the point's largest input into [2, 4); every later panel is stored at
# the scale that does the same for the largest value of the panel BEFORE it (the operands it was computed from), the
# re-normalising factor phi = 2^e being kept a normal fp16 (-14 <= e <= 0)
# ------------------------------------------------------------------------------------------------------------------------
def floor_log2(x):
    _, e = np.frexp(x)
    return e - 1


def next_pscale(ps_in, true_max_in):
    stored = true_max_in / ps_in
    E = np.where(stored > 0, floor_log2(np.where(stored > 0, stored, 1.0)) + 1, 2)
    e = np.clip(-4 - E, -14, 0)
    return ps_in * 2.0 ** (-6 - e), 2.0 ** e


def predicted_pscale(g, d_sigma):
    """(10, P) scales and (10, P) phi that the documented rule gives for gradients g (exact only when g is what the chain
    computes, i.e. in the exact regime; one binade off at worst otherwise)"""
    P = g[9].shape[0]
    ps, phi = np.ones((10, P)), np.ones((10, P))
    mxin = np.maximum(np.abs(np.asarray(d_sigma, np.float64).reshape(-1)), np.abs(g[9]).max(1))
    ps[9] = np.where(mxin > 0, 2.0 ** (floor_log2(np.where(mxin > 0, mxin, 1.0)) - 1), 1.0)
    ps[8], phi[8] = ps[9], 2.0 ** -6
    for panel in range(7, -1, -1):
        ps[panel], phi[panel] = next_pscale(ps[panel + 1], np.abs(g[panel + 1]).max(1))
    return ps, phi


def sig_bits(x):
    """significant bits of every element (0 for zero)"""
    m, _ = np.frexp(np.abs(x))
    k = np.zeros(x.shape, np.int64)
    r = m.copy()
    for b in range(1, 54):
        r = r * 2.0
        r -= np.floor(r)
        k = np.where((r == 0) & (k == 0) & (m != 0), b, k)
    return k


def assert_exact_regime(g, d_sigma, what=""):
    """every true gradient has at most 11 significant bits, and -- at the point's predicted scale -- is a normal-or-exact fp16
    both as stored (x phi) and before the re-normalisation (the accumulator, rounded to fp16 first): the chain's result then
    does not depend on the term count and must equal g bit for bit"""
    ps, phi = predicted_pscale(g, d_sigma)
    for panel in range(10):
        bits = int(sig_bits(g[panel]).max())
        assert bits <= 11, f"{what}: panel {panel} has a {bits}-bit gradient"
        stored = g[panel] / ps[panel][:, None]
        with np.errstate(over="ignore"):
            ok = (stored.astype(np.float16).astype(np.float64) == stored).all()
            acc = stored / phi[panel][:, None]
            ok = ok and (acc.astype(np.float16).astype(np.float64) == acc).all()
        assert ok, f"{what}: panel {panel} leaves fp16 at the point's scale"
    return ps


# ------------------------------------------------------------------------------------------------------------------------
# error model for real-valued inputs
# ------------------------------------------------------------------------------------------------------------------------
def hulp16(x):
    """half a unit in the last place of fp16 at magnitude x (normal range): the error bound of one rounding to nearest.
    = 2^-12 x (the power of two above x), between 2^-12 x and 2^-11 x"""
    x = np.asarray(x, np.float64)
    return np.where(x > 0, 2.0 ** (floor_log2(np.where(x > 0, x, 1.0)) - 11), 0.0)


def _gamma(n):
    return n * U32 / (1.0 - n * U32)


def error_bounds(sd, masks, d_rgb, d_sigma, mode, g, stop_grad=False, literal=False):
    """elementwise bound on |stored value x pscale - g| for the chain run on `mode` terms, propagated layer by layer:

        E_out = [ |M|^T (E_in + r_g) + dM^T (|g_in| + E_in + r_g) + (3 terms: H_g H_w, the dropped lo x lo products)
                  + gamma_n S ] masked,      S = sum of the magnitudes of everything accumulated

    r_g: rounding of the incoming gradient to the operand -- half an fp16 ulp where the layer uses its `hi` alone (1 or 2
    terms), 2^-12 of that for hi + lo (3 terms) -- plus one fp16 denormal step at the point's scale; dM: the same for the
    weight (hi alone on one-term layers, hi + lo otherwise; 64 W is what is rounded); gamma_n: n = terms x K fp32
    accumulations (+ 1 for the density head's FMA); the prologue is three fp32 roundings.  The stored value adds one rounding
    to fp16 and the denormal step.  E is the error of the masked fp32 value the kernel holds BEFORE that rounding.
    `literal`: 2^-12 |x| in place of half an ulp (what half an ulp is at the top of a binade; NOT a bound below it).
    Returns the ten bounds."""
    f8 = np.float64
    r16 = (lambda x: 2.0 ** -12 * np.asarray(x, f8)) if literal else hulp16
    M32 = [m.astype(np.float32) for m in layer_mats(sd, stop_grad)]
    keep = {p: (~np.asarray(masks[p], bool)).astype(f8) for p in MASK_PANELS}
    keep[8] = 1.0
    d_rgb, d_sigma = np.abs(np.asarray(d_rgb, f8)), np.abs(np.asarray(d_sigma, f8).reshape(-1))
    wsig = np.abs(np.asarray(sd["sigma.weight"], f8).reshape(-1))
    ps, _ = predicted_pscale(g, d_sigma)
    den = 2.0 ** -24 * ps                                                          # one fp16 denormal step, true scale
    bound = [None] * 10
    Ex = _gamma(3) * (d_rgb @ np.abs(np.asarray(sd["rgb.0.weight"], f8))) * keep[9]
    bound[9] = Ex + r16(np.abs(g[9]) + Ex) + den[9][:, None]
    for lam in range(9):
        pin, pout = (9 if lam == 0 else 9 - lam), 8 - lam
        nt = nt_of(mode, lam)
        X = np.abs(np.float32(64.0) * M32[lam]).astype(f8)
        Hw = np.where(X > 0, np.maximum(r16(X), 2.0 ** -25), 0.0) / 64.0           # hi alone
        dM = Hw if nt == 1 else np.where(X > 0, np.maximum(2.0 ** -12 * Hw * 64.0, 2.0 ** -25), 0.0) / 64.0
        a = np.abs(g[pin]) + Ex
        Hg = r16(a)
        rg = (Hg if nt <= 2 else 2.0 ** -12 * Hg) + den[pin][:, None]
        Eop = Ex + rg
        absM = np.abs(M32[lam]).astype(f8)
        S = (np.abs(g[pin]) + Eop) @ (absM + dM)
        n = nt * absM.shape[0]
        if lam == 1:
            S = S + d_sigma[:, None] * wsig[None, :]
            n += 1
        Eacc = Eop @ absM + (np.abs(g[pin]) + Eop) @ dM + _gamma(n) * S
        if nt == 3:
            Eacc = Eacc + Hg @ Hw
        Ex = Eacc * keep[pout]
        bound[pout] = Ex + r16(np.abs(g[pout]) + Ex) + den[pout][:, None]
    return bound


# ------------------------------------------------------------------------------------------------------------------------
# emulation of the three arithmetics (fp16 operand splits, exact products, ONE fp32 rounding of every accumulated sum): what
# the error model must bound (tests/test_chain_units_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------
def emulate_chain(sd, masks, d_rgb, d_sigma, mode, stop_grad=False):
    """-> (stored [10] float16 (P, rows), pscale (10, P), gmax (10,) float32)"""
    f4, f8, f16 = np.float32, np.float64, np.float16
    mats = layer_mats(sd, stop_grad)
    keep = {p: ~np.asarray(masks[p], bool) for p in MASK_PANELS}
    keep[8] = True
    d_rgb, gs = np.asarray(d_rgb, f4), np.asarray(d_sigma, f4).reshape(-1)
    P = d_rgb.shape[0]
    wr = np.asarray(sd["rgb.0.weight"], f4)
    wsig = np.asarray(sd["sigma.weight"], f4).reshape(-1)
    v = wr[0][None, :] * d_rgb[:, 0:1]
    for c in (1, 2):
        v = (wr[c][None, :].astype(f8) * d_rgb[:, c:c + 1].astype(f8) + v.astype(f8)).astype(f4)
    dz = np.where(keep[9], v, f4(0))
    stored, ps, gmax = [None] * 10, np.ones((10, P)), np.zeros(10, f4)
    mxin = np.maximum(np.abs(gs), np.abs(dz).max(1)).astype(f8)
    S = np.where(mxin > 0, 2.0 ** (1 - floor_log2(np.where(mxin > 0, mxin, 1.0))), 1.0)
    hi, lo = split_f16((dz * S[:, None].astype(f4)).astype(f4))
    stored[9], ps[9], gmax[9] = hi, 1.0 / S, np.abs(dz).max()
    cinv, phi, mx_stored = 1.0 / S, np.ones(P), np.full(P, 3.0)
    for lam in range(9):
        pout, nt = 8 - lam, nt_of(mode, lam)
        Xhi, Xlo = split_f16(f4(64.0) * mats[lam].astype(f4))
        cinv = cinv / 64.0 / phi
        E = np.where(mx_stored > 0, floor_log2(np.where(mx_stored > 0, mx_stored, 1.0)) + 1, 2)
        phi = 2.0 ** np.clip(-4 - E, -14, 0)
        H, L = hi.astype(f8), lo.astype(f8)
        acc = H @ Xhi.astype(f8)
        if nt >= 2:
            acc = acc + H @ Xlo.astype(f8)
        if nt == 3:
            acc = acc + L @ Xhi.astype(f8)
        acc = acc.astype(f4)
        if lam == 1:
            sig = (gs.astype(f8) / cinv).astype(f4)
            acc = (wsig[None, :].astype(f8) * sig[:, None].astype(f8) + acc.astype(f8)).astype(f4)
        x = np.where(keep[pout], acc, f4(0))
        mx = np.abs(x).max(1).astype(f8)
        gmax[pout] = (mx * cinv).max()
        phi4 = phi[:, None].astype(f4)
        hi = x.astype(f16) * phi4.astype(f16)
        lo = ((x * phi4).astype(f4) - hi.astype(f4)).astype(f16)
        stored[pout], ps[pout] = hi, cinv / phi
        mx_stored = mx * phi
    return stored, ps, gmax


# ------------------------------------------------------------------------------------------------------------------------
# operands of the exact regime
# ------------------------------------------------------------------------------------------------------------------------
# special points of every case (all below 32, so they exist at every P and share a wave with the whole range of scales)
PT_ALL_ZERO, PT_SIGMA_ONLY, PT_DEAD_AT_4 = 3, 5, 7
BLOCK_ALL_SET, BLOCK_ALL_CLEAR = (5, 2), (2, 5)     # (panel, 32-feature block)
EXACT_CASES = OrderedDict((f"P{P}", dict(P=P, seed=100 + P)) for P in (32, 128, 160, 288, 544))


def exact_case(P, seed):
    """-> (sd, masks, d_rgb (P, 3), d_sigma (P,)), float32 / bool.

    Every matrix the chain reads is a signed selection times a power of two in {1/4 .. 4}: column n of M_lam (output feature n)
    has ONE non-zero, in row k(n), and k is onto the layer's K inputs -- a dropped, duplicated or misrouted k-step or block
    changes a visible output.  64 W is exact in fp16, so every lo piece of the stream is zero.  The exponents are chosen so that
    the cumulative power of two of any path from the colour head to a feature stays in {1/2, 1, 2} (the range of one point's
    gradients stays far inside fp16's at the point's scale).  rgb.weight, sigma.weight, d_rgb, d_sigma are integers of
    magnitude <= 3 / 3 / 4 / 4, the inputs times the point's own power of two (2^-40 .. 2^20 inside every wave): |dzc| <= 36,
    and below the density head |2^c (+-2^c' dzc + wsigma d_sigma)| <= 2 (72 + 12) in units of 1/4 -- at most 10 bits.
    Everything the chain must NOT read is SENTINEL: columns 0..62 of the skip layer, columns 256..282 of dir_encoding.weight,
    xyz_encoding_1.weight, all biases."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict((k, np.full(shape, SENTINEL, np.float32)) for k, shape in STATE_DICT_SPEC.items())
    cum_in = np.zeros(128, np.int64)                   # cumulative exponent of the layer's input features
    for lam in range(9):
        K = 128 if lam == 0 else 256
        k_of = rng.permutation(256) % K                # onto
        cum_out = rng.integers(-1, 2, 256)
        val = rng.choice([-1.0, 1.0], 256) * 2.0 ** (cum_out - cum_in[k_of])     # exponents in -2 .. 2
        M = np.zeros((K, 256), np.float32)
        M[k_of, np.arange(256)] = val
        if lam == 0:
            sd["dir_encoding.0.weight"][:, :256] = M
        elif lam == 1:
            sd["xyz_encoding_final.weight"][:] = M
        elif lam == 5:
            sd["xyz_encoding_5.0.weight"][:, 63:] = M
        else:
            sd[f"xyz_encoding_{10 - lam}.0.weight"][:] = M
        cum_in = cum_out
    sd["rgb.0.weight"][:] = rng.integers(-3, 4, (3, 128))
    sd["sigma.weight"][:] = rng.integers(-3, 4, (1, 256))
    masks = {p: rng.random((P, PANEL_ROWS[p])) < 0.5 for p in MASK_PANELS}
    pa, ba = BLOCK_ALL_SET
    masks[pa][:, 32 * ba:32 * ba + 32] = True
    pa, ba = BLOCK_ALL_CLEAR
    masks[pa][:, 32 * ba:32 * ba + 32] = False
    masks[3][PT_DEAD_AT_4] = True                      # trunk layer 4's ReLU zeroed the whole point: panels 3..0 are exact zeros
    scale = 2.0 ** (-40 + 2 * np.minimum(np.arange(P) % 32, 30)).astype(np.float64)
    d_rgb = rng.integers(-4, 5, (P, 3)).astype(np.float64)
    d_sigma = rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], P).astype(np.float64)
    d_rgb[PT_ALL_ZERO], d_sigma[PT_ALL_ZERO] = 0.0, 0.0
    d_rgb[PT_SIGMA_ONLY] = 0.0
    return sd, masks, (d_rgb * scale[:, None]).astype(np.float32), (d_sigma * scale).astype(np.float32)


def real_case(P, seed):
    """make_state_dict weights, Bernoulli(1/2) masks, randn inputs times per-point scales 2^-30 .. 2^10"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = make_state_dict(seed=seed)
    masks = {p: rng.random((P, PANEL_ROWS[p])) < 0.5 for p in MASK_PANELS}
    scale = 2.0 ** rng.integers(-30, 11, P)
    d_rgb = (rng.standard_normal((P, 3)) * scale[:, None]).astype(np.float32)
    d_sigma = (rng.standard_normal(P) * scale).astype(np.float32)
    return sd, masks, d_rgb, d_sigma
