"""Restatement of the chain path's ray gradient (csrc/nsr_train_raygrad_f16.hip; include/nsr_train.h, nsr_train_backward_r) in
numpy float64: from the backward chain's gradient panels (the STORED fp16 values, tests/chain_ref.decode_panels' form), their
per-point power-of-two scales, the weights, the rays and the depths to the rows of d(loss) / d(rays).

    g_pe (P, 63) = dz_1 W_1 + dz_5 W_5[:, 0:63]        g_de (P, 27) = dz_dir W_dir[:, 256:283]       dz = stored x pscale
    g_x = backward of [x, sin(2^k x), cos(2^k x)] at x = o + z d;   g_dv = the same of the direction encoding, per point
    row = [sum_k g_x | sum_k z g_x (+ sum_k g_dv at 8 columns) | 0 0 | sum_k g_dv at 11 columns]

The reference of tests/test_chain_ray_grads_cpu.py (against torch autograd) and tests/test_gpu_chain_ray_grad_units.py.
``variant`` selects a deliberately WRONG form, for the test that the restatement tells them apart."""
import numpy as np

VARIANTS = ("skip_cols", "dir_cols", "no_pscale", "swap_sincos", "no_z")
PANEL_1, PANEL_5, PANEL_DIR = 0, 4, 9      # gradient panels of trunk layer 1, of the skip layer, of dir_encoding
W_1, W_5, W_DIR = "xyz_encoding_1.0.weight", "xyz_encoding_5.0.weight", "dir_encoding.0.weight"


def encoded_columns(panels, pscale, sd, stop_grad=False, variant=None):
    """(g_pe (P, 63), g_de (P, 27) or None) in float64.  panels[p]: (P, rows) stored values; pscale: (10, >= P)."""
    f8 = np.float64
    P = np.asarray(panels[PANEL_1]).shape[0]
    ps = np.ones((10, P)) if variant == "no_pscale" else np.asarray(pscale, f8)[:, :P]
    dz = lambda p: np.asarray(panels[p], f8) * ps[p][:, None]
    w1, w5, wd = (np.asarray(sd[k], f8) for k in (W_1, W_5, W_DIR))
    c5 = 63 if variant == "skip_cols" else 0
    g_pe = dz(PANEL_1) @ w1 + dz(PANEL_5) @ w5[:, c5:c5 + 63]
    if stop_grad:
        return g_pe, None
    cd = 0 if variant == "dir_cols" else 256
    return g_pe, dz(PANEL_DIR) @ wd[:, cd:cd + 27]


def posenc64(x, deg):
    """[x, sin(2^k x), cos(2^k x)]_k in float64"""
    x = np.asarray(x, np.float64)
    return np.concatenate([x] + [f(2.0 ** k * x) for k in range(deg) for f in (np.sin, np.cos)], -1)


def encode_bwd(g, enc, deg, variant=None):
    """(n, 3) from the gradients g (n, 3 + 6 deg) of the encoded columns and the encoded rows enc (n, 3 + 6 deg)"""
    g, enc = np.asarray(g, np.float64), np.asarray(enc, np.float64)
    out = g[:, 0:3].copy()
    for k in range(deg):
        c = 3 + 6 * k
        sn, cs = enc[:, c:c + 3], enc[:, c + 3:c + 6]
        if variant == "swap_sincos":
            sn, cs = cs, sn
        out += 2.0 ** k * (g[:, c:c + 3] * cs - g[:, c + 3:c + 6] * sn)
    return out


def points_f32(rays, z):
    """o + z d as the kernels form it: one fp32 multiply, one fp32 add"""
    rays, z = np.asarray(rays, np.float32), np.asarray(z, np.float32)
    return (rays[:, None, 0:3] + z[:, :, None] * rays[:, None, 3:6]).astype(np.float32).reshape(-1, 3)


def rows(panels, pscale, sd, rays, z, stop_grad=False, enc_pos=None, enc_dir=None, variant=None, per_point_f32=False):
    """(R, stride) float64 rows.  rays (R, 8 | 11), z (R, N).  enc_pos (R N, 63) / enc_dir (R, 27): the encodings to differentiate
    at (default: float64 sin / cos of the fp32 sample points / of the direction).  per_point_f32: g_x and g_dv are rounded to fp32
    per point, as the kernel stores them, before the per-ray sums."""
    rays, z = np.asarray(rays), np.asarray(z, np.float64)
    R, N = z.shape
    stride = rays.shape[1]
    g_pe, g_de = encoded_columns(panels, pscale, sd, stop_grad, variant)
    if enc_pos is None:
        enc_pos = posenc64(points_f32(rays, z), 10)
    g_x = encode_bwd(g_pe, enc_pos, 10, variant)
    if per_point_f32:
        g_x = g_x.astype(np.float32).astype(np.float64)
    g_x = g_x.reshape(R, N, 3)
    out = np.zeros((R, stride))
    out[:, 0:3] = g_x.sum(1)
    out[:, 3:6] = g_x.sum(1) if variant == "no_z" else (z[:, :, None] * g_x).sum(1)
    if g_de is not None:
        if enc_dir is None:
            enc_dir = posenc64(np.asarray(rays, np.float32)[:, 8:11] if stride == 11 else np.asarray(rays, np.float32)[:, 3:6], 4)
        g_dv = encode_bwd(g_de, np.repeat(np.asarray(enc_dir, np.float64), N, axis=0), 4, variant)
        if per_point_f32:
            g_dv = g_dv.astype(np.float32).astype(np.float64)
        dv = g_dv.reshape(R, N, 3).sum(1)
        if stride == 8:
            out[:, 3:6] += dv
        else:
            out[:, 8:11] = dv
    return out
