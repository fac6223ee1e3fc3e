"""CPU checks of the backward chain's reference (tests/chain_ref.py), on which every assertion of tests/test_gpu_chain_units.py
rests: the panel decoder and sign-word encoder against their inverses and against a thread-by-thread restatement of the test
writer pack_panel_kernel; the fp64 chain against torch.autograd through the oracle's network; the exact regime of every case
in the table; the error model against an emulation of the three arithmetics."""
import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import STATE_DICT_SPEC, make_state_dict
from oracle import nerf_oracle
from tests import chain_ref as cr


def _random_masks(rng, P):
    return {p: rng.random((P, cr.PANEL_ROWS[p])) < 0.5 for p in cr.MASK_PANELS}


# ------------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------------
def _pack_panel_threads(src_u16, n_groups, rows, panel_u8, gbytes):
    """tests/csrc/nsr_test_hooks.hip::pack_panel_kernel, one loop iteration per thread, same arithmetic"""
    dst16 = panel_u8.view(np.uint16)
    ld = src_u16.shape[1]
    flat = src_u16.reshape(-1)
    for t in range(n_groups * (rows // 16) * 64):
        lane, unit = t & 63, t >> 6
        m, h = lane & 31, lane >> 5
        g, ub = divmod(unit, rows // 16)
        blk, u = ub >> 1, ub & 1
        p = (32 * g + m) * ld + 32 * blk + 16 * u + 4 * h
        v = [flat[p + 0], flat[p + 1], flat[p + 2], flat[p + 3], flat[p + 8], flat[p + 9], flat[p + 10], flat[p + 11]]
        byte = g * gbytes + 32 * blk * 64 + 1024 * u + 16 * ((2 * m + h) ^ (8 * u))
        dst16[byte // 2:byte // 2 + 8] = v


@pytest.mark.parametrize("P", (32, 160))
def test_panel_decoder_inverts_the_panel_writer(P):
    rng = np.random.Generator(np.random.PCG64(1))
    ng = cr.n_groups(P)
    want = [rng.integers(0, 0x7C00, (ng * 32, rows), dtype=np.uint16) for rows in cr.PANEL_ROWS]   # all points: distinct finite halves
    buf = np.zeros(cr.BWD_ROWS * 64 * ng, np.uint8)
    for panel, rows in enumerate(cr.PANEL_ROWS):
        first = 256 * panel * 64 * ng                                              # panel_rows_before * 64 * n_groups
        _pack_panel_threads(want[panel], ng, rows, buf[first:first + rows * 64 * ng], rows * 64)
    got = cr.decode_panels(buf, P)
    for panel in range(10):
        assert got[panel].shape == (P, cr.PANEL_ROWS[panel])
        assert np.array_equal(got[panel].view(np.uint16), want[panel][:P]), panel
    # and the decoder's own inverse
    again = cr.decode_panels(cr.encode_panels(got, P), P)
    assert all(np.array_equal(a.view(np.uint16), b.view(np.uint16)) for a, b in zip(again, got))


def test_sign_encoder_bit_positions_and_round_trip():
    P = 160
    rng = np.random.Generator(np.random.PCG64(2))
    masks = _random_masks(rng, P)
    words = cr.encode_signs(masks, P)
    assert words.shape == (cr.n_groups(P) * 34 * 64,)
    back = cr.decode_signs(words, P)
    assert all(np.array_equal(back[p], masks[p]) for p in cr.MASK_PANELS)
    # one bit at a time, from the documented layout: point (group, m), panel, feature -> (pair, lane, bit)
    for panel, point, feat in ((0, 0, 0), (3, 37, 100), (7, 159, 255), (9, 64, 127), (9, 5, 33), (5, 131, 68)):
        one = {p: np.zeros((P, cr.PANEL_ROWS[p]), bool) for p in cr.MASK_PANELS}
        one[panel][point, feat] = True
        w = cr.encode_signs(one, P, pad=False).reshape(-1, 34, 64)
        nb, f = divmod(feat, 32)
        h = (f >> 2) & 1
        r = 4 * (f >> 3) + (f & 3)
        pair = (32 if panel == 9 else 4 * panel) + (nb >> 1)
        bit = (31 - r) if nb % 2 == 0 else (15 - r)
        want = np.zeros_like(w)
        want[point // 32, pair, (point % 32) + 32 * h] = np.uint32(1) << np.uint32(bit)
        assert np.array_equal(w, want), (panel, point, feat)
    # padding points carry "zeroed" everywhere
    pad = cr.decode_signs(cr.encode_signs(masks, P), cr.n_groups(P) * 32)
    assert all(pad[p][P:].all() for p in cr.MASK_PANELS)


def test_stream_packer_layout_spot_checks():
    """a handful of words of the numpy packer from the documented piece layout, element by element"""
    sd = make_state_dict(seed=5)
    for mode, stop_grad in ((3, 0), (1, 0), (12, 0), (2, 1)):
        words = cr.pack_stream(sd, mode, bool(stop_grad))
        assert words.size == cr.stream_pieces(mode) * 256 + 768
        mats = cr.layer_mats(sd, bool(stop_grad))
        piece = 0
        for lam in range(9):
            two = cr.nt_of(mode, lam) > 1
            for nb, s, part, lane, jj in ((0, 0, 0, 0, 0), (3, 7, 1, 45, 2), (7, 15, 0, 63, 3), (5, 9, 1, 17, 1)):
                if part and not two:
                    continue
                idx = piece + (nb * 16 + s) * (2 if two else 1) + part
                i, h = lane & 31, lane >> 5
                vals = []
                for j in (2 * jj, 2 * jj + 1):
                    k = cr.act_feature(8 * s + j, h)
                    x = np.float32(64.0) * (mats[lam][k, 32 * nb + i] if k < mats[lam].shape[0] else np.float32(0))
                    hi = np.float16(x)
                    vals.append(np.float16(x - np.float32(hi)) if part else hi)
                want = int(vals[0].view(np.uint16)) | (int(vals[1].view(np.uint16)) << 16)
                assert int(words[idx * 256 + lane * 4 + jj]) == want, (mode, lam, nb, s, part, lane, jj)
            piece += 256 if two else 128
        aux = words[cr.stream_pieces(mode) * 256:].view(np.float32)
        assert np.array_equal(aux[:512].reshape(128, 4)[:, :3], sd["rgb.0.weight"].T) and not aux[:512].reshape(128, 4)[:, 3].any()
        assert np.array_equal(aux[512:], sd["sigma.weight"].reshape(-1))
    assert np.array_equal(cr.pack_stream(sd, 2), cr.pack_stream(sd, 3))


# ------------------------------------------------------------------------------------------------------------------------
# the fp64 chain = autograd through the oracle's network
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stop_grad", (False, True))
def test_reference_chain_equals_autograd(stop_grad):
    P = 6
    rng = np.random.Generator(np.random.PCG64(7 + stop_grad))
    sd = {k: rng.standard_normal(shape) * (2.0 / shape[-1]) ** 0.5 for k, shape in STATE_DICT_SPEC.items()}   # float64, biases too
    x = rng.standard_normal((P, 90))
    d_rgb, d_sigma = rng.standard_normal((P, 3)), rng.standard_normal(P)

    # masks of the forward pass: the pre-activations, restated here and checked against the oracle's outputs
    pe, h, masks = x[:, :63], x[:, :63], {}
    for l in range(1, 9):
        z = (np.concatenate([pe, h], 1) if l == 5 else h) @ sd[f"xyz_encoding_{l}.0.weight"].T + sd[f"xyz_encoding_{l}.0.bias"]
        masks[l - 1], h = z < 0, np.maximum(z, 0)
    gfin = h @ sd["xyz_encoding_final.weight"].T + sd["xyz_encoding_final.bias"]
    zc = np.concatenate([gfin, x[:, 63:]], 1) @ sd["dir_encoding.0.weight"].T + sd["dir_encoding.0.bias"]
    masks[9] = zc < 0
    out_np = np.concatenate([np.maximum(zc, 0) @ sd["rgb.0.weight"].T + sd["rgb.0.bias"], h @ sd["sigma.weight"].T + sd["sigma.bias"]], 1)

    got = cr.ref_chain(sd, masks, d_rgb, d_sigma, stop_grad=stop_grad)
    tsd = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    bias_of = [f"xyz_encoding_{l}.0.bias" for l in range(1, 9)] + ["xyz_encoding_final.bias", "dir_encoding.0.bias"]
    for p in range(P):                                   # one point at a time: the bias gradients ARE the panels' rows
        out = nerf_oracle.mlp_forward(tsd, torch.tensor(x[p:p + 1]), color_activation="none", stop_grad=stop_grad)
        assert np.allclose(out.detach().numpy(), out_np[p:p + 1], rtol=1e-12, atol=1e-14)
        loss = (out[0, :3] * torch.tensor(d_rgb[p])).sum() + out[0, 3] * d_sigma[p]
        grads = torch.autograd.grad(loss, [tsd[k] for k in bias_of], allow_unused=True)
        for panel, gr in enumerate(grads):
            want = np.zeros(cr.PANEL_ROWS[panel]) if gr is None else gr.numpy()
            assert gr is not None or (stop_grad and panel == 8)
            scale = max(np.abs(want).max(), 1e-300)
            assert np.abs(got[panel][p] - want).max() <= 1e-12 * scale, (p, panel)
    if stop_grad:
        assert not got[8].any()


# ------------------------------------------------------------------------------------------------------------------------
# the exact regime
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cr.EXACT_CASES))
@pytest.mark.parametrize("stop_grad", (False, True))
def test_exact_cases_stay_inside_eleven_bits(name, stop_grad):
    case = cr.EXACT_CASES[name]
    sd, masks, d_rgb, d_sigma = cr.exact_case(**case)
    g = cr.ref_chain(sd, masks, d_rgb, d_sigma, stop_grad=stop_grad)
    ps = cr.assert_exact_regime(g, d_sigma, name)
    assert (np.log2(ps) % 1 == 0).all()
    # what the builder promises
    for lam, M in enumerate(cr.layer_mats(sd)):
        assert ((M != 0).sum(0) == 1).all() and (M != 0).any(1).all(), lam          # one per output feature, onto the inputs
        assert set(np.abs(M[M != 0]).tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0}
    for mode in cr.MODES:                                                            # every lo piece is zero
        w = cr.pack_stream(sd, mode, stop_grad)
        if mode != 1:
            pcs = w[:1536 * 256].reshape(-1, 2, 256)
            assert not pcs[:, 1].any()
    with np.errstate(over="ignore"):
        assert not np.isfinite((np.float32(64.0) * cr.SENTINEL).astype(np.float16))
    assert not g[9][cr.PT_ALL_ZERO].any() and not g[7][cr.PT_ALL_ZERO].any()
    assert not g[9][cr.PT_SIGMA_ONLY].any() and g[7][cr.PT_SIGMA_ONLY].any()
    assert g[4][cr.PT_DEAD_AT_4].any() and not any(g[p][cr.PT_DEAD_AT_4].any() for p in range(4))
    # the emulated arithmetic agrees with itself across the term settings and with the reference, bit for bit
    if case["P"] <= 160:
        for mode in cr.MODES:
            stored, eps, gmax = cr.emulate_chain(sd, masks, d_rgb, d_sigma, mode, stop_grad)
            assert np.array_equal(eps, ps), mode
            for panel in range(10):
                assert np.array_equal(stored[panel].astype(np.float64) * eps[panel][:, None], g[panel]), (mode, panel)
                assert gmax[panel] == np.float32(np.abs(g[panel]).max())


# ------------------------------------------------------------------------------------------------------------------------
# the error model bounds the emulated arithmetic
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cr.MODES)
def test_error_model_bounds_the_emulated_arithmetic(mode):
    sd, masks, d_rgb, d_sigma = cr.real_case(96, 21)
    g = cr.ref_chain(sd, masks, d_rgb, d_sigma)
    bound = cr.error_bounds(sd, masks, d_rgb, d_sigma, mode, g)
    literal = cr.error_bounds(sd, masks, d_rgb, d_sigma, mode, g, literal=True)
    stored, ps, _ = cr.emulate_chain(sd, masks, d_rgb, d_sigma, mode)
    for panel in range(10):
        assert (np.log2(ps[panel]) % 1 == 0).all()
        err = np.abs(stored[panel].astype(np.float64) * ps[panel][:, None] - g[panel])
        nz = bound[panel] > 0
        ratio = float((err[nz] / bound[panel][nz]).max())
        lit = float((err[nz] / literal[panel][nz]).max())
        print(f"terms {mode:2d} panel {panel}: emulated err / bound {ratio:.3f} (with 2^-12 |x| for half an fp16 ulp: {lit:.3f})")
        assert (err <= bound[panel]).all(), (mode, panel, ratio)
        assert not err[~nz].any()


def test_half_ulp_of_fp16_is_not_two_to_the_minus_twelve():
    """why error_bounds takes half an ulp (2^-12 x the power of two above |x|) and not 2^-12 |x| for one rounding to fp16: just
    above a power of two the rounding error of a CORRECT conversion is twice the latter"""
    x = np.float64(1.0 + 2.0 ** -11 + 2.0 ** -20)
    err = abs(np.float64(np.float16(x)) - x)
    assert 2.0 ** -12 * x < err <= cr.hulp16(x) <= 2.0 ** -11 * x
