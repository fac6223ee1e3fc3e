"""The launcher of the chain path's ray gradient alone (csrc/nsr_train_raygrad_f16.hip: raygrad_f16_pack, raygrad_f16, through
tests/csrc/nsr_test_hooks_chain_raygrad.hip) against the float64 restatement tests/chain_ray_grads_ref.py.  The gradient panels
are built with tests/chain_ref.encode_panels, so what the kernel reads is the backward chain's documented layout.

Exact regime (bit for bit): panel values are integers of magnitude <= 8, weights integers of magnitude <= 4 (64 w is exact in
fp16: every lo half is zero), pscale in {2^-3, 1, 2^2} varying per point and panel, o = d = 0 (every sin is 0, every cos 1).  A
panel's partial sum is an integer <= 256 x 8 x 256 = 2^19 in units of the weight scale: no fp32 accumulation rounds; g_x = g_id +
sum_k 2^k g_sin,k is a multiple of 2^-3 below 2^27, exact in the kernel's double arithmetic, then rounded ONCE to fp32 per point
(the (P, 3) matrices) and ONCE per row after the per-ray sums in double, which do not round either (depths are k / 16)."""
from collections import OrderedDict
from ctypes import POINTER, c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import STATE_DICT_SPEC, make_state_dict
from tests import chain_ray_grads_ref as cr
from tests import chain_ref

pytestmark = pytest.mark.gpu

KEYS = list(STATE_DICT_SPEC)
POISON = np.float32(1.0e30)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from tests import hooks
    h = hooks.load()
    h.nsr_test_chain_raygrad_image_floats.restype, h.nsr_test_chain_raygrad_image_floats.argtypes = c_int64, []
    h.nsr_test_chain_raygrad_pack.restype, h.nsr_test_chain_raygrad_pack.argtypes = c_int, [POINTER(c_void_p), c_void_p, POINTER(c_void_p),
                                                                                            c_void_p, c_void_p]
    h.nsr_test_chain_raygrad.restype, h.nsr_test_chain_raygrad.argtypes = c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                                                                  c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                                                  c_int, c_void_p]
    return h


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _pack(lib, sd):
    """the packed weight columns of sd (as both networks; the coarse image is returned)"""
    w = [torch.from_numpy(np.ascontiguousarray(sd[k], np.float32)).cuda() for k in KEYS]
    ptrs = (c_void_p * 24)(*[c_void_p(t.data_ptr()) for t in w])
    n = lib.nsr_test_chain_raygrad_image_floats()
    assert n == 144 * 256
    img = [torch.full((n,), float("nan"), device="cuda") for _ in range(2)]
    assert lib.nsr_test_chain_raygrad_pack(ptrs, c_void_p(img[0].data_ptr()), ptrs, c_void_p(img[1].data_ptr()), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(img[0].view(torch.int32), img[1].view(torch.int32))
    return img[0]


def _run(lib, img, panels, pscale, rays, z, stop_grad=False, acc=0, prev=None):
    """-> the (R, stride) rows; four guard rows behind them must stay 7.0"""
    R, N = z.shape
    P, stride = R * N, rays.shape[1]
    ng = chain_ref.n_groups(P)
    pan = torch.from_numpy(chain_ref.encode_panels(panels, P).copy()).cuda()
    ps = np.full((10, ng * 32), np.nan, np.float32)      # padding points: never read
    ps[:, :P] = pscale
    psd, rd, zd = torch.from_numpy(ps).cuda(), torch.from_numpy(rays).cuda(), torch.from_numpy(np.ascontiguousarray(z, np.float32)).cuda()
    gx, gdv = torch.full((P + 4, 3), 7.0, device="cuda"), torch.full((P + 4, 3), 7.0, device="cuda")
    out = torch.full((R + 4, stride), 7.0, device="cuda")
    out[:R] = torch.from_numpy(prev).cuda() if acc else float("nan")
    rc = lib.nsr_test_chain_raygrad(c_void_p(img.data_ptr()), c_void_p(pan.data_ptr()), c_void_p(psd.data_ptr()), c_void_p(rd.data_ptr()),
                                    stride, c_void_p(zd.data_ptr()), R, N, int(stop_grad), c_void_p(gx.data_ptr()),
                                    c_void_p(gdv.data_ptr()), c_void_p(out.data_ptr()), acc, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[R:] == 7.0).all(), "guard rows behind g_rays"
    assert bool((gx[P:] == 7.0).all()) and bool((gdv[P:] == 7.0).all()), "guard rows behind the per-point matrices"
    return got[:R]


def _exact_inputs(seed, R, N):
    rng = np.random.default_rng(seed)
    P = R * N
    sd = OrderedDict((k, np.full(s, POISON, np.float32)) for k, s in STATE_DICT_SPEC.items())      # nothing else may be read
    sd[cr.W_1] = rng.integers(-4, 5, (256, 63)).astype(np.float32)
    sd[cr.W_5] = rng.integers(-4, 5, (256, 319)).astype(np.float32)      # columns 63: are non-zero and must not be read
    sd[cr.W_DIR] = rng.integers(-4, 5, (128, 283)).astype(np.float32)    # as are columns 0:256
    panels = [rng.integers(-8, 9, (P, rows)).astype(np.float16) for rows in chain_ref.PANEL_ROWS]      # panels 1-3, 5-8 too
    pscale = rng.choice([2.0 ** -3, 1.0, 2.0 ** 2], (10, P)).astype(np.float32)
    z = (rng.integers(32, 97, (R, N)) / 16.0).astype(np.float32)
    return sd, panels, pscale, z


@pytest.mark.parametrize("R,N", ((4, 8), (2, 48), (5, 32)))      # P = 32; 96: a ray starts mid-group; 160: a second, part-filled workgroup
@pytest.mark.parametrize("stride", (8, 11))
def test_mfma_stage_bit_exact(lib, R, N, stride):
    sd, panels, pscale, z = _exact_inputs(1000 * R + N + stride, R, N)
    img = _pack(lib, sd)
    rays = np.zeros((R, stride), np.float32)
    rays[:, 6:8] = (2.0, 6.0)
    want = cr.rows(panels, pscale, sd, rays, z, per_point_f32=True).astype(np.float32)
    # the integer form of the same thing, spelled out: sin = 0 and cos = 1 leave g_id + sum_k 2^k g_sin,k
    g_pe, g_de = cr.encoded_columns(panels, pscale, sd)
    g_x = g_pe[:, 0:3] + sum(2.0 ** k * g_pe[:, 3 + 6 * k:6 + 6 * k] for k in range(10))
    g_dv = g_de[:, 0:3] + sum(2.0 ** k * g_de[:, 3 + 6 * k:6 + 6 * k] for k in range(4))
    assert (g_x * 8 == np.round(g_x * 8)).all() and np.abs(g_x).max() < 2.0 ** 27
    f32 = lambda a: a.astype(np.float32).astype(np.float64).reshape(R, N, 3)
    ints = np.zeros((R, stride))
    ints[:, 0:3] = f32(g_x).sum(1)
    ints[:, 3:6] = (z[:, :, None].astype(np.float64) * f32(g_x)).sum(1)
    ints[:, (slice(3, 6) if stride == 8 else slice(8, 11))] += f32(g_dv).sum(1)
    assert np.array_equal(ints.astype(np.float32), want)
    got = _run(lib, img, panels, pscale, rays, z)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (R, N, stride, np.abs(got - want).max())
    assert (got[:, 6:8] == 0).all() and np.abs(got[:, :6]).max() > 0
    # what must not be read was not: other panels, the other columns (POISON elsewhere would have shown as inf / NaN)
    assert np.isfinite(got).all()
    for variant in cr.VARIANTS:
        if variant == "swap_sincos":
            continue      # at sin = 0, cos = 1 the swapped form is another integer form; the real-valued test sees it
        assert not np.array_equal(cr.rows(panels, pscale, sd, rays, z, per_point_f32=True, variant=variant).astype(np.float32), want), variant


def _real_inputs(seed, R, N, stride):
    rng = np.random.default_rng(seed)
    P = R * N
    sd = make_state_dict(seed=seed)
    panels = [(rng.standard_normal((P, rows)) * 2.5).astype(np.float16) for rows in chain_ref.PANEL_ROWS]
    pscale = (2.0 ** rng.integers(-12, 3, (10, P))).astype(np.float32)
    rays = np.zeros((R, stride), np.float32)
    rays[:, 0:3] = rng.uniform(-1, 1, (R, 3))
    d = rng.standard_normal((R, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 6:8] = (2.0, 6.0)
    if stride == 11:
        v = rng.standard_normal((R, 3))
        rays[:, 8:11] = v / np.linalg.norm(v, axis=1, keepdims=True)
    z = np.sort(rng.uniform(2.0, 6.0, (R, N)), 1).astype(np.float32)
    return sd, panels, pscale, rays, z


def _device_encodings(rays, z):
    """the stand-alone encoder's own fp32 sin / cos (nsr_posenc: bit-identical to the in-kernel expression)"""
    from nerf_sr_amd import ops
    x = torch.from_numpy(cr.points_f32(rays, z)).cuda()
    v = torch.from_numpy(np.ascontiguousarray(rays[:, 8:11] if rays.shape[1] == 11 else rays[:, 3:6])).cuda()
    return ops.PositionalEncoding(3, 10)(x).cpu().numpy(), ops.PositionalEncoding(3, 4)(v).cpu().numpy()


BOUND = 1e-5      # of each block's norm: ~90 fp32 roundings of 2^-24 are 5e-6 at the worst; twice that


def _blocks(got, want):
    rel = lambda a, b: float(np.linalg.norm(got[:, a:b].astype(np.float64) - want[:, a:b]) / np.linalg.norm(want[:, a:b]))
    res = {"g_o": rel(0, 3), "g_d": rel(3, 6)}
    if got.shape[1] == 11 and np.linalg.norm(want[:, 8:11]) > 0:
        res["g_v"] = rel(8, 11)
    return res


@pytest.mark.parametrize("R,N", ((4, 8), (2, 48), (3, 64)))
@pytest.mark.parametrize("stride", (8, 11))
def test_whole_launcher_on_real_values(lib, R, N, stride):
    sd, panels, pscale, rays, z = _real_inputs(50 + R + stride, R, N, stride)
    img = _pack(lib, sd)
    enc_pos, enc_dir = _device_encodings(rays, z)
    want = cr.rows(panels, pscale, sd, rays, z, enc_pos=enc_pos, enc_dir=enc_dir)
    got = _run(lib, img, panels, pscale, rays, z)
    fig = _blocks(got, want)
    print(f"chain ray gradient launcher, R={R} N={N} stride={stride}: {fig}")
    assert max(fig.values()) <= BOUND, (R, N, stride, fig)
    swapped = cr.rows(panels, pscale, sd, rays, z, enc_pos=enc_pos, enc_dir=enc_dir, variant="swap_sincos")
    assert max(_blocks(got, swapped).values()) > 1e-2


def test_options(lib):
    R, N = 2, 48
    sd, panels, pscale, rays, z = _real_inputs(77, R, N, 11)
    img = _pack(lib, sd)
    enc_pos, enc_dir = _device_encodings(rays, z)
    full = _run(lib, img, panels, pscale, rays, z)
    # stop_grad: exact zeros in the direction part, the rest unchanged
    sg = _run(lib, img, panels, pscale, rays, z, stop_grad=True)
    assert (sg[:, 8:11] == 0).all() and not np.signbit(sg[:, 6:11]).any() and np.array_equal(sg[:, :6], full[:, :6])
    assert np.abs(full[:, 8:11]).max() > 0
    # stride 11 puts the direction term in 8:11 and nothing of it in 3:6: the point part alone is the stop_grad row at stride 8
    rays8 = np.ascontiguousarray(rays[:, :8])
    sg8 = _run(lib, img, panels, pscale, rays8, z, stop_grad=True)
    assert np.array_equal(sg8[:, :6], full[:, :6])
    # at 8 columns the direction term (of d) joins 3:6
    full8 = _run(lib, img, panels, pscale, rays8, z)
    assert np.array_equal(full8[:, :3], full[:, :3]) and not np.array_equal(full8[:, 3:6], full[:, 3:6])
    enc_d8 = _device_encodings(rays8, z)[1]
    fig = _blocks(full8, cr.rows(panels, pscale, sd, rays8, z, enc_pos=enc_pos, enc_dir=enc_d8))
    assert max(fig.values()) <= BOUND, fig
    # accumulate: the fine pass adds onto the coarse rows, one fp32 addition per element; columns 6:8 stay zero
    prev = np.random.default_rng(3).integers(-50, 51, (R, 11)).astype(np.float32)
    prev[:, 6:8] = 0.0
    acc = _run(lib, img, panels, pscale, rays, z, acc=1, prev=prev)
    assert np.array_equal(acc, (prev + full).astype(np.float32)) and (acc[:, 6:8] == 0).all()


def test_launcher_refuses_what_it_cannot_run(lib):
    t = torch.zeros(1 << 16, device="cuda")
    p = c_void_p(t.data_ptr())
    s = _stream()
    assert lib.nsr_test_chain_raygrad(p, p, p, p, 9, p, 4, 8, 0, p, p, p, 0, s) == -1       # stride 9
    assert lib.nsr_test_chain_raygrad(p, p, p, None, 8, p, 4, 8, 0, p, p, p, 0, s) == -1    # no rays
    assert lib.nsr_test_chain_raygrad(p, p, p, p, 8, p, 3, 8, 0, p, p, p, 0, s) == -2       # 24 points: no whole 32-point group
    assert lib.nsr_test_chain_raygrad(p, p, p, p, 8, p, 0, 8, 0, p, p, p, 0, s) == 0        # nothing to do
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0
