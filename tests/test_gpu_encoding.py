"""The in-kernel positional encodings, bit for bit (reference: tests/encoding_ref.py, proven in tests/test_encoding_cpu.py).

Every ray-level kernel computes cast_rays and both encodings itself through ``nsr_sincos`` (csrc/nsr_common.h), in five
hand-copied places with their own maps from (frequency, lane half, component, sin / cos) to an operand register.  The function
is IEEE arithmetic in a fixed order, so the reference restates it in numpy and every sin / cos column is known exactly:

(a) the function itself, through a one-line kernel, over ~2.5M arguments;
(b) ``encode_arch`` (the layer-by-layer training path's encoder, run-time degree, several destinations);
(c) every ray-level entry point of the default network against ``VanillaMLP`` on the restated rows, dense random weights;
(d) one-hot networks: each raw output is one encoded column with its sign, so a wrong column names itself;
(e) the TRAIN forward's encoding panels 10 and 11, byte for byte.

Comparisons are on the uint32 images.  One exception, in (d): an expected zero may arrive with either sign (a one-hot network
returns relu(v) - relu(-v), which is +0 for v = -0).  The density-only pass has no raw output: its depth, opacity and weights are
compared with the stand-alone compositor on the rows route's density column."""
from ctypes import c_int, c_int64, c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import encoding_ref as enc
from tests import hooks
from tests.panel_layout import dircol as _dircol, panel_rows as _panel_rows, pecol as _pecol   # the panels' row order

pytestmark = pytest.mark.gpu

GUARD = 4096                     # elements (or bytes) behind every hook output that must keep their fill


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def hk():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return hooks.load()


def _nan(n):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")


def _bits_t(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _diff(name, got, want, zero_sign_free=False):
    """None if the float32 arrays agree in every bit (zero_sign_free: an expected zero may be +-0), else a line that says where."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape} != {want.shape}"
    same = got.view(np.uint32) == want.view(np.uint32)
    if zero_sign_free:
        same |= (want == 0) & (got == 0)
    if same.all():
        return None
    bad = np.argwhere(~same)
    i = tuple(bad[0])
    return (f"{name}: {len(bad)} of {want.size} elements differ, first at {i}: got {got[i]!r} ({got.view(np.uint32)[i]:#010x}), "
            f"want {want[i]!r} ({want.view(np.uint32)[i]:#010x}); columns {sorted(set(bad[:, -1].tolist()))[:12]}")


# ---------------------------------------------------------------------------------------------------------------------
# (a) the function
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(enc.sincos_sets()))
def test_sincos_bits(hk, name):
    """nsr_sincos per element over one argument set: both results equal the restatement in every bit (with
    tests/test_encoding_cpu.py this holds the device to the header's 1.5e-7 on the sets inside the claimed range); outside it
    only the bits are asked; on +-inf and NaN both results are NaN."""
    x = enc.sincos_sets()[name]
    n = x.size
    xd = torch.from_numpy(np.array(x)).cuda()
    sn, cs = _nan(n), _nan(n)
    assert hk.nsr_test_sincos(hooks.ptr(xd), n, hooks.ptr(sn), hooks.ptr(cs), hooks.stream()) == hooks.NSR_OK
    torch.cuda.synchronize()
    assert torch.isnan(sn[n:]).all() and torch.isnan(cs[n:]).all()
    got_s, got_c = sn[:n].cpu().numpy(), cs[:n].cpu().numpy()
    if name == "nonfinite":
        assert np.isnan(got_s).all() and np.isnan(got_c).all()
        return
    want_s, want_c = enc.nsr_sincos(x)
    bad = [_diff(f"{name} sin", got_s, want_s), _diff(f"{name} cos", got_c, want_c)]
    assert not any(bad), "\n".join(b for b in bad if b)
    if name == "special":
        assert got_s[:2].view(np.uint32).tolist() == [0, 0] and got_c[:2].tolist() == [1.0, 1.0]       # (+0, 1) at +-0
        assert np.array_equal(got_s[2:4].view(np.uint32), x[2:4].view(np.uint32))                      # a denormal is not flushed


# ---------------------------------------------------------------------------------------------------------------------
# (b) encode_arch
# ---------------------------------------------------------------------------------------------------------------------
ARCH_P = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("deg", (0, 1, 4, 10, 16))
def test_encode_arch_bits(hk, deg):
    """nsr::encode_arch at one degree: position and view-direction mode, stride 8 and 11, n_groups = ceil((3 + 6 deg) / 4) and
    three more, row stride 8 floats above 4 n_groups, 1 / 2 / 3 destinations, P in {1, 63, 64, 65, 257} with N in {1, 64}: the
    row equals encode_arch of the reference, zeros behind 3 + 6 deg, the NaN between the rows and behind the buffer survives,
    every destination holds the same bytes."""
    g_min = -(-(3 + 6 * deg) // 4)
    bad, n_launch = [], 0
    for stride in enc.STRIDES:
        for N in (1, 64):
            for P in ARCH_P:
                R = -(-P // N)
                rays, z = enc.make_rays(R, N, stride)
                z = z.reshape(-1)[:P]
                rays_d, z_d = torch.from_numpy(np.array(rays)).cuda(), torch.from_numpy(np.array(z)).cuda()
                for view_dir in (0, 1):
                    for n_groups in (g_min, g_min + 3):
                        want = enc.encode_arch(rays, z, N, deg, view_dir, n_groups, P)
                        assert not want[:, 3 + 6 * deg:].any()
                        ld = 4 * n_groups + 8
                        for n_dst in (1, 2, 3):
                            dst = [_nan(P * ld) for _ in range(n_dst)]
                            ptrs = (c_void_p * n_dst)(*[c_void_p(d.data_ptr()) for d in dst])
                            rc = hk.nsr_test_encode_arch(hooks.ptr(rays_d), stride, None if view_dir else hooks.ptr(z_d), P, N, deg,
                                                         view_dir, ptrs, n_dst, ld, n_groups, hooks.stream())
                            assert rc == hooks.NSR_OK
                            n_launch += 1
                            torch.cuda.synchronize()
                            name = f"deg {deg} stride {stride} N {N} P {P} view {view_dir} groups {n_groups} dst {n_dst}"
                            first = dst[0].cpu().numpy()
                            rows = first[:P * ld].reshape(P, ld)
                            bad.append(_diff(name, rows[:, :4 * n_groups], want))
                            if not (np.isnan(rows[:, 4 * n_groups:]).all() and np.isnan(first[P * ld:]).all()):
                                bad.append(f"{name}: wrote outside its columns")
                            for d in dst[1:]:
                                if not np.array_equal(d.cpu().numpy().view(np.uint32), first.view(np.uint32)):
                                    bad.append(f"{name}: destinations differ")
    bad = [b for b in bad if b]
    assert n_launch == 240 and not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------------------------------------------------------------
# (c) the ray route against the rows route
# ---------------------------------------------------------------------------------------------------------------------
def _net(ops, sd, precision):
    return ops.VanillaMLP(SimpleNamespace(color_activation="none"), precision=precision).load_state_dict(sd)


def _wide(hk):
    fn = hk.nsr_test_f16x3_render_composite_wide            # tests/csrc/nsr_test_hooks_testtime.hip
    fn.restype = c_int
    fn.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int] + [c_void_p] * 7
    return fn


def _shapes(precision):
    return enc.SHAPES if precision == "f16x3" else enc.SHAPES[:1]


@pytest.mark.parametrize("precision", enc.PRECISIONS)
def test_ray_route_equals_rows_route(ops, hk, precision):
    """A dense random network; 5 x 64 (f16x3 also 2 x 128) at stride 8 and at stride 11 with its own view direction: the raw
    (R N, 4) output of ops.render_rays, of ops.render_rays_composited(want_raw=True) (fp32 at 64 samples, f16x3), of the wide
    compositing hook (f16x3, 5 x 192 and 5 x 256) equals VanillaMLP on encode_rays(rays, z) in every bit; the density-only pass
    (f16x3) returns the stand-alone compositor's depth, opacity and weights of the rows route's density; status words 0.
    Teeth on the device: the rows with two sin / cos blocks exchanged, and with the view direction taken from d at stride 11,
    do not give the ray route's output."""
    net = _net(ops, enc.dense_network(), precision)
    bad = []
    shapes = list(_shapes(precision)) + ([(5, 192), (5, 256)] if precision == "f16x3" else [])
    for (R, N) in shapes:
        for stride in enc.STRIDES:
            rays, z = enc.make_rays(R, N, stride)
            rows = enc.encode_rays(rays, z)
            rays_d, z_d = torch.from_numpy(np.array(rays)).cuda(), torch.from_numpy(np.array(z)).cuda()
            want_t = net(torch.from_numpy(rows).cuda())
            want = want_t.cpu().numpy()
            assert np.isfinite(want).all()
            name = f"{precision} {R}x{N} stride {stride}"
            if N <= 128:
                rgbs, sigmas = ops.render_rays(net, rays_d, z_d)
                got = torch.cat([rgbs, sigmas[..., None]], -1).reshape(R * N, 4).cpu().numpy()
                bad.append(_diff(name + " render_rays", got, want))
                if precision == "f16x3" or (precision == "fp32" and N == 64):
                    raw = ops.render_rays_composited(net, rays_d, z_d, False, want_raw=True)[4]
                    bad.append(_diff(name + " render_rays_composited", raw.reshape(R * N, 4).cpu().numpy(), want))
                for variant in ("swap_sin_cos",) + (("view_from_d",) if stride == 11 else ()):
                    wrong = net(torch.from_numpy(enc.encode_rays(rays, z, variant=variant)).cuda()).cpu().numpy()
                    if _diff("", got, wrong) is None:
                        bad.append(f"{name}: the rows of variant {variant} give the ray route's output")
            else:
                raw, comp, w = _nan(R * N * 4), _nan(R * 3), _nan(R * N)
                depth, opac = _nan(R), _nan(R)
                rc = _wide(hk)(hooks.ptr(net.packed), hooks.ptr(rays_d), stride, hooks.ptr(z_d), R, N, ops.renderer_flags(False, "relu"),
                               hooks.ptr(raw), hooks.ptr(comp), hooks.ptr(depth), hooks.ptr(opac), hooks.ptr(w), None, hooks.stream())
                assert rc == hooks.NSR_OK
                torch.cuda.synchronize()
                assert torch.isnan(raw[R * N * 4:]).all()
                bad.append(_diff(name + " wide compositing hook", raw[:R * N * 4].reshape(R * N, 4).cpu().numpy(), want))
            if precision == "f16x3":
                for act in ("relu", "softplus"):
                    _, d0, o0, w0 = ops.VolumetricRenderer(SimpleNamespace(sigma_activation=act))(
                        want_t[:, :3].reshape(R, N, 3).contiguous(), want_t[:, 3].reshape(R, N).contiguous(), z_d, False)
                    d1, o1, w1 = ops.render_rays_density(net, rays_d, z_d, sigma_activation=act)
                    for what, a, b in (("depth", d1, d0), ("opacity", o1, o0), ("weights", w1, w0)):
                        bad.append(_diff(f"{name} density-only {act} {what}", a.cpu().numpy(), b.cpu().numpy()))
                    if act == "relu" and not (w0 > 0).any():
                        bad.append(f"{name}: no sample has weight: the density-only comparison sees nothing")
    if net.status() != 0:
        bad.append(f"{precision}: status {net.status():#x}")
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# (d) one-hot networks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", enc.PLACES)
@pytest.mark.parametrize("precision", enc.PRECISIONS)
def test_onehot_columns(ops, precision, place):
    """Every sin / cos column of one place (L1's 60, the skip layer's 60, dir_encoding's 24) through networks whose four raw
    outputs are four columns with their signs: ops.render_rays at every precision and render_rays_composited(want_raw=True)
    at f16x3, on the rays of (c) -- the direction part also on 37 rays, for the values -- equal the precision's operand
    conversion of the restated column (an expected zero: either sign)."""
    sets = [enc.make_rays(R, N, stride) for (R, N) in _shapes(precision) + ((enc.MANY,) if place == "dir" else ()) for stride in enc.STRIDES]
    staged = [(rays, z, enc.encode_rays(rays, z), torch.from_numpy(np.array(rays)).cuda(), torch.from_numpy(np.array(z)).cuda())
              for rays, z in sets]
    bad = []
    for name, sd, taps in enc.onehot_networks(place):
        net = _net(ops, sd, precision)
        for rays, z, rows, rays_d, z_d in staged:
            R, N = z.shape
            want = enc.onehot_expected(rows, taps, precision)
            tag = f"{precision} {name} {R}x{N} stride {rays.shape[1]} taps {taps}"
            rgbs, sigmas = ops.render_rays(net, rays_d, z_d)
            got = torch.cat([rgbs, sigmas[..., None]], -1).reshape(R * N, 4).cpu().numpy()
            bad.append(_diff(tag + " render_rays", got, want, zero_sign_free=True))
            # teeth: the neighbouring column's value (the taps rotated by one output) is not what the device returns
            if _diff("", got, enc.onehot_expected(rows, taps[1:] + taps[:1], precision), zero_sign_free=True) is None:
                bad.append(tag + ": the output also equals the rotated taps' expectation")
            if precision == "f16x3":
                raw = ops.render_rays_composited(net, rays_d, z_d, False, want_raw=True)[4]
                bad.append(_diff(tag + " render_rays_composited", raw.reshape(R * N, 4).cpu().numpy(), want, zero_sign_free=True))
        if net.status() != 0:
            bad.append(f"{precision} {name}: status {net.status():#x}")
    bad = [b for b in bad if b]
    assert not bad, f"{len(bad)} differences\n" + "\n".join(bad[:24])


# ---------------------------------------------------------------------------------------------------------------------
# (e) the TRAIN forward's encoding panels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", enc.SHAPES, ids=[f"{R}x{N}" for R, N in enc.SHAPES])
@pytest.mark.parametrize("stride", enc.STRIDES)
def test_train_forward_panels(ops, hk, shape, stride):
    """nsr_f16x3_train_forward on the rays of (c): panel 10 holds RN_f16 of the restated position encoding and panel 11 of the
    direction encoding, in enc_row() order, byte for byte (the expected rows are packed by nsr_test_pack_panel); the 32 pad
    rows of panel 11 are zero; nothing is written behind the buffers; the raw output is complete and the status word 0.  The
    raw output itself is not compared: the TRAIN forward runs xyz_encoding_final unfolded, the inference kernels folded."""
    R, N = shape
    P = R * N
    assert P % 32 == 0
    rays, z = enc.make_rays(R, N, stride)
    rows = enc.encode_rays(rays, z)
    net = _net(ops, enc.dense_network(), "f16x3")
    rays_d, z_d = torch.from_numpy(np.array(rays)).cuda(), torch.from_numpy(np.array(z)).cuda()
    pan_bytes, sgn_words = int(hk.nsr_test_train_panel_bytes(P)), int(hk.nsr_test_train_sign_words(P))
    n_groups = -(-P // 128) * 4
    assert pan_bytes == 2560 * 64 * n_groups
    pan = torch.full((pan_bytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    sgn = torch.full((sgn_words + GUARD,), -1, dtype=torch.int32, device="cuda")
    raw = _nan(P * 4)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    rc = hk.nsr_test_f16x3_train_forward(hooks.ptr(net.packed), hooks.ptr(rays_d), stride, hooks.ptr(z_d), R, N, hooks.ptr(raw), hooks.ptr(pan),
                                         hooks.ptr(sgn), hooks.ptr(status), hooks.stream())
    assert rc == hooks.NSR_OK
    torch.cuda.synchronize()
    assert (pan[pan_bytes:] == 0xFF).all() and (sgn[sgn_words:] == -1).all() and torch.isnan(raw[P * 4:]).all()
    assert torch.isfinite(raw[:P * 4]).all() and status.tolist() == [0, 0, 0, 0]
    pan_h = pan.cpu().numpy()
    pe16, used_pe = _panel_rows(rows, 32, _pecol, 0)
    de16, used_de = _panel_rows(rows, 16, _dircol, enc.POS)
    assert len(used_pe) == 64 and used_de == set(range(32))          # the direction panel's rows 32..63 are padding
    for panel, src, rows_before in ((10, pe16, 2304 + 128), (11, de16, 2304 + 192)):
        src_d = torch.from_numpy(src.view(np.int16)).cuda()
        want = torch.full((P // 32 * 4096 + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        assert hk.nsr_test_pack_panel(hooks.ptr(src_d), 64, P, 64, hooks.ptr(want), 4096, hooks.stream()) == hooks.NSR_OK
        torch.cuda.synchronize()
        want_h = want.cpu().numpy()
        assert (want_h[P // 32 * 4096:] == 0xFF).all()
        off = rows_before * 64 * n_groups
        got = pan_h[off:off + P // 32 * 4096]
        if not np.array_equal(got, want_h[:P // 32 * 4096]):
            g16, w16 = got.view(np.uint16), want_h[:P // 32 * 4096].view(np.uint16)
            i = np.flatnonzero(g16 != w16)
            pytest.fail(f"panel {panel}: {i.size} of {w16.size} halves differ, first at half {i[0]} (group {i[0] // 2048}): "
                        f"{g16[i[0]]:#06x} != {w16[i[0]]:#06x}")
        if panel == 11:      # the pad rows, decoded without the packer: block 1 of every group (its second 2 KiB) is zero
            blocks = got.reshape(P // 32, 2, 2048)
            assert not blocks[:, 1].any() and blocks[:, 0].any()
