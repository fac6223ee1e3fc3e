"""The two kernels of the gradient with respect to the rays, alone and on exact inputs (csrc/nsr_train_gemm.hip:
encode_bwd_kernel, ray_grad_kernel, through the launchers of csrc/nsr_train_work.h that tests/csrc/nsr_test_hooks_raygrad.hip
exports) against the float64 restatement tests/ray_grads_ref.py, BIT FOR BIT.

Inputs are small-integer gradients, dyadic kept sin / cos values (k / 8) and dyadic depths (k / 16); a band is a power of two or
an fp32 value of the linear table (24 bits).  Every product then has at most 24 + 4 + 4 + 5 bits and every sum of the at most
3 x 64 x 256 terms stays far inside the 53 bits of the kernels' double accumulators, so no sum rounds, the order of the
additions does not matter, and the ONE rounding to fp32 at the end is the restatement's own."""
import ctypes
from ctypes import POINTER, c_int, c_int64, c_uint, c_void_p

import numpy as np
import pytest
import torch

from tests import ray_grads_ref as rr

pytestmark = pytest.mark.gpu

NO_XYZ, LINEAR = rr.NO_XYZ, rr.LINEAR_FREQS


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from tests import hooks
    h = hooks.load()
    h.nsr_test_encode_bwd.restype, h.nsr_test_encode_bwd.argtypes = c_int, [POINTER(c_void_p), c_int, c_int64, c_void_p, c_int64,
                                                                            c_int64, c_int, c_int, c_uint, c_void_p, c_void_p]
    h.nsr_test_ray_grad.restype, h.nsr_test_ray_grad.argtypes = c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p,
                                                                        c_int64, c_int, c_uint, c_void_p, c_int, c_int, c_void_p]
    return h


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _r32(n):
    return max(32, (n + 31) // 32 * 32)


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def _embeds(deg):
    return [e for e in (0, NO_XYZ, LINEAR, NO_XYZ | LINEAR) if not ((e & NO_XYZ) and deg == 0)]


@pytest.mark.parametrize("P", (32, 96))
@pytest.mark.parametrize("deg", (0, 6, 10))
@pytest.mark.parametrize("n_src", (1, 2, 3))      # layer 0 alone, with one and with two skip destinations
def test_encode_bwd_bit_exact(lib, P, deg, n_src):
    rng = np.random.default_rng(100 * P + 10 * deg + n_src)
    for embed in _embeds(deg):
        C, Kx = rr.n_cols(deg, embed), _r32(rr.n_cols(deg, embed))
        ld_enc = Kx + 32                                  # the kept rows lie in a wider matrix (x = [pe | h])
        g = _ints(rng, (n_src, P, Kx), -4, 4)             # padding columns hold non-zero values too: they must not be read as bands
        enc = _ints(rng, (P, ld_enc), -8, 8) / 8.0
        want = rr.encode_bwd(g[:, :, :C], enc[:, :C], deg, embed).astype(np.float32)
        gd = [torch.from_numpy(g[j]).cuda() for j in range(n_src)]
        encd = torch.from_numpy(enc.astype(np.float32)).cuda()
        out = torch.full((P + 4, 3), 7.0, device="cuda")   # four guard rows behind the result
        src = (c_void_p * n_src)(*[c_void_p(t.data_ptr()) for t in gd])
        rc = lib.nsr_test_encode_bwd(src, n_src, Kx, c_void_p(encd.data_ptr()), ld_enc, P, deg, Kx // 4, embed,
                                     c_void_p(out.data_ptr()), _stream())
        assert rc == 0, (embed, rc)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:P].view(np.uint32), want.view(np.uint32)), (P, deg, n_src, embed, np.abs(got[:P] - want).max())
        assert (got[P:] == 7.0).all()
        if deg > 0:      # the restatement tells the wrong forms apart on these very inputs
            for variant in ("swap_sign", "no_f"):
                if variant == "no_f" and deg == 1:
                    continue
                assert not np.array_equal(rr.encode_bwd(g[:, :, :C], enc[:, :C], deg, embed, variant).astype(np.float32), want), variant


@pytest.mark.parametrize("R", (1, 4, 5))
@pytest.mark.parametrize("N", (8, 64, 128))
@pytest.mark.parametrize("deg_dir,no_dir", ((0, False), (2, False), (4, False), (4, True)))
def test_ray_grad_bit_exact(lib, R, N, deg_dir, no_dir):
    rng = np.random.default_rng(1000 * R + 10 * N + deg_dir + int(no_dir))
    for embed in _embeds(deg_dir):
        for stride in (8, 11):
            C, Dp = rr.n_cols(deg_dir, embed), _r32(rr.n_cols(deg_dir, embed))
            ld_enc = Dp + 64                              # the kept direction rows lie behind xyz_encoding_final's columns
            g_x = _ints(rng, (R, N, 3), -6, 6)
            z = _ints(rng, (R, N), 0, 96) / 16.0
            g_dir = None if no_dir else _ints(rng, (R, N, Dp), -4, 4)
            enc_ray = _ints(rng, (R, ld_enc), -8, 8) / 8.0
            enc = np.repeat(enc_ray[:, None, :], N, axis=1).astype(np.float32)      # every sample of a ray holds the same row
            part = rr.ray_grad(g_x, z, None if no_dir else g_dir[:, :, :C], enc_ray[:, :C], deg_dir, embed, stride)
            prev = _ints(rng, (R, stride), -50, 50)
            prev[:, 6:8] = 0.0
            gxd, zd = torch.from_numpy(g_x).cuda(), torch.from_numpy(z.astype(np.float32)).cuda()
            gdd = None if no_dir else torch.from_numpy(g_dir).cuda()
            encd = torch.from_numpy(enc).cuda()
            for acc in (0, 1):
                out = torch.full((R + 2, stride), 7.0, device="cuda")
                out[:R] = torch.from_numpy(prev).cuda() if acc else float("nan")      # overwritten whatever it held
                rc = lib.nsr_test_ray_grad(c_void_p(gxd.data_ptr()), c_void_p(zd.data_ptr()), R, N,
                                           c_void_p(0 if no_dir else gdd.data_ptr()), Dp, c_void_p(encd.data_ptr()), ld_enc, deg_dir,
                                           embed, c_void_p(out.data_ptr()), stride, acc, _stream())
                assert rc == 0, (embed, stride, rc)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                want = (part.astype(np.float32).astype(np.float64) + (prev if acc else 0.0)).astype(np.float32)
                assert np.array_equal(got[:R].view(np.uint32), want.view(np.uint32)), (R, N, deg_dir, embed, stride, acc,
                                                                                       np.abs(got[:R] - want).max())
                assert (got[:R, 6:8] == 0.0).all() and not np.signbit(got[:R, 6:8]).any()
                assert (got[R:] == 7.0).all()
            if not no_dir and stride == 11:
                assert (part[:, 8:11] != 0).any()
                assert not np.array_equal(rr.ray_grad(g_x, z, g_dir[:, :, :C], enc_ray[:, :C], deg_dir, embed, 11, "dir_at_11"), part)
            assert not np.array_equal(rr.ray_grad(g_x, z, None, None, deg_dir, embed, stride, "no_z"),
                                      rr.ray_grad(g_x, z, None, None, deg_dir, embed, stride))


def test_launchers_refuse_what_they_cannot_run(lib):
    t = torch.zeros(64, 32, device="cuda")
    p = c_void_p(t.data_ptr())
    src = (c_void_p * 1)(p)
    assert lib.nsr_test_encode_bwd(src, 0, 32, p, 32, 4, 1, 8, 0, p, _stream()) == -1        # no source
    assert lib.nsr_test_encode_bwd(src, 1, 32, p, 32, 4, 6, 8, 0, p, _stream()) == -1        # 39 columns in 8 groups of 4
    assert lib.nsr_test_encode_bwd(src, 1, 30, p, 32, 4, 1, 8, 0, p, _stream()) == -1        # rows not 16-byte aligned
    assert lib.nsr_test_ray_grad(p, p, 4, 8, None, 0, None, 0, 0, 0, p, 9, 0, _stream()) == -1        # stride 9
    assert lib.nsr_test_ray_grad(p, p, 4, 8, p, 32, None, 0, 0, 0, p, 8, 0, _stream()) == -1          # direction columns without the kept row
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0
