"""CPU side of the chain path's ray gradient (include/nsr_train.h: nsr_train_backward_r, nsr_train_workspace_bytes_r): the ABI,
the argument checks that come before any launch, the Python keyword's default, and the numpy restatement
tests/chain_ray_grads_ref.py -- the reference of tests/test_gpu_chain_ray_grad_units.py -- against torch fp64 autograd."""
import os
import re
from collections import OrderedDict
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib, build as nsr_build
from nerf_sr_amd.weights import STATE_DICT_SPEC, make_state_dict
from tests import chain_ray_grads_ref as cr
from tests import chain_ref
from tests import ray_grads_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = ("f16x3", "f16x3_bwd3", "f16x3_bwd2", "f16x3_bwdm", "f16x3_bwd1")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


def test_declared_exported_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "nsr_train.h")).read(), flags=re.S)
    for name in ("nsr_train_backward_r", "nsr_train_workspace_bytes_r"):
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/nsr_train.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert re.search(r"#define\s+NSR_BACKWARD_NO_WEIGHT_GRADS\s+1u", text) and _lib.NSR_BACKWARD_NO_WEIGHT_GRADS == 1
    assert lib.nsr_version() == 131
    assert "nsr_train_raygrad_f16.hip" in [u for u, _ in nsr_build.UNITS]
    flags = dict(nsr_build.UNITS)["nsr_train_raygrad_f16.hip"]
    assert "-ffp-contract=off" in flags


def test_size_query(lib):
    for prec in CHAIN + ("fp32", "f16x3_gemm"):
        p = _lib.TRAIN_PRECISIONS[prec]
        for chunk, nc, ni in ((4, 8, 8), (2048, 64, 64), (96, 64, 128)):
            a, b = lib.nsr_train_workspace_bytes_r(p, chunk, nc, ni), lib.nsr_train_workspace_bytes_for(p, chunk, nc, ni)
            assert a == lib.nsr_train_workspace_bytes_r(p, chunk, nc, ni) and a >= b > 0, (prec, chunk, a, b)
            if prec in CHAIN:      # two (P, 3) matrices and 144 KiB of packed weight columns per network, in 256-byte granules
                P = chunk * (nc + ni)
                assert a - b == 2 * ((P * 12 + 255) // 256 * 256) + 2 * 144 * 1024, (prec, chunk, a - b)
    p = _lib.NSR_F16X3
    assert lib.nsr_train_workspace_bytes_r(p, 0, 64, 64) == 0 and lib.nsr_train_workspace_bytes_r(p, 64, 1, 64) == 0
    assert lib.nsr_train_workspace_bytes_r(p, 64, 64, 256) == 0 and lib.nsr_train_workspace_bytes_r(5, 64, 64, 64) == 0
    # all chain precisions take the same buffers
    assert len({lib.nsr_train_workspace_bytes_r(_lib.TRAIN_PRECISIONS[q], 128, 64, 64) for q in CHAIN}) == 1


def test_argument_checks_come_before_any_launch(lib):
    """Every refusal below returns before the saved header is read: the pointers are never dereferenced (there is no device)."""
    null, ok = c_void_p(0), c_void_p(256)
    p24 = (c_void_p * 24)(*[ok] * 24)
    hole = (c_void_p * 24)(*[ok] * 23, null)
    g8 = (c_void_p * 8)()

    def call(w=p24, rays=ok, stride=8, g_outs=g8, gc=p24, gf=p24, g_rays=ok, g_stride=8, flags=0, ws=ok, saved=ok):
        return lib.nsr_train_backward_r(w, p24, rays, stride, g_outs, gc, gf, g_rays, g_stride, flags, ws, 1 << 20, saved, 1 << 20, null)

    assert call(w=None) == -1 and call(w=hole) == -1
    assert call(g_outs=None) == -1
    assert call(gc=None) == -1 and call(gf=None) == -1 and call(gc=hole) == -1          # with weight gradients: required
    assert call(ws=null) == -1 and call(saved=null) == -1 and call(ws=c_void_p(16)) == -1
    assert call(rays=null) == -1, "g_rays without the forward call's rays"
    assert call(g_stride=9, stride=9) == -1 and call(g_stride=11, stride=8) == -1 and call(g_stride=8, stride=11) == -1
    assert call(g_rays=null, flags=_lib.NSR_BACKWARD_NO_WEIGHT_GRADS) == -1, "the flag without g_rays: nothing to compute"
    assert call(flags=2) == -1 and call(flags=3) == -1, "unknown option bits"
    # under the flag the gradient arrays may be null, the weights may not
    assert call(w=None, gc=None, gf=None, flags=1) == -1


def test_keyword_defaults_to_the_refusal(monkeypatch):
    from nerf_sr_amd import train as tr
    # the refusal comes right behind the look at the rays, which asks for a device tensor: waived here, there is no device
    monkeypatch.setattr(tr, "_f32", lambda t, name: t)
    sd = {k: torch.zeros(s) for k, s in STATE_DICT_SPEC.items()}
    rays = torch.zeros(32, 8, requires_grad=True)
    for prec in ("f16x3", "f16x3_bwd2"):
        for kw in ({}, {"chain_ray_grad": False}):
            with pytest.raises(ValueError, match="fp32") as e:
                tr.forward_rays_train(sd, sd, rays, None, precision=prec, **kw)
            assert "do not differentiate through the encodings" in str(e.value)
    import inspect
    assert inspect.signature(tr.forward_rays_train).parameters["chain_ray_grad"].default is False
    assert inspect.signature(tr.Trainer.__init__).parameters["chain_ray_grad"].default is False


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def _random_case(seed, R, N, stride):
    rng = np.random.default_rng(seed)
    P = R * N
    sd = make_state_dict(seed=seed)
    panels = [rng.standard_normal((P, rows)).astype(np.float16) for rows in chain_ref.PANEL_ROWS]
    pscale = 2.0 ** rng.integers(-6, 4, (10, P)).astype(np.float64)
    rays = rng.standard_normal((R, stride)).astype(np.float32)
    z = np.sort(rng.uniform(2.0, 6.0, (R, N)), 1).astype(np.float32)
    return sd, panels, pscale, rays, z


@pytest.mark.parametrize("stride", (8, 11))
@pytest.mark.parametrize("stop_grad", (False, True))
def test_restatement_is_autograd_of_the_encodings(stride, stop_grad):
    sd, panels, pscale, rays, z = _random_case(7 + stride, 3, 16, stride)
    R, N = z.shape
    # the gradients of the encoded columns, in torch, from the definitions
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    dz = lambda p: t(panels[p]) * t(pscale[p])[:, None]
    g_pe = dz(0) @ t(sd[cr.W_1]) + dz(4) @ t(sd[cr.W_5])[:, :63]
    g_de = None if stop_grad else (dz(9) @ t(sd[cr.W_DIR])[:, 256:]).view(R, N, 27)
    # float64 points: the restatement's default differentiates at the fp32 points, so it is given these encodings instead
    x64 = rays[:, None, 0:3].astype(np.float64) + z[:, :, None].astype(np.float64) * rays[:, None, 3:6].astype(np.float64)
    want = rr.autograd_rows(rays, z, g_pe.view(R, N, 63), g_de, 10, 4, 0)
    got = cr.rows(panels, pscale, sd, rays, z, stop_grad, enc_pos=cr.posenc64(x64.reshape(-1, 3), 10))
    for a, b in ((0, 3), (3, 6)) + (((8, 11),) if stride == 11 and not stop_grad else ()):
        err = np.linalg.norm(got[:, a:b] - want[:, a:b]) / np.linalg.norm(want[:, a:b])
        assert err < 1e-12, (a, b, err)
    assert (got[:, 6:8] == 0).all()
    if stop_grad and stride == 11:
        assert (got[:, 8:11] == 0).all()


@pytest.mark.parametrize("stride", (8, 11))
def test_restatement_tells_wrong_variants_apart(stride):
    sd, panels, pscale, rays, z = _random_case(31, 2, 16, stride)
    want = cr.rows(panels, pscale, sd, rays, z)
    for variant in cr.VARIANTS:
        bad = cr.rows(panels, pscale, sd, rays, z, variant=variant)
        blocks = [(0, 3), (3, 6)] + ([(8, 11)] if stride == 11 else [])
        worst = max(np.linalg.norm(bad[:, a:b] - want[:, a:b]) / np.linalg.norm(want[:, a:b]) for a, b in blocks)
        assert worst > 1e-2, (variant, worst)
    # the skip columns and the direction columns are where include/nsr_train.h says: perturbing the others changes nothing
    sd2 = OrderedDict((k, np.array(v, copy=True)) for k, v in sd.items())
    sd2[cr.W_5][:, 63:] += 1.0
    sd2[cr.W_DIR][:, :256] -= 1.0
    assert np.array_equal(cr.rows(panels, pscale, sd2, rays, z), want)
    other = [p if i in (0, 4, 9) else p + np.float16(1) for i, p in enumerate(panels)]
    assert np.array_equal(cr.rows(other, pscale, sd, rays, z), want)
