"""Host-side contract of the training forward / backward pair (include/nsr_train.h: nsr_train_saved_bytes, nsr_train_forward,
nsr_train_backward) and of the pieces of nerf_sr_amd.train around it that need no GPU: argument validation before any launch,
the saved-state size, gradient clipping and the TV loss against torch's own definitions."""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from nerf_sr_amd.weights import make_state_dict, STATE_DICT_SPEC


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except ImportError as e:
        pytest.fail(f"libnsr.so not built: {e}")


def test_pair_symbols_exported_and_bound(lib):
    for name in ("nsr_train_saved_bytes", "nsr_train_forward", "nsr_train_backward"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_saved_bytes(lib):
    f16, fp32 = _lib.TRAIN_PRECISIONS["f16x3"], _lib.TRAIN_PRECISIONS["fp32"]
    assert lib.nsr_train_saved_bytes(f16, 0, 64, 64, 0) == 0
    assert lib.nsr_train_saved_bytes(f16, -4, 64, 64, 0) == 0
    assert lib.nsr_train_saved_bytes(f16, 64, 1, 64, 0) == 0            # sample counts
    assert lib.nsr_train_saved_bytes(f16, 64, 64, 0, 0) == 0
    assert lib.nsr_train_saved_bytes(f16, 64, 200, 100, 0) == 0
    assert lib.nsr_train_saved_bytes(7, 64, 64, 64, 0) == 0             # precision
    assert lib.nsr_train_saved_bytes(f16, 3, 40, 24, 0) == 0            # 3 x 40 points: not a multiple of 32
    prev = 0
    for R in (1, 4, 64, 256, 2048):
        b = lib.nsr_train_saved_bytes(f16, R, 64, 64, 0)
        assert b > prev and b % 256 == 0, R
        prev = b
    # the chain path keeps ~5.4 KB per sample point (2-byte panels, sign words, rgb / sigma / z); the GEMM path ~10 KB
    P = 2048 * (64 + 128)
    chain, gemm = lib.nsr_train_saved_bytes(f16, 2048, 64, 64, 0), lib.nsr_train_saved_bytes(fp32, 2048, 64, 64, 0)
    assert 4.5e3 * P < chain < 6e3 * P and 9e3 * P < gemm < 1.1e4 * P
    for p in _lib.TRAIN_PRECISIONS.values():
        assert lib.nsr_train_saved_bytes(p, 2048, 64, 64, 0) in (chain, gemm)
    # chunked: one region per chunk, each sized for a full chunk
    assert lib.nsr_train_saved_bytes(f16, 2048, 64, 64, 512) >= chain - 4 * 1024 * 1024


def _fwd(lib, **kw):
    one = c_void_p(256)
    p24 = (c_void_p * 24)(*[one] * 24)
    outs = (c_void_p * 8)(*[one] * 8)
    a = dict(wc=p24, wf=p24, rays=one, stride=8, R=64, nc=64, ni=64, flags=0, lindisp=0, uc=None, uf=None, nc_=None, nf=None,
             std=0.0, prec=_lib.TRAIN_PRECISIONS["f16x3"], chunk=0, outs=outs, ws=one, ws_bytes=1 << 40, saved=one,
             saved_bytes=1 << 40)
    a.update(kw)
    return lib.nsr_train_forward(a["wc"], a["wf"], a["rays"], a["stride"], a["R"], a["nc"], a["ni"], a["flags"], a["lindisp"],
                                 a["uc"], a["uf"], a["nc_"], a["nf"], a["std"], a["prec"], a["chunk"], a["outs"], a["ws"],
                                 a["ws_bytes"], a["saved"], a["saved_bytes"], None)


def test_forward_rejects_every_invalid_argument_before_any_launch(lib):
    """Non-NULL dummy pointers that are never dereferenced: every check comes before anything is enqueued."""
    null = c_void_p(0)
    p24_null = (c_void_p * 24)(*[c_void_p(256)] * 23, null)
    assert _fwd(lib, wc=None) == -1
    assert _fwd(lib, wf=p24_null) == -1
    assert _fwd(lib, outs=None) == -1
    assert _fwd(lib, outs=(c_void_p * 8)(null, *[c_void_p(256)] * 7)) == -1           # outs[0] required
    assert _fwd(lib, outs=(c_void_p * 8)(*[c_void_p(256)] * 4, null, *[c_void_p(256)] * 3)) == -1   # outs[4] required
    assert _fwd(lib, rays=null) == -1
    assert _fwd(lib, stride=9) == -1
    assert _fwd(lib, R=-1) == -1
    assert _fwd(lib, ws=null) == -1 and _fwd(lib, saved=null) == -1
    assert _fwd(lib, ws=c_void_p(16)) == -1 and _fwd(lib, saved=c_void_p(16)) == -1     # 256-byte alignment
    assert _fwd(lib, nc=1) == -2 and _fwd(lib, ni=0) == -2 and _fwd(lib, nc=200, ni=100) == -2
    assert _fwd(lib, prec=7) == -2
    assert _fwd(lib, R=3, nc=40, ni=24) == -2                                           # 120 points: the 32-point rule
    assert _fwd(lib, R=64, chunk=3, nc=40, ni=24) == -2                                  # ... in every chunk
    assert _fwd(lib, flags=32) == -1                                                     # unknown option bit
    assert _fwd(lib, flags=_lib.NSR_TRAIN_GAMMA_CORRECT | _lib.NSR_TRAIN_COLOR_NONE) == -2
    assert _fwd(lib, ws_bytes=1024) == -4
    need = lib.nsr_train_saved_bytes(_lib.TRAIN_PRECISIONS["f16x3"], 64, 64, 64, 0)
    assert _fwd(lib, saved_bytes=need - 1) == -4
    assert _fwd(lib, R=0) == 0                                                           # zero-sized work: a no-op


def test_backward_rejects_invalid_arguments_before_reading_the_saved_state(lib):
    one, null = c_void_p(256), c_void_p(0)
    p24 = (c_void_p * 24)(*[one] * 24)
    p24_null = (c_void_p * 24)(*[one] * 23, null)
    g8 = (c_void_p * 8)()
    bwd = lambda wc=p24, wf=p24, g=g8, gc=p24, gf=p24, ws=one, saved=one, sb=1 << 30: \
        lib.nsr_train_backward(wc, wf, g, gc, gf, ws, 1 << 40, saved, sb, None)
    assert bwd(wc=None) == -1 and bwd(wf=p24_null) == -1
    assert bwd(g=None) == -1
    assert bwd(gc=None) == -1 and bwd(gf=p24_null) == -1
    assert bwd(ws=null) == -1 and bwd(saved=null) == -1
    assert bwd(ws=c_void_p(16)) == -1 and bwd(saved=c_void_p(48)) == -1
    assert bwd(sb=255) == -4                                                             # smaller than its header


def test_rays_that_require_grad_are_refused():
    from nerf_sr_amd import train as tr
    with pytest.raises(ValueError, match="rays"):
        tr.forward_rays_train({}, {}, torch.zeros(64, 8, requires_grad=True))


def _cpu_trainer(**kw):
    from nerf_sr_amd import train as tr
    return tr.Trainer(make_state_dict(1), make_state_dict(2), device="cpu", **kw)


def test_gradient_clipping_matches_torch():
    """clip_grads = nn.utils.clip_grad_norm_ / clip_grad_value_ over both networks' parameters together (:403-407)."""
    gen = torch.Generator().manual_seed(0)
    for kind, val in (("norm", 0.05), ("norm", 1e3), ("value", 1e-3)):
        t = _cpu_trainer(grad_clip_val=val, grad_clip_type=kind)
        params = []
        for n in range(2):
            for k, s in STATE_DICT_SPEC.items():
                g = torch.randn(*s, generator=gen) * 1e-2
                t.grads[n][k].copy_(g)
                p = torch.nn.Parameter(torch.zeros(*s))
                p.grad = g.clone()
                params.append(p)
        total = t.clip_grads()
        if kind == "norm":
            want = torch.nn.utils.clip_grad_norm_(params, val)
            assert abs(float(total) - float(want)) <= 1e-6 * float(want)
        else:
            torch.nn.utils.clip_grad_value_(params, val)
        got = [g for n in range(2) for g in t.grads[n].values()]
        for a, p in zip(got, params):
            torch.testing.assert_close(a, p.grad, rtol=1e-6, atol=0)
    t = _cpu_trainer()
    assert t.grad_clip_val == 0 and t.clip_grads() is None
    with pytest.raises(ValueError):
        _cpu_trainer(grad_clip_type="max")


def test_tv_loss_is_the_reference_definition():
    from nerf_sr_amd import train as tr
    x = torch.rand(8, 8, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    h = ((x[1:] - x[:-1]) ** 2).sum() / (7 * 8 * 3)
    w = ((x[:, 1:] - x[:, :-1]) ** 2).sum() / (8 * 7 * 3)
    assert abs(float(tr.tv_loss(x)) - float(h + w)) < 1e-15
    assert float(tr.tv_loss(torch.ones(4, 4, 3))) == 0.0
