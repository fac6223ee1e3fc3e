"""Host-side contract of the rays + z entry point of the fused split-fp16 forward for non-default architectures
(include/nsr_train.h: nsr_arch_fused_render_rays; ops.render_rays / ops.render_rays_sigma on a fused GenericMLP;
default_options(arch_fused_rays=)): the prototype, every rejection and the empty call -- all before a device is touched, with
fake pointers that are never dereferenced, so none of this needs a GPU."""
import ctypes
import os
import re

import pytest

from nerf_sr_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2


def _arch(D=4, W=128, skips=(2,), deg_pos=6, deg_dir=2, no_dir=0):
    bits = 0
    for s in skips:
        bits |= 1 << s
    return _lib.NsrArch(D, W, bits, deg_pos, deg_dir, no_dir)


def _call(lib, arch=None, packed=16, rays=32, stride=8, z=16, R=4, N=64, flags=0, out=16, ldo=4):
    a = _arch() if arch is None else arch
    ref = None if arch == "null" else ctypes.byref(a)
    return lib.nsr_arch_fused_render_rays(ref, ctypes.c_void_p(packed), ctypes.c_void_p(rays), stride, ctypes.c_void_p(z), R, N, flags,
                                          ctypes.c_void_p(out), ldo, None, None)


def test_the_symbol_and_its_prototype():
    lib = _lib.load()
    assert hasattr(lib, "nsr_arch_fused_render_rays")
    res, args = _lib.SIGNATURES["nsr_arch_fused_render_rays"]
    c = ctypes
    assert res is c.c_int
    assert args == [c.POINTER(_lib.NsrArch), c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_int64, c.c_int, c.c_int, c.c_void_p,
                    c.c_int64, c.c_void_p, c.c_void_p]
    text = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "nsr_train.h")).read())
    assert ("int nsr_arch_fused_render_rays(const nsr_arch* arch, const void* packed, const float* rays, int ray_stride, "
            "const float* z, int64_t R, int n_samples, int flags, float* out, int64_t ldo, unsigned* status, void* stream);") in text
    assert lib.nsr_version() == 131                               # additive: the version stays


@pytest.mark.parametrize("kw", [dict(D=9), dict(W=258), dict(deg_pos=11), dict(deg_dir=5)])
def test_a_descriptor_outside_the_fused_set_is_unsupported(kw):
    assert _call(_lib.load(), _arch(**kw)) == UNSUPPORTED


@pytest.mark.parametrize("kw", [dict(D=0), dict(W=3), dict(W=0), dict(deg_pos=-1), dict(no_dir=2), dict(D=4, skips=(4,)), dict(skips=(0,))])
def test_a_malformed_descriptor_is_an_invalid_argument(kw):
    lib = _lib.load()
    assert _call(lib, _arch(**kw)) == INVALID
    assert _call(lib, "null") == INVALID


def test_every_argument_is_checked_before_anything_is_enqueued():
    lib = _lib.load()
    assert _call(lib, flags=4) == INVALID and _call(lib, flags=1 | 8, ldo=1) == INVALID          # an undefined flag bit
    for stride in (0, 3, 7, 9, 10, 12, -8):
        assert _call(lib, stride=stride) == INVALID, stride
    assert _call(lib, rays=40, stride=8) == INVALID               # float4 loads: 16-byte aligned rays at stride 8 ...
    assert _call(lib, rays=40, stride=11, R=0) == OK              # ... only there
    assert _call(lib, N=0) == INVALID and _call(lib, N=-1) == INVALID
    assert _call(lib, R=-1) == INVALID
    for name in ("packed", "rays", "z", "out"):
        assert _call(lib, **{name: 0}) == INVALID, name
    assert _call(lib, packed=8) == INVALID                        # the stream is read 16 bytes at a time
    assert _call(lib, ldo=3) == INVALID                           # output rows shorter than [rgb, sigma]
    assert _call(lib, flags=1, ldo=0) == INVALID                  # ... than sigma
    # more than 2^31 - 1 tiles of 128 points; the product R * n_samples must not wrap on the way to that answer either
    assert _call(lib, R=(2 ** 31 - 1) * 128 + 1, N=1) == INVALID
    assert _call(lib, R=2 ** 31, N=128) == INVALID
    assert _call(lib, R=2 ** 62, N=2 ** 31 - 1) == INVALID
    # a bad argument is refused even when there is nothing to do
    assert _call(lib, R=0, stride=9) == INVALID and _call(lib, R=0, out=0) == INVALID


def test_no_rays_is_ok_and_launches_nothing():
    lib = _lib.load()
    assert _call(lib, R=0) == OK
    assert _call(lib, R=0, stride=11) == OK
    assert _call(lib, R=0, N=1, flags=1, ldo=1) == OK
    assert _call(lib, R=0, flags=2, ldo=7) == OK


def test_render_rays_refuses_a_layer_by_layer_network(monkeypatch):
    import torch
    from nerf_sr_amd import ops
    monkeypatch.setattr(ops, "_check_device", lambda *a, **k: None)           # the constructor allocates nothing
    net = ops.GenericMLP(precision="f16x3", D=4, W=128, skips=[2], deg_pos=6, deg_dir=2)
    assert not net.fused
    rays, z = torch.zeros(2, 8), torch.zeros(2, 4)
    with pytest.raises(ValueError, match="explicit route"):
        ops.render_rays(net, rays, z)
    with pytest.raises(ValueError, match="explicit route"):
        ops.render_rays_sigma(net, rays, z)
    with pytest.raises(TypeError):
        ops.render_rays_sigma(object(), rays, z)
    fused = ops.GenericMLP(precision="f16x3", fused=True, D=4, W=128, skips=[2], deg_pos=6, deg_dir=2)
    with pytest.raises(RuntimeError, match="load_state_dict"):    # accepted as a type; nothing is loaded yet
        ops.render_rays(fused, rays, z)


def test_default_options_carries_the_route():
    from nerf_sr_amd.model import default_options
    opt = default_options(arch_fused=True, precision="f16x3", D=4, W=128, skips=[2], deg_pos=6, deg_dir=2)
    assert opt.arch_fused is True and opt.arch_fused_rays is True
    assert default_options().arch_fused_rays is True              # without arch_fused it selects nothing
    assert default_options(arch_fused=True, precision="f16x3", W=128, arch_fused_rays=False).arch_fused_rays is False
