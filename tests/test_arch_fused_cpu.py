"""Host-side contract of the fused split-fp16 forward for non-default architectures (include/nsr_train.h:
nsr_arch_fused_packed_bytes / _pack / _forward; ops.GenericMLP(fused=True); default_options(arch_fused=True)): the supported
set, the error codes, and the ValueErrors -- all before a device is touched, so none of this needs a GPU."""
import ctypes

import pytest

from nerf_sr_amd import _lib


def _arch(D=8, W=256, skips=(4,), deg_pos=10, deg_dir=4, no_dir=0):
    bits = 0
    for s in skips:
        bits |= 1 << s
    return _lib.NsrArch(D, W, bits, deg_pos, deg_dir, no_dir)


def _pieces(D, W, skips, deg_pos, no_dir):
    """The stream's size from its description in csrc/nsr_mlp_arch_f16.hip: 4 pieces per 32-column input block + 1 bias piece
    per chunk, one chunk per 32-row output block."""
    nb, hb, kxb = (W + 31) // 32, (W // 2 + 31) // 32, (3 + 6 * deg_pos + 31) // 32
    n = 0
    for l in range(D):
        n += nb * (4 * (kxb if l == 0 else (kxb + nb if l in skips else nb)) + 1)
    return n + (4 * nb + 1) + nb * (4 * nb + 1) + hb * (4 * (nb + (0 if no_dir else 1)) + 1) + (4 * hb + 1)


@pytest.mark.parametrize("kw", [dict(D=1, W=2, skips=()), dict(D=8, W=256, skips=(1, 2, 3, 4, 5, 6, 7)),
                                dict(D=3, W=100, skips=(1,), deg_pos=0, deg_dir=0), dict(D=2, W=64, skips=(), deg_pos=10, deg_dir=4),
                                dict(D=4, W=128, skips=(2,), no_dir=1)])
def test_packed_bytes_is_nonzero_on_the_supported_corners(kw):
    lib = _lib.load()
    a = _arch(**kw)
    n = lib.nsr_arch_fused_packed_bytes(ctypes.byref(a))
    assert n == 1024 * _pieces(a.D, a.W, kw["skips"], a.deg_pos, a.no_dir) and n > 0
    assert n <= 3 << 20          # the whole network stays L2-resident


@pytest.mark.parametrize("kw", [dict(D=9), dict(W=258), dict(deg_pos=11), dict(deg_dir=5)])
def test_outside_the_supported_set_is_refused(kw):
    lib = _lib.load()
    a = _arch(**kw)
    assert lib.nsr_arch_n_tensors(ctypes.byref(a)) == 2 * a.D + 8          # the layer-by-layer route still takes it
    assert lib.nsr_arch_fused_packed_bytes(ctypes.byref(a)) == 0
    one = ctypes.c_void_p(16)          # never dereferenced: the descriptor is checked first
    ptrs = (ctypes.c_void_p * (2 * a.D + 8))(*[one] * (2 * a.D + 8))
    assert lib.nsr_arch_fused_pack(ctypes.byref(a), ptrs, one, None, None) == -2
    assert lib.nsr_arch_fused_forward(ctypes.byref(a), one, one, 90, 4, 0, one, 4, None, None) == -2


@pytest.mark.parametrize("kw", [dict(D=0), dict(W=3), dict(W=0), dict(deg_pos=-1), dict(no_dir=2), dict(D=4, skips=(4,)), dict(skips=(0,))])
def test_a_malformed_descriptor_is_an_invalid_argument(kw):
    lib = _lib.load()
    a = _arch(**kw)
    one = ctypes.c_void_p(16)
    assert lib.nsr_arch_fused_packed_bytes(ctypes.byref(a)) == 0
    assert lib.nsr_arch_fused_packed_bytes(None) == 0
    ptrs = (ctypes.c_void_p * 40)(*[one] * 40)
    assert lib.nsr_arch_fused_pack(ctypes.byref(a), ptrs, one, None, None) == -1
    assert lib.nsr_arch_fused_forward(ctypes.byref(a), one, one, 90, 4, 0, one, 4, None, None) == -1
    assert lib.nsr_arch_fused_forward(None, one, one, 90, 4, 0, one, 4, None, None) == -1


def test_forward_checks_its_arguments_before_anything_is_enqueued():
    lib = _lib.load()
    a = _arch(D=4, W=128, skips=(2,), deg_pos=6, deg_dir=2)      # rows of 39 + 15
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    ref = ctypes.byref(a)
    assert lib.nsr_arch_fused_forward(ref, null, one, 54, 4, 0, one, 4, None, None) == -1
    assert lib.nsr_arch_fused_forward(ref, one, null, 54, 4, 0, one, 4, None, None) == -1
    assert lib.nsr_arch_fused_forward(ref, one, one, 54, 4, 0, null, 4, None, None) == -1
    assert lib.nsr_arch_fused_forward(ref, ctypes.c_void_p(8), one, 54, 4, 0, one, 4, None, None) == -1      # misaligned stream
    assert lib.nsr_arch_fused_forward(ref, one, one, 53, 4, 0, one, 4, None, None) == -1       # rows shorter than the encodings
    assert lib.nsr_arch_fused_forward(ref, one, one, 38, 4, 1, one, 1, None, None) == -1       # ... than the encoded position
    assert lib.nsr_arch_fused_forward(ref, one, one, 54, 4, 0, one, 3, None, None) == -1       # output rows shorter than 4
    assert lib.nsr_arch_fused_forward(ref, one, one, 54, -1, 0, one, 4, None, None) == -1
    assert lib.nsr_arch_fused_forward(ref, one, one, 54, 4, 4, one, 4, None, None) == -1       # an undefined flag bit
    assert lib.nsr_arch_fused_forward(ref, one, one, 54, 0, 0, one, 4, None, None) == 0        # no rows: nothing is launched
    assert lib.nsr_arch_fused_forward(ref, one, one, 39, 0, 1, one, 1, None, None) == 0
    ptrs = (ctypes.c_void_p * 16)(*[one] * 15, null)
    assert lib.nsr_arch_fused_pack(ref, ptrs, one, None, None) == -1                           # a null tensor
    assert lib.nsr_arch_fused_pack(ref, None, one, None, None) == -1


def test_generic_mlp_fused_refuses_on_the_host(monkeypatch):
    import torch
    from nerf_sr_amd import ops

    def no_device(*a, **k):
        raise AssertionError("a device was touched before the option was refused")
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    monkeypatch.setattr(ops, "_check_device", no_device)
    with pytest.raises(ValueError, match="'f16x3' only"):
        ops.GenericMLP(precision="fp32", fused=True, W=128)
    for kw, limit in ((dict(D=9), "D <= 8"), (dict(W=258), "W <= 256"), (dict(deg_pos=11), "deg_pos <= 10"),
                      (dict(deg_dir=5), "deg_dir <= 4"), (dict(dim_rgb=4), "dim_rgb == 3")):
        with pytest.raises(ValueError, match=limit):
            ops.GenericMLP(precision="f16x3", fused=True, **kw)
    with pytest.raises(ValueError, match="'f16x3' only"):
        ops.make_mlp(ops_options(W=128), precision="fp32", arch_fused=True)
    with pytest.raises(ValueError):                              # a malformed architecture stays what it was
        ops.GenericMLP(precision="f16x3", fused=True, W=127)


def ops_options(**kw):
    from types import SimpleNamespace
    return SimpleNamespace(**kw)


def test_default_options_refuses_arch_fused_on_the_host():
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    assert default_options().arch_fused is False
    with pytest.raises(ValueError, match="'f16x3' only"):
        default_options(arch_fused=True, precision="fp32", W=128)
    with pytest.raises(ValueError, match="D <= 8"):
        default_options(arch_fused=True, precision="f16x3", D=9)
    opt = default_options(precision="fp32", W=128)
    opt.arch_fused = True                                        # set after the fact: the model's constructor refuses it
    with pytest.raises(ValueError, match="'f16x3' only"):
        NeRFDownXModel(opt, device="cpu")
    # the option does not concern the default architecture, whatever the precision
    assert default_options(arch_fused=True, precision="fp32").arch_fused is True
    assert default_options(arch_fused=True, precision="f16x3", W=128, skips=[2], D=4).arch_fused is True
