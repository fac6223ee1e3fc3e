"""Test-time mode (include/nsr.h, "test-time mode"), everything that needs no GPU:

1. ``nsr_render_rays_density`` and ``nsr_forward_rays_density_coarse`` are declared, exported, bound and documented, and make
   their argument checks before anything touches the device (null device pointers, no GPU); the fused route's sample counts
   as the workspace query reports them;
2. the Python mirror: ``default_options(coarse_rgb=...)`` and the ValueErrors raised before a device is touched;
3. the new instantiations of the split-fp16 render kernel compile without scratch, at one wave per SIMD."""
import os
import re
from ctypes import c_void_p
from types import SimpleNamespace

import pytest

from nerf_sr_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nsr_render_rays_density", "nsr_forward_rays_density_coarse")
OK, INVALID, UNSUPPORTED = 0, -1, -2
F32, BF16, F16X3, F16 = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ 1. header and ABI
def test_entry_points_are_declared_exported_bound_and_documented():
    with open(os.path.join(REPO, "include", "nsr.h")) as f:
        header = f.read()
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name in doc
    assert lib.nsr_version() == 131
    # the driver's argument list is nsr_forward_rays_ert's
    assert _lib.SIGNATURES["nsr_forward_rays_density_coarse"] == _lib.SIGNATURES["nsr_forward_rays_ert"]


def test_density_launch_checks_its_arguments_before_the_device():
    lib = _lib.load()
    null, one = c_void_p(0), c_void_p(16)

    def dens(packed=one, prec=F16X3, rays=one, stride=8, z=one, R=10, n=64, flags=0):
        return lib.nsr_render_rays_density(packed, prec, rays, stride, z, R, n, flags, null, null, null, null)

    assert dens(packed=null) == INVALID and dens(R=-1) == INVALID and dens(n=0) == INVALID and dens(stride=9) == INVALID
    assert dens(flags=4) == INVALID                                     # an unknown renderer bit
    for prec in (F32, BF16, F16):                                       # fp32 and the single-operand fast paths
        assert dens(prec=prec) == UNSUPPORTED, prec
    assert dens(prec=7) == UNSUPPORTED
    for n in (32, 96, 160, 224, 288, 512):
        assert dens(n=n) == UNSUPPORTED, n
    for n in (64, 128, 192, 256):
        for flags in (0, 1, 2, 3):                                      # either density; the background bit is accepted (unused)
            assert dens(n=n, R=0, rays=null, z=null, flags=flags) == OK     # empty batch: nothing is read
        assert dens(n=n, rays=null) == INVALID and dens(n=n, z=null) == INVALID
        assert dens(n=n, rays=c_void_p(8)) == INVALID                  # 8-wide rays are read as float4
    assert dens(n=96, R=0) == UNSUPPORTED and dens(prec=F32, R=0) == UNSUPPORTED     # refused even for an empty batch


def test_density_coarse_driver_checks_its_arguments_before_the_device():
    lib = _lib.load()
    null, one = c_void_p(0), c_void_p(16)
    PtrArray = c_void_p * 8

    def fwd(prec=F16X3, nc=64, ni=64, outs="nulls", out0=None, R=10, eps=0.0, flags=0, packed=one, fine=one, ws=null, ws_bytes=0):
        arr = None if outs is None else PtrArray(*([out0] + [None] * 7))
        return lib.nsr_forward_rays_density_coarse(packed, fine, prec, null, 8, R, nc, ni, flags, 0, arr, ws, ws_bytes, null, None, eps,
                                                   null)

    assert fwd(outs=None) == INVALID                                    # no output array at all
    assert fwd(out0=16) == INVALID and fwd(out0=16, R=0) == INVALID     # a coarse colour buffer would never be written
    assert fwd(out0=16, prec=F32) == INVALID                            # ... checked first
    assert fwd(ni=0) == INVALID and fwd(ni=-1) == INVALID               # no fine pass: the coarse colour is the image
    for prec in (F32, BF16, F16):
        assert fwd(prec=prec) == UNSUPPORTED and fwd(prec=prec, R=0) == UNSUPPORTED, prec
    for nc in (32, 96, 100, 512):
        assert fwd(nc=nc) == UNSUPPORTED and fwd(nc=nc, R=0) == UNSUPPORTED, nc
    for bad in (float("nan"), -1e-3, 1.0):
        assert fwd(eps=bad) == INVALID
    assert fwd(eps=1e-4, ni=128) == UNSUPPORTED and fwd(eps=1e-4, nc=128, ni=128) == UNSUPPORTED     # early termination stays at 64 / 128
    assert fwd(eps=1e-4, flags=2) == UNSUPPORTED                        # ... and under the relu density
    assert fwd(packed=null) == INVALID and fwd(fine=null) == INVALID
    for nc, ni in ((64, 64), (64, 128), (128, 128), (192, 64), (256, 128)):
        assert fwd(nc=nc, ni=ni, R=0) == OK                             # empty batch
        assert fwd(nc=nc, ni=ni, R=0, eps=1e-4 if nc + ni <= 128 else 0.0) == OK
        assert fwd(nc=nc, ni=ni) == -4                                  # 10 rays and no workspace: NSR_ERR_WORKSPACE
        need = lib.nsr_forward_rays_workspace_bytes_for(F16X3, 10, nc, ni)
        assert fwd(nc=nc, ni=ni, ws=null, ws_bytes=need) == INVALID     # only now the null pointers are looked at


def test_workspace_query_knows_the_fused_sample_counts():
    lib = _lib.load()
    a = lambda n: (n + 255) & ~255      # noqa: E731
    R = 1000
    for prec in (F32, BF16, F16X3, F16):
        for nc, ni in ((64, 64), (64, 128), (64, 192), (128, 128), (64, 32), (192, 0), (256, 0), (96, 0)):
            nf = nc + ni
            fused = lambda n: (n in (64, 128) and prec in (F32, F16X3)) or (n in (192, 256) and prec == F16X3)      # noqa: E731
            want = 2 * a(R * nc * 4) + (0 if fused(nc) else a(R * nc * 16))
            if ni:
                want += a(R * nf * 4) + (0 if fused(nf) else a(R * nf * 16))
            assert lib.nsr_forward_rays_workspace_bytes_for(prec, R, nc, ni) == want, (prec, nc, ni)


# ------------------------------------------------------------------------------------------------ 2. the Python mirror
def test_default_options_and_refusals_before_any_device():
    from nerf_sr_amd import ops
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    assert default_options().coarse_rgb is True and default_options(coarse_rgb=False).coarse_rgb is False
    good = dict(coarse_rgb=False, precision="f16x3")
    for kw, word in ((dict(good, precision="fp32"), "f16x3"), (dict(good, precision="f16"), "f16x3"),
                     (dict(good, N_importance=0), "N_importance"), (dict(good, N_coarse=96), "64, 128, 192 or 256"),
                     (dict(good, D=4), "architecture")):
        with pytest.raises(ValueError, match=re.escape(word)) as e:
            NeRFDownXModel(default_options(**kw), device="cuda")
        assert "coarse_rgb" in str(e.value)                            # the message names the option
    # the per-call check of ops.render_rays_density / ops.forward_rays, on a network object that owns no device memory
    net = object.__new__(ops.VanillaMLP)
    net.precision = "f16x3"
    for n in ops.FUSED_SAMPLES_F16X3:
        ops.check_density_coarse(net, n)
        ops.check_density_coarse(net, n, 64)
    for args, word in (((net, 96), "64, 128, 192 or 256"), ((net, 64, 0), "N_importance"), ((net, 32, 64), "64, 128, 192 or 256"),
                       ((SimpleNamespace(precision="f16x3"), 64), "f16x3"), ((None, 64), "f16x3")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.check_density_coarse(*args)
    net.precision = "fp32"
    with pytest.raises(ValueError, match="f16x3"):
        ops.check_density_coarse(net, 64, 64)
    # forward_rays refuses before it looks at the rays or the library
    net.precision = "f16x3"
    with pytest.raises(ValueError, match="N_importance"):
        ops.forward_rays(net, None, None, 64, 0, coarse_rgb=False)
    with pytest.raises(ValueError, match="64, 128, 192 or 256"):
        ops.forward_rays(net, net, None, 96, 64, coarse_rgb=False)
    net.precision = "fp32"
    with pytest.raises(ValueError, match="f16x3"):
        ops.forward_rays(net, net, None, 64, 64, coarse_rgb=False)


# ------------------------------------------------------------------------------------------------ 3. register budget
NEW_KERNELS = [(False, 192), (False, 256), (True, 64), (True, 128), (True, 192), (True, 256)]     # (density-only, samples per ray)


@pytest.fixture(scope="module")
def listing():
    from nerf_sr_amd import build
    return build.compile_listing("nsr_mlp_f16.hip")


@pytest.mark.parametrize("dens,ns", NEW_KERNELS)
def test_new_instantiations_compile_without_scratch(listing, dens, ns):
    """mlp_f16x3_kernel<1, SIGMA_ONLY, NS, COMP = true>: no private segment, no spilled VGPR, and within the 512 registers
    (256 VGPR + 256 AGPR) a wave has at one wave per SIMD."""
    name = f"_Z16mlp_f16x3_kernelILi1ELb{int(dens)}ELi{ns}ELb1ELb0ELb0EE"
    m = re.search(r"\.amdhsa_kernel (" + re.escape(name) + r"\w*)\n(.*?)\.end_amdhsa_kernel", listing, re.S)
    assert m, f"{name} is not in the listing"
    desc = m.group(2)
    field = lambda key: int(re.search(r"\." + key + r"\s+(\d+)", desc).group(1))      # noqa: E731
    assert field("amdhsa_private_segment_fixed_size") == 0
    assert field("amdhsa_next_free_vgpr") <= 512
    meta = re.search(r"\.name:\s+" + re.escape(m.group(1)) + r"\n(.*?)\.wavefront_size", listing, re.S)
    assert meta, "no metadata note for the kernel"
    for key, limit in (("private_segment_fixed_size", 0), ("vgpr_spill_count", 0), ("vgpr_count", 512)):
        assert int(re.search(r"\." + key + r":\s+(\d+)", meta.group(1)).group(1)) <= limit, key
    print(f"{name}: {field('amdhsa_next_free_vgpr')} VGPR + AGPR, scratch 0")
