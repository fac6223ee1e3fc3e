"""Host-side contract of training a NON-DEFAULT architecture (include/nsr_train.h: struct nsr_arch, nsr_arch_n_tensors,
nsr_arch_tensor_numel, nsr_train_arch_workspace_bytes / _saved_bytes, nsr_train_arch_forward / _backward, nsr_adam_step_n)
and of the Python layer around it, as far as no GPU is needed: descriptor validation, sizes, rejection before any launch
with the codes of the default pair, the documented ValueErrors, and the fixture tests/golden/train_arch.npz against the
fp64 restatement of the same iteration (tests/arch_util.py)."""
import ctypes
import warnings
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from nerf_sr_amd.weights import arch_spec, make_state_dict_arch
from tests import arch_util as au
from tests.util import sample_idx

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
FP32, GEMM = _lib.TRAIN_PRECISIONS["fp32"], _lib.TRAIN_PRECISIONS["f16x3_gemm"]
CHAIN = [_lib.TRAIN_PRECISIONS[k] for k in ("f16x3", "f16x3_bwd3", "f16x3_bwd2", "f16x3_bwd1", "f16x3_bwdm")]


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except ImportError as e:
        pytest.fail(f"libnsr.so not built: {e}")


def A(D=8, W=256, skips=(4,), deg_pos=10, deg_dir=4, no_dir=0):
    bits = skips if isinstance(skips, int) else sum(1 << s for s in skips)
    return _lib.NsrArch(D, W, bits, deg_pos, deg_dir, no_dir)


SMALL, ODD = dict(D=4, W=128, skips=(2,), deg_pos=6, deg_dir=2), dict(D=6, W=192, skips=(1, 3))
MALFORMED = [dict(D=0), dict(W=0), dict(W=191), dict(deg_pos=-1), dict(deg_dir=-1), dict(no_dir=2), dict(skips=1),   # bit 0
             dict(D=4, skips=(4,)), dict(D=4, skips=(2, 9))]                                                            # bit >= D
BEYOND = [dict(D=17, skips=(4,)), dict(W=514), dict(deg_pos=17), dict(deg_dir=17)]


def test_symbols_exported_and_bound(lib):
    for name in ("nsr_arch_n_tensors", "nsr_arch_tensor_numel", "nsr_train_arch_workspace_bytes", "nsr_train_arch_saved_bytes",
                 "nsr_train_arch_forward", "nsr_train_arch_backward", "nsr_adam_step_n"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.nsr_version() == 131      # additive entry points: the version stays


def test_tensor_count_and_sizes_follow_the_state_dict(lib):
    for kw in (dict(), SMALL, ODD, dict(SMALL, no_dir=1), dict(D=1, W=2, skips=0, deg_pos=0, deg_dir=0),
               dict(D=16, W=512, skips=tuple(range(1, 16)), deg_pos=16, deg_dir=16), dict(D=3, W=100, skips=(1,))):
        a = A(**kw)
        skips = tuple(i for i in range(32) if (a.skips >> i) & 1)
        spec = arch_spec(D=a.D, W=a.W, skips=skips, deg_pos=a.deg_pos, deg_dir=a.deg_dir, no_dir=bool(a.no_dir))
        assert lib.nsr_arch_n_tensors(ctypes.byref(a)) == len(spec) == 2 * a.D + 8
        for t, shape in enumerate(spec.values()):
            assert lib.nsr_arch_tensor_numel(ctypes.byref(a), t) == int(np.prod(shape)), (kw, t)
        assert lib.nsr_arch_tensor_numel(ctypes.byref(a), -1) == 0 and lib.nsr_arch_tensor_numel(ctypes.byref(a), len(spec)) == 0
    assert lib.nsr_arch_n_tensors(None) == INVALID and lib.nsr_arch_tensor_numel(None, 0) == 0


def test_malformed_and_unsupported_descriptors(lib):
    for kw in MALFORMED:
        a = A(**kw)
        assert lib.nsr_arch_n_tensors(ctypes.byref(a)) == INVALID, kw
        assert lib.nsr_arch_tensor_numel(ctypes.byref(a), 0) == 0, kw
        assert lib.nsr_train_arch_workspace_bytes(ctypes.byref(a), FP32, 64, 64, 64) == 0, kw
        assert lib.nsr_train_arch_saved_bytes(ctypes.byref(a), FP32, 64, 64, 64, 0) == 0, kw
        assert _fwd(lib, arch=a) == INVALID and _bwd(lib, arch=a) == INVALID, kw
    for kw in BEYOND:
        a = A(**kw)
        assert lib.nsr_arch_n_tensors(ctypes.byref(a)) == UNSUPPORTED, kw
        assert lib.nsr_train_arch_workspace_bytes(ctypes.byref(a), FP32, 64, 64, 64) == 0, kw
        assert lib.nsr_train_arch_saved_bytes(ctypes.byref(a), FP32, 64, 64, 64, 0) == 0, kw
        assert _fwd(lib, arch=a) == UNSUPPORTED and _bwd(lib, arch=a) == UNSUPPORTED, kw


def test_size_functions(lib):
    a = A(**ODD)
    ws, sv = lib.nsr_train_arch_workspace_bytes, lib.nsr_train_arch_saved_bytes
    for p in CHAIN + [7]:
        assert ws(ctypes.byref(a), p, 64, 64, 64) == 0 and sv(ctypes.byref(a), p, 64, 64, 64, 0) == 0, p
    assert ws(None, FP32, 64, 64, 64) == 0 and sv(None, FP32, 64, 64, 64, 0) == 0
    assert ws(ctypes.byref(a), FP32, 0, 64, 64) == 0 and ws(ctypes.byref(a), FP32, 64, 1, 64) == 0
    assert ws(ctypes.byref(a), FP32, 64, 64, 0) == 0 and ws(ctypes.byref(a), FP32, 64, 200, 100) == 0
    assert sv(ctypes.byref(a), FP32, 0, 64, 64, 0) == 0 and sv(ctypes.byref(a), FP32, -4, 64, 64, 0) == 0
    assert sv(ctypes.byref(a), FP32, 64, 1, 64, 0) == 0 and sv(ctypes.byref(a), FP32, 64, 64, 0, 0) == 0
    assert sv(ctypes.byref(a), FP32, 3, 40, 24, 0) == 0                       # 3 x 40 points: not a multiple of 32
    prev_s = prev_w = 0
    for R in (1, 4, 64, 256, 2048):
        s, w = sv(ctypes.byref(a), FP32, R, 64, 64, 0), ws(ctypes.byref(a), FP32, R, 64, 64)
        assert s > prev_s and s % 256 == 0 and w > prev_w and w % 256 == 0, R
        assert s == sv(ctypes.byref(a), FP32, R, 64, 64, 0) and s == sv(ctypes.byref(a), GEMM, R, 64, 64, 0)
        prev_s, prev_w = s, w
    assert ws(ctypes.byref(a), GEMM, 64, 64, 64) > ws(ctypes.byref(a), FP32, 64, 64, 64)      # + the split halves
    # floats kept per sample point: the formula of include/nsr_train.h
    r32 = lambda n: (n + 31) // 32 * 32
    for kw in (dict(), SMALL, ODD, dict(SMALL, no_dir=1), dict(D=3, W=100, skips=0)):
        a = A(**kw)
        n_sk = bin(a.skips).count("1")
        Kx, Wp, Hp, Dp = r32(3 + 6 * a.deg_pos), r32(a.W), r32(a.W // 2), (0 if a.no_dir else r32(3 + 6 * a.deg_dir))
        n_x = max(1, n_sk)
        per_point = n_x * (Kx + (Wp if n_sk else 0)) + (a.D - n_sk) * Wp + (Wp + Dp) + Hp + 6
        R = 2048
        P = R * 64 + R * 128
        got = sv(ctypes.byref(a), FP32, R, 64, 64, 0)
        assert 4 * per_point * P <= got <= 4 * per_point * P + 65536, (kw, got, 4 * per_point * P)
    # the default network keeps what the default pair's GEMM path keeps, up to the 32-float sigma block
    d = A()
    mine, theirs = sv(ctypes.byref(d), FP32, 2048, 64, 64, 0), lib.nsr_train_saved_bytes(FP32, 2048, 64, 64, 0)
    assert abs(mine - theirs) <= 4 * 32 * 2048 * 192 + 65536


def _fwd(lib, arch=None, **kw):
    one = c_void_p(256)
    arch = A(**ODD) if arch is None else arch
    n = max(lib.nsr_arch_n_tensors(ctypes.byref(arch)), 8) if arch is not False else 8
    pn = (c_void_p * n)(*[one] * n)
    outs = (c_void_p * 8)(*[one] * 8)
    a = dict(wc=pn, wf=pn, rays=one, stride=8, R=64, nc=64, ni=64, flags=0, lindisp=0, uc=None, uf=None, nc_=None, nf=None,
             std=0.0, prec=FP32, chunk=0, outs=outs, ws=one, ws_bytes=1 << 40, saved=one, saved_bytes=1 << 40)
    a.update(kw)
    return lib.nsr_train_arch_forward(None if arch is False else ctypes.byref(arch), a["wc"], a["wf"], a["rays"], a["stride"], a["R"],
                                      a["nc"], a["ni"], a["flags"], a["lindisp"], a["uc"], a["uf"], a["nc_"], a["nf"], a["std"],
                                      a["prec"], a["chunk"], a["outs"], a["ws"], a["ws_bytes"], a["saved"], a["saved_bytes"], None)


def _bwd(lib, arch=None, **kw):
    one = c_void_p(256)
    arch = A(**ODD) if arch is None else arch
    n = max(lib.nsr_arch_n_tensors(ctypes.byref(arch)), 8) if arch is not False else 8
    pn = (c_void_p * n)(*[one] * n)
    a = dict(wc=pn, wf=pn, g=(c_void_p * 8)(), gc=pn, gf=pn, ws=one, saved=one, sb=1 << 30)
    a.update(kw)
    return lib.nsr_train_arch_backward(None if arch is False else ctypes.byref(arch), a["wc"], a["wf"], a["g"], a["gc"], a["gf"],
                                       a["ws"], 1 << 40, a["saved"], a["sb"], None)


def test_forward_rejects_every_invalid_argument_before_any_launch(lib):
    """Non-NULL dummy pointers that are never dereferenced.  Every mistake nsr_train_forward rejects
    (tests/test_train_autograd_cpu.py) gets the same code here."""
    null, one = c_void_p(0), c_void_p(256)
    n = 2 * 6 + 8
    pn_null = (c_void_p * n)(*[one] * (n - 1), null)
    assert _fwd(lib, arch=False) == INVALID
    assert _fwd(lib, wc=None) == INVALID
    assert _fwd(lib, wf=pn_null) == INVALID                                              # the LAST of the 2 D + 8 tensors
    assert _fwd(lib, outs=None) == INVALID
    assert _fwd(lib, outs=(c_void_p * 8)(null, *[one] * 7)) == INVALID
    assert _fwd(lib, outs=(c_void_p * 8)(*[one] * 4, null, *[one] * 3)) == INVALID
    assert _fwd(lib, rays=null) == INVALID
    assert _fwd(lib, stride=9) == INVALID
    assert _fwd(lib, R=-1) == INVALID
    assert _fwd(lib, ws=null) == INVALID and _fwd(lib, saved=null) == INVALID
    assert _fwd(lib, ws=c_void_p(16)) == INVALID and _fwd(lib, saved=c_void_p(16)) == INVALID
    assert _fwd(lib, nc=1) == UNSUPPORTED and _fwd(lib, ni=0) == UNSUPPORTED and _fwd(lib, nc=200, ni=100) == UNSUPPORTED
    assert _fwd(lib, prec=7) == UNSUPPORTED
    for p in CHAIN:                                                                      # the chain kernels are the default network's
        assert _fwd(lib, prec=p) == UNSUPPORTED, p
    assert _fwd(lib, prec=GEMM, ws_bytes=1024) == WORKSPACE                              # ... f16x3_gemm is accepted
    assert _fwd(lib, R=3, nc=40, ni=24) == UNSUPPORTED
    assert _fwd(lib, R=64, chunk=3, nc=40, ni=24) == UNSUPPORTED
    assert _fwd(lib, flags=32) == INVALID
    assert _fwd(lib, flags=_lib.NSR_TRAIN_GAMMA_CORRECT | _lib.NSR_TRAIN_COLOR_NONE) == UNSUPPORTED
    assert _fwd(lib, ws_bytes=1024) == WORKSPACE
    a = A(**ODD)
    assert _fwd(lib, ws_bytes=lib.nsr_train_arch_workspace_bytes(ctypes.byref(a), FP32, 64, 64, 64) - 1) == WORKSPACE
    assert _fwd(lib, saved_bytes=lib.nsr_train_arch_saved_bytes(ctypes.byref(a), FP32, 64, 64, 64, 0) - 1) == WORKSPACE
    assert _fwd(lib, R=0) == OK                                                          # zero-sized work: a no-op
    # the default architecture is a valid descriptor
    assert _fwd(lib, arch=A(), ws_bytes=1024) == WORKSPACE


def test_backward_rejects_invalid_arguments_before_reading_the_saved_state(lib):
    one, null = c_void_p(256), c_void_p(0)
    n = 2 * 6 + 8
    pn_null = (c_void_p * n)(*[one] * (n - 1), null)
    assert _bwd(lib, arch=False) == INVALID
    assert _bwd(lib, wc=None) == INVALID and _bwd(lib, wf=pn_null) == INVALID
    assert _bwd(lib, g=None) == INVALID
    assert _bwd(lib, gc=None) == INVALID and _bwd(lib, gf=pn_null) == INVALID
    assert _bwd(lib, ws=null) == INVALID and _bwd(lib, saved=null) == INVALID
    assert _bwd(lib, ws=c_void_p(16)) == INVALID and _bwd(lib, saved=c_void_p(48)) == INVALID
    assert _bwd(lib, sb=255) == WORKSPACE                                                 # smaller than its header


def test_adam_step_n_rejects_invalid_arguments(lib):
    one = c_void_p(256)
    p2 = (c_void_p * 2)(one, one)
    n2 = (ctypes.c_int64 * 2)(4, 4)
    f = lambda n=2, numel=n2, w=p2, g=p2, m=p2, v=p2, step=1: lib.nsr_adam_step_n(n, numel, w, g, m, v, step, 1e-3, 0.9, 0.999, 1e-8, None)
    assert f(n=0) == INVALID and f(n=41) == INVALID and f(numel=None) == INVALID and f(step=0) == INVALID
    assert f(w=None) == INVALID and f(g=(c_void_p * 2)(one, c_void_p(0))) == INVALID
    assert f(numel=(ctypes.c_int64 * 2)(4, -1)) == INVALID


# ---- the fixture against the fp64 restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", au.CASES)
def test_fixture_agrees_with_fp64_restatement(golden_dir, tag):
    """The reference's own fp32 iteration needs no allowance: losses within 1e-6, every gradient norm within 2e-3, the
    subsample digests within the bound of tests/test_gpu_train.py (4e-3), for every tensor of both networks."""
    g = au.load_case(golden_dir, tag)
    sd_c, sd_f = au.state_dicts(g)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    res, gc, gf = au.loss_and_grads(sd_c, sd_f, g)
    print(tag, "loss", float(g["loss_tot"]), res["loss_tot"])
    assert abs(res["loss_coarse_mse"] - float(g["loss_coarse_mse"])) < 1e-6
    assert abs(res["loss_fine_mse"] - float(g["loss_fine_mse"])) < 1e-6
    assert abs(res["loss_tot"] - float(g["loss_tot"])) < 1e-6
    np.testing.assert_allclose(res["coarse_comp_rgbs"].numpy(), g["hr_coarse"], rtol=0, atol=2e-6)
    spec = arch_spec(**g["arch"])
    assert len(spec) == 2 * g["arch"]["D"] + 8
    for name, grads in (("coarse", gc), ("fine", gf)):
        for k in spec:
            want = grads[k]
            ref_norm = float(g[f"gnorm_{name}.{k}"])
            assert abs(float(want.norm()) - ref_norm) <= 2e-3 * ref_norm + 1e-9, (name, k, float(want.norm()), ref_norm)
            sub = want.reshape(-1).numpy()[sample_idx(want.numel())]
            ref_sub = g[f"grad_{name}.{k}"].astype(np.float64)
            assert sub.shape == ref_sub.shape
            assert np.linalg.norm(sub - ref_sub) <= 4e-3 * np.linalg.norm(ref_sub) + 1e-9, (name, k)


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def _cpu_trainer(arch, **kw):
    from nerf_sr_amd import train as tr
    a = tr.normalize_arch(arch)
    a.pop("dim_rgb")
    return tr.Trainer(make_state_dict_arch(1, **a), make_state_dict_arch(2, **a), device="cpu", arch=arch, **kw)


def test_trainer_holds_the_architectures_tensors():
    arch = dict(D=4, W=128, skips=(2,), deg_pos=6, deg_dir=2)
    t = _cpu_trainer(arch, precision="fp32")
    spec = arch_spec(**arch)
    for n in range(2):
        assert list(t.params[n]) == list(spec) == list(t.grads[n]) == list(t.exp_avg[n])
        for k, shape in spec.items():
            assert tuple(t.params[n][k].shape) == tuple(shape) == tuple(t.grads[n][k].shape)
    sds = t.state_dicts()
    assert [tuple(v.shape) for v in sds[0].values()] == [tuple(s) for s in spec.values()]
    assert t.update_learning_rate(25, "exp", n_epochs=20, n_epochs_decay=10) < t._lr_initial
    assert t.status() == 0
    # --no_dir natively: the narrow dir_encoding, no padded columns
    t = _cpu_trainer(dict(arch, no_dir=True), precision="f16x3_gemm")
    assert tuple(t.params[0]["dir_encoding.0.weight"].shape) == (64, 128) and t.no_dir


def test_documented_value_errors_without_a_device():
    from nerf_sr_amd import train as tr
    arch = dict(D=4, W=128, skips=(2,), deg_pos=6, deg_dir=2)
    for bad in (dict(arch, W=127), dict(arch, skips=(0,)), dict(arch, skips=(4,)), dict(arch, D=0), dict(arch, deg_pos=-1),
                dict(arch, dim_rgb=4)):
        with pytest.raises(ValueError):
            _cpu_trainer(bad)
        with pytest.raises(ValueError):
            tr.forward_rays_train({}, {}, torch.zeros(64, 8), arch=bad)
    for prec in ("f16x3_bwd3", "f16x3_bwd2", "f16x3_bwd1", "f16x3_bwdm", "bf16", "nope"):
        with pytest.raises(ValueError, match="precision"):
            _cpu_trainer(arch, precision=prec)
    sd = make_state_dict_arch(1, **arch)
    for prec in ("f16x3_bwd3", "f16x3_bwdm"):
        with pytest.raises(ValueError, match="precision"):
            tr.forward_rays_train(sd, sd, torch.zeros(64, 8), arch=arch, precision=prec)
    with pytest.raises(ValueError, match="rays"):
        tr.forward_rays_train(sd, sd, torch.zeros(64, 8, requires_grad=True), arch=arch)
    # weights of another architecture
    other = {k: torch.from_numpy(v) for k, v in make_state_dict_arch(1, **dict(arch, W=192)).items()}
    with pytest.raises(ValueError, match="shape"):
        tr.forward_rays_train(other, other, torch.zeros(64, 8), arch=arch, precision="fp32")
    with pytest.raises(ValueError):
        tr.Trainer(make_state_dict_arch(1, **dict(arch, W=192)), make_state_dict_arch(2, **arch), device="cpu", arch=arch,
                   precision="fp32")
    with pytest.raises(ValueError, match="tensors"):
        tr.forward_rays_train(list(other.values())[:-1], other, torch.zeros(64, 8), arch=arch, precision="fp32")
    with pytest.raises(ValueError, match="gamma_correct"):
        tr.forward_rays_train(other, other, torch.zeros(64, 8), arch=arch, gamma_correct=True, color_activation="none")
    # arch=None keeps the default network's order of checks and its messages: the rays come first there
    with pytest.raises(ValueError, match="rays must live on the GPU"):
        tr.forward_rays_train(list(other.values()), other, torch.zeros(64, 8))
    with pytest.raises(ValueError, match="expected 24 tensors"):
        tr._weights(list(other.values()), "params_c")


def test_f16x3_maps_to_f16x3_gemm_with_one_warning_per_architecture():
    from nerf_sr_amd import train as tr
    arch = dict(D=3, W=64, skips=(1,), deg_pos=5, deg_dir=3)          # an architecture no other test names
    with pytest.warns(RuntimeWarning, match="f16x3_gemm"):
        t = _cpu_trainer(arch, precision="f16x3")
    assert t.precision == "f16x3_gemm"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _cpu_trainer(arch, precision="f16x3").precision == "f16x3_gemm"      # the second time: silent
        assert _cpu_trainer(arch, precision="fp32").precision == "fp32"
