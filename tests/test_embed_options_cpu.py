"""The embedding options --no_xyz / --no_logscale (models/embedding.py:17-18) without a device: the band table and the sizes
of the C ABI (include/nsr.h, include/nsr_train.h: the option word ``embed`` of the ``_e`` entry points), every refusal of the
library and of the Python layer, and the fp64 restatement tests/embed_ref.py against the reference's own record
(tests/golden/embed.npz, made by tests/golden/make_golden_embed.py)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib, weights
from oracle import nerf_oracle as oc
from tests import embed_ref as er

NO_XYZ, LINEAR = _lib.NSR_EMBED_NO_XYZ, _lib.NSR_EMBED_LINEAR_FREQS
INVALID = -1
ATOL = 2e-6      # tests/test_oracle_golden.py


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "embed.npz"))


def _freqs(lib, deg, embed):
    f = (ctypes.c_float * 16)()
    assert lib.nsr_posenc_freqs(deg, embed, f) == 0
    return np.array(f[:deg], dtype=np.float32)


def _arch(**kw):
    a = weights.normalize_arch({**er.SMALL, **kw})
    return _lib.NsrArch.from_arch(a)


def test_option_word_values():
    assert (NO_XYZ, LINEAR) == (1, 2) == (weights.EMBED_NO_XYZ, weights.EMBED_LINEAR_FREQS)
    assert weights.embed_of(None) == 0 and weights.embed_of(SimpleNamespace()) == 0
    assert weights.embed_of(SimpleNamespace(no_xyz=True)) == NO_XYZ
    assert weights.embed_of(SimpleNamespace(no_logscale=True, no_xyz=False)) == LINEAR
    assert weights.embed_of(SimpleNamespace(no_logscale=True, no_xyz=True)) == NO_XYZ | LINEAR


@pytest.mark.parametrize("deg", range(1, 17))
def test_freq_table_is_the_references_bit_for_bit(lib, g, deg):
    """nsr_posenc_freqs: torch.linspace(1, 2^(deg-1), deg) as the reference's PositionalEncoding holds it, and 2^k for word 0
    (and for NO_XYZ alone, which does not touch the bands)."""
    want = g[f"freq_bands_{deg}"]
    assert want.dtype == np.float32 and want.shape == (deg,)
    for embed in (LINEAR, LINEAR | NO_XYZ):
        assert np.array_equal(_freqs(lib, deg, embed).view(np.uint32), want.view(np.uint32)), (deg, embed)
    for embed in (0, NO_XYZ):
        assert np.array_equal(_freqs(lib, deg, embed), np.float32(2.0) ** np.arange(deg, dtype=np.float32))
    if deg <= 2:      # [1] and [1, 2]: the log-scale bands
        assert np.array_equal(_freqs(lib, deg, LINEAR), _freqs(lib, deg, 0))


def test_freq_table_refusals(lib):
    f = (ctypes.c_float * 16)()
    assert lib.nsr_posenc_freqs(3, 4, f) == INVALID                       # unknown bit
    assert lib.nsr_posenc_freqs(17, 0, f) == INVALID and lib.nsr_posenc_freqs(-1, 0, f) == INVALID
    assert lib.nsr_posenc_freqs(3, LINEAR, None) == INVALID
    assert lib.nsr_posenc_freqs(0, LINEAR, None) == 0                     # nothing to write


@pytest.mark.parametrize("case", list(er.CASES))
def test_tensor_numel_gives_the_references_shapes(lib, g, case):
    arch, embed, _, _ = er.CASES[case]
    c_arch = _lib.NsrArch.from_arch(weights.normalize_arch(arch))
    spec = er.spec_of(arch, embed)
    assert lib.nsr_arch_n_tensors(ctypes.byref(c_arch)) == len(spec) == 2 * arch["D"] + 8
    for t, (k, shape) in enumerate(spec.items()):
        assert tuple(g[f"{case}_shape.{k}"]) == tuple(shape), k          # arch_spec(no_xyz=) is the reference's module
        assert lib.nsr_arch_tensor_numel_e(ctypes.byref(c_arch), embed, t) == int(np.prod(shape)), k
    if case == "both":      # the shapes the issue quotes
        assert tuple(g["both_shape.xyz_encoding_1.0.weight"]) == (128, 36)
        assert tuple(g["both_shape.xyz_encoding_3.0.weight"]) == (128, 164)
        assert tuple(g["both_shape.dir_encoding.0.weight"]) == (64, 140)


def test_size_functions_at_word_0_equal_the_plain_ones(lib):
    for arch in (er.SMALL, er.DEFAULT, {**er.SMALL, "no_dir": True}):
        a = ctypes.byref(_lib.NsrArch.from_arch(weights.normalize_arch(arch)))
        for t in range(2 * arch["D"] + 8):
            assert lib.nsr_arch_tensor_numel_e(a, 0, t) == lib.nsr_arch_tensor_numel(a, t) > 0
        for prec in (_lib.NSR_FP32, _lib.NSR_F16X3_GEMM):
            assert lib.nsr_train_arch_workspace_bytes_e(a, 0, prec, 96, 64, 64) == lib.nsr_train_arch_workspace_bytes(a, prec, 96, 64, 64) > 0
            assert lib.nsr_train_arch_saved_bytes_e(a, 0, prec, 96, 64, 64, 0) == lib.nsr_train_arch_saved_bytes(a, prec, 96, 64, 64, 0) > 0
        assert lib.nsr_arch_fused_packed_bytes_e(a, 0) == lib.nsr_arch_fused_packed_bytes(a) > 0
        # LINEAR changes no size; NO_XYZ never makes one larger
        assert lib.nsr_train_arch_saved_bytes_e(a, LINEAR, _lib.NSR_FP32, 96, 64, 64, 0) == lib.nsr_train_arch_saved_bytes(a, _lib.NSR_FP32, 96, 64, 64, 0)
        assert 0 < lib.nsr_train_arch_saved_bytes_e(a, NO_XYZ, _lib.NSR_FP32, 96, 64, 64, 0) <= lib.nsr_train_arch_saved_bytes(a, _lib.NSR_FP32, 96, 64, 64, 0)
        assert 0 < lib.nsr_arch_fused_packed_bytes_e(a, NO_XYZ) <= lib.nsr_arch_fused_packed_bytes(a)


def test_library_refusals_before_anything_is_enqueued(lib):
    """An unknown bit everywhere; NO_XYZ with deg_pos == 0; NO_XYZ with deg_dir == 0 unless no_dir.  Every pointer is NULL:
    a call that got past the check of the word would answer differently or touch a device."""
    ok = ctypes.byref(_arch())
    cases = [(ok, 4), (ok, 8 | NO_XYZ), (ctypes.byref(_arch(deg_pos=0)), NO_XYZ), (ctypes.byref(_arch(deg_dir=0)), NO_XYZ | LINEAR)]
    for a, embed in cases:
        assert lib.nsr_arch_tensor_numel_e(a, embed, 0) == 0
        assert lib.nsr_train_arch_workspace_bytes_e(a, embed, _lib.NSR_FP32, 96, 64, 64) == 0
        assert lib.nsr_train_arch_saved_bytes_e(a, embed, _lib.NSR_FP32, 96, 64, 64, 0) == 0
        assert lib.nsr_arch_fused_packed_bytes_e(a, embed) == 0
        assert lib.nsr_arch_fused_pack_e(a, embed, None, None, None, None) == INVALID
        assert lib.nsr_arch_fused_forward_e(a, embed, None, None, 0, 0, 0, None, 4, None, None) == INVALID
        assert lib.nsr_arch_fused_render_rays_e(a, embed, None, None, 8, None, 0, 64, 0, None, 4, None, None) == INVALID
        assert lib.nsr_train_arch_forward_e(a, embed, None, None, None, 8, 0, 64, 64, 0, 0, None, None, None, None, 0.0, _lib.NSR_FP32, 0,
                                            None, None, 0, None, 0, None) == INVALID
        assert lib.nsr_train_arch_backward_e(a, embed, None, None, None, None, None, None, 0, None, 0, None) == INVALID
    assert lib.nsr_posenc_e(None, 0, 4, 4, None, None) == INVALID
    # the networks the reference can build pass the same checks: deg_dir == 0 under no_dir, and the words on degree >= 1
    nodir = ctypes.byref(_arch(deg_dir=0, no_dir=True))
    assert lib.nsr_arch_tensor_numel_e(nodir, NO_XYZ, 0) == 128 * 36
    assert lib.nsr_arch_fused_packed_bytes_e(ok, NO_XYZ | LINEAR) > 0
    assert lib.nsr_posenc_e(None, 0, 4, NO_XYZ | LINEAR, None, None) == 0     # n == 0: nothing to do


def test_python_layer_shapes():
    from nerf_sr_amd import ops
    pe = ops.PositionalEncoding(3, 10, SimpleNamespace(no_xyz=True))
    assert pe.out_channels == 60 and pe.embed == NO_XYZ
    assert ops.PositionalEncoding(3, 10).out_channels == 63 == ops.PositionalEncoding(3, 10, SimpleNamespace(no_logscale=True)).out_channels
    assert ops.PositionalEncoding(3, 4, SimpleNamespace(no_xyz=True, no_logscale=True)).out_channels == 24
    lin = ops.PositionalEncoding(3, 6, SimpleNamespace(no_logscale=True)).freq_bands
    assert np.array_equal(lin, torch.linspace(1, 32, 6).numpy())
    # every dict and default that exists today stays as it is
    assert weights.arch_spec() == weights.STATE_DICT_SPEC == weights.arch_spec(no_xyz=False)
    assert "no_xyz" not in weights.arch_of(SimpleNamespace(no_xyz=True)) and "no_xyz" not in weights.normalize_arch(None)
    spec = weights.arch_spec(no_xyz=True)
    assert spec["xyz_encoding_1.0.weight"] == (256, 60) and spec["xyz_encoding_5.0.weight"] == (256, 316)
    assert spec["dir_encoding.0.weight"] == (128, 280)
    sd = weights.make_state_dict_arch(5, no_xyz=True, **er.SMALL)
    weights.check_state_dict_arch(sd, no_xyz=True, **er.SMALL)
    with pytest.raises(ValueError, match="no_xyz"):
        weights.check_state_dict_arch(weights.make_state_dict_arch(5, **er.SMALL), no_xyz=True, **er.SMALL)
    a, b = weights.make_state_dict_arch(5, **er.SMALL), weights._generate(5, "smooth", 0.05, er.SMALL)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_python_refusals_before_a_device_is_touched():
    """Everything that needs the 8 x 256 kernels names the embedding option it refuses; nothing here initialises a device."""
    from nerf_sr_amd import ops, train
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    for kw, name in (({"no_xyz": True}, "--no_xyz"), ({"no_logscale": True}, "--no_logscale")):
        opt = SimpleNamespace(**kw)
        with pytest.raises(ValueError, match=name):
            ops.check_mlp_options(opt)                    # fused=True: what VanillaMLP asks
        with pytest.raises(ValueError, match=name):
            ops.VanillaMLP(opt)
        ops.check_mlp_options(opt, fused=False)           # make_mlp / NeRFDownXModel serve them
        for prec in ("f16", "bf16"):
            with pytest.raises(ValueError, match=name):
                ops.make_mlp(default_options(precision=prec, **kw), precision=prec)
        with pytest.raises(ValueError, match=name):
            NeRFDownXModel(default_options(precision="f16x3", early_stop=0.01, **kw))
        with pytest.raises(ValueError, match=name):
            NeRFDownXModel(default_options(precision="f16x3", coarse_rgb=False, **kw))
        net = SimpleNamespace(embed=weights.embed_of(opt), precision="f16x3", color_activation="sigmoid")
        with pytest.raises(ValueError, match=name):
            ops.check_early_stop(0.01, net, 64)
        with pytest.raises(ValueError, match=name):
            ops.check_density_coarse(net, 64, 64)
        sd = weights.make_state_dict_arch(3, no_xyz=bool(kw.get("no_xyz")), **er.DEFAULT)
        for prec in ("f16x3", "f16x3_bwd3", "f16x3_bwd2", "f16x3_bwd1", "f16x3_bwdm"):      # the chain training precisions
            with pytest.raises(ValueError, match=name):
                train.Trainer(sd, sd, precision=prec, embed=weights.embed_of(opt), device="cpu")
            with pytest.raises(ValueError, match=name):
                train.forward_rays_train(sd, sd, torch.zeros(4, 8), precision=prec, embed=weights.embed_of(opt))
    # the words the library refuses are refused on the host too
    with pytest.raises(ValueError, match="no_xyz"):
        ops.GenericMLP(SimpleNamespace(no_xyz=True, deg_pos=0), device="cpu")
    with pytest.raises(ValueError, match="embed"):
        weights.check_embed(4, weights.normalize_arch(None))
    # a --no_xyz checkpoint loaded into a network built without the option: the message names the shape it expected, and the
    # other way round the option
    with pytest.raises(ValueError, match="no_xyz"):
        weights.check_state_dict_arch(weights.make_state_dict_arch(3, **er.DEFAULT), no_xyz=True, **er.DEFAULT)


@pytest.mark.parametrize("case", list(er.CASES))
def test_restatement_reproduces_the_fixture(g, golden_dir, case):
    """tests/embed_ref.py in fp32 against the reference's record, at the bounds tests/test_oracle_golden.py uses for arch.npz."""
    arch, embed, tag, white = er.CASES[case]
    assert int(g[f"{case}_embed"]) == embed and bool(g[f"{case}_white_bkgd"]) == white
    sd_c, sd_f = (oc.to_torch_sd(sd) for sd in er.state_dicts(g, arch, embed))
    pts, dirs = torch.from_numpy(g[f"{case}_xyz_256"]), torch.from_numpy(g[f"{case}_dir_256"])
    x = torch.cat([er.posenc(pts, arch["deg_pos"], embed), er.posenc(dirs, arch["deg_dir"], embed)], -1)
    np.testing.assert_allclose(x.numpy(), g[f"{case}_mlp_in_256"], rtol=0, atol=ATOL)
    x = torch.from_numpy(g[f"{case}_mlp_in_256"])
    np.testing.assert_allclose(oc.mlp_forward(sd_c, x).numpy(), g[f"{case}_mlp_out_256"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(oc.mlp_forward(sd_c, x[:64], sigma_only=True).numpy(), g[f"{case}_mlp_sigma_only_64"], rtol=0, atol=1e-5)
    rays = torch.from_numpy(np.load(os.path.join(golden_dir, f"path_{tag}.npz"))["rays"])[:int(g[f"{case}_n_rays"])]
    out = er.forward_rays(sd_c, sd_f, rays, arch, embed, 64, 64, white)
    for k, v in out.items():
        np.testing.assert_allclose(v.numpy(), g[f"{case}_{k}"], rtol=0, atol=1e-5 if "depth" in k else ATOL, err_msg=k)


@pytest.mark.parametrize("tag", er.TRAIN_CASES)
def test_restatement_reproduces_the_training_fixture(golden_dir, tag):
    """... and one training iteration: the reference's losses and gradient digests (the bounds of tests/test_train_arch_cpu.py's
    restatement check are not borrowed blindly: fp64 against the reference's fp32 autograd, 1e-6 on the losses, 2e-3 of the
    norm on every gradient tensor)."""
    gt = er.load_train_case(golden_dir, tag)
    sd_c, sd_f = weights.make_state_dict_arch(gt["seed_coarse"], no_xyz=bool(gt["embed"] & NO_XYZ), **gt["arch"]), \
        weights.make_state_dict_arch(gt["seed_fine"], no_xyz=bool(gt["embed"] & NO_XYZ), **gt["arch"])
    info, g_c, g_f = er.loss_and_grads(sd_c, sd_f, gt)
    for k in ("loss_coarse_mse", "loss_fine_mse", "loss_tot"):
        assert abs(info[k] - float(gt[k])) <= 1e-6, (k, info[k], float(gt[k]))
    for name, grads in (("coarse", g_c), ("fine", g_f)):
        for k, v in grads.items():
            want = float(gt[f"gnorm_{name}.{k}"])
            assert abs(float(v.norm()) - want) <= 2e-3 * want + 1e-9, (name, k)
