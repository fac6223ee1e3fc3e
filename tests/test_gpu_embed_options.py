"""The embedding options --no_xyz / --no_logscale (models/embedding.py:17-18) on the device, from the stand-alone encoder up
to the model and the training pair, against the reference's own record (tests/golden/embed.npz, train_embed.npz) and the fp64
restatement tests/embed_ref.py.  Bounds are those the existing tests apply to tests/golden/arch.npz on the same routes
(tests/test_gpu_options.py, tests/test_gpu_arch_fused.py, tests/test_gpu_train_arch.py); under the linear bands
``embed_ref.bound`` allows 2 x the reference's own fp32-vs-fp64 gap where that is larger.  With NSR_RECORD_PROFILES set the
measured figures of every case and route go to profiles/embed_options_parity.json."""
import ctypes
import json
import os
import warnings
from ctypes import c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from nerf_sr_amd.weights import make_state_dict_arch
from tests import arch_util as au
from tests import embed_ref as er

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_XYZ, LINEAR = _lib.NSR_EMBED_NO_XYZ, _lib.NSR_EMBED_LINEAR_FREQS
WORDS = (NO_XYZ, LINEAR, NO_XYZ | LINEAR)
INPUT_RANGE = 2
_PARITY = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "embed.npz"))


@pytest.fixture(scope="module")
def record():
    yield _PARITY
    if os.environ.get("NSR_RECORD_PROFILES") and _PARITY:
        with open(os.path.join(REPO, "profiles", "embed_options_parity.json"), "w") as f:
            json.dump({"reference": "tests/golden/embed.npz, train_embed.npz (the reference's own fp32 run); gap = its fp32 vs fp64",
                       "bound": "the bound of the same route on arch.npz; under --no_logscale max(that, 2 x gap)",
                       "cases": _PARITY}, f, indent=1, sort_keys=True)
            f.write("\n")


def _opt(embed, **kw):
    return SimpleNamespace(**er.options_of(embed), **kw)


def _posenc_e(x, deg, embed):
    out = torch.empty(x.shape[0], (0 if embed & NO_XYZ else 3) + 6 * deg, device="cuda")
    _lib.check(_lib.load().nsr_posenc_e(c_void_p(x.data_ptr()), x.shape[0], deg, embed, c_void_p(out.data_ptr()), None), "nsr_posenc_e")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. nsr_posenc_e: bit identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 255, 257))
def test_posenc_bit_identities(ops, n):
    rng = np.random.Generator(np.random.PCG64(n))
    x = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    x = np.concatenate([x, np.array([[0.0, 1e-40, 65504.0], [-0.0, -1e-40, -65504.0]], np.float32)])      # 0, a denormal, 65504
    x = torch.from_numpy(x).cuda()
    for deg in (0, 1, 2, 4, 10, 16):
        plain = ops.PositionalEncoding(3, deg)(x)
        assert torch.equal(_posenc_e(x, deg, 0).view(torch.int32), plain.view(torch.int32)), deg          # word 0 = nsr_posenc
        if deg > 0:
            assert torch.equal(_posenc_e(x, deg, NO_XYZ).view(torch.int32), plain[:, 3:].contiguous().view(torch.int32)), deg
        if deg in (1, 2):                                    # [1] and [1, 2] are the log-scale bands
            assert torch.equal(_posenc_e(x, deg, LINEAR).view(torch.int32), plain.view(torch.int32)), deg
            assert torch.equal(_posenc_e(x, deg, LINEAR | NO_XYZ).view(torch.int32), plain[:, 3:].contiguous().view(torch.int32)), deg
        if deg > 2:                                          # ... and beyond them the linear bands are other numbers
            assert not torch.equal(_posenc_e(x, deg, LINEAR), plain), deg
            assert torch.equal(_posenc_e(x, deg, LINEAR)[:, :9], plain[:, :9])                            # x and the band 1


# ---------------------------------------------------------------------------------------------------------------------
# 2. nsr_posenc_e against the reference's rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(er.CASES))
def test_posenc_against_the_fixture(ops, g, record, case):
    """PositionalEncoding(opt) on the points and directions behind mlp_in_256, within 2e-6 (tests/test_gpu_parity.py
    test_posenc).  Fails on a build that ignores ``opt``: the widths differ."""
    arch, embed, _, _ = er.CASES[case]
    pts, dirs = torch.from_numpy(g[f"{case}_xyz_256"]).cuda(), torch.from_numpy(g[f"{case}_dir_256"]).cuda()
    pe, de = ops.PositionalEncoding(3, arch["deg_pos"], _opt(embed)), ops.PositionalEncoding(3, arch["deg_dir"], _opt(embed))
    want = torch.from_numpy(g[f"{case}_mlp_in_256"])
    assert pe.out_channels + de.out_channels == want.shape[1]
    got = torch.cat([pe(pts), de(dirs)], -1).cpu()
    err = float((got - want).abs().max())
    record[f"{case}/posenc"] = {"err": err, "bound": 2e-6, "gap": float(g[f"{case}_gap_mlp_in_256"])}
    print(f"{case}: posenc {err:.3e}")
    assert got.shape == want.shape and err <= 2e-6, (case, err)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the network on the reference's encoded rows
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = {"fp32": dict(precision="fp32"), "f16x3": dict(precision="f16x3"), "f16x3_fused": dict(precision="f16x3", fused=True)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", list(er.CASES))
def test_network_on_encoded_rows(ops, g, record, case, route):
    arch, embed, _, _ = er.CASES[case]
    sd_c, _ = er.state_dicts(g, arch, embed)
    net = ops.GenericMLP(_opt(embed), **ROUTES[route], **arch).load_state_dict(sd_c)
    assert net.embed == embed and net.in_xyz + net.in_dir == g[f"{case}_mlp_in_256"].shape[1]
    x = torch.from_numpy(g[f"{case}_mlp_in_256"]).cuda()
    for key, got in (("mlp_out_256", net(x)), ("mlp_sigma_only_64", net(x[:64].contiguous(), sigma_only=True))):
        err = float((got.cpu() - torch.from_numpy(g[f"{case}_{key}"])).abs().max())
        bound = er.bound(g, case, key, 2e-5)
        record[f"{case}/{route}/{key}"] = {"err": err, "bound": bound, "gap": float(g[f"{case}_gap_{key}"])}
        print(f"{case} {route} {key}: {err:.3e} (bound {bound:.1e})")
        assert err <= bound, (case, route, key, err)
    assert net.status() == 0
    assert all(torch.equal(v.cpu(), torch.from_numpy(sd_c[k])) for k, v in net.state_dict().items())


# ---------------------------------------------------------------------------------------------------------------------
# 4. fused kernel: the rays entry equals the rows entry, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _rays(R, N, stride, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    cols = [rng.uniform(-1, 1, (R, 3)), rng.uniform(-1, 1, (R, 3)), np.zeros((R, 1)), np.ones((R, 1))]
    if stride == 11:
        v = rng.standard_normal((R, 3))
        cols.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    rays = torch.from_numpy(np.concatenate(cols, 1).astype(np.float32)).cuda()
    z = torch.from_numpy(np.sort(rng.uniform(0, 1, (R, N)), axis=1).astype(np.float32)).cuda()
    return rays, z


def _both_entries(ops, net, rays, z):
    """((R, N, 4), sigma only, status) of the rows entry fed with nsr_posenc_e's rows, and of the rays entry."""
    R, N = z.shape
    opt = _opt(net.embed)
    pts = ops.cast_rays(rays[:, 0:3], rays[:, 3:6], z).reshape(-1, 3).contiguous()
    dirs = (rays[:, 8:11] if rays.shape[1] == 11 else rays[:, 3:6]).contiguous()
    x = torch.cat([ops.PositionalEncoding(3, net.arch["deg_pos"], opt)(pts),
                   ops.PositionalEncoding(3, net.arch["deg_dir"], opt)(dirs).repeat_interleave(N, dim=0)], -1).contiguous()
    net.status(clear=True)
    want, want_sig = net(x).view(R, N, 4), net(x, sigma_only=True).view(R, N)
    st_rows = net.status(clear=True)
    rgb, sig = ops.render_rays(net, rays, z)
    sig_only = ops.render_rays_sigma(net, rays, z)
    st_rays = net.status(clear=True)
    return (want, want_sig, st_rows), (torch.cat([rgb, sig[..., None]], -1), sig_only, st_rays)


@pytest.mark.parametrize("embed", (0,) + WORDS)
def test_rays_entry_equals_rows_entry_bit_for_bit(ops, embed):
    """R in {1, 3, 33} x N in {1, 64}: one point, a tail tile, tiles that span rays, at strides 8 and 11; word 0 rides the same
    `_e` entry points and must keep the promise it had."""
    arch = {**er.SMALL, "no_dir": False}
    net = ops.GenericMLP(_opt(embed), precision="f16x3", fused=True, **arch).load_state_dict(
        make_state_dict_arch(31, no_xyz=bool(embed & NO_XYZ), **arch))
    for R in (1, 3, 33):
        for N in (1, 64):
            for stride in (8, 11):
                rays, z = _rays(R, N, stride, 100 * R + N + stride)
                (want, want_sig, st_rows), (got, got_sig, st_rays) = _both_entries(ops, net, rays, z)
                tag = (embed, R, N, stride)
                assert torch.isfinite(want).all(), tag
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (tag, float((got - want).abs().max()))
                assert torch.equal(got_sig.view(torch.int32), want_sig.view(torch.int32)), tag
                assert st_rays == st_rows == 0, (tag, st_rays, st_rows)
    # a ray whose origin is 1e6 away: the raw coordinate is a network input (beyond fp16's 65,504) under word 0 and under
    # LINEAR alone, and is not one under NO_XYZ, whose columns are sines and cosines
    rays, z = _rays(3, 33, 8, 5)
    rays[1, 0:3] = torch.tensor([1.0e6, 0.0, 0.0])
    (want, _, st_rows), (got, _, st_rays) = _both_entries(ops, net, rays, z)
    assert st_rows == st_rays, (embed, st_rows, st_rays)
    assert bool(st_rows & INPUT_RANGE) == (not embed & NO_XYZ), (embed, st_rows)
    assert torch.equal(got[[0, 2]], want[[0, 2]])
    if embed & NO_XYZ:
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. NeRFDownXModel.forward_rays on the fixture rays
# ---------------------------------------------------------------------------------------------------------------------
MODEL_ROUTES = {"fp32": dict(precision="fp32"), "f16x3": dict(precision="f16x3"), "f16x3_fused": dict(precision="f16x3", arch_fused=True)}
BORROWED = {"coarse_comp_rgbs": 1e-4, "fine_comp_rgbs": 1e-4, "coarse_opacity": 1e-4, "fine_opacity": 1e-4, "coarse_weights": 1e-5,
            # the arch.npz model test bounds the five above; the other three take the colour bound, which is also what the
            # oracle test allows the weights of a pass whose colours it holds to 1e-4 (depth: of NDC / Blender size, <= 6)
            "coarse_depth": 1e-4, "fine_depth": 1e-4, "fine_weights": 1e-4}


@pytest.mark.parametrize("route", list(MODEL_ROUTES))
@pytest.mark.parametrize("case", list(er.CASES))
def test_model_forward_rays(ops, g, golden_dir, record, case, route):
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    from nerf_sr_amd import ops as ops_mod
    arch, embed, tag, white = er.CASES[case]
    sd_c, sd_f = er.state_dicts(g, arch, embed)
    opt_kw = dict(white_bkgd=white, **MODEL_ROUTES[route], **er.options_of(embed), **{**arch, "skips": list(arch["skips"])})
    if case == "default_both" and route == "fp32":
        # the default network with an embedding option is "a non-default architecture": it warns once, by a key and a text
        # that name the options, and never enters a VanillaMLP
        ops_mod._GENERIC_WARNED.clear()
        with pytest.warns(RuntimeWarning, match="--no_xyz --no_logscale"):
            m = NeRFDownXModel(default_options(**opt_kw))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            NeRFDownXModel(default_options(**opt_kw))
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            m = NeRFDownXModel(default_options(**opt_kw))
    m.load_networks(sd_c, sd_f).eval()
    for net in (m.netCoarse, m.netFine):
        assert isinstance(net, ops.GenericMLP) and not isinstance(net, ops.VanillaMLP) and net.embed == embed
        assert net.fused == (route == "f16x3_fused") and net.precision == MODEL_ROUTES[route]["precision"]
    assert not m.fused and m.arch_fused == (route == "f16x3_fused")
    rays = torch.from_numpy(np.load(os.path.join(golden_dir, f"path_{tag}.npz"))["rays"])[:int(g[f"{case}_n_rays"])].cuda()
    out = m.forward_rays(rays)
    assert set(out) == set(er.OUT_KEYS)
    worst = None
    for k in er.OUT_KEYS:
        err = float((out[k].cpu() - torch.from_numpy(g[f"{case}_{k}"])).abs().max())
        bound = er.bound(g, case, k, BORROWED[k])
        record[f"{case}/{route}/{k}"] = {"err": err, "bound": bound, "gap": float(g[f"{case}_gap_{k}"])}
        print(f"{case} {route} {k}: {err:.3e} (bound {bound:.1e})")
        if err > bound and worst is None:
            worst = (k, err, bound)
    assert worst is None, (case, route, worst)
    if route == "f16x3_fused":      # the rays entry and the encoded-rows route of the model: the same bits
        m.opt.arch_fused_rays = False
        rows = m.forward_rays(rays)
        for k in er.OUT_KEYS:
            assert torch.equal(rows[k], out[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 6. training
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import train as _tr
    return _tr


_ORACLE64 = {}


def _train_case(golden_dir, tag):
    gt = er.load_train_case(golden_dir, tag)
    no_xyz = bool(gt["embed"] & NO_XYZ)
    sds = [make_state_dict_arch(gt[s], no_xyz=no_xyz, **gt["arch"]) for s in ("seed_coarse", "seed_fine")]
    if tag not in _ORACLE64:
        _ORACLE64[tag] = er.loss_and_grads(sds[0], sds[1], gt)
    return gt, sds, _ORACLE64[tag]


def _pair(tr, gt, sds, precision, embed, arch="case"):
    """forward_rays_train + the reference's loss_tot + autograd: (losses, outputs, gradients per network)."""
    p = [{k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in sd.items()} for sd in sds]
    draws = {k: torch.from_numpy(v).cuda() for k, v in er.draws_of(gt).items()}
    out = tr.forward_rays_train(p[0], p[1], torch.from_numpy(gt["rays"]).cuda(), draws, white_bkgd=bool(gt["white_bkgd"]),
                                noise_std=float(gt["noise_std"]), precision=precision, arch=gt["arch"] if arch == "case" else arch,
                                embed=embed)
    target, s2 = torch.from_numpy(gt["target_lr"]).cuda(), int(gt["s2"])
    mse = torch.nn.functional.mse_loss
    lc = mse(out["coarse_comp_rgbs"].view(-1, s2, 3).mean(1), target) * float(gt["lambda_coarse"])
    lf = mse(out["fine_comp_rgbs"].view(-1, s2, 3).mean(1), target) * float(gt["lambda_fine"])
    (lc + lf).backward()
    return (float(lc.detach()), float(lf.detach())), {k: v.detach() for k, v in out.items()}, [{k: v.grad for k, v in n.items()} for n in p]


@pytest.mark.parametrize("prec", ("fp32", "f16x3_gemm"))
@pytest.mark.parametrize("tag", er.TRAIN_CASES)
def test_training_pair_vs_reference_and_restatement(tr, golden_dir, record, tag, prec):
    gt, sds, (res64, gc64, gf64) = _train_case(golden_dir, tag)
    losses, out, grads = _pair(tr, gt, sds, prec, gt["embed"])
    record[f"train/{tag}/{prec}/losses"] = {"got": losses, "reference": [float(gt["loss_coarse_mse"]), float(gt["loss_fine_mse"])],
                                           "fp64": [res64["loss_coarse_mse"], res64["loss_fine_mse"]], "bound": 1e-6}
    print(tag, prec, "losses", losses, float(gt["loss_coarse_mse"]), float(gt["loss_fine_mse"]))
    assert abs(losses[0] - float(gt["loss_coarse_mse"])) <= 1e-6 and abs(losses[1] - float(gt["loss_fine_mse"])) <= 1e-6
    spec = er.spec_of(gt["arch"], gt["embed"])
    for n, (name, ref) in enumerate((("coarse", gc64), ("fine", gf64))):
        assert list(grads[n]) == list(spec)
        rel, worst = au.assert_grads_close(grads[n], ref, spec, f"{tag}-{prec} {name}")
        record[f"train/{tag}/{prec}/grads_{name}"] = {"whole": rel, "worst": worst[0], "worst_tensor": worst[1]}
    # two identical calls give identical bits
    losses2, out2, grads2 = _pair(tr, gt, sds, prec, gt["embed"])
    assert losses2 == losses and all(torch.equal(out[k], out2[k]) for k in out)
    assert all(torch.equal(grads[n][k], grads2[n][k]) for n in range(2) for k in spec)


@pytest.mark.parametrize("prec", ("fp32", "f16x3_gemm"))
def test_pair_at_word_0_is_the_plain_pair_bit_for_bit(tr, golden_dir, prec):
    """nsr_train_arch_forward / _backward ARE the `_e` forms at embed = 0: called directly, both give the same bits."""
    gt = au.load_case(golden_dir, "small")
    lib, arch = _lib.load(), _lib.NsrArch.from_arch(tr.normalize_arch(gt["arch"]))
    rays = torch.from_numpy(gt["rays"]).cuda()
    draws = [torch.from_numpy(gt[k]).cuda() for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine")]
    w = [[torch.from_numpy(v).cuda() for v in sd.values()] for sd in au.state_dicts(gt)]
    R, p = rays.shape[0], _lib.TRAIN_PRECISIONS[prec]
    a = ctypes.byref(arch)
    n_saved, n_ws = lib.nsr_train_arch_saved_bytes(a, p, R, 64, 64, 0), lib.nsr_train_arch_workspace_bytes(a, p, R, 64, 64)
    assert n_saved == lib.nsr_train_arch_saved_bytes_e(a, 0, p, R, 64, 64, 0) > 0
    g_rgb = torch.ones(R, 3, device="cuda")      # upstream of both colours: the fine pass does not reach the coarse network
    g8 = (c_void_p * 8)(c_void_p(g_rgb.data_ptr()), *[c_void_p(0)] * 3, c_void_p(g_rgb.data_ptr()), *[c_void_p(0)] * 3)
    res = []
    for lead, fwd, bwd in (((a,), lib.nsr_train_arch_forward, lib.nsr_train_arch_backward),
                           ((a, 0), lib.nsr_train_arch_forward_e, lib.nsr_train_arch_backward_e)):
        outs = tr._alloc_outs(R, 64, 64, "cuda")
        saved = torch.zeros(n_saved, dtype=torch.uint8, device="cuda")
        ws = torch.zeros(n_ws, dtype=torch.uint8, device="cuda")
        grads = [[torch.zeros_like(t) for t in n] for n in w]
        rc = fwd(*lead, tr._ptr_array(w[0]), tr._ptr_array(w[1]), c_void_p(rays.data_ptr()), 8, R, 64, 64, 0, 0,
                 *[c_void_p(d.data_ptr()) for d in draws], float(gt["noise_std"]), p, 0, tr._ptr_array(outs), c_void_p(ws.data_ptr()),
                 ws.numel(), c_void_p(saved.data_ptr()), saved.numel(), tr._stream())
        assert rc == 0
        if len(lead) == 2:      # a backward with another word than the forward's: refused, nothing written
            for other in WORDS:
                assert bwd(a, other, tr._ptr_array(w[0]), tr._ptr_array(w[1]), g8, tr._ptr_array(grads[0]), tr._ptr_array(grads[1]),
                           c_void_p(ws.data_ptr()), ws.numel(), c_void_p(saved.data_ptr()), saved.numel(), tr._stream()) == -1
            torch.cuda.synchronize()
            assert all(float(t.abs().max()) == 0.0 for n in grads for t in n)
        rc = bwd(*lead, tr._ptr_array(w[0]), tr._ptr_array(w[1]), g8, tr._ptr_array(grads[0]), tr._ptr_array(grads[1]),
                 c_void_p(ws.data_ptr()), ws.numel(), c_void_p(saved.data_ptr()), saved.numel(), tr._stream())
        assert rc == 0
        res.append((outs, grads))
    assert all(torch.equal(x, y) for x, y in zip(res[0][0], res[1][0]))
    for n in range(2):
        for i, (x, y) in enumerate(zip(res[0][1][n], res[1][1][n])):
            assert torch.equal(x, y), (n, i)
            assert float(x.abs().max()) > 0, (n, i)


def test_trainer_step_and_render(tr, ops, golden_dir):
    """One Trainer(embed=) step is torch.optim.Adam on the pair's gradients (tests/test_gpu_train_arch.py: within one ulp of
    O(1) weights), arch=None with a non-zero word is the default descriptor, and the trained state_dicts load into the
    matching GenericMLP, whose eval render equals the trainer's deterministic forward."""
    gt, sds, _ = _train_case(golden_dir, "both")
    embed, spec = gt["embed"], er.spec_of(gt["arch"], gt["embed"])
    t = tr.Trainer(sds[0], sds[1], white_bkgd=bool(gt["white_bkgd"]), downscale=2, randomized=True, noise_std=float(gt["noise_std"]),
                   lr=float(gt["lr"]), beta1=float(gt["beta1"]), arch=gt["arch"], embed=embed, precision="fp32")
    rays = torch.from_numpy(gt["rays"]).cuda()
    t.set_input(rays, torch.from_numpy(gt["target_lr"]).cuda())
    t.loss_and_grads({k: torch.from_numpy(v).cuda() for k, v in er.draws_of(gt).items()})
    assert abs(float(t.losses[0]) - float(gt["loss_coarse_mse"])) <= 1e-6 and abs(float(t.losses[1]) - float(gt["loss_fine_mse"])) <= 1e-6
    ref = [{k: torch.nn.Parameter(v.clone()) for k, v in n.items()} for n in t.params]
    for n in range(2):
        for k in spec:
            ref[n][k].grad = t.grads[n][k].clone()
    opt = torch.optim.Adam([v for n in ref for v in n.values()], lr=float(gt["lr"]), betas=(float(gt["beta1"]), 0.999), eps=1e-8)
    t.optimizer_step()
    opt.step()
    for n in range(2):
        for k in spec:
            assert float((t.params[n][k] - ref[n][k].detach()).abs().max()) <= 2.4e-7, (n, k)
    # the reference's own coarse weights after its step (the update, as in test_adam_step_vs_reference)
    from tests.util import sample_idx
    for k in spec:
        got = t.params[0][k].cpu().numpy().reshape(-1)
        idx = sample_idx(got.size)
        upd, upd_ref = got[idx] - sds[0][k].reshape(-1)[idx], gt[f"w1_coarse.{k}"] - sds[0][k].reshape(-1)[idx]
        assert (np.abs(upd - upd_ref) > 2e-5).mean() <= 0.02, k
    sd_c, sd_f = t.state_dicts()
    nets = [ops.GenericMLP(_opt(embed), precision="fp32", **gt["arch"]).load_state_dict(sd) for sd in (sd_c, sd_f)]
    assert nets[0].embed == embed
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m = NeRFDownXModel(default_options(white_bkgd=bool(gt["white_bkgd"]), precision="fp32", **er.options_of(embed),
                                           **{**gt["arch"], "skips": list(gt["arch"]["skips"])}))
    ev = m.load_networks(sd_c, sd_f).eval().forward_rays(rays)
    t2 = tr.Trainer(sd_c, sd_f, white_bkgd=bool(gt["white_bkgd"]), downscale=2, randomized=False, arch=gt["arch"], embed=embed, precision="fp32")
    t2.set_input(rays, torch.from_numpy(gt["target_lr"]).cuda())
    with torch.no_grad():
        det = t2.forward()
    # Two fp32 routes to one function, each held to the reference at BORROWED above; that is the bound between them.  The 2e-6
    # of the log-scale round trip (tests/test_gpu_train_arch.py) does not carry over: the eval encoder is sinf / cosf, the
    # training encoder nsr_sincos (<= 1.5e-7 from it per column), and the resampler amplifies such differences as it does the
    # reference's own rounding (its fp32-vs-fp64 gap on fine_weights under these options: 1.3e-5, embed.npz)
    for k in tr.OUT_KEYS:
        d = float((ev[k] - det[k]).abs().max())
        print("eval render vs train-mode forward", k, d)
        assert d <= BORROWED[k], (k, d)
    # arch=None + a word: the default descriptor on the arch pair
    d = er.DEFAULT
    sd = make_state_dict_arch(7, no_xyz=True, **d)
    t3 = tr.Trainer(sd, sd, arch=None, embed=NO_XYZ | LINEAR, precision="f16x3_gemm", downscale=2)
    assert t3.arch is not None and t3.arch["D"] == 8 and t3.arch["W"] == 256 and t3.params[0]["xyz_encoding_1.0.weight"].shape == (256, 60)
