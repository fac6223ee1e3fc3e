"""Train-mode forward_rays as a torch.autograd.Function (nsr_train_forward / nsr_train_backward, include/nsr_train.h):
the same kernels as the fused step split at the loss, against the fused step bit for bit, the fp64 training oracle and the
reference's own fixtures.  Bounds as in tests/test_gpu_train.py (see its docstring): every gradient tensor within 2e-3 of its
norm of the fp64 oracle, 5e-4 on the heads, the whole network within 2e-3."""
import os
import re

import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import make_state_dict, STATE_DICT_SPEC
from oracle import nerf_oracle as oc
from oracle import train_oracle as to
from tests.util import train_draws

pytestmark = pytest.mark.gpu

HEAD = ("rgb.0.weight", "rgb.0.bias", "dir_encoding.0.weight", "dir_encoding.0.bias", "xyz_encoding_final.weight",
        "xyz_encoding_final.bias", "sigma.weight", "sigma.bias")
OPTIONS = {"llff_det": {}, "llff_rand": {}, "blender_rand": {}, "blender_var": {}, "llff_gamma": {"gamma_correct": True},
           "blender_softplus": {"sigma_activation": "softplus"}, "llff_colornone": {"color_activation": "none"},
           "blender_stopgrad": {"stop_grad": True}}
ALL_PRECISIONS = ("f16x3", "fp32", "f16x3_gemm", "f16x3_bwd3", "f16x3_bwd2", "f16x3_bwd1", "f16x3_bwdm")


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import train as _tr
    return _tr


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"train_{name}.npz"))


def _trainer(tr, g, **kw):
    sd_c, sd_f = make_state_dict(int(g["seed_coarse"])), make_state_dict(int(g["seed_fine"]))
    t = tr.Trainer(sd_c, sd_f, white_bkgd=bool(g["white_bkgd"]), downscale=int(round(int(g["s2"]) ** 0.5)),
                   randomized=bool(g["randomized"]), noise_std=float(g["noise_std"]), lr=float(g["lr"]),
                   beta1=float(g["beta1"]), lambda_coarse_mse=float(g["lambda_coarse"]),
                   lambda_fine_mse=float(g["lambda_fine"]), **kw)
    t.set_input(torch.from_numpy(g["rays"]).cuda(), torch.from_numpy(g["target_lr"]).cuda())
    return t, sd_c, sd_f


def _draws(g):
    return {k: torch.from_numpy(v).cuda() for k, v in train_draws(g).items() if k != "noise_std"}


def _assert_grads(got, refs, what, head_bound=5e-4):
    """got: per network a dict of device tensors; refs: per network the fp64 oracle's."""
    for n in range(2):
        num = den = 0.0
        for k in STATE_DICT_SPEC:
            x, want = got[n][k].detach().cpu().double(), refs[n][k]
            err, nrm = float((x - want).norm()), float(want.norm())
            num, den = num + err ** 2, den + nrm ** 2
            assert err <= 2e-3 * nrm + 1e-9, (what, n, k, err / max(nrm, 1e-30))
            if k in HEAD:
                assert err <= head_bound * nrm + 1e-9, (what, n, k, err / max(nrm, 1e-30))
        assert den == 0.0 or (num / den) ** 0.5 < 2e-3, (what, n, (num / den) ** 0.5)


def _sr_mean(x, s2):
    return x.reshape(-1, s2, x.shape[-1] if x.ndim == 2 else 1).mean(1)


def _reference_loss(out, tgt, s2, lam_c, lam_f, lam_var=None, far=None):
    """calculate_losses (models/nerf_downX_model.py:326-378) written in torch on the autograd outputs."""
    mse = torch.nn.functional.mse_loss
    loss = mse(_sr_mean(out["coarse_comp_rgbs"], s2), tgt) * lam_c + mse(_sr_mean(out["fine_comp_rgbs"], s2), tgt) * lam_f
    if lam_var is not None:
        n_lr = tgt.shape[0]
        var = lambda t: torch.sum(torch.var(torch.reshape(t, (n_lr, s2, -1)), dim=1))
        loss = loss + lam_var[0] * var(out["coarse_comp_rgbs"]) + lam_var[1] * var(out["fine_comp_rgbs"]) \
            + lam_var[2] * var(out["coarse_depth"] / far) + lam_var[3] * var(out["fine_depth"] / far)
    return loss


# ---- 4. the same arithmetic as the fused step ------------------------------------------------------------------------
def _fused_g_comp(comp, target, s2, lam, n_lr_total):
    """lr_loss_kernel's dL/d(comp) (nsr_train.hip): fp32 sequential s2 sum, fp32 divide, fp32 difference, then
    float32(2.0 * lambda * d * scale / s2) evaluated in double left to right with scale = 1 / (3 N_lr)."""
    c = comp.cpu().numpy().reshape(-1, s2, 3)
    acc = np.zeros((c.shape[0], 3), np.float32)
    for k in range(s2):
        acc = (acc + c[:, k]).astype(np.float32)
    lr = (acc / np.float32(s2)).astype(np.float32)
    d = (lr - target.astype(np.float32)).astype(np.float32)
    scale = 1.0 / (3.0 * float(n_lr_total))
    gc = (2.0 * float(np.float32(lam)) * d.astype(np.float64) * scale / float(s2)).astype(np.float32)
    return torch.from_numpy(np.repeat(gc[:, None, :], s2, axis=1).reshape(-1, 3)).cuda()


@pytest.mark.parametrize("prec", ALL_PRECISIONS)
def test_pair_is_the_fused_step_bit_for_bit(golden_dir, tr, prec):
    """Forward outputs equal nsr_train_loss_and_grads's, and the backward given the fused step's own dL/d(comp) returns its
    gradients, bit for bit -- in one chunk and in three."""
    g = _load(golden_dir, "llff_rand")
    R = g["rays"].shape[0]
    for chunk in (R, 32):
        t, _, _ = _trainer(tr, g, precision=prec, ray_chunk=chunk)
        t.loss_and_grads(_draws(g))
        fused_out = {k: t.out[k].clone() for k in tr.OUT_KEYS}
        fused_g = [{k: v.clone() for k, v in t.grads[n].items()} for n in range(2)]
        t2, _, _ = _trainer(tr, g, precision=prec, ray_chunk=chunk)
        out = t2.forward(_draws(g))
        for k in tr.OUT_KEYS:
            assert torch.equal(out[k].detach(), fused_out[k]), (prec, chunk, k)
        s2, n_lr = int(g["s2"]), R // int(g["s2"])
        gcc = _fused_g_comp(out["coarse_comp_rgbs"].detach(), g["target_lr"], s2, float(g["lambda_coarse"]), n_lr)
        gcf = _fused_g_comp(out["fine_comp_rgbs"].detach(), g["target_lr"], s2, float(g["lambda_fine"]), n_lr)
        leaves = t2._weight_leaves()
        grads = torch.autograd.grad([out["coarse_comp_rgbs"], out["fine_comp_rgbs"]], leaves[0] + leaves[1], [gcc, gcf])
        for n in range(2):
            for i, k in enumerate(STATE_DICT_SPEC):
                assert torch.equal(grads[24 * n + i], fused_g[n][k]), (prec, chunk, n, k)


# ---- 2. reference parity through autograd ----------------------------------------------------------------------------
_ORACLE = {}


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("name", list(OPTIONS))
def test_reference_losses_through_autograd(golden_dir, tr, name, prec):
    """The eight training fixtures with calculate_losses written in torch over forward_rays_train's outputs (the variance
    terms of blender_var included): losses against the reference's, gradients against the fp64 oracle."""
    g = _load(golden_dir, name)
    opts = OPTIONS[name]
    lam_var = g["lambda_var"].tolist() if "lambda_var" in g else None
    t, sd_c, sd_f = _trainer(tr, g, precision=prec, **opts)
    out = t.forward(_draws(g))
    s2 = int(g["s2"])
    far = float(g["rays"][0, 7])
    tgt = t.data_rgbs
    loss = _reference_loss(out, tgt, s2, float(g["lambda_coarse"]), float(g["lambda_fine"]), lam_var, far)
    scale = max(1.0, float(np.abs(g["hr_fine"]).max()))
    assert abs(float(loss.detach()) - float(g["loss_tot"])) < 2e-5 * scale * scale, (float(loss.detach()), float(g["loss_tot"]))
    with torch.no_grad():
        lc = torch.nn.functional.mse_loss(_sr_mean(out["coarse_comp_rgbs"], s2), tgt) * float(g["lambda_coarse"])
    assert abs(float(lc) - float(g["loss_coarse_mse"])) < 1e-6 * scale * scale
    t.backward(loss)
    _, gc, gf = to.loss_and_grads(sd_c, sd_f, g["rays"], g["target_lr"], s2, 64, 64, bool(g["white_bkgd"]),
                                  float(g["lambda_coarse"]), float(g["lambda_fine"]), dtype=torch.float64, lambda_var=lam_var,
                                  **opts, **train_draws(g))
    _assert_grads(t.grads, (gc, gf), (name, prec))
    assert t.status() == 0


# ---- 3. every output's gradient --------------------------------------------------------------------------------------
def _oracle_grads(sd_c, sd_f, rays, draws, white, loss_fn, **opts):
    sc = {k: v.clone().requires_grad_(True) for k, v in oc.to_torch_sd(sd_c, torch.float64).items()}
    sf = {k: v.clone().requires_grad_(True) for k, v in oc.to_torch_sd(sd_f, torch.float64).items()}
    d = {k: torch.as_tensor(v).double() for k, v in draws.items() if k != "noise_std"}
    out = to.forward_train(sc, sf, torch.as_tensor(rays).double(), 64, 64, white, noise_std=draws["noise_std"], **d, **opts)
    loss_fn(out).backward()
    grad = lambda v: v.grad.detach() if v.grad is not None else torch.zeros_like(v)
    return {k: grad(v) for k, v in sc.items()}, {k: grad(v) for k, v in sf.items()}


@pytest.mark.parametrize("name", ["llff_rand", "blender_rand"])        # white background off / on
def test_every_output_has_its_gradient(golden_dir, tr, name):
    """A loss on ONE output at a time -- comp_rgbs, depth, opacity, weights of either network -- through the compositing
    backward's new upstream terms, against the fp64 oracle's autograd of the same loss; then an HR-colour MSE (--sisr_path)."""
    g = _load(golden_dir, name)
    draws = train_draws(g)
    gen = torch.Generator().manual_seed(7)
    R = g["rays"].shape[0]
    for key in tr.OUT_KEYS:
        shape = (R, 3) if key.endswith("rgbs") else ((R,) if not key.endswith("weights") else (R, 64 if key.startswith("coarse") else 128))
        wgt = torch.randn(*shape, generator=gen)
        if key.endswith("depth"):
            wgt = wgt * 0.1
        t, sd_c, sd_f = _trainer(tr, g, precision="f16x3")
        out = t.forward(_draws(g))
        t.backward((out[key] * wgt.cuda()).sum())
        refs = _oracle_grads(sd_c, sd_f, g["rays"], draws, bool(g["white_bkgd"]), lambda o: (o[key] * wgt.double()).sum())
        _assert_grads(t.grads, refs, (name, key))
        if key.startswith("coarse"):          # the fine pass resamples from DETACHED coarse weights
            assert not any(bool(v.any()) for v in t.grads[1].values()), key
    hr = torch.rand(R, 3, generator=gen)
    t, sd_c, sd_f = _trainer(tr, g, precision="f16x3")
    out = t.forward(_draws(g))
    mse = torch.nn.functional.mse_loss
    t.backward(mse(out["coarse_comp_rgbs"], hr.cuda()) + mse(out["fine_comp_rgbs"], hr.cuda()))
    refs = _oracle_grads(sd_c, sd_f, g["rays"], draws, bool(g["white_bkgd"]),
                         lambda o: mse(o["coarse_comp_rgbs"], hr.double()) + mse(o["fine_comp_rgbs"], hr.double()))
    _assert_grads(t.grads, refs, (name, "sisr"))


def test_two_forwards_feed_one_loss(golden_dir, tr):
    """Main batch + patch (or --with_ref batch): each forward keeps its own saved state; the gradient of the summed loss is
    the sum of the two single backwards, bit for bit."""
    g = _load(golden_dir, "llff_rand")
    t, _, _ = _trainer(tr, g, precision="f16x3")
    from nerf_sr_amd import ops, cameras
    patch = ops.subpixel_rays(cameras.spiral_pose(0.3), (64, 48), cameras.llff_focal(64), 2, True)[:16].reshape(-1, 8).contiguous()
    gen = torch.Generator().manual_seed(1)
    d2 = {"u_coarse": torch.rand(64, 64, generator=gen).cuda(), "u_fine": torch.rand(64, 64, generator=gen).cuda()}
    leaves = t._weight_leaves()
    flat = leaves[0] + leaves[1]
    loss_a = lambda o: ((o["fine_comp_rgbs"] - 0.5) ** 2).mean() + o["coarse_opacity"].mean()
    loss_b = lambda o: tr.tv_loss(o["fine_comp_rgbs"].view(8, 8, 3)) + o["fine_depth"].mean() * 0.1
    ga = torch.autograd.grad(loss_a(t.forward(_draws(g))), flat)
    gb = torch.autograd.grad(loss_b(t.forward(d2, rays=patch)), flat)
    both = torch.autograd.grad(loss_a(t.forward(_draws(g))) + loss_b(t.forward(d2, rays=patch)), flat)
    for a, b, s in zip(ga, gb, both):
        assert torch.equal(s, a + b)
    assert any(bool(b.any()) for b in gb)


# ---- 5. hygiene ------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    """A module whose parameters() come in state_dict order, like the reference's VanillaMLP."""

    def __init__(self, sd):
        super().__init__()
        self.names = []
        for k in STATE_DICT_SPEC:
            n = k.replace(".", "_")
            setattr(self, n, torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(sd[k])).cuda()))
            self.names.append(n)


def test_hygiene(golden_dir, tr):
    g = _load(golden_dir, "llff_rand")
    rays = torch.from_numpy(g["rays"]).cuda()
    net_c, net_f = _Net(make_state_dict(99)), _Net(make_state_dict(100))
    out = tr.forward_rays_train(net_c, net_f, rays, _draws(g))
    loss = out["fine_comp_rgbs"].sum()
    opt = torch.optim.Adam(list(net_c.parameters()) + list(net_f.parameters()), lr=1e-3)
    for p in list(net_c.parameters()) + list(net_f.parameters()):
        p.grad = torch.ones_like(p)
    opt.step()                               # an in-place update between forward and backward
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    out = tr.forward_rays_train(net_c, net_f, rays, _draws(g))
    loss = out["coarse_comp_rgbs"].sum()
    loss.backward()
    with pytest.raises(RuntimeError):        # a second backward
        loss.backward()
    with pytest.raises(ValueError):
        tr.forward_rays_train(net_c, net_f, rays.clone().requires_grad_(True))
    # out-of-range weights: NSR_FLAG_WEIGHT_RANGE in the sticky word of the shared workspace, as the fused step does
    t, _, _ = _trainer(tr, g, precision="f16x3")
    t.backward(t.forward(_draws(g))["fine_comp_rgbs"].sum())
    assert t.status() == 0
    t.params[1]["xyz_encoding_3.0.weight"][5, 7] = 2000.0
    t.forward(_draws(g))
    assert t.status(clear=True) & 1


def test_default_device_trainer_keeps_its_workspace(golden_dir, tr):
    """Trainer(device="cuda") -- no index -- keeps ONE workspace across steps: no re-allocation, reset or status read per step."""
    g = _load(golden_dir, "llff_rand")
    t = tr.Trainer(make_state_dict(99), make_state_dict(100), downscale=2, noise_std=1.0)
    assert t.device == torch.device("cuda")
    t.set_input(torch.from_numpy(g["rays"]).cuda(), torch.from_numpy(g["target_lr"]).cuda())
    t.optimize_parameters()
    ptr = t._ws.data_ptr()
    t.optimize_parameters()
    assert t._ws.data_ptr() == ptr
    t.backward(t.forward()["fine_comp_rgbs"].sum())          # the autograd pair shares it too
    assert t._ws.data_ptr() == ptr


def test_trainer_adam_step_between_forward_and_backward_raises(golden_dir, tr):
    """optimizer_step writes the weights through raw pointers; it marks them modified, so a backward of a forward made before
    it fails autograd's version check instead of mixing two sets of weights -- on both paths."""
    g = _load(golden_dir, "llff_rand")
    for prec in ("f16x3", "fp32"):
        t, _, _ = _trainer(tr, g, precision=prec)
        t.backward(t.forward(_draws(g))["fine_comp_rgbs"].sum())
        t.optimizer_step()                                   # after a backward: fine
        loss = t.forward(_draws(g))["fine_comp_rgbs"].sum()
        t.optimizer_step()
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            t.backward(loss)


def test_backward_checks_the_saved_header(golden_dir, tr):
    """A saved buffer that no forward wrote is NSR_ERR_INVALID_ARG, a valid one handed over with fewer bytes than its header
    says is NSR_ERR_WORKSPACE -- both before anything is enqueued; the real buffer then works."""
    from ctypes import c_void_p
    from nerf_sr_amd import _lib
    g = _load(golden_dir, "llff_rand")
    t, _, _ = _trainer(tr, g, precision="f16x3")
    out = t.forward(_draws(g))
    node = out["fine_comp_rgbs"].grad_fn                     # the Function's ctx
    saved, ws = node.state, t._ws
    lib = _lib.load()
    leaves = t._weight_leaves()
    grads = [[torch.empty_like(p) for p in n] for n in leaves]
    gf = torch.ones_like(out["fine_comp_rgbs"])
    g8 = (c_void_p * 8)(*[c_void_p(0)] * 4, c_void_p(gf.data_ptr()), *[c_void_p(0)] * 3)

    def bwd(buf, nbytes):
        rc = lib.nsr_train_backward(tr._ptr_array(leaves[0]), tr._ptr_array(leaves[1]), g8, tr._ptr_array(grads[0]),
                                    tr._ptr_array(grads[1]), c_void_p(ws.data_ptr()), ws.numel(), c_void_p(buf.data_ptr()),
                                    nbytes, tr._stream())
        torch.cuda.synchronize()
        return rc
    zeros = torch.zeros_like(saved)
    assert bwd(zeros, zeros.numel()) == -1
    garbage = saved.clone()
    garbage[16:24] = 7                                       # R of the header: no longer the layout the size was made for
    assert bwd(garbage, garbage.numel()) == -1
    assert bwd(saved, saved.numel() - 1) == -4
    assert bwd(saved, 256) == -4
    assert bwd(saved, saved.numel()) == 0
    (want,) = torch.autograd.grad(out["fine_comp_rgbs"], [leaves[1][0]], gf)
    assert torch.equal(grads[1][0], want)


def test_no_dir_modules_go_through_the_function(golden_dir, tr):
    """--no_dir: a (128, 256) dir_encoding weight is padded with 27 zero columns inside forward_rays_train (as Trainer holds
    it); outputs and gradients are the padded network's, the narrow weight gets the gradient of its 256 columns."""
    from nerf_sr_amd.weights import pad_no_dir, DIR_W
    g = _load(golden_dir, "llff_rand")
    rays = torch.from_numpy(g["rays"]).cuda()
    sd = [make_state_dict(99), make_state_dict(100)]
    narrow = [{k: torch.from_numpy(np.ascontiguousarray(v[:, :256] if k == DIR_W else v)).cuda().requires_grad_(True)
               for k, v in s.items()} for s in sd]
    wide = [{k: (pad_no_dir(v.detach()) if k == DIR_W else v.detach()).clone().requires_grad_(True) for k, v in n.items()}
            for n in narrow]
    res = []
    for p in (narrow, wide):
        out = tr.forward_rays_train(p[0], p[1], rays, _draws(g), noise_std=float(g["noise_std"]))
        loss = out["fine_comp_rgbs"].square().sum() + out["coarse_depth"].sum()
        res.append((out, torch.autograd.grad(loss, [p[n][k] for n in range(2) for k in STATE_DICT_SPEC])))
    for k in tr.OUT_KEYS:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    for i, (a, b) in enumerate(zip(res[0][1], res[1][1])):
        k = list(STATE_DICT_SPEC)[i % 24]
        assert torch.equal(a, b[:, :256] if k == DIR_W else b), k


def test_regularize_patch_and_clipping_steps(golden_dir, tr):
    """Trainer.regularize_patch (TV loss of a rendered HR patch + its own Adam step) against the same iteration in fp64 on the
    oracle, and a clipped optimize_parameters: clip_grad_norm_ scales the gradient to the bound; with grad_clip_val = 0 the
    step is exactly the unclipped one."""
    g = _load(golden_dir, "llff_rand")
    from nerf_sr_amd import ops, cameras
    patch = ops.subpixel_rays(cameras.spiral_pose(0.5), (64, 48), cameras.llff_focal(64), 2, True)
    patch = patch.reshape(24, 32, 2, 2, 8)[4:8, 4:8].permute(0, 2, 1, 3, 4).reshape(-1, 8).contiguous()   # 8 x 8 HR raster
    gen = torch.Generator().manual_seed(2)
    draws = {"u_coarse": torch.rand(64, 64, generator=gen), "noise_coarse": torch.randn(64, 64, generator=gen),
             "u_fine": torch.rand(64, 64, generator=gen), "noise_fine": torch.randn(64, 128, generator=gen)}
    t, sd_c, sd_f = _trainer(tr, g, precision="f16x3")
    w0 = {k: v.clone() for k, v in t.params[0].items()}
    tv = t.regularize_patch(patch, 4, 0.7, draws={k: v.cuda() for k, v in draws.items()}).cpu()
    refs = _oracle_grads(sd_c, sd_f, patch.cpu(), {**draws, "noise_std": float(g["noise_std"])}, False,
                         lambda o: 0.7 * (tr.tv_loss(o["coarse_comp_rgbs"].view(8, 8, 3)) + tr.tv_loss(o["fine_comp_rgbs"].view(8, 8, 3))))
    _assert_grads(t.grads, refs, "patch")
    assert float(tv.sum()) > 0 and t.step == 1
    assert any(not torch.equal(t.params[0][k], w0[k]) for k in STATE_DICT_SPEC)
    # clipping: the same fused step with and without a bound far below the gradient's norm
    runs = {}
    for clip in (0.0, 1e-3):
        t, _, _ = _trainer(tr, g, precision="f16x3", grad_clip_val=clip)
        t.loss_and_grads(_draws(g))
        pre = torch.linalg.vector_norm(torch.cat([t.flat_grads[0], t.flat_grads[1]]))
        t2, _, _ = _trainer(tr, g, precision="f16x3", grad_clip_val=clip)
        t2.optimize_parameters(_draws(g))
        runs[clip] = (pre, t2)
    pre, tc = runs[1e-3]
    post = torch.linalg.vector_norm(torch.cat([tc.flat_grads[0], tc.flat_grads[1]]))
    assert float(pre) > 1e-2 and abs(float(post) / 1e-3 - 1.0) < 1e-4
    t_ref, _, _ = _trainer(tr, g, precision="f16x3")
    t_ref.optimize_parameters(_draws(g))
    for n in range(2):
        for k in STATE_DICT_SPEC:
            assert torch.equal(runs[0.0][1].params[n][k], t_ref.params[n][k])


def _assert_update_like_reference(t, g, w0):
    """The weights after the step against the reference's (test_gpu_train.py::test_adam_step_vs_reference's rule: compare the
    UPDATE; a relu flip may turn a zero gradient into a tiny one -- update 0 vs lr -- on a few entries)."""
    from tests.util import sample_idx
    for n, name in enumerate(("coarse", "fine")):
        for k in STATE_DICT_SPEC:
            got = t.params[n][k].cpu().numpy().reshape(-1)
            idx = sample_idx(got.size)
            before = w0[n][k].cpu().numpy().reshape(-1)[idx]
            assert np.array_equal(before, g[f"w0_{name}.{k}"])
            bad = np.abs((got[idx] - before) - (g[f"w1_{name}.{k}"] - before)) > 2e-5
            assert bad.mean() <= 0.02, (name, k, float(bad.mean()))


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_regularize_patch_vs_reference(golden_dir, tr, prec):
    """Trainer.regularize_patch on the reference's own regularize_patch iteration (tests/golden/train_patch_tv.npz): both TV
    losses, every gradient tensor against the fp64 oracle and the reference's digests, the weights after its Adam step."""
    g = np.load(os.path.join(golden_dir, "train_patch_tv.npz"))
    sd_c, sd_f = make_state_dict(int(g["seed_coarse"])), make_state_dict(int(g["seed_fine"]))
    t = tr.Trainer(sd_c, sd_f, downscale=2, randomized=True, noise_std=float(g["noise_std"]), lr=float(g["lr"]),
                   beta1=float(g["beta1"]), precision=prec)
    w0 = [{k: v.clone() for k, v in p.items()} for p in t.params]
    draws = _draws(g)
    tv = t.regularize_patch(torch.from_numpy(g["rays"]).cuda(), int(g["patch_len"]), float(g["reg_lambda_tv"]), draws=draws).cpu()
    assert abs(float(tv[0]) - float(g["loss_coarse_tv"])) < 1e-6 and abs(float(tv[1]) - float(g["loss_fine_tv"])) < 1e-6, tv
    side = int(g["patch_len"]) * 2
    lam = float(g["reg_lambda_tv"])
    refs = _oracle_grads(sd_c, sd_f, g["rays"], train_draws(g), False,
                         lambda o: lam * (tr.tv_loss(o["coarse_comp_rgbs"].view(side, side, 3)) + tr.tv_loss(o["fine_comp_rgbs"].view(side, side, 3))))
    _assert_grads(t.grads, refs, ("patch_tv", prec))
    for n, name in enumerate(("coarse", "fine")):
        for k in STATE_DICT_SPEC:
            ref_norm = float(g[f"gnorm_{name}.{k}"])
            assert abs(float(t.grads[n][k].double().norm()) - ref_norm) <= 2e-3 * ref_norm + 1e-9, (name, k)
    _assert_update_like_reference(t, g, w0)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_clipped_step_vs_reference(golden_dir, tr, prec):
    """optimize_parameters with --grad_clip_val on the reference's own clipped iteration (tests/golden/train_llff_clip.npz):
    the pre-clip total norm, the clipped gradients and the weights after the step."""
    g = np.load(os.path.join(golden_dir, "train_llff_clip.npz"))
    clip = float(g["grad_clip_val"])
    t, sd_c, sd_f = _trainer(tr, g, precision=prec, grad_clip_val=clip)
    w0 = [{k: v.clone() for k, v in p.items()} for p in t.params]
    t.loss_and_grads(_draws(g))
    pre = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(v) for p in t.grads for v in p.values()])))
    assert abs(pre - float(g["pre_clip_norm"])) <= 2e-3 * float(g["pre_clip_norm"]), (pre, float(g["pre_clip_norm"]))
    _, gc, gf = to.loss_and_grads(sd_c, sd_f, g["rays"], g["target_lr"], 4, 64, 64, False, float(g["lambda_coarse"]),
                                  float(g["lambda_fine"]), dtype=torch.float64, **train_draws(g))
    _assert_grads(t.grads, (gc, gf), ("clip, before", prec))
    total = t.clip_grads()
    assert abs(float(total) - pre) <= 1e-6 * pre
    coef = clip / (float(g["pre_clip_norm"]) + 1e-6)
    _assert_grads(t.grads, ({k: v * coef for k, v in gc.items()}, {k: v * coef for k, v in gf.items()}), ("clip, after", prec))
    for n, name in enumerate(("coarse", "fine")):
        for k in STATE_DICT_SPEC:
            ref_norm = float(g[f"gnorm_{name}.{k}"])       # the reference's CLIPPED gradients
            assert abs(float(t.grads[n][k].double().norm()) - ref_norm) <= 2e-3 * ref_norm + 1e-9, (name, k)
    t.optimizer_step()
    _assert_update_like_reference(t, g, w0)
    # the same through optimize_parameters (clipping between the all-reduce and the Adam step)
    t2, _, _ = _trainer(tr, g, precision=prec, grad_clip_val=clip)
    t2.optimize_parameters(_draws(g))
    for n in range(2):
        for k in STATE_DICT_SPEC:
            assert torch.equal(t2.params[n][k], t.params[n][k]), (n, k)


def test_integration_stub_runs_verbatim(golden_dir, tr):
    """INTEGRATION.md §4's autograd stub for the reference's NeRFDownXModel.forward_rays, executed as written against modules
    of nn.Parameters; the reference's own calculate_losses / backward / torch.optim.Adam then run unchanged."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    m = re.search(r"```python\n(# nsr-autograd-stub\n.*?)```", text, re.S)
    assert m, "stub block missing"
    ns = {}
    exec(compile(m.group(1), "INTEGRATION.md#autograd-stub", "exec"), ns)
    g = _load(golden_dir, "llff_rand")
    from types import SimpleNamespace
    opt = SimpleNamespace(N_coarse=64, N_importance=64, white_bkgd=False, lindisp=False, noise_std=float(g["noise_std"]),
                          gamma_correct=False, sigma_activation="relu", color_activation="sigmoid", stop_grad=False,
                          downscale=2)
    model = SimpleNamespace(opt=opt, randomized=False, netCoarse=_Net(make_state_dict(99)), netFine=_Net(make_state_dict(100)))
    rays = torch.from_numpy(g["rays"]).cuda()
    out = ns["forward_rays"](model, rays)
    tgt = torch.from_numpy(g["target_lr"]).cuda()
    loss = _reference_loss(out, tgt, 4, 1.0, 1.0)
    params = list(model.netCoarse.parameters()) + list(model.netFine.parameters())
    adam = torch.optim.Adam(params, lr=5e-4)
    adam.zero_grad()
    loss.backward()
    _, gc, gf = to.loss_and_grads(make_state_dict(99), make_state_dict(100), g["rays"], g["target_lr"], 4, 64, 64, False,
                                  dtype=torch.float64)
    got = [{k: p.grad for k, p in zip(STATE_DICT_SPEC, net.parameters())} for net in (model.netCoarse, model.netFine)]
    _assert_grads(got, (gc, gf), "stub")
    before = [p.detach().clone() for p in params]
    adam.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, params) if bool(p.grad.any()))
