"""Training NON-DEFAULT architectures (--D --W --skips --deg_pos --deg_dir --no_dir) on the GPU: the layer-by-layer pair
nsr_train_arch_forward / nsr_train_arch_backward and nsr_adam_step_n (include/nsr_train.h) behind
``train.forward_rays_train(..., arch=)`` and ``train.Trainer(..., arch=)``, against the reference's own iteration
(tests/golden/train_arch.npz, made by its optimize_parameters) and the fp64 restatement of it (tests/arch_util.py).

Tolerances are those of tests/test_gpu_train.py, for the reasons given there (a ReLU mask within rounding of zero flips
between two correct fp32 implementations): losses 1e-6, coarse outputs 2e-6, fine outputs 1e-4 (the resampler's
conditioning), every gradient tensor within 2e-3 of its norm of the fp64 restatement, 5e-4 on the layers above the trunk,
the whole gradient 2e-3, norms within 2e-3 of the reference's digests.  No ray and no tensor is excluded anywhere."""
import ctypes
import os
import time

import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import arch_spec, make_state_dict, make_state_dict_arch, STATE_DICT_SPEC
from oracle import train_oracle as to
from tests import arch_util as au
from tests.util import sample_idx, train_draws

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "f16x3_gemm")


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import train as _tr   # raises if libnsr.so is missing: no fallback
    t0 = time.time()
    yield _tr
    print(f"\ntests/test_gpu_train_arch.py: {time.time() - t0:.1f} s wall")


def _trainer(tr, g, **kw):
    sd_c, sd_f = au.state_dicts(g)
    t = tr.Trainer(sd_c, sd_f, white_bkgd=bool(g["white_bkgd"]), downscale=int(round(int(g["s2"]) ** 0.5)),
                   randomized=bool(g["randomized"]), noise_std=float(g["noise_std"]), lr=float(g["lr"]), beta1=float(g["beta1"]),
                   lambda_coarse_mse=float(g["lambda_coarse"]), lambda_fine_mse=float(g["lambda_fine"]), arch=g["arch"], **kw)
    t.set_input(torch.from_numpy(g["rays"]).cuda(), torch.from_numpy(g["target_lr"]).cuda())
    return t


_ORACLE64 = {}


def _oracle(golden_dir, tag, **flags):
    key = (tag, tuple(sorted(flags.items())))
    if key not in _ORACLE64:
        g = au.load_case(golden_dir, tag)
        _ORACLE64[key] = au.loss_and_grads(*au.state_dicts(g), g, **flags)
    return _ORACLE64[key]


@pytest.fixture(scope="module", params=[(c, p) for c in au.CASES for p in PRECISIONS], ids=lambda cp: f"{cp[0]}-{cp[1]}")
def case(request, golden_dir, tr):
    tag, prec = request.param
    g = au.load_case(golden_dir, tag)
    t = _trainer(tr, g, precision=prec)
    t.loss_and_grads(au.draws_of(g))
    res64, gc64, gf64 = _oracle(golden_dir, tag)
    return g, t, res64, (gc64, gf64), f"{tag}-{prec}"


def test_forward_and_losses_vs_reference(case):
    g, t, res64, _, what = case
    losses = t.losses.cpu().numpy()
    dev = lambda k, ref: float(np.abs(t.out[k].cpu().numpy() - ref).max())
    print(what, "losses", losses, float(g["loss_coarse_mse"]), float(g["loss_fine_mse"]),
          "lr_c", dev("lr_coarse", g["lr_coarse"]), "hr_c", dev("coarse_comp_rgbs", g["hr_coarse"]),
          "lr_f", dev("lr_fine", g["lr_fine"]), "hr_f", dev("fine_comp_rgbs", g["hr_fine"]))
    assert abs(losses[0] - float(g["loss_coarse_mse"])) < 1e-6
    assert abs(losses[1] - float(g["loss_fine_mse"])) < 1e-6
    assert abs(losses[0] - res64["loss_coarse_mse"]) < 1e-6
    np.testing.assert_allclose(t.out["lr_coarse"].cpu().numpy(), g["lr_coarse"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(t.out["coarse_comp_rgbs"].cpu().numpy(), g["hr_coarse"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(t.out["lr_fine"].cpu().numpy(), g["lr_fine"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(t.out["fine_comp_rgbs"].cpu().numpy(), g["hr_fine"], rtol=0, atol=1e-4)
    assert float(t.var_losses.abs().max()) == 0.0 and t.status() == 0


def test_gradients_vs_oracle_and_reference(case):
    g, t, _, refs, what = case
    spec = arch_spec(**g["arch"])
    for n, name in enumerate(("coarse", "fine")):
        assert list(t.grads[n]) == list(spec)
        au.assert_grads_close(t.grads[n], refs[n], spec, f"{what} {name}")
        for k in spec:
            got = t.grads[n][k].cpu().double()
            ref_norm = float(g[f"gnorm_{name}.{k}"])
            assert abs(float(got.norm()) - ref_norm) <= 2e-3 * ref_norm + 1e-9, (name, k)
            sub = got.reshape(-1).numpy()[sample_idx(got.numel())]
            want_sub = g[f"grad_{name}.{k}"].astype(np.float64)
            assert np.linalg.norm(sub - want_sub) <= 4e-3 * np.linalg.norm(want_sub) + 1e-9, (name, k)


def test_adam_step_vs_reference(case, tr):
    g, t, _, _, _ = case
    spec = arch_spec(**g["arch"])
    w0 = {k: v.clone() for k, v in t.params[0].items()}
    t.optimizer_step()
    for k in spec:
        got = t.params[0][k].cpu().numpy().reshape(-1)
        idx = sample_idx(got.size)
        # the first Adam step moves every weight by ~lr * sign(g): compare the UPDATE (tests/test_gpu_train.py)
        upd = got[idx] - w0[k].cpu().numpy().reshape(-1)[idx]
        upd_ref = g[f"w1_coarse.{k}"] - w0[k].cpu().numpy().reshape(-1)[idx]
        bad = np.abs(upd - upd_ref) > 2e-5
        assert bad.mean() <= 0.02, (k, float(bad.mean()))
    # the optimiser kernel itself, on random state, against the oracle's restatement of torch.optim.Adam
    gen = torch.Generator().manual_seed(5)
    p = {k: torch.randn(*s, generator=gen) for k, s in spec.items()}
    gr = {k: torch.randn(*s, generator=gen) * 1e-2 for k, s in spec.items()}
    m = {k: torch.randn(*s, generator=gen) * 1e-3 for k, s in spec.items()}
    v = {k: torch.rand(*s, generator=gen) * 1e-5 for k, s in spec.items()}
    t2 = tr.Trainer(p, p, arch=g["arch"], precision="fp32")
    for k in spec:
        t2.grads[0][k].copy_(gr[k]); t2.exp_avg[0][k].copy_(m[k]); t2.exp_avg_sq[0][k].copy_(v[k])
    t2.step = 6
    t2.optimizer_step()
    pc = {k: x.clone() for k, x in p.items()}
    to.adam_step(pc, gr, {k: x.clone() for k, x in m.items()}, {k: x.clone() for k, x in v.items()}, step=7)
    for k in spec:
        assert float((t2.params[0][k].cpu() - pc[k]).abs().max()) <= 2.4e-7, k      # within one ulp of O(1) weights


def _aux_loss(g):
    """A loss over every output but the colours alone: depth, opacity and weights of both passes (+ the colours, so that
    the colour head is reached), with fixed coefficients -- the same function for the GPU tensors and the fp64 oracle."""
    gen = torch.Generator().manual_seed(17)
    R = g["rays"].shape[0]
    co = {"coarse_depth": torch.rand(R, generator=gen, dtype=torch.float64), "coarse_opacity": torch.rand(R, generator=gen, dtype=torch.float64),
          "coarse_weights": torch.rand(R, 64, generator=gen, dtype=torch.float64), "fine_depth": torch.rand(R, generator=gen, dtype=torch.float64),
          "fine_opacity": torch.rand(R, generator=gen, dtype=torch.float64), "fine_weights": torch.rand(R, 128, generator=gen, dtype=torch.float64),
          "coarse_comp_rgbs": torch.rand(R, 3, generator=gen, dtype=torch.float64), "fine_comp_rgbs": torch.rand(R, 3, generator=gen, dtype=torch.float64)}

    def f(out):
        ref = out["fine_depth"]
        return sum((out[k] * c.to(device=ref.device, dtype=ref.dtype)).sum() for k, c in co.items()) / R
    return f


@pytest.mark.parametrize("prec", PRECISIONS)
def test_loss_over_depth_opacity_weights(golden_dir, tr, prec):
    g = au.load_case(golden_dir, "odd")
    f = _aux_loss(g)
    t = _trainer(tr, g, precision=prec)
    out = t.forward(au.draws_of(g))
    t.backward(f(out))
    key = ("odd", "aux")
    if key not in _ORACLE64:
        _ORACLE64[key] = au.loss_and_grads(*au.state_dicts(g), g, loss_fn=f)
    res64, gc64, gf64 = _ORACLE64[key]
    spec = arch_spec(**g["arch"])
    for n, (name, ref) in enumerate((("coarse", gc64), ("fine", gf64))):
        au.assert_grads_close(t.grads[n], ref, spec, f"aux odd-{prec} {name}")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_default_architecture_matches_the_default_pair(golden_dir, tr, prec):
    """The default network through the descriptor route against nsr_train_forward / nsr_train_backward: one implementation
    behind two families of entry points, so all eight outputs and all 48 gradient tensors are equal bit for bit."""
    g = np.load(os.path.join(golden_dir, "train_llff_rand.npz"))
    rays = torch.from_numpy(g["rays"]).cuda()
    draws = {k: v for k, v in train_draws(g).items() if k != "noise_std"}
    sds = [make_state_dict(int(g["seed_coarse"])), make_state_dict(int(g["seed_fine"]))]
    res = []
    for arch in (None, au.DEFAULT_ARCH):
        p = [{k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in sd.items()} for sd in sds]
        out = tr.forward_rays_train(p[0], p[1], rays, draws, noise_std=float(g["noise_std"]), precision=prec, arch=arch)
        loss = out["fine_comp_rgbs"].square().sum() + out["coarse_comp_rgbs"].square().sum() + out["coarse_depth"].sum()
        res.append((out, torch.autograd.grad(loss, [p[n][k] for n in range(2) for k in STATE_DICT_SPEC])))
    assert len(res[0][1]) == len(res[1][1]) == 48
    for k in tr.OUT_KEYS:
        assert torch.equal(res[0][0][k].detach(), res[1][0][k].detach()), k
    for i, (a, b) in enumerate(zip(res[0][1], res[1][1])):
        assert float(a.abs().max()) > 0.0 and torch.equal(a, b), (i // 24, list(STATE_DICT_SPEC)[i % 24])


def test_saved_state_does_not_cross_entry_point_families(golden_dir, tr):
    """One saved-state format serves nsr_train_* and nsr_train_arch_*; the descriptor it records keeps a buffer of one
    family's forward out of the other family's backward when the networks differ: NSR_ERR_INVALID_ARG both ways, the
    gradient buffers untouched."""
    from ctypes import c_void_p
    from nerf_sr_amd import _lib
    g = au.load_case(golden_dir, "small")
    lib = _lib.load()
    rays = torch.from_numpy(g["rays"]).cuda()
    draws = au.draws_of(g)
    small = _lib.NsrArch.from_arch(tr.normalize_arch(g["arch"]))
    w_small = [[torch.from_numpy(v).cuda() for v in sd.values()] for sd in au.state_dicts(g)]
    w_def = [[torch.from_numpy(v).cuda() for v in make_state_dict(s).values()] for s in (3, 4)]
    g_fine = torch.ones(rays.shape[0], 3, device="cuda")
    g8 = (c_void_p * 8)(*[c_void_p(0)] * 4, c_void_p(g_fine.data_ptr()), *[c_void_p(0)] * 3)

    def untouched_after(call, weights):
        grads = [[torch.full_like(p, 7.0) for p in n] for n in weights]
        rc = call(tr._ptr_array(weights[0]), tr._ptr_array(weights[1]), tr._ptr_array(grads[0]), tr._ptr_array(grads[1]))
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for n in grads for t in n)
        return rc

    # nsr_train_forward (default network, fp32) -> nsr_train_arch_backward with the `small` descriptor
    out = tr.forward_rays_train(*[[p.clone().requires_grad_(True) for p in n] for n in w_def], rays, draws, precision="fp32")
    saved, ws = out["fine_comp_rgbs"].grad_fn.state, tr._DEFAULT_WS[rays.device].buf
    assert untouched_after(lambda wc, wf, gc, gf: lib.nsr_train_arch_backward(
        ctypes.byref(small), wc, wf, g8, gc, gf, c_void_p(ws.data_ptr()), ws.numel(), c_void_p(saved.data_ptr()), saved.numel(),
        tr._stream()), w_small) == -1
    # nsr_train_arch_forward (`small`, fp32) -> nsr_train_backward
    out = tr.forward_rays_train(*[[p.clone().requires_grad_(True) for p in n] for n in w_small], rays, draws, precision="fp32",
                                arch=g["arch"])
    saved, ws = out["fine_comp_rgbs"].grad_fn.state, tr._DEFAULT_WS[rays.device].buf
    assert untouched_after(lambda wc, wf, gc, gf: lib.nsr_train_backward(
        wc, wf, g8, gc, gf, c_void_p(ws.data_ptr()), ws.numel(), c_void_p(saved.data_ptr()), saved.numel(), tr._stream()),
        w_def) == -1


def _run(tr, g, chunk, prec="f16x3_gemm"):
    t = _trainer(tr, g, ray_chunk=chunk, precision=prec)
    t.loss_and_grads(au.draws_of(g))
    return t.losses.clone(), [{k: v.clone() for k, v in t.grads[n].items()} for n in range(2)], t.out["fine_comp_rgbs"].clone()


def test_ray_chunk_invariance(golden_dir, tr):
    """Losses and gradients do not depend on the ray chunking beyond fp32 summation order; 40-ray chunks leave a ragged
    last one (96 rays = 40 + 40 + 16)."""
    g = au.load_case(golden_dir, "small")
    spec = arch_spec(**g["arch"])
    whole = _run(tr, g, 4096)
    for chunk in (32, 40):
        part = _run(tr, g, chunk)
        assert torch.equal(whole[2], part[2]), chunk
        assert float((whole[0] - part[0]).abs().max()) < 1e-6, chunk
        for n in range(2):
            for k in spec:
                a, b = whole[1][n][k].double(), part[1][n][k].double()
                assert float((a - b).norm()) <= 1e-5 * float(a.norm()) + 1e-12, (chunk, n, k)


@pytest.mark.parametrize("tag", ("small", "odd"))
def test_run_to_run_identity(golden_dir, tr, tag):
    g = au.load_case(golden_dir, tag)
    a, b = _run(tr, g, 4096), _run(tr, g, 4096)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for n in range(2):
        for k in a[1][n]:
            assert torch.equal(a[1][n][k], b[1][n][k]), (n, k)
    a, b = _run(tr, g, 40, "fp32"), _run(tr, g, 40, "fp32")          # accumulating chunks too
    for n in range(2):
        for k in a[1][n]:
            assert torch.equal(a[1][n][k], b[1][n][k]), (n, k)


FLAGS = {"gamma": dict(gamma_correct=True), "softplus": dict(sigma_activation="softplus"),
         "colornone": dict(color_activation="none"), "stopgrad": dict(stop_grad=True)}


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("flag", list(FLAGS))
def test_flags_vs_oracle(golden_dir, tr, flag, prec):
    g = au.load_case(golden_dir, "odd")
    kw = FLAGS[flag]
    t = _trainer(tr, g, precision=prec, **kw)
    t.loss_and_grads(au.draws_of(g))
    res64, gc64, gf64 = _oracle(golden_dir, "odd", **kw)
    losses = t.losses.cpu().numpy()
    print(flag, prec, "losses", losses, res64["loss_coarse_mse"], res64["loss_fine_mse"])
    assert abs(losses[0] - res64["loss_coarse_mse"]) < 1e-6
    np.testing.assert_allclose(t.out["coarse_comp_rgbs"].cpu().numpy(), res64["coarse_comp_rgbs"].numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(t.out["fine_comp_rgbs"].cpu().numpy(), res64["fine_comp_rgbs"].numpy(), rtol=0, atol=1e-4)
    spec = arch_spec(**g["arch"])
    for n, (name, ref) in enumerate((("coarse", gc64), ("fine", gf64))):
        au.assert_grads_close(t.grads[n], ref, spec, f"{flag} odd-{prec} {name}")
    if flag == "stopgrad":
        for n in range(2):
            assert float(t.grads[n]["xyz_encoding_final.weight"].abs().max()) == 0.0
            assert float(t.grads[n]["xyz_encoding_final.bias"].abs().max()) == 0.0


def test_round_trip_train_then_render(golden_dir, tr):
    """Train `odd` for 200 steps against a teacher of the same architecture rendered on the same rays: the loss falls, the
    trained state_dicts load into GenericMLP / NeRFDownXModel, and its eval render equals the deterministic train-mode
    forward of the trainer."""
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    from nerf_sr_amd import ops
    g = au.load_case(golden_dir, "odd")
    arch = g["arch"]
    rays = torch.from_numpy(g["rays"]).cuda()
    # the fixture's own weights are the teacher: its coarse field is empty on these rays (zero opacity, zero gradient), so a
    # student made from them would never train its coarse network; the student's seeds give both networks density here
    teacher = [{k: torch.from_numpy(v).cuda() for k, v in sd.items()} for sd in au.state_dicts(g)]
    with torch.no_grad():
        hr = tr.forward_rays_train(teacher[0], teacher[1], rays, None, white_bkgd=True, precision="fp32", arch=arch)["fine_comp_rgbs"]
    target = hr.view(-1, int(g["s2"]), 3).mean(1)
    t = tr.Trainer(make_state_dict_arch(41, **arch), make_state_dict_arch(42, **arch), white_bkgd=True, downscale=2, randomized=True, noise_std=0.0, lr=5e-4, arch=arch,
                   precision="f16x3_gemm")
    t.set_input(rays, target)
    hist = []
    for i in range(200):
        torch.manual_seed(1000 + i)
        hist.append(float(t.optimize_parameters().sum()))
    print("round trip: loss", hist[0], "->", hist[-1])
    assert all(np.isfinite(hist)) and hist[-1] < 0.9 * hist[0], (hist[0], hist[-1])
    assert t.step == 200 and t.status() == 0
    sds = t.state_dicts()
    m = NeRFDownXModel(default_options(white_bkgd=True, precision="fp32", **{**arch, "skips": list(arch["skips"])}))
    m.load_networks(sds[0], sds[1]).eval()
    assert isinstance(m.netCoarse, ops.GenericMLP)
    ev = m.forward_rays(rays)
    t2 = tr.Trainer(sds[0], sds[1], white_bkgd=True, downscale=2, randomized=False, arch=arch, precision="fp32")
    t2.set_input(rays, target)
    with torch.no_grad():
        det = t2.forward()
    for k in tr.OUT_KEYS:
        d = float((ev[k] - det[k]).abs().max())
        print("round trip eval vs train-mode", k, d)
        assert d <= 2e-6, (k, d)


def test_misuse_is_rejected(golden_dir, tr):
    """A damaged header, a backward with another descriptor, a short buffer, and a backward after the weights changed."""
    from ctypes import c_void_p
    from nerf_sr_amd import _lib
    g = au.load_case(golden_dir, "small")
    t = _trainer(tr, g, precision="fp32")
    out = t.forward(au.draws_of(g))
    node = out["fine_comp_rgbs"].grad_fn
    saved, ws = node.state, t._ws
    lib = _lib.load()
    leaves = t._weight_leaves()
    grads = [[torch.empty_like(p) for p in n] for n in leaves]
    gf = torch.ones_like(out["fine_comp_rgbs"])
    g8 = (c_void_p * 8)(*[c_void_p(0)] * 4, c_void_p(gf.data_ptr()), *[c_void_p(0)] * 3)
    mine = _lib.NsrArch.from_arch(tr.normalize_arch(g["arch"]))

    def bwd(buf, nbytes, arch=mine):
        rc = lib.nsr_train_arch_backward(ctypes.byref(arch), tr._ptr_array(leaves[0]), tr._ptr_array(leaves[1]), g8,
                                         tr._ptr_array(grads[0]), tr._ptr_array(grads[1]), c_void_p(ws.data_ptr()), ws.numel(),
                                         c_void_p(buf.data_ptr()), nbytes, tr._stream())
        torch.cuda.synchronize()
        return rc
    zeros = torch.zeros_like(saved)
    assert bwd(zeros, zeros.numel()) == -1                     # a buffer no forward wrote
    garbage = saved.clone()
    garbage[16:24] = 7                                         # R of the header
    assert bwd(garbage, garbage.numel()) == -1
    garbage = saved.clone()
    garbage[48:52] = 9                                         # D of the recorded descriptor
    assert bwd(garbage, garbage.numel()) == -1
    same_shapes = _lib.NsrArch.from_arch(tr.normalize_arch(dict(g["arch"], deg_dir=g["arch"]["deg_dir"] + 1)))
    assert bwd(saved, saved.numel(), same_shapes) == -1        # another descriptor with as many tensors
    assert bwd(saved, saved.numel() - 1) == -4
    assert bwd(saved, 256) == -4
    # the default pair does not take this buffer either
    d24 = (c_void_p * 24)(*[c_void_p(ws.data_ptr())] * 24)
    assert lib.nsr_train_backward(d24, d24, g8, d24, d24, c_void_p(ws.data_ptr()), ws.numel(), c_void_p(saved.data_ptr()),
                                  saved.numel(), tr._stream()) == -1
    assert bwd(saved, saved.numel()) == 0
    (want,) = torch.autograd.grad(out["fine_comp_rgbs"], [leaves[1][0]], gf)
    assert torch.equal(grads[1][0], want)
    # the weights changed between a forward and its backward
    loss = t.forward(au.draws_of(g))["fine_comp_rgbs"].sum()
    t.optimizer_step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        t.backward(loss)


def test_reference_style_modules_and_no_dir(golden_dir, tr):
    """The nn.Module form: a module whose parameters() are the 2 D + 8 tensors in state_dict order (as the reference's
    VanillaMLP built with the same flags yields them) goes through the function and gets its gradients; --no_dir natively."""
    g = au.load_case(golden_dir, "nodir")
    arch = g["arch"]

    class Net(torch.nn.Module):
        def __init__(self, sd):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v).cuda()) for v in sd.values()])
    nets = [Net(sd) for sd in au.state_dicts(g)]
    out = tr.forward_rays_train(nets[0], nets[1], torch.from_numpy(g["rays"]).cuda(), {k: torch.from_numpy(v).cuda() for k, v in au.draws_of(g).items()},
                                white_bkgd=True, noise_std=float(g["noise_std"]), precision="fp32", arch=arch)
    tgt = torch.from_numpy(g["target_lr"]).cuda()
    mse = torch.nn.functional.mse_loss
    loss = mse(out["coarse_comp_rgbs"].view(-1, 4, 3).mean(1), tgt) + mse(out["fine_comp_rgbs"].view(-1, 4, 3).mean(1), tgt)
    loss.backward()
    _, gc64, gf64 = _oracle(golden_dir, "nodir")
    spec = arch_spec(**arch)
    assert tuple(spec["dir_encoding.0.weight"]) == (64, 128)
    for net, ref, name in ((nets[0], gc64, "coarse"), (nets[1], gf64, "fine")):
        got = {k: p.grad for k, p in zip(spec, net.parameters())}
        au.assert_grads_close(got, ref, spec, f"module nodir {name}")


# Encoding degrees whose padded widths differ from the fixtures' (deg_pos 6 and 10 both pad to Kx = 64, deg_dir 2 and 4 to
# Dp = 32, where a wrong degree only fills padding columns that meet zero weights), and a width that is not a multiple of 32
# (every layer padded).  No reference fixture: the fp64 restatement on the `small` case's rays, draws and targets.
RUNTIME_ARCHS = {"deg12_6": {"D": 3, "W": 64, "skips": (1,), "deg_pos": 12, "deg_dir": 6, "no_dir": False},
                 "w100_deg11_5": {"D": 3, "W": 100, "skips": (2,), "deg_pos": 11, "deg_dir": 5, "no_dir": False},
                 "noskip_deg3_0": {"D": 2, "W": 32, "skips": (), "deg_pos": 3, "deg_dir": 0, "no_dir": False}}


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(RUNTIME_ARCHS))
def test_runtime_degrees_and_padded_widths_vs_oracle(golden_dir, tr, name, prec):
    g = dict(au.load_case(golden_dir, "small"))
    # weights: seeds with which the loss reaches both networks on these rays (53 / 54 for the two-layer network, whose fine
    # field is empty under 51 / 52: checked below)
    g["arch"] = RUNTIME_ARCHS[name]
    g["seed_coarse"], g["seed_fine"] = (53, 54) if name == "noskip_deg3_0" else (51, 52)
    key = ("runtime", name)
    if key not in _ORACLE64:
        _ORACLE64[key] = au.loss_and_grads(*au.state_dicts(g), g)
    res64, gc64, gf64 = _ORACLE64[key]
    t = _trainer(tr, g, precision=prec)
    t.loss_and_grads(au.draws_of(g))
    losses = t.losses.cpu().numpy()
    print(name, prec, "losses", losses, res64["loss_coarse_mse"], res64["loss_fine_mse"])
    assert abs(losses[0] - res64["loss_coarse_mse"]) < 1e-6
    np.testing.assert_allclose(t.out["coarse_comp_rgbs"].cpu().numpy(), res64["coarse_comp_rgbs"].numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(t.out["fine_comp_rgbs"].cpu().numpy(), res64["fine_comp_rgbs"].numpy(), rtol=0, atol=1e-4)
    spec = arch_spec(**g["arch"])
    for n, (net, ref) in enumerate((("coarse", gc64), ("fine", gf64))):
        assert float(sum(v.norm() ** 2 for v in ref.values())) > 0.0, net       # the case must reach both networks
        au.assert_grads_close(t.grads[n], ref, spec, f"{name}-{prec} {net}")


LAMBDA_VAR = (0.05, 0.08, 0.3, 0.2)      # the weights of train_blender_var.npz: the terms matter next to the MSEs


@pytest.mark.parametrize("prec", PRECISIONS)
def test_variance_losses_vs_oracle(golden_dir, tr, prec):
    """--use_var_loss / --use_depth_var_loss with an architecture: the terms are written in torch over the pair's outputs."""
    g = au.load_case(golden_dir, "odd_dense")
    n_lr, s2 = g["target_lr"].shape[0], int(g["s2"])

    def loss_fn(out):
        tgt = torch.as_tensor(g["target_lr"]).to(out["fine_depth"].dtype)
        total, lc, lf = au.mse_loss_of(tgt, s2)(out)
        far = float(g["rays"][0, 7])
        var_of = lambda x: torch.sum(torch.var(torch.reshape(x, (n_lr, s2, -1)), dim=1))
        terms = [var_of(out["coarse_comp_rgbs"]), var_of(out["fine_comp_rgbs"]), var_of(out["coarse_depth"] / far), var_of(out["fine_depth"] / far)]
        loss_fn.terms = [float(l * x.detach()) for l, x in zip(LAMBDA_VAR, terms)]
        return total + sum(l * x for l, x in zip(LAMBDA_VAR, terms)), lc, lf
    key = ("odd_dense", "var")
    if key not in _ORACLE64:
        _ORACLE64[key] = au.loss_and_grads(*au.state_dicts(g), g, loss_fn=loss_fn) + (loss_fn.terms,)
    res64, gc64, gf64, terms64 = _ORACLE64[key]
    t = _trainer(tr, g, precision=prec, use_var_loss=True, lambda_coarse_var=LAMBDA_VAR[0], lambda_fine_var=LAMBDA_VAR[1],
                 use_depth_var_loss=True, lambda_coarse_depth_var=LAMBDA_VAR[2], lambda_fine_depth_var=LAMBDA_VAR[3])
    t.loss_and_grads(au.draws_of(g))
    got = t.var_losses.cpu().numpy()
    print("variance losses", prec, got, terms64)
    assert abs(float(t.losses[0]) - res64["loss_coarse_mse"]) < 1e-6
    # sums of 24 (x 3) variances of fp32 outputs that are within 2e-6 (coarse) / 1e-4 (fine) of the restatement's
    np.testing.assert_allclose(got[[0, 2]], np.array(terms64)[[0, 2]], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got[[1, 3]], np.array(terms64)[[1, 3]], rtol=1e-3, atol=1e-5)
    spec = arch_spec(**g["arch"])
    for n, (net, ref) in enumerate((("coarse", gc64), ("fine", gf64))):
        au.assert_grads_close(t.grads[n], ref, spec, f"var odd_dense-{prec} {net}")


def test_regularize_patch_and_clipping_with_an_architecture(golden_dir, tr):
    """Trainer.regularize_patch (TV loss of an 8 x 8 HR patch, backward, its own Adam step) against the restatement's gradient
    of the same loss, and clip_grads inside optimize_parameters: the clipped gradient has the bound's norm."""
    g = dict(au.load_case(golden_dir, "odd_dense"))
    for k in ("rays", "u_coarse", "u_fine"):
        g[k] = g[k][:64]
    tv = lambda out: tr.tv_loss(out["coarse_comp_rgbs"].view(8, 8, 3)) + tr.tv_loss(out["fine_comp_rgbs"].view(8, 8, 3))
    _, gc64, gf64 = au.loss_and_grads(*au.state_dicts(g), g, loss_fn=tv)
    t = tr.Trainer(*au.state_dicts(g), white_bkgd=True, downscale=2, randomized=True, noise_std=0.0, arch=g["arch"], precision="fp32")
    w0 = t.params[1]["xyz_encoding_1.0.weight"].clone()
    tvs = t.regularize_patch(torch.from_numpy(g["rays"]).cuda(), 4, 1.0, draws=au.draws_of(g))
    assert tvs.shape == (2,) and t.step == 1 and not torch.equal(w0, t.params[1]["xyz_encoding_1.0.weight"])
    spec = arch_spec(**g["arch"])
    for n, (net, ref) in enumerate((("coarse", gc64), ("fine", gf64))):
        au.assert_grads_close(t.grads[n], ref, spec, f"tv patch {net}")
    full = au.load_case(golden_dir, "odd_dense")
    t = _trainer(tr, full, precision="fp32", grad_clip_val=1e-3, grad_clip_type="norm")
    t.optimize_parameters(au.draws_of(full))
    total = torch.linalg.vector_norm(torch.stack([v.norm() for n in range(2) for v in t.grads[n].values()]))
    ref_total = float(np.sqrt(sum(float(full[k]) ** 2 for k in full if k.startswith("gnorm_"))))
    assert ref_total > 1e-3 and abs(float(total) - 1e-3) <= 1e-5 * 1e-3 + 1e-9, (float(total), ref_total)
