"""Training of the refinement network on the GPU (include/nsr_refine.h, "training"; nerf_sr_amd.refine.forward_train /
RefineTrainer) against the reference's recorded train-mode runs (tests/golden/refine_train.npz: y, running statistics,
the reference's own fp32-vs-fp64 gaps, its training curve) and, for FULL gradient tensors, against the fp64 restatement
tests/refine_train_ref.py (pinned to the same fixture by tests/test_refine_train_cpu.py).

Gradient acceptance (per tensor: ||g - g64|| / ||g64||).  TIGHT = 8 x the largest per-tensor gap the reference's own fp32
run has on the case (~3.5e-6: a different summation order through 19 layers), i.e. ~3e-5.  A ReLU / max kink event (an
activation a rounding error from 0, two references a rounding error apart) legitimately moves a handful of tensors by up
to ~1e-2 in ONE case; a wrong formula shows in every case.  So: per case at most 10 of the 55 live tensors over TIGHT,
none over 5e-2, no tensor over TIGHT in two or more cases, the 17 cancelled biases exactly 0.0.

Measured (profiles/refine_train_parity.json, one MI355X): cases B and C have every tensor at <= 2.4e-6 (whole gradient
2.1e-6 / 1.9e-6; the reference's own fp32: 3.5e-6 / 2.9e-6).  Case A has ONE kink event: the fp64 network's E.conv4
pre-activation of a reference patch, channel 108, lies 2.6e-7 from 0; the flip is one channel of E.conv4_bnorm.bias (8.0e-4
of its norm, the next channel 4e-7) and puts the 10 tensors of E.conv1 .. E.conv4 at 4.1e-4 .. 8.0e-4 (whole gradient
3.0e-4), every other tensor at <= 2.9e-6.  The forward sums K in chains of 32 added in double for this reason: summed in
one MFMA chain (K up to 13,824) it was 2.5 - 4 x further from fp64 than the reference's fp32 and flipped a decoder ReLU
in every case (38 / 50 / 50 tensors at 6e-4 .. 7.8e-3)."""
import json
import os
from collections import OrderedDict
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from nerf_sr_amd.refine import REFINE_SPEC, RUNNING_KEYS, TRAIN_PARAM_KEYS, make_refine_state_dict

from . import refine_train_ref as ref

pytestmark = pytest.mark.gpu
CASES = ("A", "B", "C")
LOOSE = 5e-2


@pytest.fixture(scope="module")
def fx(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return np.load(os.path.join(golden_dir, "refine_train.npz"))


@pytest.fixture(scope="module")
def sd_np(fx):
    return make_refine_state_dict(int(fx["weights_seed"]))


@pytest.fixture(scope="module")
def ref64(fx, sd_np):
    """tag -> (y, running, loss, grads) of the fp64 restatement, computed once on the CPU and left unchanged."""
    return {tag: ref.grads_fp64(sd_np, fx[f"{tag}_x"], fx[f"{tag}_c"], fx[f"{tag}_gt"], *fx[f"{tag}_lambdas"]) for tag in CASES}


def _ptrs(ts):
    return (c_void_p * len(ts))(*[c_void_p(t.data_ptr()) for t in ts])


class Abi:
    """The C ABI pair on fresh device copies of a state dict."""

    def __init__(self, sd_np):
        self.lib = _lib.load()
        self.sd = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda()) for k in REFINE_SPEC)
        self.stream = c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward(self, x, c, img_chunk=0, momentum=0.1):
        B, R, H, W = c.shape[0], c.shape[1], c.shape[3], c.shape[4]
        self.ws = torch.empty(self.lib.nsr_refine_train_workspace_bytes(B, R, H, W, img_chunk), dtype=torch.uint8, device="cuda")
        self.saved = torch.empty(self.lib.nsr_refine_train_saved_bytes(B, R, H, W), dtype=torch.uint8, device="cuda")
        assert self.ws.numel() > 0 and self.saved.numel() > 0
        y = torch.empty(B, 3, H, W, device="cuda")
        rc = self.lib.nsr_refine_train_forward(_ptrs(list(self.sd.values())), _ptrs([self.sd[k] for k in RUNNING_KEYS]), momentum,
                                               c_void_p(x.data_ptr()), c_void_p(c.data_ptr()), B, R, H, W, img_chunk, c_void_p(y.data_ptr()),
                                               c_void_p(self.ws.data_ptr()), self.ws.numel(), c_void_p(self.saved.data_ptr()),
                                               self.saved.numel(), self.stream)
        assert rc == 0, rc
        return y

    def backward(self, g_out, saved=None, saved_bytes=None):
        saved = self.saved if saved is None else saved
        grads = [torch.full_like(self.sd[k], float("nan")) for k in TRAIN_PARAM_KEYS]        # OVERWRITTEN, whatever was there
        rc = self.lib.nsr_refine_train_backward(_ptrs(list(self.sd.values())), c_void_p(g_out.data_ptr()), _ptrs(grads),
                                                c_void_p(self.ws.data_ptr()), self.ws.numel(), c_void_p(saved.data_ptr()),
                                                saved.numel() if saved_bytes is None else saved_bytes, self.stream)
        return rc, OrderedDict(zip(TRAIN_PARAM_KEYS, grads))


def _inputs(fx, tag):
    return tuple(torch.from_numpy(fx[f"{tag}_{k}"]).cuda() for k in ("x", "c", "gt"))


def _dloss_dy(y, gt, l1, mse):
    y = y.detach().clone().requires_grad_(True)
    ref.loss_of(y, gt, float(l1), float(mse)).backward()
    return y.grad.contiguous()


def _rel(g, g64):
    return float((g.double().cpu() - g64).norm() / g64.norm())


@pytest.mark.parametrize("tag", CASES)
def test_forward_and_running_statistics(fx, sd_np, tag):
    """|y - y64| <= 8 x the reference's own fp32-vs-fp64 max |dy|; every running statistic within 8 x the reference's own gap of
    the recorded fp64 value -- the encoder's show TWO updates (synthesised call, then reference call): one update misses by
    ~10 % of the value."""
    x, c, _ = _inputs(fx, tag)
    a = Abi(sd_np)
    y = a.forward(x, c)
    dy = float((y.double().cpu() - torch.from_numpy(fx[f"{tag}_y64"])).abs().max())
    run = torch.cat([a.sd[k] for k in RUNNING_KEYS]).double().cpu()
    dr = float((run - torch.from_numpy(fx[f"{tag}_running64"])).abs().max())
    print(f"case {tag}: max |dy| {dy:.2e} (reference fp32: {float(fx[f'{tag}_dy_max']):.2e}), running statistics {dr:.2e} "
          f"(reference fp32: {float(fx[f'{tag}_running_gap']):.2e})")
    assert dy <= 8 * float(fx[f"{tag}_dy_max"])
    assert dr <= 8 * float(fx[f"{tag}_running_gap"])
    # the parameters themselves are inputs: untouched
    for k in TRAIN_PARAM_KEYS:
        assert torch.equal(a.sd[k].cpu(), torch.from_numpy(sd_np[k])), k


def test_gradients_against_the_fp64_restatement(fx, sd_np, ref64):
    report, over = {}, {}
    for tag in CASES:
        x, c, gt = _inputs(fx, tag)
        a = Abi(sd_np)
        y = a.forward(x, c)
        rc, g = a.backward(_dloss_dy(y, gt, *fx[f"{tag}_lambdas"]))
        assert rc == 0, rc
        g64 = ref64[tag][3]
        tight = 8 * float(fx[f"{tag}_grad_gap"].max())
        for k in ref.CANCELLED:
            assert float(g[k].abs().max()) == 0.0, (tag, k)
        gaps = {k: _rel(g[k], g64[k]) for k in ref.LIVE}
        whole = float(torch.cat([(g[k].double().cpu() - g64[k]).flatten() for k in ref.LIVE]).norm()
                      / torch.cat([g64[k].flatten() for k in ref.LIVE]).norm())
        over[tag] = sorted(k for k, v in gaps.items() if v > tight)
        worst = max(gaps, key=gaps.get)
        report[tag] = {"shape_BRHW": [int(v) for v in fx[f"{tag}_shape"]], "lambda_l1_mse": [float(v) for v in fx[f"{tag}_lambdas"]],
                       "tight_bound": tight, "worst_tensor": worst, "worst_gap": gaps[worst], "whole_gradient_gap": whole,
                       "over_tight": {k: gaps[k] for k in over[tag]},
                       "reference_fp32_worst_gap": float(fx[f"{tag}_grad_gap"].max()), "reference_fp32_whole_gap": float(fx[f"{tag}_whole_gap"])}
        print(f"case {tag}: worst {worst} {gaps[worst]:.2e}, whole gradient {whole:.2e}, tight bound {tight:.2e}, over it: {over[tag]}")
    out = os.environ.get("NSR_REFINE_TRAIN_REPORT")
    if out:                                     # keep the numbers (profiles/refine_train_parity.json)
        with open(out, "w") as f:
            json.dump(report, f, indent=1)
    for tag in CASES:
        assert len(over[tag]) <= 10, (tag, report[tag]["over_tight"])
        assert report[tag]["worst_gap"] <= LOOSE, (tag, report[tag]["worst_tensor"], report[tag]["worst_gap"])
    twice = [k for k in ref.LIVE if sum(k in over[tag] for tag in CASES) >= 2]
    assert not twice, {k: [report[tag]["over_tight"].get(k) for tag in CASES] for k in twice}


def test_chunking_and_determinism(fx, sd_np):
    """img_chunk in {1, 3, all} on case C: y bit-identical, gradients within the tight bound of each other; two identical
    calls and a second backward on the same saved state give identical bits; the backward leaves `saved` alone and rejects
    a buffer no forward wrote (-1) or one shorter than its header says (-4)."""
    x, c, gt = _inputs(fx, "C")
    tight = 8 * float(fx["C_grad_gap"].max())
    runs = {}
    for chunk in (0, 1, 3):
        a = Abi(sd_np)
        y = a.forward(x, c, img_chunk=chunk)
        go = _dloss_dy(y, gt, *fx["C_lambdas"])
        before = a.saved.clone()
        rc, g = a.backward(go)
        assert rc == 0
        if chunk == 0:
            rc2, g2 = a.backward(go)                       # second backward on the same saved state
            assert rc2 == 0 and all(torch.equal(g[k], g2[k]) for k in TRAIN_PARAM_KEYS)
            assert torch.equal(before, a.saved)
            b = Abi(sd_np)                                 # two identical calls
            yb = b.forward(x, c, img_chunk=0)
            rcb, gb = b.backward(go)
            assert rcb == 0 and torch.equal(y, yb) and all(torch.equal(g[k], gb[k]) for k in TRAIN_PARAM_KEYS)
            assert all(torch.equal(a.sd[k], b.sd[k]) for k in RUNNING_KEYS)
            assert a.backward(go, saved=torch.zeros_like(a.saved))[0] == -1           # no forward wrote it
            assert a.backward(go, saved_bytes=a.saved.numel() - 256)[0] == -4         # shorter than its header says
        runs[chunk] = (y, g)
    for chunk in (1, 3):
        assert torch.equal(runs[chunk][0], runs[0][0]), chunk
        for k in ref.LIVE:
            d = float((runs[chunk][1][k] - runs[0][1][k]).double().norm() / runs[0][1][k].double().norm())
            assert d <= tight, (chunk, k, d)


def test_autograd_binding_equals_the_c_abi(fx, sd_np):
    """forward_train -> torch L1 -> .backward() fills .grad of all 72 leaves with the bits of the C-ABI backward on torch's dL/dy;
    the running statistics move in place; the images get no gradient."""
    from nerf_sr_amd import refine
    x, c, gt = _inputs(fx, "A")
    params = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda().requires_grad_(True)) for k in TRAIN_PARAM_KEYS)
    running = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda()) for k in RUNNING_KEYS)
    xg = x.clone().requires_grad_(True)
    y = refine.forward_train(params, running, xg, c)
    torch.nn.functional.l1_loss(y, gt).backward()
    assert xg.grad is None
    a = Abi(sd_np)
    ya = a.forward(x, c)
    rc, g = a.backward(_dloss_dy(ya, gt, 1.0, 0.0))
    assert rc == 0 and torch.equal(y.detach(), ya)
    for k in TRAIN_PARAM_KEYS:
        assert params[k].grad is not None and torch.equal(params[k].grad, g[k]), k
    for k in RUNNING_KEYS:
        assert torch.equal(running[k], a.sd[k]) and not torch.equal(running[k].cpu(), torch.from_numpy(sd_np[k])), k
    with pytest.raises(ValueError):
        refine.forward_train(params, running, x[:, :, :12], c[:, :, :, :12])       # H = 12


def test_trainer(fx, sd_np):
    """One optimize_parameters = torch.optim.Adam on the GPU over the same gradients (<= 1e-7 absolute); 20 iterations on case
    A's batch end at or below the reference's recorded loss after 10 iterations (half the steps as margin; the recorded curve
    is fixture A_curve); eval_model() runs."""
    from nerf_sr_amd import refine
    x, c, gt = _inputs(fx, "A")
    tr = refine.RefineTrainer(sd_np, lr=5e-4)
    tr.set_input({"sr_patch": x, "ref_patches": c, "gt_patch": gt})
    w0 = [tr.params[k].detach().clone().requires_grad_(True) for k in TRAIN_PARAM_KEYS]
    tr.optimize_parameters()
    opt = torch.optim.Adam(w0, lr=5e-4, betas=(0.9, 0.999))
    for w, k in zip(w0, TRAIN_PARAM_KEYS):
        w.grad = tr.params[k].grad.clone()
    opt.step()
    for w, k in zip(w0, TRAIN_PARAM_KEYS):
        assert float((w.detach() - tr.params[k].detach()).abs().max()) <= 1e-7, k
    for k in ref.CANCELLED:                     # exact-zero gradients: Adam never moves the cancelled biases
        assert torch.equal(tr.params[k].detach().cpu(), torch.from_numpy(sd_np[k])), k
    assert abs(float(tr.loss_tot.detach()) - float(fx["A_curve"][0])) <= 1e-4 and float(tr.loss_mse) == 0.0
    assert torch.isfinite(tr.loss_psnr_input) and torch.isfinite(tr.loss_psnr_refine)
    for _ in range(19):
        tr.optimize_parameters()
    print(f"loss after 20 iterations {float(tr.loss_tot.detach()):.4f}; reference: {float(fx['A_curve'][9]):.4f} after 10, {float(fx['A_curve'][19]):.4f} after 20")
    assert float(tr.loss_tot.detach()) <= float(fx["A_curve"][9])
    assert tr.step == 20 and tr.update_learning_rate(25, n_epochs=30) < 5e-4
    sd = tr.state_dict()
    assert list(sd) == list(REFINE_SPEC)
    y = tr.eval_model()(x, c)
    assert tuple(y.shape) == tuple(x.shape) and bool(torch.isfinite(y).all())
