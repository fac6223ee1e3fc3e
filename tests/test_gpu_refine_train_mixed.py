"""The refinement network's opt-in training precision NSR_F16X3 ("f16x3_mixed": forward convolutions and stride-1 input gradients
on the split-fp16 MFMA with implicit gather; BatchNorm, the stride-2 input gradients and every weight gradient fp32) on the GPU:
nsr_refine_train_forward_p / _backward_p, forward_train(precision=...), RefineTrainer(precision=...), on the cases of
tests/golden/refine_train.npz.

The backward is tested where it can be tested without ReLU-kink noise: the saved state does not depend on the precision, so the
NSR_F16X3 backward runs against the fp32 backward on the SAME saved state and g_out -- same masks, same winners -- and every
live tensor must lie within TIGHT = 8 x the largest per-tensor gap the reference's own fp32 run has on the case (~3e-5) of
the fp32 backward's, relative to its norm.  The full NSR_F16X3 pair against the fp64 restatement is expected to show kink
events (one fp32 summation chain per output in the forward) and is gated at LOOSE = 5e-2 only; its figures are recorded.

Measured (profiles/refine_train_mixed_parity.json, one MI355X; NSR_REFINE_TRAIN_MIXED_REPORT=path writes it): forward max |dy|
2.1 / 2.6 / 3.1 x the reference's own fp32 on cases A / B / C (bound 8 x); backward on a shared saved state: worst tensor
2.7e-6 .. 3.0e-6 on all six (case, saved state) pairs (bound 2.8e-5), g_out x 2^-16 / 2^8 scale every gradient exactly; full
pair against fp64: 38 / 43 / 0 of 55 tensors over the tight bound, worst 1.5e-3 / 2.0e-2 / 9.6e-6."""
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
FP32, F16X3 = _lib.NSR_FP32, _lib.NSR_F16X3
REPORT = {}


@pytest.fixture(scope="module")
def fx(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return np.load(os.path.join(golden_dir, "refine_train.npz"))


@pytest.fixture(scope="module")
def sd_np(fx):
    return make_refine_state_dict(int(fx["weights_seed"]))


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    out = os.environ.get("NSR_REFINE_TRAIN_MIXED_REPORT")
    if out and REPORT:
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1)


def _ptrs(ts):
    return (c_void_p * len(ts))(*[c_void_p(t.data_ptr()) for t in ts])


class Abi:
    """The C ABI pair with a precision argument on fresh device copies of a state dict."""

    def __init__(self, sd_np):
        self.lib = _lib.load()
        self.sd = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda()) for k in REFINE_SPEC)
        self.stream = c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward(self, prec, x, c, img_chunk=0, momentum=0.1):
        B, R, H, W = c.shape[0], c.shape[1], c.shape[3], c.shape[4]
        self.ws = torch.empty(self.lib.nsr_refine_train_workspace_bytes(B, R, H, W, img_chunk), dtype=torch.uint8, device="cuda")
        self.saved = torch.empty(self.lib.nsr_refine_train_saved_bytes(B, R, H, W), dtype=torch.uint8, device="cuda")
        assert self.ws.numel() > 0 and self.saved.numel() > 0
        y = torch.empty(B, 3, H, W, device="cuda")
        rc = self.lib.nsr_refine_train_forward_p(prec, _ptrs(list(self.sd.values())), _ptrs([self.sd[k] for k in RUNNING_KEYS]), momentum,
                                                 c_void_p(x.data_ptr()), c_void_p(c.data_ptr()), B, R, H, W, img_chunk,
                                                 c_void_p(y.data_ptr()), c_void_p(self.ws.data_ptr()), self.ws.numel(),
                                                 c_void_p(self.saved.data_ptr()), self.saved.numel(), self.stream)
        assert rc == 0, rc
        return y

    def backward(self, prec, g_out):
        grads = [torch.full_like(self.sd[k], float("nan")) for k in TRAIN_PARAM_KEYS]        # OVERWRITTEN, whatever was there
        rc = self.lib.nsr_refine_train_backward_p(prec, _ptrs(list(self.sd.values())), c_void_p(g_out.data_ptr()), _ptrs(grads),
                                                  c_void_p(self.ws.data_ptr()), self.ws.numel(), c_void_p(self.saved.data_ptr()),
                                                  self.saved.numel(), self.stream)
        assert rc == 0, rc
        return OrderedDict(zip(TRAIN_PARAM_KEYS, grads))


def _inputs(fx, tag):
    return tuple(torch.from_numpy(fx[f"{tag}_{k}"]).cuda() for k in ("x", "c", "gt"))


def _dloss_dy(y, gt, l1, mse):
    y = y.detach().clone().requires_grad_(True)
    ref.loss_of(y, gt, float(l1), float(mse)).backward()
    return y.grad.contiguous()


def _gap(g, g0):
    return float((g.double() - g0.double()).norm() / g0.double().norm())


def _same(ga, gb):
    return all(torch.equal(ga[k], gb[k]) for k in TRAIN_PARAM_KEYS)


@pytest.mark.parametrize("tag", CASES)
def test_forward_and_running_statistics(fx, sd_np, tag):
    """NSR_F16X3 forward: max |y - y64| <= 8 x the reference's own fp32-vs-fp64 max |dy|, running statistics within 8 x the
    reference's own gap (the bounds of the fp32 forward), the parameters untouched."""
    x, c, _ = _inputs(fx, tag)
    a = Abi(sd_np)
    y = a.forward(F16X3, x, c)
    dy = float((y.double().cpu() - torch.from_numpy(fx[f"{tag}_y64"])).abs().max())
    run = torch.cat([a.sd[k] for k in RUNNING_KEYS]).double().cpu()
    dr = float((run - torch.from_numpy(fx[f"{tag}_running64"])).abs().max())
    REPORT.setdefault("forward", {})[tag] = {"max_dy": dy, "reference_fp32_max_dy": float(fx[f"{tag}_dy_max"]),
                                             "ratio_to_reference_fp32": dy / float(fx[f"{tag}_dy_max"]), "running_gap": dr,
                                             "reference_fp32_running_gap": float(fx[f"{tag}_running_gap"])}
    print(f"case {tag}: max |dy| {dy:.2e} = {dy / float(fx[f'{tag}_dy_max']):.2f} x the reference's fp32 ({float(fx[f'{tag}_dy_max']):.2e}), "
          f"running statistics {dr:.2e} (reference fp32: {float(fx[f'{tag}_running_gap']):.2e})")
    assert dy <= 8 * float(fx[f"{tag}_dy_max"])
    assert dr <= 8 * float(fx[f"{tag}_running_gap"])
    for k in TRAIN_PARAM_KEYS:
        assert torch.equal(a.sd[k].cpu(), torch.from_numpy(sd_np[k])), k


@pytest.mark.parametrize("fwd_prec", (FP32, F16X3), ids=("saved_fp32", "saved_f16x3"))
@pytest.mark.parametrize("tag", CASES)
def test_backward_on_a_shared_saved_state(fx, sd_np, tag, fwd_prec):
    """backward_p(NSR_F16X3) against backward_p(NSR_FP32) on the same `saved` and g_out: every live tensor within the tight
    bound (no kink allowance: the masks are the same), D.conv9.weight / .bias bit-equal (no input gradient precedes them),
    the 17 cancelled biases exactly 0.0.  Then the range word: g_out x 2^-16 and x 2^8 give the gradients x 2^-16 / 2^8
    (within the same bound; exact equality is recorded), g_out = 0 gives exact zeros."""
    x, c, gt = _inputs(fx, tag)
    tight = 8 * float(fx[f"{tag}_grad_gap"].max())
    a = Abi(sd_np)
    y = a.forward(fwd_prec, x, c)
    go = _dloss_dy(y, gt, *fx[f"{tag}_lambdas"])
    before = a.saved.clone()
    g32, g16 = a.backward(FP32, go), a.backward(F16X3, go)
    assert torch.equal(before, a.saved)
    for k in ref.CANCELLED:
        assert float(g16[k].abs().max()) == 0.0, (tag, k)
    assert torch.equal(g16["D.conv9.weight"], g32["D.conv9.weight"]) and torch.equal(g16["D.conv9.bias"], g32["D.conv9.bias"])
    gaps = {k: _gap(g16[k], g32[k]) for k in ref.LIVE}
    worst = max(gaps, key=gaps.get)
    rec = REPORT.setdefault("backward_shared_state", {}).setdefault(tag, {})
    rec["saved_fp32" if fwd_prec == FP32 else "saved_f16x3"] = r = {"tight_bound": tight, "worst_tensor": worst, "worst_gap": gaps[worst]}
    print(f"case {tag}, forward precision {fwd_prec}: worst {worst} {gaps[worst]:.2e} (tight bound {tight:.2e})")
    assert gaps[worst] <= tight, (worst, gaps[worst])
    # ---- range word
    for name, s in (("2^-16", 2.0 ** -16), ("2^8", 2.0 ** 8)):
        gs = a.backward(F16X3, go * s)
        d = {k: _gap(gs[k] / s, g16[k]) for k in ref.LIVE}
        r[f"g_out_x_{name}_worst_gap"] = max(d.values())
        r[f"g_out_x_{name}_exactly_scaled"] = all(torch.equal(gs[k] / s, g16[k]) for k in TRAIN_PARAM_KEYS)
        print(f"  g_out x {name}: worst gap to the unscaled run {max(d.values()):.2e}, exact: {r[f'g_out_x_{name}_exactly_scaled']}")
        assert max(d.values()) <= tight, (name, max(d, key=d.get))
    gz = a.backward(F16X3, torch.zeros_like(go))
    for k in TRAIN_PARAM_KEYS:
        assert float(gz[k].abs().max()) == 0.0, k


def test_full_pair_against_the_fp64_restatement(fx, sd_np):
    """NSR_F16X3 forward and backward against refine_train_ref.grads_fp64: no tensor over LOOSE; the whole-gradient gap and the
    tensors over the tight bound are recorded, not gated (kink events are expected: module docstring)."""
    for tag in CASES:
        x, c, gt = _inputs(fx, tag)
        g64 = ref.grads_fp64(sd_np, fx[f"{tag}_x"], fx[f"{tag}_c"], fx[f"{tag}_gt"], *fx[f"{tag}_lambdas"])[3]
        a = Abi(sd_np)
        y = a.forward(F16X3, x, c)
        g = a.backward(F16X3, _dloss_dy(y, gt, *fx[f"{tag}_lambdas"]))
        tight = 8 * float(fx[f"{tag}_grad_gap"].max())
        for k in ref.CANCELLED:
            assert float(g[k].abs().max()) == 0.0, (tag, k)
        gaps = {k: _gap(g[k].cpu(), g64[k]) for k in ref.LIVE}
        whole = float(torch.cat([(g[k].double().cpu() - g64[k]).flatten() for k in ref.LIVE]).norm()
                      / torch.cat([g64[k].flatten() for k in ref.LIVE]).norm())
        worst = max(gaps, key=gaps.get)
        REPORT.setdefault("full_pair_vs_fp64", {})[tag] = {
            "tight_bound": tight, "worst_tensor": worst, "worst_gap": gaps[worst], "whole_gradient_gap": whole,
            "over_tight": {k: v for k, v in sorted(gaps.items()) if v > tight}, "reference_fp32_whole_gap": float(fx[f"{tag}_whole_gap"])}
        print(f"case {tag}: worst {worst} {gaps[worst]:.2e}, whole gradient {whole:.2e}, "
              f"{sum(v > tight for v in gaps.values())} of {len(gaps)} tensors over the tight bound {tight:.2e}")
        assert gaps[worst] <= LOOSE, (tag, worst, gaps[worst])


def test_chunking_and_determinism(fx, sd_np):
    """img_chunk in {0, 1, 3} on case C: y bit-identical, gradients within the tight bound of each other (the fp32 weight
    gradients' summation order follows the chunk); two identical calls and a second backward on the same saved state give
    identical bits; the backward leaves `saved` alone."""
    x, c, gt = _inputs(fx, "C")
    tight = 8 * float(fx["C_grad_gap"].max())
    runs = {}
    for chunk in (0, 1, 3):
        a = Abi(sd_np)
        y = a.forward(F16X3, x, c, img_chunk=chunk)
        go = _dloss_dy(y, gt, *fx["C_lambdas"])
        before = a.saved.clone()
        g = a.backward(F16X3, go)
        if chunk == 0:
            assert _same(g, a.backward(F16X3, go)) and torch.equal(before, a.saved)
            b = Abi(sd_np)
            yb = b.forward(F16X3, x, c)
            assert torch.equal(y, yb) and _same(g, b.backward(F16X3, go))
            assert all(torch.equal(a.sd[k], b.sd[k]) for k in RUNNING_KEYS)
            runs["saved"] = before
        runs[chunk] = (y, g)
    for chunk in (1, 3):
        assert torch.equal(runs[chunk][0], runs[0][0]), chunk
        for k in ref.LIVE:
            d = _gap(runs[chunk][1][k], runs[0][1][k])
            assert d <= tight, (chunk, k, d)


def test_fp32_entry_points_are_the_fp32_precision(fx, sd_np):
    """nsr_refine_train_forward / _backward give the bits of the _p pair at NSR_FP32, saved state included"""
    x, c, gt = _inputs(fx, "B")
    a, b = Abi(sd_np), Abi(sd_np)
    y = a.forward(FP32, x, c)
    b.ws, b.saved = torch.empty_like(a.ws), torch.empty_like(a.saved)
    yb = torch.empty_like(y)
    B, R, H, W = c.shape[0], c.shape[1], c.shape[3], c.shape[4]
    assert b.lib.nsr_refine_train_forward(_ptrs(list(b.sd.values())), _ptrs([b.sd[k] for k in RUNNING_KEYS]), 0.1, c_void_p(x.data_ptr()),
                                          c_void_p(c.data_ptr()), B, R, H, W, 0, c_void_p(yb.data_ptr()), c_void_p(b.ws.data_ptr()),
                                          b.ws.numel(), c_void_p(b.saved.data_ptr()), b.saved.numel(), b.stream) == 0
    assert torch.equal(y, yb) and all(torch.equal(a.sd[k], b.sd[k]) for k in RUNNING_KEYS)
    go = _dloss_dy(y, gt, *fx["B_lambdas"])
    ga = a.backward(FP32, go)
    gb = [torch.full_like(b.sd[k], float("nan")) for k in TRAIN_PARAM_KEYS]
    assert b.lib.nsr_refine_train_backward(_ptrs(list(b.sd.values())), c_void_p(go.data_ptr()), _ptrs(gb), c_void_p(b.ws.data_ptr()),
                                           b.ws.numel(), c_void_p(b.saved.data_ptr()), b.saved.numel(), b.stream) == 0
    assert all(torch.equal(ga[k], t) for k, t in zip(TRAIN_PARAM_KEYS, gb))


def test_autograd_binding_equals_the_c_abi(fx, sd_np):
    """forward_train(precision="f16x3_mixed") -> torch L1 -> .backward() = the C ABI pair at NSR_F16X3, bit for bit"""
    from nerf_sr_amd import refine
    x, c, gt = _inputs(fx, "A")
    params = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda().requires_grad_(True)) for k in TRAIN_PARAM_KEYS)
    running = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda()) for k in RUNNING_KEYS)
    y = refine.forward_train(params, running, x, c, precision="f16x3_mixed")
    torch.nn.functional.l1_loss(y, gt).backward()
    a = Abi(sd_np)
    ya = a.forward(F16X3, x, c)
    g = a.backward(F16X3, _dloss_dy(ya, gt, 1.0, 0.0))
    assert torch.equal(y.detach(), ya)
    for k in TRAIN_PARAM_KEYS:
        assert params[k].grad is not None and torch.equal(params[k].grad, g[k]), k
    for k in RUNNING_KEYS:
        assert torch.equal(running[k], a.sd[k]), k
    b = Abi(sd_np)                                      # and it is not the fp32 pair under another name
    assert not torch.equal(b.forward(FP32, x, c), ya)


def test_trainer(fx, sd_np):
    """RefineTrainer(precision="f16x3_mixed"): one optimize_parameters = torch.optim.Adam over its gradients (<= 1e-7 absolute);
    20 iterations on case A's batch end at or below the reference's recorded loss after 10 (the fp32 trainer's criterion)."""
    from nerf_sr_amd import refine
    x, c, gt = _inputs(fx, "A")
    tr = refine.RefineTrainer(sd_np, lr=5e-4, precision="f16x3_mixed")
    tr.set_input({"sr_patch": x, "ref_patches": c, "gt_patch": gt})
    w0 = [tr.params[k].detach().clone().requires_grad_(True) for k in TRAIN_PARAM_KEYS]
    tr.optimize_parameters()
    opt = torch.optim.Adam(w0, lr=5e-4, betas=(0.9, 0.999))
    for w, k in zip(w0, TRAIN_PARAM_KEYS):
        w.grad = tr.params[k].grad.clone()
    opt.step()
    for w, k in zip(w0, TRAIN_PARAM_KEYS):
        assert float((w.detach() - tr.params[k].detach()).abs().max()) <= 1e-7, k
    for k in ref.CANCELLED:
        assert torch.equal(tr.params[k].detach().cpu(), torch.from_numpy(sd_np[k])), k
    assert abs(float(tr.loss_tot.detach()) - float(fx["A_curve"][0])) <= 1e-4
    for _ in range(19):
        tr.optimize_parameters()
    REPORT["trainer"] = {"loss_after_20": float(tr.loss_tot.detach()), "reference_after_10": float(fx["A_curve"][9]),
                         "reference_after_20": float(fx["A_curve"][19])}
    print(f"loss after 20 iterations {float(tr.loss_tot.detach()):.4f}; reference: {float(fx['A_curve'][9]):.4f} after 10")
    assert float(tr.loss_tot.detach()) <= float(fx["A_curve"][9])
