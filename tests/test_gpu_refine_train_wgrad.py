"""The refinement network's opt-in weight-gradient route weight_grad = NSR_F16X3 ("f16x3": every weight gradient but E.conv1's as
one implicit split-fp16 GEMM per site, csrc/nsr_refine_wgrad_f16.hip) on the GPU: nsr_refine_train_backward_w,
forward_train(weight_grad=...), RefineTrainer(weight_grad=...), on the cases of tests/golden/refine_train.npz.

The route changes the weight gradients and nothing else, and the saved state does not depend on it: so it runs against the fp32
route on the SAME saved state and g_out, for both `precision`s of the backward and both of the forward that wrote the state.
Every convolution weight must lie within the tight bound tests/test_gpu_refine_train_mixed.py uses for its shared-saved-state
comparison (8 x the largest per-tensor gap the reference's own fp32 run has on the case: 2.8e-5 of the norm on this fixture);
every other tensor -- gamma, beta, the biases, the 17 cancelled biases, E.conv1's weight -- must be BIT-EQUAL.  precision = fp32
with weight_grad = f16x3 must pass the gates tests/test_gpu_refine_train.py applies to the fp32 pair against the fp64
restatement (three split terms are fp32-grade).

Measured (profiles/refine_train_wgrad_parity.json, one MI355X; NSR_REFINE_TRAIN_WGRAD_REPORT=path writes it): the worst
convolution weight against the fp32 route 4.1e-7 .. 5.0e-7 of its norm on all twelve (case, saved state, backward precision)
combinations (E.conv2.weight; bound 2.8e-5), every other tensor bit-equal, g_out x 2^-16 / 2^8 exact; fp32 pair with the route
against fp64: cases B / C worst 2.4e-6 / 2.3e-6, case A the fp32 pair's one kink event (ten tensors of E.conv1 .. E.conv4, worst
8.0e-4); the trainer ends at 0.0907 after 20 iterations."""
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
from .test_gpu_refine_train_mixed import Abi as MixedAbi, _dloss_dy, _gap, _inputs, _ptrs

pytestmark = pytest.mark.gpu
CASES = ("A", "B", "C")
LOOSE = 5e-2
FP32, F16X3 = _lib.NSR_FP32, _lib.NSR_F16X3
NAMES = {FP32: "fp32", F16X3: "f16x3"}
# the tensors the new route computes: every convolution weight but E.conv1's (cin 3: fp32 route)
CONV_W = [k for k in TRAIN_PARAM_KEYS if len(REFINE_SPEC[k]) == 4 and REFINE_SPEC[k][1] != 3]
OTHER = [k for k in TRAIN_PARAM_KEYS if k not in CONV_W]
REPORT = {}


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
    """tag -> gradients of the fp64 restatement, computed once on the CPU and left unchanged."""
    return {tag: ref.grads_fp64(sd_np, fx[f"{tag}_x"], fx[f"{tag}_c"], fx[f"{tag}_gt"], *fx[f"{tag}_lambdas"])[3] for tag in CASES}


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    out = os.environ.get("NSR_REFINE_TRAIN_WGRAD_REPORT")
    if out and REPORT:
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1)


class Abi(MixedAbi):
    """... with the weight-gradient route as an argument of the backward"""

    def backward_w(self, prec, wgrad, g_out):
        grads = [torch.full_like(self.sd[k], float("nan")) for k in TRAIN_PARAM_KEYS]        # OVERWRITTEN, whatever was there
        rc = self.lib.nsr_refine_train_backward_w(prec, wgrad, _ptrs(list(self.sd.values())), c_void_p(g_out.data_ptr()), _ptrs(grads),
                                                  c_void_p(self.ws.data_ptr()), self.ws.numel(), c_void_p(self.saved.data_ptr()),
                                                  self.saved.numel(), self.stream)
        assert rc == 0, rc
        return OrderedDict(zip(TRAIN_PARAM_KEYS, grads))


def test_the_tensor_lists():
    assert len(CONV_W) == 18 and "E.conv1.weight" in OTHER and "D.conv9.weight" in CONV_W and len(OTHER) == 72 - 18
    assert set(ref.CANCELLED) <= set(OTHER) and len(ref.CANCELLED) == 17


@pytest.mark.parametrize("fwd_prec", (FP32, F16X3), ids=("saved_fp32", "saved_f16x3"))
@pytest.mark.parametrize("tag", CASES)
def test_route_against_fp32_on_a_shared_saved_state(fx, sd_np, tag, fwd_prec):
    """backward_w(p, NSR_F16X3) against backward_w(p, NSR_FP32) = backward_p(p) on the same `saved` and g_out, p in both
    precisions: convolution weights within the tight bound, every other tensor bit-equal.  Then the range word: g_out x 2^-16
    and x 2^8 scale EVERY gradient exactly, g_out = 0 gives exact zeros."""
    x, c, gt = _inputs(fx, tag)
    tight = 8 * float(fx[f"{tag}_grad_gap"].max())
    a = Abi(sd_np)
    y = a.forward(fwd_prec, x, c)
    go = _dloss_dy(y, gt, *fx[f"{tag}_lambdas"])
    before = a.saved.clone()
    for prec in (FP32, F16X3):
        g32, g16 = a.backward_w(prec, FP32, go), a.backward_w(prec, F16X3, go)
        gp = a.backward(prec, go)
        assert all(torch.equal(g32[k], gp[k]) for k in TRAIN_PARAM_KEYS)             # _p is _w with NSR_FP32
        assert torch.equal(before, a.saved)
        gaps = {k: _gap(g16[k], g32[k]) for k in CONV_W}
        worst = max(gaps, key=gaps.get)
        rec = REPORT.setdefault("route_vs_fp32_shared_state", {}).setdefault(tag, {}).setdefault("saved_" + NAMES[fwd_prec], {})
        rec["backward_" + NAMES[prec]] = {"tight_bound": tight, "worst_tensor": worst, "worst_gap": gaps[worst]}
        print(f"case {tag}, saved by {NAMES[fwd_prec]}, backward {NAMES[prec]}: worst {worst} {gaps[worst]:.2e} (tight bound {tight:.2e})")
        for k in OTHER:
            assert torch.equal(g16[k], g32[k]), (tag, k)
        for k in ref.CANCELLED:
            assert float(g16[k].abs().max()) == 0.0, (tag, k)
        assert gaps[worst] <= tight, (worst, gaps[worst])
        assert not all(torch.equal(g16[k], g32[k]) for k in CONV_W)                  # and it is another route
        for s in (2.0 ** -16, 2.0 ** 8):
            gs = a.backward_w(prec, F16X3, go * s)
            for k in TRAIN_PARAM_KEYS:
                assert torch.equal(gs[k], g16[k] * s), (tag, s, k)
        gz = a.backward_w(prec, F16X3, torch.zeros_like(go))
        for k in TRAIN_PARAM_KEYS:
            assert float(gz[k].abs().max()) == 0.0, k


def test_fp32_pair_with_the_route_against_the_fp64_restatement(fx, sd_np, ref64):
    """precision = fp32, weight_grad = f16x3 under the gates of tests/test_gpu_refine_train.py: per case at most 10 of the 55
    live tensors over the tight bound, none over 5e-2, no tensor over it in two or more cases, the cancelled biases 0.0."""
    over = {}
    for tag in CASES:
        x, c, gt = _inputs(fx, tag)
        a = Abi(sd_np)
        y = a.forward(FP32, x, c)
        g = a.backward_w(FP32, F16X3, _dloss_dy(y, gt, *fx[f"{tag}_lambdas"]))
        g64 = ref64[tag]
        tight = 8 * float(fx[f"{tag}_grad_gap"].max())
        for k in ref.CANCELLED:
            assert float(g[k].abs().max()) == 0.0, (tag, k)
        gaps = {k: _gap(g[k].cpu(), g64[k]) for k in ref.LIVE}
        whole = float(torch.cat([(g[k].double().cpu() - g64[k]).flatten() for k in ref.LIVE]).norm()
                      / torch.cat([g64[k].flatten() for k in ref.LIVE]).norm())
        over[tag] = sorted(k for k, v in gaps.items() if v > tight)
        worst = max(gaps, key=gaps.get)
        REPORT.setdefault("fp32_pair_with_route_vs_fp64", {})[tag] = {
            "tight_bound": tight, "worst_tensor": worst, "worst_gap": gaps[worst], "whole_gradient_gap": whole,
            "worst_conv_weight_gap": max(gaps[k] for k in CONV_W), "over_tight": {k: gaps[k] for k in over[tag]},
            "reference_fp32_worst_gap": float(fx[f"{tag}_grad_gap"].max()), "reference_fp32_whole_gap": float(fx[f"{tag}_whole_gap"])}
        print(f"case {tag}: worst {worst} {gaps[worst]:.2e}, whole gradient {whole:.2e}, tight bound {tight:.2e}, over it: {over[tag]}")
    for tag in CASES:
        rec = REPORT["fp32_pair_with_route_vs_fp64"][tag]
        assert len(over[tag]) <= 10, (tag, rec["over_tight"])
        assert rec["worst_gap"] <= LOOSE, (tag, rec["worst_tensor"], rec["worst_gap"])
    twice = [k for k in ref.LIVE if sum(k in over[tag] for tag in CASES) >= 2]
    assert not twice, twice


def test_chunking_and_determinism(fx, sd_np):
    """img_chunk in {0, 1, 3} on case C: the new route's weight gradients are bit-identical (the slices are a function of the
    shape), with either precision of the backward; so is every other gradient but E.conv1's weight, the one product left on the
    fp32 route, whose summation order follows the chunk.  Two identical calls give identical bits."""
    x, c, gt = _inputs(fx, "C")
    runs = {}
    for chunk in (0, 1, 3):
        a = Abi(sd_np)
        y = a.forward(F16X3, x, c, img_chunk=chunk)
        go = _dloss_dy(y, gt, *fx["C_lambdas"])
        runs[chunk] = (y, a.backward_w(F16X3, F16X3, go), a.backward_w(FP32, F16X3, go))
        if chunk == 0:
            again = a.backward_w(F16X3, F16X3, go)
            assert all(torch.equal(again[k], runs[0][1][k]) for k in TRAIN_PARAM_KEYS)
    for chunk in (1, 3):
        assert torch.equal(runs[chunk][0], runs[0][0]), chunk
        for which in (1, 2):
            for k in TRAIN_PARAM_KEYS:
                if k != "E.conv1.weight":
                    assert torch.equal(runs[chunk][which][k], runs[0][which][k]), (chunk, which, k)


def test_autograd_binding_equals_the_c_abi(fx, sd_np):
    """forward_train(precision=..., weight_grad="f16x3") -> torch L1 -> .backward() = the C ABI pair, bit for bit"""
    from nerf_sr_amd import refine
    x, c, gt = _inputs(fx, "A")
    for name, prec in (("fp32", FP32), ("f16x3_mixed", F16X3)):
        params = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda().requires_grad_(True)) for k in TRAIN_PARAM_KEYS)
        running = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda()) for k in RUNNING_KEYS)
        y = refine.forward_train(params, running, x, c, precision=name, weight_grad="f16x3")
        torch.nn.functional.l1_loss(y, gt).backward()
        a = Abi(sd_np)
        ya = a.forward(prec, x, c)
        go = _dloss_dy(ya, gt, 1.0, 0.0)
        g = a.backward_w(prec, F16X3, go)
        assert torch.equal(y.detach(), ya)
        for k in TRAIN_PARAM_KEYS:
            assert params[k].grad is not None and torch.equal(params[k].grad, g[k]), k
        # the default is the fp32 route
        params2 = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda().requires_grad_(True)) for k in TRAIN_PARAM_KEYS)
        running2 = OrderedDict((k, torch.from_numpy(sd_np[k]).cuda()) for k in RUNNING_KEYS)
        torch.nn.functional.l1_loss(refine.forward_train(params2, running2, x, c, precision=name), gt).backward()
        g32 = a.backward(prec, go)
        for k in TRAIN_PARAM_KEYS:
            assert torch.equal(params2[k].grad, g32[k]), k


def test_trainer(fx, sd_np):
    """RefineTrainer(precision="f16x3_mixed", weight_grad="f16x3"): 20 iterations on case A's batch end at or below the
    reference's recorded loss after 10 (0.1628: the mixed trainer's criterion)."""
    from nerf_sr_amd import refine
    x, c, gt = _inputs(fx, "A")
    tr = refine.RefineTrainer(sd_np, lr=5e-4, precision="f16x3_mixed", weight_grad="f16x3")
    tr.set_input({"sr_patch": x, "ref_patches": c, "gt_patch": gt})
    for _ in range(20):
        tr.optimize_parameters()
    for k in ref.CANCELLED:
        assert torch.equal(tr.params[k].detach().cpu(), torch.from_numpy(sd_np[k])), k
    REPORT["trainer"] = {"loss_after_20": float(tr.loss_tot.detach()), "reference_after_10": float(fx["A_curve"][9]),
                         "reference_after_20": float(fx["A_curve"][19])}
    print(f"loss after 20 iterations {float(tr.loss_tot.detach()):.4f}; reference: {float(fx['A_curve'][9]):.4f} after 10")
    assert float(tr.loss_tot.detach()) <= float(fx["A_curve"][9])
