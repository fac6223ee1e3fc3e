#!/usr/bin/env python3
"""Overfit the refinement network on ONE synthetic patch batch (needs an MI355X): the "ground truth" is a smooth random
pattern, the synthesised patch is that pattern blurred and noised, the reference patches are shifted crops of the ground
truth -- the shape of the reference's protocol (scripts/train_llff_refine.sh: patch sets of 1 + 8 patches at 64 x 64, L1
loss, Adam at 5e-4) without its dataset.  The loop is the reference's train.py: set_input -> optimize_parameters.

    python examples/train_refine_toy.py [--iters 200] [--batch 4] [--ssim LAMBDA] [--grad-loss LAMBDA]

--ssim LAMBDA adds LAMBDA * (1 - SSIM) to the L1 loss (RefineTrainer's refine_with_ssim: the device SSIM under autograd).
--grad-loss LAMBDA adds LAMBDA * GradientLoss(pred, gt) (the reference's --refine_with_grad, refine_model.py:162-164) the way
RefineTrainer's own error message says: the loss is composed here over refine.forward_train, which back-propagates it.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_sr_amd import losses, refine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "f16x3_mixed"),
                    help="f16x3_mixed: forward and input gradients on the split-fp16 MFMA")
    ap.add_argument("--weight-grad", default="fp32", choices=("fp32", "f16x3"),
                    help="f16x3: the weight gradients as one implicit split-fp16 GEMM per layer (fp32: im2col + fp32 GEMM)")
    ap.add_argument("--ssim", type=float, default=None, metavar="LAMBDA", help="add LAMBDA * (1 - SSIM) to the loss")
    ap.add_argument("--grad-loss", type=float, default=None, metavar="LAMBDA", help="add LAMBDA * GradientLoss(pred, gt) to the loss")
    a = ap.parse_args()
    B, R, P = a.batch, 8, 64
    gen = torch.Generator().manual_seed(0)
    big = F.interpolate(torch.rand(B, 3, 12, 12, generator=gen), size=(P + 16, P + 16), mode="bicubic", align_corners=False).clamp(0, 1) * 2 - 1
    gt = big[:, :, 8:8 + P, 8:8 + P].contiguous()
    sr = (F.avg_pool2d(F.pad(gt, (2, 2, 2, 2), mode="reflect"), 5, 1) + 0.05 * torch.randn(B, 3, P, P, generator=gen)).clamp(-1, 1)
    offs = torch.randint(0, 17, (R, 2), generator=gen)
    refs = torch.stack([big[:, :, int(oy):int(oy) + P, int(ox):int(ox) + P] for oy, ox in offs], 1).contiguous()
    tr = refine.RefineTrainer(refine.make_refine_state_dict(7), lr=5e-4, precision=a.precision, weight_grad=a.weight_grad,
                              refine_with_ssim=a.ssim is not None, lambda_refine_ssim=1.0 if a.ssim is None else a.ssim)
    tr.set_input({"sr_patch": sr, "ref_patches": refs, "gt_patch": gt})
    t0 = time.time()
    grad_loss = losses.GradientLoss()
    for it in range(1, a.iters + 1):
        if a.grad_loss is None:
            tr.optimize_parameters()
        else:                                  # optimize_parameters with one more term: forward_train, the losses, one backward
            tr.forward()
            tr.calculate_losses()
            loss_grad = grad_loss(tr.pred, tr.data_gt_patch)
            for p in tr.params.values():
                p.grad = None
            (tr.loss_tot + a.grad_loss * loss_grad).backward()
            tr.optimizer_step()
            loss_grad = loss_grad.detach()
        if it == 1 or it % 25 == 0:
            ssim = f"  1-SSIM {float(tr.loss_ssim) / a.ssim:.4f}" if a.ssim else ""
            ssim += f"  grad {float(loss_grad):.4f}" if a.grad_loss is not None else ""
            print(f"iter {it:4d}  L1 {float(tr.loss_l1):.4f}{ssim}  PSNR in {float(tr.loss_psnr_input):.2f} dB -> out {float(tr.loss_psnr_refine):.2f} dB")
    torch.cuda.synchronize()
    print(f"{a.iters} iterations in {time.time() - t0:.1f} s")
    y = tr.eval_model()(sr.cuda(), refs.cuda())          # eval mode: BatchNorm on the running statistics the training moved
    print(f"eval-mode PSNR {float(-10 * torch.log10(torch.mean((y - gt.cuda()) ** 2))):.2f} dB")


if __name__ == "__main__":
    main()
