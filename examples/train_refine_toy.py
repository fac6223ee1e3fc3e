#!/usr/bin/env python3
"""Overfit the refinement network on ONE synthetic patch batch (needs an MI355X): the "ground truth" is a smooth random
pattern, the synthesised patch is that pattern blurred and noised, the reference patches are shifted crops of the ground
truth -- the shape of the reference's protocol (scripts/train_llff_refine.sh: patch sets of 1 + 8 patches at 64 x 64, L1
loss, Adam at 5e-4) without its dataset.  The loop is the reference's train.py: set_input -> optimize_parameters.

    python examples/train_refine_toy.py [--iters 200] [--batch 4] [--ssim LAMBDA]

--ssim LAMBDA adds LAMBDA * (1 - SSIM) to the L1 loss (RefineTrainer's refine_with_ssim: the device SSIM under autograd).
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_sr_amd import refine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ssim", type=float, default=None, metavar="LAMBDA", help="add LAMBDA * (1 - SSIM) to the loss")
    a = ap.parse_args()
    B, R, P = a.batch, 8, 64
    gen = torch.Generator().manual_seed(0)
    big = F.interpolate(torch.rand(B, 3, 12, 12, generator=gen), size=(P + 16, P + 16), mode="bicubic", align_corners=False).clamp(0, 1) * 2 - 1
    gt = big[:, :, 8:8 + P, 8:8 + P].contiguous()
    sr = (F.avg_pool2d(F.pad(gt, (2, 2, 2, 2), mode="reflect"), 5, 1) + 0.05 * torch.randn(B, 3, P, P, generator=gen)).clamp(-1, 1)
    offs = torch.randint(0, 17, (R, 2), generator=gen)
    refs = torch.stack([big[:, :, int(oy):int(oy) + P, int(ox):int(ox) + P] for oy, ox in offs], 1).contiguous()
    tr = refine.RefineTrainer(refine.make_refine_state_dict(7), lr=5e-4, refine_with_ssim=a.ssim is not None,
                              lambda_refine_ssim=1.0 if a.ssim is None else a.ssim)
    tr.set_input({"sr_patch": sr, "ref_patches": refs, "gt_patch": gt})
    t0 = time.time()
    for it in range(1, a.iters + 1):
        tr.optimize_parameters()
        if it == 1 or it % 25 == 0:
            ssim = f"  1-SSIM {float(tr.loss_ssim) / a.ssim:.4f}" if a.ssim else ""
            print(f"iter {it:4d}  L1 {float(tr.loss_l1):.4f}{ssim}  PSNR in {float(tr.loss_psnr_input):.2f} dB -> out {float(tr.loss_psnr_refine):.2f} dB")
    torch.cuda.synchronize()
    print(f"{a.iters} iterations in {time.time() - t0:.1f} s")
    y = tr.eval_model()(sr.cuda(), refs.cuda())          # eval mode: BatchNorm on the running statistics the training moved
    print(f"eval-mode PSNR {float(-10 * torch.log10(torch.mean((y - gt.cuda()) ** 2))):.2f} dB")


if __name__ == "__main__":
    main()
