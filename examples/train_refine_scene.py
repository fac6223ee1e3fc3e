#!/usr/bin/env python3
"""Train the refinement network from an image pair with nothing on the host (needs an MI355X): a synthetic "ground truth"
image and its blurred, noised "synthesised" twin go to the device as bytes once; every batch -- perspective-warped sr / gt
patches and the reference patches around them -- is produced there by RefinePatchSet.sample and fed to RefineTrainer, the
shape of the reference's protocol (scripts/train_llff_refine.sh: 200 augmentations, 1 + 8 patches of 64 x 64, L1, Adam at
5e-4).  Real images: RefinePatchSet.from_files(gt_path, sr_path, img_wh).

    python examples/train_refine_scene.py [--iters 200] [--batch 4] [--wh 504 378]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_sr_amd import refine  # noqa: E402
from nerf_sr_amd.refine_data import RefinePatchSet  # noqa: E402


def synthetic_pair(W, H, seed=0):
    from PIL import Image, ImageFilter
    rng = np.random.default_rng(seed)
    gt = Image.fromarray(rng.integers(16, 256, (H // 12, W // 12, 3), dtype=np.uint8)).resize((W, H), Image.BICUBIC)
    sr = np.asarray(gt.filter(ImageFilter.GaussianBlur(2.0)), dtype=np.int16) + rng.integers(-8, 9, (H, W, 3))
    return np.maximum(np.asarray(gt, dtype=np.uint8), 16), np.clip(sr, 16, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--wh", type=int, nargs=2, default=(504, 378))
    ap.add_argument("--aug-num", type=int, default=200)
    ap.add_argument("--with-gt-patch", action="store_true")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "f16x3_mixed"),
                    help="f16x3_mixed: forward and input gradients on the split-fp16 MFMA")
    ap.add_argument("--weight-grad", default="fp32", choices=("fp32", "f16x3"),
                    help="f16x3: the weight gradients as one implicit split-fp16 GEMM per layer (fp32: im2col + fp32 GEMM)")
    a = ap.parse_args()
    gt, sr = synthetic_pair(*a.wh)
    ps = RefinePatchSet(gt, sr, patch_len=64, num_ref_patches=8, ref_offset=64, with_gt_patch=a.with_gt_patch, aug_num=a.aug_num,
                        generator=torch.Generator().manual_seed(0))
    print(f"patch set: {ps.aug_num} augmentations of {a.wh[0]} x {a.wh[1]}, {ps.resident_bytes() / 1e6:.2f} MB resident "
          f"(the reference's fp32 stacks: {2 * ps.aug_num * 3 * a.wh[0] * a.wh[1] * 4 / 1e6:.0f} MB)")
    tr = refine.RefineTrainer(refine.make_refine_state_dict(7), lr=5e-4, precision=a.precision, weight_grad=a.weight_grad)
    gen = torch.Generator(device="cuda").manual_seed(1)
    t0, it = time.time(), 0
    for batch in ps.epoch(a.batch, a.iters * a.batch, gen):
        it += 1
        tr.set_input(batch)
        tr.optimize_parameters()
        if it == 1 or it % 25 == 0:
            print(f"iter {it:4d}  L1 {float(tr.loss_l1.detach()):.4f}  PSNR in {float(tr.loss_psnr_input):.2f} dB -> out {float(tr.loss_psnr_refine):.2f} dB")
    torch.cuda.synchronize()
    print(f"{it} iterations in {time.time() - t0:.1f} s; status word {ps.status()}")


if __name__ == "__main__":
    main()
