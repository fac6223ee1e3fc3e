#!/usr/bin/env python3
"""Cost of producing one refinement training batch, in one process on one MI355X:

    sample   nerf_sr_amd.refine_data.RefinePatchSet.sample: one torch.randint of position words + one launch
             (nsr_refine_patch_batch) from the two 8-bit images and the coefficient / box tables
    batch    RefinePatchSet.batch at positions given up front: the launch alone
    sliced   the reference's layout kept on the device: gt_pspc_imgs / sr_pspc_imgs materialised as fp32 (aug_num, 3, H, W)
             stacks, every patch a torch slice at the same positions (host integers, as the reference's __getitem__ has them),
             torch.stack per sample and per batch

Set: one 504 x 378 image pair, 200 augmentations, patch_len 64, 8 reference patches, batch 32.  `--repeats` (5) alternating
runs of `--block` batches each, every run timed with device events around the block.  Resident bytes of both layouts are
derived from the shapes.  Recorded, not gated.  Prints one JSON object (also written to --out).

    python scripts/time_refine_batches.py --out profiles/refine_batches_timing.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from nerf_sr_amd.refine_data import RefinePatchSet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wh", type=int, nargs=2, default=(504, 378))
    ap.add_argument("--aug-num", type=int, default=200)
    ap.add_argument("--patch-len", type=int, default=64)
    ap.add_argument("--num-ref", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = a.wh
    P, R, B = a.patch_len, a.num_ref, a.batch
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.clip(np.stack([127 + 100 * np.sin(xx / 31.0), (xx + yy) % 240, 255 - (xx // 16 + yy // 12) % 240], -1)
                 + rng.integers(-10, 11, (H, W, 3)), 16, 255).astype(np.uint8)
    sr = np.clip(gt.astype(np.int64) + rng.integers(-12, 13, (H, W, 3)), 16, 255).astype(np.uint8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ps = RefinePatchSet(gt, sr, patch_len=P, num_ref_patches=R, ref_offset=64, aug_num=a.aug_num, generator=torch.Generator().manual_seed(0))
    e1.record()
    e1.synchronize()
    setup_ms = e0.elapsed_time(e1)
    # the reference's layout, built once by the set itself (bit-identical images)
    gt_stack = torch.stack([ps.warped_image(k, "gt") for k in range(ps.aug_num)])
    sr_stack = torch.stack([ps.warped_image(k, "sr") for k in range(ps.aug_num)])
    gt_img = gt_stack[0]
    gen = torch.Generator(device="cuda").manual_seed(0)
    idx = [torch.arange(k * B, (k + 1) * B, device="cuda") for k in range(a.block)]
    drawn = [ps.sample(i, gen) for i in idx]
    assert ps.status() == 0
    aug = [d["aug_idx"] for d in drawn]
    starts = [d["starts"] for d in drawn]
    aug_h = [t.tolist() for t in aug]
    starts_h = [t.tolist() for t in starts]
    del drawn

    def sliced(k):
        srs, gts, refs = [], [], []
        for m, s in zip(aug_h[k], starts_h[k]):
            x, y = s[0], s[1]
            srs.append(sr_stack[m][:, y:y + P, x:x + P])
            gts.append(gt_stack[m][:, y:y + P, x:x + P])
            refs.append(torch.stack([gt_img[:, s[3 + 2 * j]:s[3 + 2 * j] + P, s[2 + 2 * j]:s[2 + 2 * j] + P] for j in range(R)], 0))
        return {"sr_patch": torch.stack(srs), "gt_patch": torch.stack(gts), "ref_patches": torch.stack(refs)}

    routes = {"sample": lambda k: ps.sample(idx[k], gen), "batch": lambda k: ps.batch(aug[k], starts[k]), "sliced": sliced}
    p, q = routes["batch"](0), sliced(0)
    same = all(bool(torch.equal(p[k], q[k])) for k in ("sr_patch", "gt_patch", "ref_patches"))
    runs = {k: [] for k in routes}
    for fn in routes.values():
        for k in range(a.warmup):
            fn(k)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, fn in routes.items():
            e0.record()
            for k in range(a.block):
                fn(k)
            e1.record()
            e1.synchronize()
            runs[name].append(e0.elapsed_time(e1) * 1e3 / a.block)
    med = {k: statistics.median(v) for k, v in runs.items()}
    out_bytes = B * (2 + R) * 3 * P * P * 4
    res = {"set": f"one {W} x {H} image pair, {ps.aug_num} augmentations, patch_len {P}, {R} reference patches, batch {B}; {a.repeats} "
                  f"alternating runs of {a.block} batches after {a.warmup} warm-up batches, device events around each run "
                  "(host enqueue time included: a run ends when its last batch is complete)",
           "device": torch.cuda.get_device_name(0), "batches_bit_identical": same,
           "us_per_batch": {k: {"median": round(med[k], 2), "runs": [round(t, 2) for t in v], "spread": round(max(v) - min(v), 2)}
                            for k, v in runs.items()},
           "sample_over_sliced": round(med["sample"] / med["sliced"], 4),
           "bytes_written_per_batch": out_bytes,
           "batch_route_achieved_write_GBps": round(out_bytes / (med["batch"] * 1e-6) / 1e9, 3),
           "setup_ms (tables + nsr_refine_aug_bbox, first call included)": round(setup_ms, 2),
           "resident_bytes": {"patch set (two u8 images + coefficient and box tables)": ps.resident_bytes(),
                              "materialised (fp32 gt / sr stacks)": int(gt_stack.numel() + sr_stack.numel()) * 4}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
