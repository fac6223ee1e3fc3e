#!/usr/bin/env python3
"""Cost of SSIM as a loss: forward + backward of the `mean` SSIM (11 x 11 Gaussian window) with respect to `output`, on one
1008 x 756 x 3 frame, one 800 x 800 x 3 frame and a 32 x 3 x 64 x 64 patch batch:

    ours    nerf_sr_amd.metrics.SSIM under autograd (nsr_ssim + nsr_ssim_backward: double arithmetic, no workspace)
    torch   autograd through the restatement tests/metrics_ref.py on the same device in fp32 -- torch-ROCm's own pad, cat,
            depthwise conv2d, elementwise passes and their backward kernels, what the reference's class runs as a loss

`--repeats` (5) alternating runs of `--block` forward + backward pairs each, every block timed by a pair of device events;
peak extra memory = torch.cuda.max_memory_allocated above what is resident before the pair, per side.  Also the distance of
both gradients from fp64 autograd of the restatement on the device.  Recorded, not gated.  Prints one JSON object (also
written to --out).

    python scripts/time_ssim_backward.py --out profiles/ssim_backward_timing.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import metrics  # noqa: E402
from tests import metrics_ref as ref  # noqa: E402

SHAPES = {"1008x756x3": (1, 3, 756, 1008), "800x800x3": (1, 3, 800, 800), "32x3x64x64": (32, 3, 64, 64)}


def pair(fn, x, y):
    x.grad = None
    fn(x, y).backward()
    return x.grad


def measure(variants, x, y, repeats, block, warmup, dev):
    runs, peaks = {k: [] for k in variants}, {}
    for name, fn in variants.items():
        for _ in range(warmup):
            pair(fn, x, y)
        x.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        pair(fn, x, y)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev) - base
    for _ in range(repeats):
        for name, fn in variants.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(block):
                pair(fn, x, y)
            stop.record()
            stop.synchronize()
            runs[name].append(start.elapsed_time(stop) * 1e3 / block)
    out = {name: {"us_per_pair_median": round(statistics.median(v), 1), "us_per_pair_runs": [round(t, 1) for t in v],
                  "spread_us": round(max(v) - min(v), 1), "peak_extra_memory_mb": round(peaks[name] / 1e6, 2)}
           for name, v in runs.items()}
    out["ours_over_torch"] = round(out["ours"]["us_per_pair_median"] / out["torch"]["us_per_pair_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=200, help="forward + backward pairs per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ssim_backward.py needs a GPU")
    dev = torch.device("cuda", 0)
    ssim = metrics.SSIM(data_range=(0, 1))
    res = {"what": f"forward + backward of mean SSIM w.r.t. output, fp32 (B, C, H, W) inputs, 11 x 11 Gaussian window, data_range (0, 1); "
                   f"{a.repeats} alternating runs of {a.block} pairs after {a.warmup} warm-up pairs, device events around each block "
                   "(one pair = enqueue to completion amortised over the block, no host read per pair)",
           "device": torch.cuda.get_device_name(dev), "shapes": {}}
    gen = torch.Generator().manual_seed(3)
    variants = {"ours": lambda x, y: ssim(x, y), "torch": lambda x, y: ref.ssim(x, y, reduction="mean")}
    for tag, shape in SHAPES.items():
        x = torch.rand(shape, generator=gen).to(dev)
        y = (x + 0.05 * torch.randn(shape, generator=gen).to(dev)).clamp(0, 1)
        x.requires_grad_(True)
        r = measure(variants, x, y, a.repeats, a.block, a.warmup, dev)
        x64 = x.detach().double().requires_grad_(True)
        g64 = pair(lambda p, q: ref.ssim(p, q, reduction="mean"), x64, y.double())
        for name, fn in variants.items():
            g = pair(fn, x, y).double()
            r[name]["grad_distance_from_fp64_over_max"] = float((g - g64).abs().max() / g64.abs().max())
        x.grad = None
        # what the backward adds: the same blocks of the forward alone (no grad), per side
        xd = x.detach()
        for name, fn in variants.items():
            ts = []
            for _ in range(a.repeats):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                for _ in range(a.block):
                    fn(xd, y)
                stop.record()
                stop.synchronize()
                ts.append(start.elapsed_time(stop) * 1e3 / a.block)
            r[name]["us_forward_only_median"] = round(statistics.median(ts), 1)
        res["shapes"][tag] = r
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
