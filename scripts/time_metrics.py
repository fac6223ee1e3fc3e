#!/usr/bin/env python3
"""Cost of scoring one frame: SSIM (11 x 11 Gaussian window) and PSNR of an (1, 3, H, W) fp32 frame against ground truth, on
one 1008 x 756 and one 800 x 800 frame:

    ours    nerf_sr_amd.metrics.SSIM / PSNR (nsr_ssim, nsr_psnr: one kernel + a fixed-order reduction each, sums in double)
    torch   the restatement tests/metrics_ref.py on the GPU in fp32 -- torch-ROCm's own pad, cat, depthwise conv2d and
            elementwise passes, the composition the reference runs

`--repeats` (5) alternating runs of `--block` calls each, every block timed by wall clock around a device synchronisation;
peak extra memory = torch.cuda.max_memory_allocated above what the two frames occupy, per side.  Recorded, not gated.
Prints one JSON object (also written to --out).

    python scripts/time_metrics.py --out profiles/metrics_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import metrics  # noqa: E402
from tests import metrics_ref as ref  # noqa: E402

FRAMES = {"1008x756": (756, 1008), "800x800": (800, 800)}


def measure(variants, repeats, block, warmup, dev):
    """{name: {metric: fn}} -> per name and metric: alternating timed blocks, and the peak memory above the resident tensors."""
    out = {}
    for metric in next(iter(variants.values())):
        runs, peaks = {k: [] for k in variants}, {}
        for name, fns in variants.items():
            for _ in range(warmup):
                fns[metric]()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            fns[metric]()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated(dev) - base
        for _ in range(repeats):
            for name, fns in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(block):
                    fns[metric]()
                torch.cuda.synchronize()
                runs[name].append((time.perf_counter() - t0) * 1e6 / block)
        out[metric] = {name: {"us_per_call_median": round(statistics.median(v), 1), "us_per_call_runs": [round(t, 1) for t in v],
                              "spread_us": round(max(v) - min(v), 1), "peak_extra_memory_mb": round(peaks[name] / 1e6, 2)}
                       for name, v in runs.items()}
        out[metric]["ours_over_torch"] = round(out[metric]["ours"]["us_per_call_median"] / out[metric]["torch"]["us_per_call_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=200, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ssim, psnr = metrics.SSIM(data_range=(0, 1)), metrics.PSNR()
    res = {"shape": f"(1, 3, H, W) fp32 frames, SSIM 11 x 11 Gaussian window, data_range (0, 1); {a.repeats} alternating runs of "
                    f"{a.block} calls after {a.warmup} warm-up calls; one call = one score of one frame, enqueue to completion amortised "
                    "over the block (no host read per call)",
           "device": torch.cuda.get_device_name(dev), "frames": {}}
    gen = torch.Generator().manual_seed(3)
    for tag, (H, W) in FRAMES.items():
        x = torch.rand(1, 3, H, W, generator=gen).to(dev)
        y = (x + 0.05 * torch.randn(1, 3, H, W, generator=gen).to(dev)).clamp(0, 1)
        variants = {"ours": {"ssim": lambda: ssim(x, y), "psnr": lambda: psnr(x, y)},
                    "torch": {"ssim": lambda: ref.ssim(x, y, reduction="mean"), "psnr": lambda: ref.psnr(x, y)}}
        r = measure(variants, a.repeats, a.block, a.warmup, dev)
        r["ssim"]["abs_difference"] = abs(float(ssim(x, y)) - float(ref.ssim(x.double(), y.double(), reduction="mean")))
        r["ssim"]["torch_fp32_vs_fp64"] = abs(float(ref.ssim(x, y, reduction="mean")) - float(ref.ssim(x.double(), y.double(), reduction="mean")))
        res["frames"][tag] = r
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
