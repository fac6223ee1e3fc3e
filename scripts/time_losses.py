#!/usr/bin/env python3
"""Cost of the image-space regularisers as losses: forward + backward of each with respect to its first input,

    ours    nerf_sr_amd.losses under autograd (include/nsr_losses.h: two launches forward, one backward, double arithmetic)
    torch   autograd through the same loss written in fp32 torch ops on the same device: train.tv_loss for TV, the
            restatement tests/losses_ref.py for the others -- the slices, pads, elementwise passes, reductions and their
            backward kernels that the reference's classes run

on TV (8, 8, 3) (the --reg_patch patch) and (64, 64, 3), Gradient (32, 3, 64, 64) (the refinement batch), Laplacian and
Bilateral Laplacian (16, 64, 64) with a 3-channel guide.

`--repeats` (5) alternating runs of `--block` (200) forward + backward pairs each, every block timed by a pair of device
events; peak extra memory = torch.cuda.max_memory_allocated above what is resident before the pair, per side.  Also the
distance of both gradients from fp64 autograd of the restatement on the device.  Recorded, not gated.  Prints one JSON object
(also written to --out).

    python scripts/time_losses.py --out profiles/losses_timing.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import losses, train  # noqa: E402
from tests import losses_ref as ref  # noqa: E402


def cases(gen, dev):
    """tag -> (inputs: the first one is differentiated, ours, torch, fp64 oracle)."""
    rnd = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).to(dev)
    tv, grad, lap, bil = losses.TVLoss(), losses.GradientLoss(), losses.LaplacianLoss(), losses.BilateralLaplacianLoss(gamma=0.1)
    bilateral_ref = lambda d, guide: ref.laplacian(d, guide, 0.1)
    return {
        "tv_8x8x3": ([rnd(8, 8, 3)], tv, train.tv_loss, ref.tv),
        "tv_64x64x3": ([rnd(64, 64, 3)], tv, train.tv_loss, ref.tv),
        "gradient_32x3x64x64": ([rnd(32, 3, 64, 64), rnd(32, 3, 64, 64)], grad, ref.gradient, ref.gradient),
        "laplacian_16x64x64": ([rnd(16, 64, 64)], lap, ref.laplacian, ref.laplacian),
        "bilateral_16x64x64_c3": ([rnd(16, 64, 64), rnd(16, 64, 64, 3) * 0.05], bil, bilateral_ref, bilateral_ref),
    }


def pair(fn, inputs):
    inputs[0].grad = None
    fn(*inputs).backward()
    return inputs[0].grad


def timed_blocks(fn, repeats, block):
    ts = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(block):
            fn()
        stop.record()
        stop.synchronize()
        ts.append(start.elapsed_time(stop) * 1e3 / block)
    return ts


def measure(variants, inputs, repeats, block, warmup, dev):
    runs, peaks = {k: [] for k in variants}, {}
    for name, fn in variants.items():
        for _ in range(warmup):
            pair(fn, inputs)
        inputs[0].grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        pair(fn, inputs)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev) - base
    for _ in range(repeats):                       # alternating: ours, torch, ours, torch, ...
        for name, fn in variants.items():
            runs[name] += timed_blocks(lambda: pair(fn, inputs), 1, block)
    out = {name: {"us_per_pair_median": round(statistics.median(v), 1), "us_per_pair_runs": [round(t, 1) for t in v],
                  "spread_us": round(max(v) - min(v), 1), "peak_extra_memory_kb": round(peaks[name] / 1e3, 1)}
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
        raise SystemExit("time_losses.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"what": f"forward + backward of each loss w.r.t. its first input, fp32 inputs in [-1, 1] (guide in [-0.05, 0.05], gamma 0.1); "
                   f"{a.repeats} alternating runs of {a.block} pairs after {a.warmup} warm-up pairs, device events around each block "
                   "(one pair = enqueue to completion amortised over the block, no host read per pair)",
           "device": torch.cuda.get_device_name(dev), "shapes": {}}
    for tag, (inputs, ours, theirs, oracle) in cases(torch.Generator().manual_seed(3), dev).items():
        inputs[0].requires_grad_(True)
        variants = {"ours": ours, "torch": theirs}
        r = measure(variants, inputs, a.repeats, a.block, a.warmup, dev)
        in64 = [t.detach().double() for t in inputs]
        in64[0].requires_grad_(True)
        g64 = pair(oracle, in64)
        for name, fn in variants.items():
            g = pair(fn, inputs).double()
            r[name]["grad_distance_from_fp64_over_max"] = float((g - g64).abs().max() / g64.abs().max())
        inputs[0].grad = None
        # what the backward adds: the same blocks of the forward alone (no grad), per side
        detached = [t.detach() for t in inputs]
        for name, fn in variants.items():
            r[name]["us_forward_only_median"] = round(statistics.median(timed_blocks(lambda: fn(*detached), a.repeats, a.block)), 1)
        res["shapes"][tag] = r
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
