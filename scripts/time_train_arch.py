#!/usr/bin/env python3
"""Cost of one training step through the layer-by-layer pair for any architecture (nsr_train_arch_forward / _backward,
nsr_adam_step_n) against the default network's own GEMM-path pair, at the bench's training shape (2,048 rays = 512 LR pixels
x 4 sub-rays, 64 + 64 samples, randomized sampling, density noise 1, one chunk).

A step of every variant is  Trainer.forward() -> MSE of the s^2 means in torch -> Trainer.backward() -> Trainer.optimizer_step().

    default_pair_*   the default network (8 x 256, skip 4, degrees 10 / 4) through nsr_train_forward / nsr_train_backward
    arch_default_*   the same network through the descriptor route
    arch_odd_*       6 x 192, skips (1, 3), degrees 10 / 4
    arch_small_*     4 x 128, skip (2), degrees 6 / 2

at precision f16x3_gemm and fp32.  All variants run interleaved in one process: `--repeats` (5) alternating runs of `--block`
steps each, every block timed by wall clock around a device synchronisation.  The yardstick (the margin of 0430cfd): the
descriptor route on the default network should cost no more than the default pair plus three times the spread (max - min)
of the default pair's repeats.  Also reported: ms per algorithmic FLOP (6 x the weight-matrix elements per sample point:
forward, input gradient and weight gradient) relative to the first variant.  Prints one JSON object (also written to --out).

    python scripts/time_train_arch.py --out profiles/train_arch_timing.json
    python scripts/time_train_arch.py --only arch_default_f16x3_gemm --repeats 1      # e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import cameras, ops  # noqa: E402
from nerf_sr_amd import train as nsr_train  # noqa: E402
from nerf_sr_amd.weights import arch_spec, make_state_dict, make_state_dict_arch  # noqa: E402

DEFAULT = {"D": 8, "W": 256, "skips": (4,), "deg_pos": 10, "deg_dir": 4}
ODD = {"D": 6, "W": 192, "skips": (1, 3), "deg_pos": 10, "deg_dir": 4}
SMALL = {"D": 4, "W": 128, "skips": (2,), "deg_pos": 6, "deg_dir": 2}


def macs_per_point(arch):
    return sum(int(np.prod(s)) for k, s in arch_spec(**arch).items() if k.endswith("weight"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=20, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variant names (default: all)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    R, s2 = a.rays - a.rays % 4, 4
    frame = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, device=dev)
    torch.manual_seed(1234)
    sel = torch.randperm(frame.shape[0], device=dev)[: R // s2]
    rays, target = frame[sel].reshape(-1, 8).contiguous(), torch.rand(R // s2, 3, device=dev)
    mse = torch.nn.functional.mse_loss

    def trainer(arch, prec, through_arch):
        kw = dict(randomized=True, noise_std=1.0, downscale=2, ray_chunk=R, precision=prec, device=dev)
        if through_arch:
            t = nsr_train.Trainer(make_state_dict_arch(21, **arch), make_state_dict_arch(22, **arch), arch=arch, **kw)
        else:
            t = nsr_train.Trainer(make_state_dict(99), make_state_dict(100), **kw)
        t.set_input(rays, target)
        return t

    def step_of(t):
        def step():
            out = t.forward()
            lr_c = out["coarse_comp_rgbs"].reshape(-1, s2, 3).mean(1)
            lr_f = out["fine_comp_rgbs"].reshape(-1, s2, 3).mean(1)
            t.backward(mse(lr_c, t.data_rgbs) * t.lambda_coarse + mse(lr_f, t.data_rgbs) * t.lambda_fine)
            t.all_reduce_grads()
            t.optimizer_step()
        return step

    plan = []
    for prec in ("f16x3_gemm", "fp32"):
        plan.append((f"default_pair_{prec}", DEFAULT, prec, False))
    for name, arch in (("default", DEFAULT), ("odd", ODD), ("small", SMALL)):
        for prec in ("f16x3_gemm", "fp32"):
            plan.append((f"arch_{name}_{prec}", arch, prec, True))
    only = [s for s in a.only.split(",") if s]
    plan = [p for p in plan if not only or p[0] in only]
    variants, flops = {}, {}
    for name, arch, prec, through in plan:
        variants[name] = step_of(trainer(arch, prec, through))
        flops[name] = 6 * macs_per_point(arch)
    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(a.repeats):
        for name, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.block):
                f()
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0) * 1e3 / a.block)
    med = {k: statistics.median(v) for k, v in runs.items()}
    first = next(iter(variants))
    res = {"shape": f"{R} rays ({R // s2} LR pixels x {s2}), 64 + 64 samples, randomized, noise_std 1, one chunk; "
                    f"{a.repeats} alternating runs of {a.block} steps",
           "device": torch.cuda.get_device_name(dev), "variants": {}}
    for k in variants:
        res["variants"][k] = {"ms_per_step_median": round(med[k], 4), "ms_per_step_runs": [round(x, 4) for x in runs[k]],
                              "algorithmic_flop_per_point": flops[k],
                              "ms_per_flop_relative_to_first": round((med[k] / flops[k]) / (med[first] / flops[first]), 4)}
    res["yardstick"] = {}
    for prec in ("f16x3_gemm", "fp32"):
        ref, new = f"default_pair_{prec}", f"arch_default_{prec}"
        if ref in runs and new in runs:
            spread = max(runs[ref]) - min(runs[ref])
            bound = med[ref] + 3.0 * spread
            res["yardstick"][prec] = {"default_pair_ms": round(med[ref], 4), "spread_ms": round(spread, 4), "bound_ms": round(bound, 4),
                                      "arch_default_ms": round(med[new], 4), "met": bool(med[new] <= bound)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
