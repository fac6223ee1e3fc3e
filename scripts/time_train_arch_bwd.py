#!/usr/bin/env python3
"""Step time of the layer-by-layer training pair under precision f16x3_gemm_bwd (every gradient product on the split-fp16 MFMA,
csrc/nsr_train_bwd_f16.hip) against f16x3_gemm and fp32, on the three networks and at the shape of scripts/time_train_arch.py
(2,048 rays = 512 LR pixels x 4 sub-rays, 64 + 64 samples, randomized sampling, density noise 1, one chunk):

    default  8 x 256, skip 4, degrees 10 / 4 (through the descriptor route)
    odd      6 x 192, skips (1, 3), degrees 10 / 4
    small    4 x 128, skip (2), degrees 6 / 2

A step is  Trainer.forward() -> MSE of the s^2 means in torch -> Trainer.backward() -> Trainer.optimizer_step().  All nine
variants run interleaved in one process: `--repeats` (5) alternating runs of `--block` steps each, every block timed with device
events.  The gate (the project's yardstick form): on `odd`, the median step of f16x3_gemm_bwd lies below the median of f16x3_gemm
by more than three times the spread (max - min) of f16x3_gemm's repeats; the same comparison is recorded for the other two.

    python scripts/time_train_arch_bwd.py --out profiles/train_arch_bwd_timing.json
    python scripts/time_train_arch_bwd.py --only odd_f16x3_gemm_bwd --repeats 1      # e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import cameras, ops  # noqa: E402
from nerf_sr_amd import train as nsr_train  # noqa: E402
from nerf_sr_amd.weights import make_state_dict_arch  # noqa: E402

NETWORKS = {"default": {"D": 8, "W": 256, "skips": (4,), "deg_pos": 10, "deg_dir": 4},
            "odd": {"D": 6, "W": 192, "skips": (1, 3), "deg_pos": 10, "deg_dir": 4},
            "small": {"D": 4, "W": 128, "skips": (2,), "deg_pos": 6, "deg_dir": 2}}
PRECISIONS = ("f16x3_gemm_bwd", "f16x3_gemm", "fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=20, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variant names <network>_<precision> (default: all)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    R, s2 = a.rays - a.rays % 4, 4
    frame = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, device=dev)
    torch.manual_seed(1234)
    sel = torch.randperm(frame.shape[0], device=dev)[: R // s2]
    rays, target = frame[sel].reshape(-1, 8).contiguous(), torch.rand(R // s2, 3, device=dev)
    mse = torch.nn.functional.mse_loss

    def step_of(arch, prec):
        t = nsr_train.Trainer(make_state_dict_arch(21, **arch), make_state_dict_arch(22, **arch), arch=arch, randomized=True,
                              noise_std=1.0, downscale=2, ray_chunk=R, precision=prec, device=dev)
        t.set_input(rays, target)

        def step():
            out = t.forward()
            lr_c = out["coarse_comp_rgbs"].reshape(-1, s2, 3).mean(1)
            lr_f = out["fine_comp_rgbs"].reshape(-1, s2, 3).mean(1)
            t.backward(mse(lr_c, t.data_rgbs) * t.lambda_coarse + mse(lr_f, t.data_rgbs) * t.lambda_fine)
            t.all_reduce_grads()
            t.optimizer_step()
        return step

    only = [s for s in a.only.split(",") if s]
    variants = {f"{n}_{p}": step_of(arch, p) for n, arch in NETWORKS.items() for p in PRECISIONS if not only or f"{n}_{p}" in only}
    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(a.repeats):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.block):
                f()
            e1.record()
            e1.synchronize()
            runs[name].append(e0.elapsed_time(e1) / a.block)
    med = {k: statistics.median(v) for k, v in runs.items()}
    res = {"shape": f"{R} rays ({R // s2} LR pixels x {s2}), 64 + 64 samples, randomized, noise_std 1, one chunk; "
                    f"{a.repeats} alternating runs of {a.block} steps, device events",
           "device": torch.cuda.get_device_name(dev),
           "variants": {k: {"ms_per_step_median": round(med[k], 4), "ms_per_step_runs": [round(x, 4) for x in runs[k]]} for k in variants},
           "comparison": {}}
    for n in NETWORKS:
        new, old, f32 = f"{n}_f16x3_gemm_bwd", f"{n}_f16x3_gemm", f"{n}_fp32"
        if new in runs and old in runs:
            spread = max(runs[old]) - min(runs[old])
            c = {"f16x3_gemm_bwd_ms": round(med[new], 4), "f16x3_gemm_ms": round(med[old], 4), "f16x3_gemm_spread_ms": round(spread, 4),
                 "gain_ms": round(med[old] - med[new], 4), "ratio_f16x3_gemm_over_bwd": round(med[old] / med[new], 4),
                 "below_by_more_than_3_spreads": bool(med[old] - med[new] > 3.0 * spread)}
            if f32 in runs:
                c["fp32_ms"] = round(med[f32], 4)
            res["comparison"][n] = c
    if "odd" in res["comparison"]:
        res["gate"] = {"network": "odd (6 x 192, skips (1, 3))", "met": res["comparison"]["odd"]["below_by_more_than_3_spreads"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
