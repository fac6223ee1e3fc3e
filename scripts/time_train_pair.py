#!/usr/bin/env python3
"""Cost of the autograd pair against the fused training step, at the bench's training shape (2,048 rays = 512 LR pixels x 4
sub-rays, 64 + 64 samples, randomized sampling, density noise 1, precision 'f16x3', one chunk).

    fused: Trainer.optimize_parameters()                       (nsr_train_loss_and_grads + nsr_adam_step)
    pair:  Trainer.forward() -> MSE of the s^2 means in torch -> Trainer.backward() -> Trainer.optimizer_step()

Both on the same batch and the same trainer state, interleaved in one process (blocks of `--block` steps, alternating), each
block timed by wall clock around a device synchronisation.  Prints one JSON object (also written to --out).

    python scripts/time_train_pair.py --steps 200 --out profiles/train_pair_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import _lib, cameras, ops  # noqa: E402
from nerf_sr_amd import train as nsr_train  # noqa: E402
from nerf_sr_amd.weights import make_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=200, help="timed steps per variant")
    ap.add_argument("--block", type=int, default=10, help="steps per timed block; the variants alternate block by block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    R, s2 = a.rays - a.rays % 4, 4
    t = nsr_train.Trainer(make_state_dict(99), make_state_dict(100), randomized=True, noise_std=1.0, downscale=2, ray_chunk=R,
                          precision=a.precision, device=dev)
    frame = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, device=dev)
    torch.manual_seed(1234)
    sel = torch.randperm(frame.shape[0], device=dev)[: R // s2]
    t.set_input(frame[sel].reshape(-1, 8).contiguous(), torch.rand(R // s2, 3, device=dev))
    mse = torch.nn.functional.mse_loss

    def fused():
        t.optimize_parameters()

    def pair():
        out = t.forward()
        lr_c = out["coarse_comp_rgbs"].reshape(-1, s2, 3).mean(1)
        lr_f = out["fine_comp_rgbs"].reshape(-1, s2, 3).mean(1)
        t.backward(mse(lr_c, t.data_rgbs) * t.lambda_coarse + mse(lr_f, t.data_rgbs) * t.lambda_fine)
        t.all_reduce_grads()
        t.optimizer_step()

    variants = {"fused": fused, "pair": pair}
    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    per_step = {k: [] for k in variants}
    for _ in range(max(1, a.steps // a.block)):
        for name, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.block):
                f()
            torch.cuda.synchronize()
            per_step[name].append((time.perf_counter() - t0) * 1e3 / a.block)
    lib = _lib.load()
    prec = _lib.TRAIN_PRECISIONS[a.precision]
    med = {k: statistics.median(v) for k, v in per_step.items()}
    res = {"shape": f"{R} rays ({R // s2} LR pixels x {s2}), 64 + 64 samples, randomized, noise_std 1, one chunk",
           "precision": a.precision, "device": torch.cuda.get_device_name(dev),
           "fused_ms_per_step_median": round(med["fused"], 4), "pair_ms_per_step_median": round(med["pair"], 4),
           "pair_over_fused": round(med["pair"] / med["fused"], 4),
           "fused_ms_blocks": [round(x, 4) for x in per_step["fused"]], "pair_ms_blocks": [round(x, 4) for x in per_step["pair"]],
           "saved_state_bytes": int(lib.nsr_train_saved_bytes(prec, R, 64, 64, R)),
           "workspace_bytes": int(lib.nsr_train_workspace_bytes_for(prec, R, 64, 64)),
           "peak_memory_bytes": int(torch.cuda.max_memory_allocated(dev)), "status": t.status()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
