#!/usr/bin/env python3
"""Cost of one training iteration of the refinement network (forward -> torch L1 -> backward -> Adam) at the reference's
batch (scripts/train_llff_refine.sh: 32 patch sets of 1 + 8 patches, 64 x 64), fp32:

    ours    nerf_sr_amd.refine.RefineTrainer.optimize_parameters (nsr_refine_train_forward / _backward, nsr_adam_step_n)
    torch   the restatement tests/refine_train_ref.py on the GPU in fp32 -- torch-ROCm's own convolutions, BatchNorm and
            autograd -- with torch.optim.Adam

`--repeats` (5) alternating runs of `--block` iterations each, every block timed by wall clock around a device
synchronisation.  Recorded, not gated: nobody had measured either number.  Prints one JSON object (also written to --out).

    python scripts/time_refine_train.py --out profiles/refine_train_timing.json
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_refine_train.py --only ours --repeats 1 --block 3
"""
import argparse
import json
import os
import statistics
import sys
import time
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import refine  # noqa: E402
from tests import refine_train_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--refs", type=int, default=8)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=3, help="iterations per timed block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="'ours' or 'torch' (default: both, alternating)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, R, P = a.batch, a.refs, a.patch
    gen = torch.Generator().manual_seed(3)
    x = (torch.rand(B, 3, P, P, generator=gen) * 2 - 1).to(dev)
    c = (torch.rand(B, R, 3, P, P, generator=gen) * 2 - 1).to(dev)
    gt = (torch.rand(B, 3, P, P, generator=gen) * 2 - 1).to(dev)
    sd = refine.make_refine_state_dict(7)
    variants = {}
    if a.only in ("", "ours"):
        tr = refine.RefineTrainer(sd, lr=5e-4, device=dev)
        tr.set_input({"sr_patch": x, "ref_patches": c, "gt_patch": gt})
        variants["ours"] = tr.optimize_parameters
    if a.only in ("", "torch"):
        tsd = OrderedDict((k, torch.from_numpy(v).to(dev)) for k, v in sd.items())
        leaves = [tsd[k].requires_grad_(True) for k in refine.TRAIN_PARAM_KEYS]
        opt = torch.optim.Adam(leaves, lr=5e-4, betas=(0.9, 0.999))

        def torch_step():
            y, running = ref.forward_train(tsd, x, c)
            opt.zero_grad()
            torch.nn.functional.l1_loss(y, gt).backward()
            opt.step()
            for k, v in running.items():        # the module's in-place buffer update
                tsd[k] = v
        variants["torch"] = torch_step
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
    res = {"shape": f"B = {B} patch sets, R = {R} references, {P} x {P}, fp32; forward -> L1 -> backward -> Adam; "
                    f"{a.repeats} alternating runs of {a.block} iterations after {a.warmup} warm-up iterations",
           "device": torch.cuda.get_device_name(dev), "conv_gmacs_forward": round(B * refine.refine_macs(P, P, R) / 1e9, 1),
           "peak_memory_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2), "variants": {}}
    for k, v in runs.items():
        res["variants"][k] = {"ms_per_iteration_median": round(statistics.median(v), 2), "ms_per_iteration_runs": [round(t, 2) for t in v],
                              "spread_ms": round(max(v) - min(v), 2)}
    if len(runs) == 2:
        res["ours_over_torch"] = round(statistics.median(runs["ours"]) / statistics.median(runs["torch"]), 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
