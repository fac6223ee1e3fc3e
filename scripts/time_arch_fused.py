#!/usr/bin/env python3
"""Cost of the fused split-fp16 forward for non-default architectures (ops.GenericMLP(fused=True): nsr_arch_fused_forward, one
launch per chunk) against the layer-by-layer f16x3 route (one nsr_linear_f16x3 launch per nn.Linear) on the same rows.

    P = 262,144 encoded rows (positional encodings of uniform points / unit directions), degrees 10 / 4, one POINT_CHUNK
    networks: 6 x 192 skips (1, 3);  4 x 128 skip (2);  8 x 256 skip (4) through the descriptor
    8 x 256 also: the default fused VanillaMLP (f16x3) on the same rows -> the per-FLOP slowdown of the generic fused kernel
    6 x 192 also: whole config-#2 frames (504 x 378 <- 252 x 189, 64 + 128 samples, eval) through NeRFDownXModel, arch_fused
                  on and off

One process runs every variant: `--repeats` (5) alternating runs, each timed by device events around `--block` forward calls.
The gate (the project's yardstick): on 6 x 192 the fused route's median must beat the layered route's median by more than
three times the spread (max - min) of the layered repeats.  Prints one JSON object (also written to --out).

    python scripts/time_arch_fused.py --out profiles/arch_fused_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import cameras, ops  # noqa: E402
from nerf_sr_amd.model import NeRFDownXModel, default_options  # noqa: E402
from nerf_sr_amd.weights import arch_spec, make_state_dict, make_state_dict_arch  # noqa: E402

NETS = {"6x192": {"D": 6, "W": 192, "skips": (1, 3), "deg_pos": 10, "deg_dir": 4},
        "4x128": {"D": 4, "W": 128, "skips": (2,), "deg_pos": 10, "deg_dir": 4},
        "8x256": {"D": 8, "W": 256, "skips": (4,), "deg_pos": 10, "deg_dir": 4}}


def macs_per_point(arch):
    return sum(int(np.prod(s)) for k, s in arch_spec(**arch).items() if k.endswith("weight"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=10, help="forward calls per timed run")
    ap.add_argument("--no-frames", action="store_true", help="skip the whole-frame runs of the 6 x 192 network")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(7)
    pts = (torch.rand(a.rows, 3, generator=g) * 2 - 1).to(dev)
    dirs = torch.randn(a.rows, 3, generator=g)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).to(dev)
    rows = torch.cat([ops.PositionalEncoding(3, 10)(pts), ops.PositionalEncoding(3, 4)(dirs)], 1).contiguous()

    variants = {}
    for name, arch in NETS.items():
        sd = make_state_dict_arch(99, **arch)
        for route in ("fused", "layered"):
            net = ops.GenericMLP(precision="f16x3", device=dev, fused=route == "fused", **arch).load_state_dict(sd)
            variants[f"{name}_{route}"] = (lambda n=net: n(rows))
    vanilla = ops.VanillaMLP(precision="f16x3", device=dev).load_state_dict(make_state_dict(99))
    variants["8x256_default_kernel"] = lambda: vanilla(rows)
    if not a.no_frames:
        arch = NETS["6x192"]
        frame = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, device=dev).view(-1, 8).contiguous()
        for route in ("fused", "layered"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)        # the slow-path warning is what this figure quantifies
                m = NeRFDownXModel(default_options(precision="f16x3", N_importance=128, arch_fused=route == "fused",
                                                   **{**arch, "skips": list(arch["skips"])}), device=dev)
            m.load_networks(make_state_dict_arch(99, **arch), make_state_dict_arch(100, **arch)).eval()
            variants[f"6x192_frame_{route}"] = (lambda mm=m: mm.forward_rays(frame))

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.no_grad():
        for f in variants.values():          # warm-up: allocator, first launches
            f()
        torch.cuda.synchronize()
        runs = {k: [] for k in variants}
        for _ in range(a.repeats):
            for name, f in variants.items():
                n = 1 if "frame" in name else a.block
                ev[0].record()
                for _ in range(n):
                    f()
                ev[1].record()
                torch.cuda.synchronize()
                runs[name].append(ev[0].elapsed_time(ev[1]) / n)
    med = {k: statistics.median(v) for k, v in runs.items()}
    res = {"shape": f"{a.rows} encoded rows (degrees 10 / 4), precision f16x3; {a.repeats} alternating runs of {a.block} calls, device events; "
                    "frames: config #2 (190,512 rays, 64 + 128 samples, eval), one call per run",
           "device": torch.cuda.get_device_name(dev), "variants": {}}
    for k in variants:
        res["variants"][k] = {"ms_median": round(med[k], 4), "ms_runs": [round(x, 4) for x in runs[k]]}
    for name, arch in NETS.items():
        fl = 2 * macs_per_point(arch)
        for route in ("fused", "layered"):
            v = res["variants"][f"{name}_{route}"]
            v["macs_per_point"] = fl // 2
            v["tflops_algorithmic"] = round(a.rows * fl / (med[f"{name}_{route}"] * 1e-3) / 1e12, 2)
        res["variants"][f"{name}_fused"]["speedup_vs_layered"] = round(med[f"{name}_layered"] / med[f"{name}_fused"], 3)
    res["per_flop_slowdown_vs_default_kernel"] = {
        "what": "8 x 256 skip (4) through the descriptor kernel / the default fused VanillaMLP kernel, same rows, same FLOPs",
        "value": round(med["8x256_fused"] / med["8x256_default_kernel"], 3), "aspiration": 1.5, "gated": False}
    if not a.no_frames:
        res["frame_6x192"] = {"fused_ms": round(med["6x192_frame_fused"], 3), "layered_ms": round(med["6x192_frame_layered"], 3),
                              "fused_rays_per_s": round(190512 / (med["6x192_frame_fused"] * 1e-3)),
                              "layered_rays_per_s": round(190512 / (med["6x192_frame_layered"] * 1e-3)),
                              "speedup": round(med["6x192_frame_layered"] / med["6x192_frame_fused"], 3)}
    lay = runs["6x192_layered"]
    spread = max(lay) - min(lay)
    res["gate"] = {"rule": "6 x 192: fused median < layered median - 3 x (max - min of the layered repeats)",
                   "layered_ms": round(med["6x192_layered"], 4), "layered_spread_ms": round(spread, 4),
                   "bound_ms": round(med["6x192_layered"] - 3.0 * spread, 4), "fused_ms": round(med["6x192_fused"], 4),
                   "met": bool(med["6x192_fused"] < med["6x192_layered"] - 3.0 * spread)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["gate"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
