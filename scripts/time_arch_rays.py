#!/usr/bin/env python3
"""A/B of the two routes of a fused non-default architecture (ops.GenericMLP(fused=True), precision f16x3):

    rows   posenc of the points + posenc of the directions + repeat_interleave + cat in HBM, then nsr_arch_fused_forward
    rays   nsr_arch_fused_render_rays: (rays, z) in, the encodings computed in the kernel (opt.arch_fused_rays, the default)

Both give the same bits (tests/test_gpu_arch_rays.py), so only the time differs.

    frames  config #2 (504 x 378 <- 252 x 189 = 190,512 rays, 64 + 128 samples, eval) through NeRFDownXModel, one model per
            network with opt.arch_fused_rays switched between the calls: 6 x 192 skips (1, 3) and 4 x 128 skip (2), degrees 10 / 4
    bare    262,144 points = 2,048 rays x 128 samples of the 6 x 192 network: the rays launch against the rows route from the
            points on (what NeRFDownXModel.render_rays does), and against the row kernel alone on rows encoded beforehand

One process runs every variant: `--repeats` (5) alternating runs, device events; a frame is one call per run, a bare variant
`--block` (10).  The gate: on the 6 x 192 frame the rays median must be below the rows median by more than three times the
spread (max - min) of the rows repeats.  `--yardstick PARENT.json THIS.json` (two outputs of scripts/time_arch_fused.py
--no-frames, the parent commit's and this build's) records whether the row-mode kernel moved: each median within three times
the parent's spread -- only then does the rows route of this build stand for the parent.

`--frame-only rows|rays` renders a few 6 x 192 frames by one route and exits: the process a kernel trace is taken of.

    python scripts/time_arch_rays.py --out profiles/arch_rays_timing.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import cameras, ops  # noqa: E402
from nerf_sr_amd.model import NeRFDownXModel, default_options  # noqa: E402
from nerf_sr_amd.weights import make_state_dict_arch  # noqa: E402

NETS = {"6x192": {"D": 6, "W": 192, "skips": (1, 3), "deg_pos": 10, "deg_dir": 4},
        "4x128": {"D": 4, "W": 128, "skips": (2,), "deg_pos": 10, "deg_dir": 4}}
FRAME_RAYS = 190512


def frame_model(arch, dev):
    opt = default_options(precision="f16x3", N_importance=128, arch_fused=True, **{**arch, "skips": list(arch["skips"])})
    m = NeRFDownXModel(opt, device=dev)
    return m.load_networks(make_state_dict_arch(99, **arch), make_state_dict_arch(100, **arch)).eval()


def frame_call(m, frame, by_rays):
    def f():
        m.opt.arch_fused_rays = by_rays
        return m.forward_rays(frame)
    return f


def yardstick(parent_path, this_path):
    parent, this = (json.load(open(p))["variants"] for p in (parent_path, this_path))
    out = {"rule": "every 262,144-row median of this build within 3 x (max - min) of the parent's repeats", "variants": {}, "met": True}
    for k, v in parent.items():
        if k not in this:
            continue
        spread = max(v["ms_runs"]) - min(v["ms_runs"])
        ok = abs(this[k]["ms_median"] - v["ms_median"]) <= 3.0 * spread
        out["variants"][k] = {"parent_ms": v["ms_median"], "parent_spread_ms": round(spread, 4), "this_ms": this[k]["ms_median"], "within": bool(ok)}
        out["met"] = bool(out["met"] and ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=10, help="calls per timed run of a bare variant")
    ap.add_argument("--frame-only", choices=("rows", "rays"), default="")
    ap.add_argument("--yardstick", nargs=2, metavar=("PARENT.json", "THIS.json"), default=None)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    frame = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, device=dev).view(-1, 8).contiguous()

    if a.frame_only:
        f = frame_call(frame_model(NETS["6x192"], dev), frame, a.frame_only == "rays")
        with torch.no_grad():
            for _ in range(4):
                f()
        torch.cuda.synchronize()
        print(f"rendered 4 frames by the {a.frame_only} route")
        return 0

    variants = {}
    for name, arch in NETS.items():
        m = frame_model(arch, dev)
        variants[f"{name}_frame_rows"] = frame_call(m, frame, False)
        variants[f"{name}_frame_rays"] = frame_call(m, frame, True)
    arch = NETS["6x192"]
    net = ops.GenericMLP(precision="f16x3", device=dev, fused=True, **arch).load_state_dict(make_state_dict_arch(99, **arch))
    R, N = 2048, 128
    rays = frame[:R].contiguous()
    z, pts = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)
    pe_pos, pe_dir = ops.PositionalEncoding(3, arch["deg_pos"]), ops.PositionalEncoding(3, arch["deg_dir"])
    dirs = rays[:, 3:6].contiguous()

    def rows_route():
        return net(torch.cat([pe_pos(pts.reshape(-1, 3)), pe_dir(dirs).repeat_interleave(N, dim=0)], -1))
    x = torch.cat([pe_pos(pts.reshape(-1, 3)), pe_dir(dirs).repeat_interleave(N, dim=0)], -1).contiguous()
    variants["6x192_bare_rows_route"] = rows_route
    variants["6x192_bare_row_kernel_alone"] = lambda: net(x)
    variants["6x192_bare_rays"] = lambda: ops.render_rays(net, rays, z)

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
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    res = {"shape": f"precision f16x3; {a.repeats} alternating runs, device events; frames: config #2 ({FRAME_RAYS} rays, 64 + 128 samples, "
                    f"eval), one call per run; bare: {R * N} points = {R} rays x {N} samples, {a.block} calls per run",
           "device": torch.cuda.get_device_name(dev),
           "variants": {k: {"ms_median": round(med[k], 4), "ms_spread": round(spread[k], 4), "ms_runs": [round(x, 4) for x in runs[k]]}
                        for k in variants}}
    for name in NETS:
        rows_ms, rays_ms = med[f"{name}_frame_rows"], med[f"{name}_frame_rays"]
        res[f"frame_{name}"] = {"rows_ms": round(rows_ms, 3), "rays_ms": round(rays_ms, 3), "saved_ms": round(rows_ms - rays_ms, 3),
                                "rows_rays_per_s": round(FRAME_RAYS / (rows_ms * 1e-3)), "rays_rays_per_s": round(FRAME_RAYS / (rays_ms * 1e-3)),
                                "speedup": round(rows_ms / rays_ms, 3)}
    res["bare_6x192"] = {"rows_route_ms": round(med["6x192_bare_rows_route"], 4), "row_kernel_alone_ms": round(med["6x192_bare_row_kernel_alone"], 4),
                         "rays_ms": round(med["6x192_bare_rays"], 4),
                         "encode_in_kernel_ms": round(med["6x192_bare_rays"] - med["6x192_bare_row_kernel_alone"], 4),
                         "encode_launches_replaced_ms": round(med["6x192_bare_rows_route"] - med["6x192_bare_row_kernel_alone"], 4)}
    bound = med["6x192_frame_rows"] - 3.0 * spread["6x192_frame_rows"]
    res["gate"] = {"rule": "6 x 192 frame: rays median < rows median - 3 x (max - min of the rows repeats)",
                   "rows_ms": round(med["6x192_frame_rows"], 3), "rows_spread_ms": round(spread["6x192_frame_rows"], 3),
                   "bound_ms": round(bound, 3), "rays_ms": round(med["6x192_frame_rays"], 3), "met": bool(med["6x192_frame_rays"] < bound)}
    if a.yardstick:
        res["yardstick_row_kernel_vs_parent"] = yardstick(*a.yardstick)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["gate"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
