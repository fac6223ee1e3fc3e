#!/usr/bin/env python3
"""Cost of producing one training batch, two routes in one process on one MI355X:

    rayset   nerf_sr_amd.data.RaySet.batch: one launch (nsr_rayset_batch) from poses + 8-bit images
    gather   the way without it: all_rays / all_rgbs / all_rgbs_ori materialised as fp32, three torch.index_select

Set: 20 views of 504 x 378 at s = 2 (LLFF `fern` at the reference's training size), batch = 512 LR pixels.  `--repeats` (5)
alternating runs of `--block` (200) batches each, every run timed with device events around the block; the index tensors
are drawn up front.  Resident bytes of both routes are derived from the shapes.  With `--train-iters N` the iterations/s
of examples/train_scene.py and examples/train_toy.py (same batch, same box, each in a child process) are recorded too.
Recorded, not gated.  Prints one JSON object (also written to --out).

    python scripts/time_ray_batches.py --train-iters 200 --out profiles/ray_batches_timing.json
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from nerf_sr_amd import cameras  # noqa: E402
from nerf_sr_amd.data import RaySet  # noqa: E402


def example_rate(script, iters, batch, timeout):
    """iterations/s an example prints on its last progress line."""
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", script), "--iters", str(iters), "--batch", str(batch)],
                         capture_output=True, text=True, timeout=timeout, check=True).stdout
    return float(re.findall(r"\(([\d.]+) it/s\)", out)[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--wh", type=int, nargs=2, default=(504, 378))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--train-iters", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = a.wh
    s = 2
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:H, 0:W]
    images = [np.clip(np.stack([127 + 100 * np.sin(xx / 31.0 + k), (xx + yy + 9 * k) % 256, 255 - (xx // 16 + yy // 12) % 256], -1)
                      + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8) for k in range(a.views)]
    poses = [cameras.spiral_pose((k + 0.5) / a.views) for k in range(a.views)]
    rs = RaySet(poses, images, (W, H), s, True, focal=cameras.llff_focal(W))
    n = len(rs)
    # the gather route's buffers, built once in view-sized pieces by the set itself (bit-identical rows)
    per = n // a.views
    parts = [rs.batch(torch.arange(v * per, (v + 1) * per, device="cuda")) for v in range(a.views)]
    all_rays, all_rgbs, all_ori = (torch.cat([p[k] for p in parts]) for k in ("rays", "rgbs", "rgbs_ori"))
    del parts
    gen = torch.Generator(device="cuda").manual_seed(0)
    idx = [torch.randint(0, n, (a.batch,), device="cuda", generator=gen) for _ in range(a.block)]
    routes = {"rayset": lambda i: rs.batch(i),
              "gather": lambda i: (all_rays.index_select(0, i), all_rgbs.index_select(0, i), all_ori.index_select(0, i))}
    b, g = rs.batch(idx[0]), routes["gather"](idx[0])
    same = bool(torch.equal(b["rays"], g[0]) and torch.equal(b["rgbs"], g[1]) and torch.equal(b["rgbs_ori"], g[2]))
    runs = {k: [] for k in routes}
    for fn in routes.values():
        for i in idx[:a.warmup]:
            fn(i)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in idx:
                fn(i)
            e1.record()
            e1.synchronize()
            runs[name].append(e0.elapsed_time(e1) * 1e3 / a.block)
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = max(runs["gather"]) - min(runs["gather"])
    out_bytes = a.batch * (s * s * 8 + 3 + s * s * 3) * 4
    res = {"set": f"{a.views} views of {W} x {H}, s = {s}: {n} LR pixels; batch {a.batch} LR pixels; {a.repeats} alternating runs of "
                  f"{a.block} batches after {a.warmup} warm-up batches, device events around each run",
           "device": torch.cuda.get_device_name(0), "rows_bit_identical": same,
           "us_per_batch": {k: {"median": round(med[k], 2), "runs": [round(t, 2) for t in v]} for k, v in runs.items()},
           "gather_spread_us": round(spread, 2),
           "rayset_minus_gather_us": round(med["rayset"] - med["gather"], 2),
           "rayset_no_slower_beyond_3_spreads": bool(med["rayset"] <= med["gather"] + 3 * spread),
           "rayset_bytes_written_per_batch": out_bytes,
           "rayset_achieved_write_GBps": round(out_bytes / (med["rayset"] * 1e-6) / 1e9, 3),
           "resident_bytes": {"rayset (poses + u8 HR and LR images)": rs.resident_bytes(),
                              "gather (fp32 rays + targets)": sum(t.numel() * 4 for t in (all_rays, all_rgbs, all_ori))}}
    if a.train_iters:
        res["train_iterations_per_s"] = {"examples/train_scene.py": example_rate("train_scene.py", a.train_iters, a.batch, 600),
                                         "examples/train_toy.py": example_rate("train_toy.py", a.train_iters, a.batch, 600),
                                         "iters": a.train_iters, "batch": a.batch}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
