"""How many depth windows of the fine pass would early ray termination cut (include/nsr.h, "early ray termination")?  CPU
only: the torch oracle on the benchmark's fields (weights.make_state_dict "smooth" and the "sharp" stress field, seeds 99 /
100 as in bench.py) and frames (BASELINE configs #2 and #3), a sample of 8,192 rays = 16 blocks of 512 consecutive rays
spread over the frame, as scripts/empty_tile_stats.py takes them.  The coarse pass runs whole (it is never cut); the rule
(tests/early_stop_ref.py) is applied to the raw densities and depths of the 128-sample fine pass, for eps in 1e-3 / 1e-4 /
1e-5:

  rays4   share of the windows (4 consecutive rays x 32 samples) the kernel's rule cuts: a group stops when ALL its rays are spent
  ray1    for contrast, the share a rule deciding ray by ray would cut (not built: a wave would idle while its group runs on)

A cut window saves all of its 1,184 k-steps, so `rays4` is the predicted saving of the fine launch, to be read against
profiles/early_stop_timing.json (scripts/time_early_stop.py).

    python scripts/early_stop_stats.py [--out profiles/early_stop_stats.json] [--blocks 16] [--block-rays 512]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from nerf_sr_amd import cameras                      # noqa: E402
from nerf_sr_amd.weights import make_state_dict      # noqa: E402
from oracle import nerf_oracle as oc                 # noqa: E402
from tests import early_stop_ref as ref              # noqa: E402

CONFIGS = {2: {"img_wh": (504, 378), "s": 2, "ndc": True, "white": False},
           3: {"img_wh": (400, 400), "s": 2, "ndc": False, "white": True}}
FIELDS = ("smooth", "sharp")
EPS = (1e-3, 1e-4, 1e-5)


def frame_rays(cfg):
    (W, H), s = cfg["img_wh"], cfg["s"]
    if cfg["ndc"]:
        c2w, focal, nf = cameras.spiral_pose(0.4), cameras.llff_focal(W), (0.0, 1.0)
    else:
        c2w, focal, nf = cameras.spheric_pose(0.0, -30.0, 4.0), cameras.blender_focal(W), (2.0, 6.0)
    return oc.subpixel_ray_grid(torch.from_numpy(c2w), H, W, focal, s, cfg["ndc"], *nf).reshape(-1, 8)


def fine_pass(sd_c, sd_f, rays, white):
    """(rgb (R, 128, 3), raw density (R, 128), depths (R, 128)) of the fine pass, as oracle.forward_rays evaluates it"""
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    de = oc.posenc(d, 4)
    z, xyz = oc.sample_coarse(o, d, near, far, 64, False)
    rgb, sig = oc.render_points(sd_c, xyz, de)
    w = oc.composite(rgb, sig, z, white)[3]
    z2, xyz2 = oc.resample_fine(o, d, z, w, 64)
    rgb2, sig2 = oc.render_points(sd_f, xyz2, de)
    return rgb2, sig2, z2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "early_stop_stats.json"))
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--block-rays", type=int, default=512)
    args = ap.parse_args()
    res = {"fields": "weights.make_state_dict, seeds 99 (coarse) / 100 (fine)", "rays": args.blocks * args.block_rays,
           "sample": f"{args.blocks} blocks of {args.block_rays} consecutive rays spread evenly over the frame",
           "pass": "fine, 64 + 64 samples: 4 windows per group of 4 rays, at most 3 of them can be cut",
           "configs": {}}
    for cid, cfg in CONFIGS.items():
        rays = frame_rays(cfg)
        step = (rays.shape[0] - args.block_rays) // max(args.blocks - 1, 1)
        step -= step % 8                                   # blocks start on a group boundary
        res["configs"][str(cid)] = {}
        for field in FIELDS:
            sd_c, sd_f = oc.to_torch_sd(make_state_dict(99, field)), oc.to_torch_sd(make_state_dict(100, field))
            parts = []
            with torch.no_grad():
                for b in range(args.blocks):
                    parts.append(fine_pass(sd_c, sd_f, rays[b * step: b * step + args.block_rays], cfg["white"]))
            rgb, sig, z = (torch.cat([p[i] for p in parts]).numpy() for i in range(3))
            R, N = sig.shape
            n_win4, n_win1 = (R // 4) * (N // 32), R * (N // 32)
            out = {"empty_rays4_win32": float(((sig <= 0).reshape(R // 4, 4, N // 32, 32).transpose(0, 2, 1, 3).reshape(-1, 128).all(-1)).mean())}
            for eps in EPS:
                t = ref.truncate(rgb, sig, z, eps)
                comp = [oc.composite(torch.from_numpy(a), torch.from_numpy(s), torch.from_numpy(z), cfg["white"])[0] for a, s in ((rgb, sig), (t.rgb, t.sigma))]
                out[f"{eps:g}"] = {"rays4": t.n_cut / n_win4, "ray1": t.n_cut_single_ray / n_win1, "marginal_windows": len(t.marginal),
                                   "max_abs_drgb_oracle": float((comp[0] - comp[1]).abs().max())}
                print(f"config #{cid} {field} eps {eps:g}: rays4 {100 * t.n_cut / n_win4:.2f} %  ray1 {100 * t.n_cut_single_ray / n_win1:.2f} %  "
                      f"max |dRGB| {out[f'{eps:g}']['max_abs_drgb_oracle']:.2e}", flush=True)
            res["configs"][str(cid)][field] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
