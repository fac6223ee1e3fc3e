"""How often is a tile of the render kernel EMPTY (every raw density <= 0, so that its colours cannot reach any output under
the relu density)?  CPU only: the torch oracle on the benchmark's own field (weights.make_state_dict, seeds 99 / 100 as in
bench.py) and frames (BASELINE configs #2 and #3), a sample of 8,192 rays = 16 blocks of 512 consecutive rays spread over
the frame.  Tilings compared, per pass (coarse: 64 samples, fine: 128):

  sample          single samples (the ceiling of any tiling)
  whole_rays      128 consecutive samples of whole rays (the tile before the windowed kernel: coarse 2 rays x 64, fine 1 x 128)
  rays4_win32     4 consecutive rays x the same window of 32 consecutive samples (the windowed kernel, csrc/nsr_mlp_f16.hip)
  ray1_win32      one wave alone: 1 ray x 32 samples
  rays8_win16     8 consecutive rays x 16 samples (not built: needs two rays per wave)

    python scripts/empty_tile_stats.py [--out profiles/empty_tile_stats.json] [--blocks 16] [--block-rays 512]
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

CONFIGS = {2: {"img_wh": (504, 378), "s": 2, "ndc": True, "white": False},
           3: {"img_wh": (400, 400), "s": 2, "ndc": False, "white": True}}


def frame_rays(cfg):
    (W, H), s = cfg["img_wh"], cfg["s"]
    if cfg["ndc"]:
        c2w, focal, nf = cameras.spiral_pose(0.4), cameras.llff_focal(W), (0.0, 1.0)
    else:
        c2w, focal, nf = cameras.spheric_pose(0.0, -30.0, 4.0), cameras.blender_focal(W), (2.0, 6.0)
    return oc.subpixel_ray_grid(torch.from_numpy(c2w), H, W, focal, s, cfg["ndc"], *nf).reshape(-1, 8)


def densities(sd_c, sd_f, rays, white):
    """raw densities (R, 64) of the coarse pass and (R, 128) of the fine pass, as oracle.forward_rays evaluates them"""
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    de = oc.posenc(d, 4)
    z, xyz = oc.sample_coarse(o, d, near, far, 64, False)
    rgb, sig = oc.render_points(sd_c, xyz, de)
    w = oc.composite(rgb, sig, z, white)[3]
    z2, xyz2 = oc.resample_fine(o, d, z, w, 64)
    return sig, oc.render_points(sd_f, xyz2, de)[1]


def empty_fraction(sig, rays_per_tile, window):
    """fraction of tiles (rays_per_tile consecutive rays x `window` consecutive samples) with every density <= 0"""
    R, N = sig.shape
    R -= R % rays_per_tile
    dead = (sig[:R] <= 0).reshape(R // rays_per_tile, rays_per_tile, N // window, window)
    return float(dead.permute(0, 2, 1, 3).reshape(-1, rays_per_tile * window).all(-1).double().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "empty_tile_stats.json"))
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--block-rays", type=int, default=512)
    args = ap.parse_args()
    sd_c, sd_f = oc.to_torch_sd(make_state_dict(99)), oc.to_torch_sd(make_state_dict(100))
    res = {"field": "smooth, seeds 99 / 100", "rays": args.blocks * args.block_rays,
           "sample": f"{args.blocks} blocks of {args.block_rays} consecutive rays spread evenly over the frame", "configs": {}}
    for cid, cfg in CONFIGS.items():
        rays = frame_rays(cfg)
        step = (rays.shape[0] - args.block_rays) // max(args.blocks - 1, 1)
        step -= step % 8                                   # blocks start on a tile boundary of every tiling
        sig_c, sig_f = [], []
        with torch.no_grad():
            for b in range(args.blocks):
                c, f = densities(sd_c, sd_f, rays[b * step: b * step + args.block_rays], cfg["white"])
                sig_c.append(c)
                sig_f.append(f)
        out = {}
        for name, sig, whole in (("coarse", torch.cat(sig_c), 2), ("fine", torch.cat(sig_f), 1)):
            out[name] = {"sample": empty_fraction(sig, 1, 1),
                         "whole_rays": empty_fraction(sig, whole, sig.shape[1]),
                         "rays4_win32": empty_fraction(sig, 4, 32),
                         "ray1_win32": empty_fraction(sig, 1, 32),
                         "rays8_win16": empty_fraction(sig, 8, 16)}
            print(f"config #{cid} {name}: " + "  ".join(f"{k} {100 * v:.1f} %" for k, v in out[name].items()), flush=True)
        res["configs"][str(cid)] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
