#!/usr/bin/env python3
"""Timing of the fused descriptor kernel around the embedding option word (--no_xyz / --no_logscale, include/nsr.h):

    parent   a libnsr.so built from the parent commit (--parent-lib), through the entry points it has
    this     this build at embed = 0, through the same entry points (which are the `_e` forms called with 0)
    embed    this build with NSR_EMBED_NO_XYZ | NSR_EMBED_LINEAR_FREQS, through the `_e` entry points

on the 6 x 192 network (skips 1, 3; degrees 10 / 4), 2,048 rays x 128 samples = 262,144 points: the rays entry
(nsr_arch_fused_render_rays) and the rows entry (nsr_arch_fused_forward) on rows encoded beforehand.  Both libraries are
loaded into ONE process through ctypes (the Python layer of this tree cannot bind the parent's library, which lacks the `_e`
symbols) and run in `--repeats` (5) alternating runs of `--block` (50) launches, device events.

Gate, the project's yardstick for "unchanged": at embed = 0 a median of this build may be at most the parent's median plus
3 x (max - min) of the parent's repeats.  The `embed` times are recorded beside them; they are figures, not gates.

    python scripts/time_embed_options.py --parent-lib /path/to/parent/libnsr.so --out profiles/embed_options_timing.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
from ctypes import c_void_p

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import _lib  # noqa: E402
from nerf_sr_amd.weights import make_state_dict_arch  # noqa: E402

ARCH = {"D": 6, "W": 192, "skips": (1, 3), "deg_pos": 10, "deg_dir": 4, "no_dir": False}
BOTH = _lib.NSR_EMBED_NO_XYZ | _lib.NSR_EMBED_LINEAR_FREQS


def bind_parent(path):
    lib = ctypes.CDLL(path)
    for name in ("nsr_arch_fused_packed_bytes", "nsr_arch_fused_pack", "nsr_arch_fused_forward", "nsr_arch_fused_render_rays"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


class Net:
    """The packed network of one library and one option word, and its two launches."""

    def __init__(self, lib, embed, use_e):
        self.lib, self.embed, self.e = lib, embed, use_e
        self.arch = _lib.NsrArch.from_arch(ARCH)
        sd = make_state_dict_arch(99, no_xyz=bool(embed & _lib.NSR_EMBED_NO_XYZ), **ARCH)
        self.w = [torch.from_numpy(v).cuda() for v in sd.values()]
        lead = (ctypes.byref(self.arch), embed) if use_e else (ctypes.byref(self.arch),)
        sfx = "_e" if use_e else ""
        nbytes = getattr(lib, "nsr_arch_fused_packed_bytes" + sfx)(*lead)
        assert nbytes > 0
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        ptrs = (c_void_p * len(self.w))(*[c_void_p(t.data_ptr()) for t in self.w])
        rc = getattr(lib, "nsr_arch_fused_pack" + sfx)(*lead, ptrs, c_void_p(self.packed.data_ptr()), c_void_p(self.status.data_ptr()), None)
        assert rc == 0 and int(self.status.item()) == 0
        self.lead, self.fwd, self.rays_fn = lead, getattr(lib, "nsr_arch_fused_forward" + sfx), getattr(lib, "nsr_arch_fused_render_rays" + sfx)

    def rows(self, x, out):
        rc = self.fwd(*self.lead, c_void_p(self.packed.data_ptr()), c_void_p(x.data_ptr()), x.shape[1], x.shape[0], 0,
                      c_void_p(out.data_ptr()), 4, c_void_p(self.status.data_ptr()), None)
        assert rc == 0

    def rays(self, rays, z, out):
        rc = self.rays_fn(*self.lead, c_void_p(self.packed.data_ptr()), c_void_p(rays.data_ptr()), 8, c_void_p(z.data_ptr()),
                          z.shape[0], z.shape[1], 0, c_void_p(out.data_ptr()), 4, c_void_p(self.status.data_ptr()), None)
        assert rc == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=50, help="launches per timed run")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    this = _lib.load()
    nets = {"parent": Net(bind_parent(args.parent_lib), 0, False), "this": Net(this, 0, False), "embed": Net(this, BOTH, True)}
    rng = np.random.Generator(np.random.PCG64(1))
    R, N = args.rays, args.samples
    rays = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (R, 6)), np.zeros((R, 1)), np.ones((R, 1))], 1).astype(np.float32)).cuda()
    z = torch.from_numpy(np.sort(rng.uniform(0, 1, (R, N)), axis=1).astype(np.float32)).cuda()
    from nerf_sr_amd import ops
    pts = ops.cast_rays(rays[:, 0:3], rays[:, 3:6], z).reshape(-1, 3).contiguous()
    x = {}
    for embed in (0, BOTH):
        opt = argparse.Namespace(no_xyz=bool(embed & 1), no_logscale=bool(embed & 2))
        x[embed] = torch.cat([ops.PositionalEncoding(3, 10, opt)(pts),
                              ops.PositionalEncoding(3, 4, opt)(rays[:, 3:6].contiguous()).repeat_interleave(N, dim=0)], -1).contiguous()
    out = torch.empty(R * N, 4, device="cuda")
    calls = {}
    for name, net in nets.items():
        calls[f"{name}/rays"] = lambda net=net: net.rays(rays, z, out)
        calls[f"{name}/rows"] = lambda net=net: net.rows(x[net.embed], out)
    # the three networks agree with themselves across the two entries, and `this` with `parent`, bit for bit
    ref = {}
    for k, f in calls.items():
        out.zero_()
        f()
        ref[k] = out.clone()
    same = {"this_rays_eq_parent_rays": bool(torch.equal(ref["this/rays"], ref["parent/rays"])),
            "this_rows_eq_parent_rows": bool(torch.equal(ref["this/rows"], ref["parent/rows"])),
            "embed_rays_eq_embed_rows": bool(torch.equal(ref["embed/rays"], ref["embed/rows"]))}
    for f in calls.values():      # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.repeats):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.block):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.block)
    res = {"network": "6 x 192, skips (1, 3), degrees 10 / 4", "points": R * N, "repeats": args.repeats, "block": args.block,
           "unit": "ms per launch", "bits": same, "variants": {}, "gate": {}}
    for k, v in times.items():
        res["variants"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
    met = all(same.values())
    for entry in ("rays", "rows"):
        p, t = res["variants"][f"parent/{entry}"], res["variants"][f"this/{entry}"]
        limit = p["median"] + 3.0 * (p["max"] - p["min"])
        res["gate"][entry] = {"parent_median": p["median"], "parent_spread": p["max"] - p["min"], "limit": limit,
                              "this_median": t["median"], "met": t["median"] <= limit}
        met = met and t["median"] <= limit
    res["gate"]["rule"] = "this (embed = 0) median <= parent median + 3 x (max - min) of the parent's repeats; `embed` is a figure"
    res["met"] = met
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
