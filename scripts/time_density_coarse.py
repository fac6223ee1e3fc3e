#!/usr/bin/env python3
"""What the density-only coarse pass (include/nsr.h "test-time mode"; csrc/nsr_mlp_f16.hip "DENS") saves, on one whole frame of
BASELINE config #2 (190,512 rays), through the C ABI with preallocated outputs:

    coarse_launch   the 64-sample coarse launch: nsr_render_rays_density of this tree's library against
                    nsr_render_rays_composited of another build of libnsr (--parent-lib: the parent commit's) and of this
                    one, on the bench field (`smooth`) and on a trained hard-surface field (tests/trained_field.py); depth,
                    opacity and weights compared bit for bit.  Bar: faster than the parent's launch by more than 3 x the
                    spread of the parent's repeats.
    frame           whole-frame rays/s of ops.forward_rays (64 + 64, no per-sample weights returned) with coarse_rgb=False
                    beside the default, outputs compared bit for bit.
    wide_route      the fused render + composite launch at 192 and 256 samples per ray against what those counts took
                    before it (nsr_render_rays, then nsr_composite), same library, bench field, outputs compared bit for bit.

`--repeats` (5) alternating runs of `--block` launches each, every block timed by wall clock around a device
synchronisation, medians and the spread of the repeats recorded.  The driver itself touches no GPU: each step is a child
process under a time limit of its own, the sides of a comparison alternate inside that one process, and nothing is started
after a step that fails.  `--stages a,b` runs a subset and merges it into an existing `--out` record.

    python scripts/time_density_coarse.py --parent-lib ab/libnsr_parent.so --out profiles/density_coarse_timing.json
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from nerf_sr_amd import _lib, ops  # noqa: E402
from nerf_sr_amd.weights import make_state_dict  # noqa: E402
from time_early_stop import F16X3, alternate, bind_parent, frame_rays, pack  # noqa: E402


class Coarse:
    """one 64-sample coarse launch of `rays` x z through library L with preallocated outputs"""

    def __init__(self, L, blob, rays, z):
        R, N = z.shape
        self.L, self.blob, self.rays, self.z = L, blob, rays, z
        self.out = [torch.empty(s, device="cuda") for s in ((R, 3), (R,), (R,), (R, N))]

    def composited(self):
        R, N = self.z.shape
        rc = self.L.nsr_render_rays_composited(self.blob.data_ptr(), F16X3, self.rays.data_ptr(), 8, self.z.data_ptr(), R, N, 0, None,
                                               *[o.data_ptr() for o in self.out], None)
        assert rc == 0, rc

    def density(self):
        R, N = self.z.shape
        rc = self.L.nsr_render_rays_density(self.blob.data_ptr(), F16X3, self.rays.data_ptr(), 8, self.z.data_ptr(), R, N, 0,
                                            *[o.data_ptr() for o in self.out[1:]], None)
        assert rc == 0, rc


def coarse_launch(lib, P, sd, rays, a):
    z = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], 64, False, False)[0].contiguous()
    parent, full, dens = Coarse(P, pack(P, sd), rays, z), Coarse(lib, pack(lib, sd), rays, z), Coarse(lib, pack(lib, sd), rays, z)
    r = alternate({"parent_composited": parent.composited, "this_composited": full.composited, "this_density": dens.density},
                  a.repeats, a.block)
    torch.cuda.synchronize()
    r["outputs_bit_identical"] = all(torch.equal(x, y) for x, y in zip(dens.out[1:], parent.out[1:]))
    saved = r["parent_composited"]["ms_median"] - r["this_density"]["ms_median"]
    r["density_minus_parent_ms"] = round(-saved, 4)
    r["density_over_parent"] = round(r["this_density"]["ms_median"] / r["parent_composited"]["ms_median"], 4)
    r["bar_3x_parent_spread_ms"] = round(3 * r["parent_composited"]["spread_ms"], 4)
    r["bar_met"] = bool(saved > 3 * r["parent_composited"]["spread_ms"])
    return r


STAGES = ("coarse_bench", "coarse_trained", "frame", "wide_route")
LIMITS = {"coarse_bench": 180, "coarse_trained": 300, "frame": 240, "wide_route": 240}     # seconds


def wide_route(lib, rays, a):
    """fused launch against network-then-compositor at 192 and 256 samples, through the C ABI with preallocated buffers"""
    blob = pack(lib, make_state_dict(100))
    out = {"field": "bench (smooth, seed 100), uniform depths", "rays": rays.shape[0]}
    R = rays.shape[0]
    for N in (192, 256):
        z = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)[0].contiguous()
        fused = [torch.empty(s, device="cuda") for s in ((R, 3), (R,), (R,), (R, N))]
        pair = [torch.empty(s, device="cuda") for s in ((R, 3), (R,), (R,), (R, N))]
        raw = torch.empty(R, N, 4, device="cuda")

        def one():
            rc = lib.nsr_render_rays_composited(blob.data_ptr(), F16X3, rays.data_ptr(), 8, z.data_ptr(), R, N, 0, None,
                                                *[o.data_ptr() for o in fused], None)
            assert rc == 0, rc

        def two():
            rc = lib.nsr_render_rays(blob.data_ptr(), F16X3, rays.data_ptr(), 8, z.data_ptr(), R, N, raw.data_ptr(), None)
            assert rc == 0, rc
            rc = lib.nsr_composite(raw.data_ptr(), 4, raw.data_ptr() + 12, 4, z.data_ptr(), R, N, 0, *[o.data_ptr() for o in pair], None)
            assert rc == 0, rc

        r = alternate({"two_call": two, "fused": one}, a.repeats, a.block)
        torch.cuda.synchronize()
        r["outputs_bit_identical"] = all(torch.equal(x, y) for x, y in zip(fused, pair))
        r["fused_over_two_call"] = round(r["fused"]["ms_median"] / r["two_call"]["ms_median"], 4)
        out[str(N)] = r
        del raw
    return out


def stage(name, a):
    torch.cuda.init()
    lib = _lib.load()
    if name == "coarse_bench":
        rays, _ = frame_rays("llff")
        return {"coarse_launch": {"bench": dict(coarse_launch(lib, bind_parent(a.parent_lib), make_state_dict(99), rays, a),
                                                field="bench (smooth, seed 99), 64 uniform depths", rays=rays.shape[0])}}
    if name == "coarse_trained":
        from tests import trained_field as tf
        t0 = time.time()
        tr = tf.train_field("llff", steps=a.train_steps)
        torch.cuda.synchronize()
        rays, _ = frame_rays("llff")
        r = coarse_launch(lib, bind_parent(a.parent_lib), tr["sd_coarse"], rays, a)
        r.update(field="trained hard-surface field, forward-facing family (coarse network)", rays=rays.shape[0],
                 train_steps=a.train_steps, train_seconds=round(time.time() - t0, 1))
        return {"coarse_launch": {"trained_llff": r}}
    rays, white = frame_rays("llff")
    if name == "wide_route":
        return {"wide_route": wide_route(lib, rays, a)}
    coarse = ops.VanillaMLP(precision="f16x3").load_state_dict(make_state_dict(99))
    fine = ops.VanillaMLP(precision="f16x3").load_state_dict(make_state_dict(100))
    R = rays.shape[0]
    state = {"default": {}, "coarse_rgb_false": {}}

    def run(which):
        state[which] = ops.forward_rays(coarse, fine, rays, 64, 64, white, outs=state[which], want_weights=False,
                                        coarse_rgb=which == "default")

    r = alternate({k: (lambda k=k: run(k)) for k in state}, a.repeats, a.block)
    torch.cuda.synchronize()
    for k in state:
        r[k]["rays_per_s"] = round(R / (r[k]["ms_median"] * 1e-3))
    keys = ("coarse_depth", "coarse_opacity", "fine_comp_rgbs", "fine_depth", "fine_opacity")
    r["outputs_bit_identical"] = all(torch.equal(state["default"][k], state["coarse_rgb_false"][k]) for k in keys)
    r["speedup"] = round(r["default"]["ms_median"] / r["coarse_rgb_false"]["ms_median"], 4)
    r.update(rays=R, field="bench (smooth, seeds 99 / 100), 64 + 64 samples", status_flags=[coarse.status(clear=True), fine.status(clear=True)])
    return {"frame": r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="another build of libnsr.so whose composited coarse launch is the baseline")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=5, help="launches per timed block")
    ap.add_argument("--train-steps", type=int, default=4000, help="0 skips the trained field")
    ap.add_argument("--out", default="")
    ap.add_argument("--stages", default="", help="comma-separated subset of the steps; merged into an existing --out record")
    ap.add_argument("--stage", default="", help="internal: run this one step and print its part of the record")
    a = ap.parse_args()
    if a.stage:
        print("@@" + json.dumps(stage(a.stage, a)), flush=True)
        return
    import subprocess
    from nerf_sr_amd import build
    res = {"source_hash": build.source_hash()[:16], "parent_lib": os.path.basename(a.parent_lib),
           "protocol": f"{a.repeats} alternating runs, each of {a.block} launches; whole frames of BASELINE config #2; "
                       "one process per step, alternation inside it"}
    if a.stages and a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = dict(json.load(f), source_hash=res["source_hash"])
    for name in STAGES:
        if a.stages and name not in a.stages.split(","):
            continue
        if (name.startswith("coarse_") and not a.parent_lib) or (name == "coarse_trained" and a.train_steps <= 0):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--stage", name, "--repeats", str(a.repeats), "--block", str(a.block),
               "--train-steps", str(a.train_steps), "--parent-lib", a.parent_lib]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            sys.exit(f"step {name} exceeded its {LIMITS[name]} s limit: stopping")
        part = [l for l in p.stdout.splitlines() if l.startswith("@@")]
        if p.returncode != 0 or not part:
            sys.exit(f"step {name} failed with status {p.returncode}: stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        for k, v in json.loads(part[-1][2:]).items():
            if isinstance(res.get(k), dict):
                res[k].update(v)
            else:
                res[k] = v
        print(json.dumps({name: json.loads(part[-1][2:])}), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
