#!/usr/bin/env python3
"""What early ray termination (include/nsr.h; csrc/nsr_mlp_f16.hip "ERT") costs and saves, on the render launch of one whole
frame of BASELINE config #2 (190,512 rays), through the C ABI with preallocated outputs:

    off_vs_parent   option off: this tree's library against another build of libnsr (--parent-lib: the parent commit's),
                    nsr_render_rays_composited with 128 and 64 samples on the bench field -- the default path must not
                    have moved by more than the spread of the repeats
    no_cut          option on where nothing cuts (bench field, eps = 1e-30) against option off, same library: the price of
                    the per-window reduce and vote
    eps_1e-4        option on at eps = 1e-4 against option off on the bench field, a dense field (sigma.bias = 1e3) and a
                    trained hard-surface field of each family (trained here as tests/test_gpu_trained.py does): time of the
                    fine launch, share of windows cut (the kernel's counter), max |dRGB| against option off.  The fine
                    launch is the 128-sample fine pass of ops.forward_rays (HIP events around it); the prediction for the
                    bench field is profiles/early_stop_stats.json (scripts/early_stop_stats.py).

`--repeats` (5) alternating runs of `--block` launches each, every block timed by wall clock around a device
synchronisation, medians and the spread of the repeats recorded.  The driver itself touches no GPU: each of the five steps
(off_vs_parent, no_cut, bench + dense, one trained field per family) is a child process under a time limit of its own, the two
sides of a comparison alternate inside that one process, and nothing is started after a step that fails.  Recorded, not gated.

    python scripts/time_early_stop.py --parent-lib ab/libnsr_parent.so --out profiles/early_stop_timing.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from ctypes import POINTER, c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from nerf_sr_amd import _lib, cameras, ops  # noqa: E402
from nerf_sr_amd.weights import make_state_dict  # noqa: E402

F16X3 = 2
WH, S = (504, 378), 2


def alternate(variants, repeats, block, warmup=2):
    """{name: fn} -> {name: {ms_median, ms_runs, spread_ms}}: alternating timed blocks of `block` calls"""
    runs = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    for _ in range(repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0) * 1e3 / block)
    return {name: {"ms_median": round(statistics.median(v), 4), "ms_runs": [round(t, 4) for t in v], "spread_ms": round(max(v) - min(v), 4)}
            for name, v in runs.items()}


def bind_parent(path):
    """the three entry points every build shares, of another libnsr in this process (as scripts/ab_libs.py binds them)"""
    L = ctypes.CDLL(path)
    L.nsr_packed_weights_bytes.restype = c_size_t
    L.nsr_packed_weights_bytes.argtypes = [c_int]
    L.nsr_pack_weights.argtypes = [POINTER(c_void_p), c_void_p, c_int, c_void_p]
    L.nsr_render_rays_composited.argtypes = _lib.SIGNATURES["nsr_render_rays_composited"][1]
    return L


def pack(L, sd):
    dev = [torch.from_numpy(np.ascontiguousarray(sd[k])).float().cuda().contiguous() for k in ops.STATE_DICT_SPEC]
    ptrs = (c_void_p * 24)(*[c_void_p(t.data_ptr()) for t in dev])
    blob = torch.zeros(L.nsr_packed_weights_bytes(F16X3) + 64, dtype=torch.uint8, device="cuda")
    rc = L.nsr_pack_weights(ptrs, blob.data_ptr(), F16X3, None)
    assert rc == 0, rc
    return blob


class Launch:
    """one composited render launch of `rays` x z through library L with preallocated outputs"""

    def __init__(self, L, blob, rays, z, white):
        R, N = z.shape
        self.L, self.blob, self.rays, self.z, self.white = L, blob, rays, z, int(white)
        self.out = [torch.empty(s, device="cuda") for s in ((R, 3), (R,), (R,), (R, N))]
        self.cut = torch.zeros(1, dtype=torch.int32, device="cuda")

    def off(self):
        R, N = self.z.shape
        rc = self.L.nsr_render_rays_composited(self.blob.data_ptr(), F16X3, self.rays.data_ptr(), 8, self.z.data_ptr(), R, N, self.white,
                                               None, *[o.data_ptr() for o in self.out], None)
        assert rc == 0, rc

    def on(self, eps):
        R, N = self.z.shape
        rc = self.L.nsr_render_rays_composited_ert(self.blob.data_ptr(), F16X3, self.rays.data_ptr(), 8, self.z.data_ptr(), R, N,
                                                   self.white, c_float(eps), *[o.data_ptr() for o in self.out], self.cut.data_ptr(), None)
        assert rc == 0, rc


def frame_rays(family="llff"):
    from tests import trained_field as tf
    wh, s, ndc, white, nf, _ = tf.FAMILIES[family]
    c2w, focal = tf.eval_pose(family)
    return ops.subpixel_rays(c2w, wh, focal, s, ndc, *nf, device="cuda").view(-1, 8).contiguous(), white


def fine_pass(sd_c, sd_f, rays, white, eps, repeats, block):
    """the 64 + 64 forward_rays of a frame with the option off / on: fine-launch time from HIP events, windows cut, |dRGB|"""
    coarse = ops.VanillaMLP(precision="f16x3").load_state_dict(sd_c)
    fine = ops.VanillaMLP(precision="f16x3").load_state_dict(sd_f)
    R = rays.shape[0]
    ev = ops.HipEvents(4)
    cut = torch.zeros(1, dtype=torch.int32, device="cuda")
    state = {k: {"outs": {}, "ms": []} for k in ("off", "on")}

    def run(which):
        st = state[which]
        st["outs"] = ops.forward_rays(coarse, fine, rays, 64, 64, white, outs=st["outs"], want_weights=False, events=ev.handles,
                                      early_stop=eps if which == "on" else 0.0, cut_count=cut if which == "on" else None)
        torch.cuda.synchronize()
        return ev.elapsed_ms(2, 3)

    for which in state:
        run(which)
    cut.zero_()
    run("on")
    n_cut = int(cut.item())
    for _ in range(repeats):
        for which in state:
            state[which]["ms"].append(statistics.median(run(which) for _ in range(block)))
    d_rgb = float((state["on"]["outs"]["fine_comp_rgbs"] - state["off"]["outs"]["fine_comp_rgbs"]).abs().max())
    n_win = ((R + 3) // 4) * 4
    res = {k: {"fine_launch_ms_median": round(statistics.median(v["ms"]), 4), "fine_launch_ms_runs": [round(t, 4) for t in v["ms"]],
               "spread_ms": round(max(v["ms"]) - min(v["ms"]), 4)} for k, v in state.items()}
    res.update(rays=R, windows=n_win, windows_cut=n_cut, share_cut=round(n_cut / n_win, 5), max_abs_drgb_vs_off=d_rgb,
               on_over_off=round(res["on"]["fine_launch_ms_median"] / res["off"]["fine_launch_ms_median"], 4),
               status_flags=[coarse.status(clear=True), fine.status(clear=True)])
    return res


STAGES = ("off_vs_parent", "no_cut", "bench_dense", "trained_llff", "trained_blender")
LIMITS = {"off_vs_parent": 180, "no_cut": 180, "bench_dense": 240, "trained_llff": 300, "trained_blender": 300}     # seconds


def stage(name, a):
    """one GPU step, in a process of its own: returns its part of the record"""
    torch.cuda.init()
    lib = _lib.load()
    bench_c, bench_f = make_state_dict(99), make_state_dict(100)
    if name.startswith("trained_"):
        from tests import trained_field as tf
        family = name.split("_", 1)[1]
        t0 = time.time()
        tr = tf.train_field(family, steps=a.train_steps)
        torch.cuda.synchronize()
        frays, fwhite = frame_rays(family)
        r = fine_pass(tr["sd_coarse"], tr["sd_fine"], frays, fwhite, 1e-4, a.repeats, a.block)
        r.update(train_steps=a.train_steps, train_seconds=round(time.time() - t0, 1), final_fine_mse=tr["history"][-1][2])
        return {"eps_1e-4": {name: r}}
    rays, white = frame_rays("llff")
    if name == "bench_dense":
        dense = [dict(sd, **{"sigma.bias": np.full((1,), 1e3, dtype=np.float32)}) for sd in (bench_c, bench_f)]
        return {"eps_1e-4": {"bench": fine_pass(bench_c, bench_f, rays, white, 1e-4, a.repeats, a.block),
                             "dense": fine_pass(*dense, rays, white, 1e-4, a.repeats, a.block)}}
    zs = {N: ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)[0].contiguous() for N in (64, 128)}
    blob = pack(lib, bench_f)
    if name == "off_vs_parent":      # option off against another build
        P = bind_parent(a.parent_lib)
        pblob = pack(P, bench_f)
        out = {"field": "bench (smooth, seed 100), uniform depths", "parent_lib": os.path.basename(a.parent_lib)}
        for N in (128, 64):
            mine, theirs = Launch(lib, blob, rays, zs[N], white), Launch(P, pblob, rays, zs[N], white)
            r = alternate({"this": mine.off, "parent": theirs.off}, a.repeats, a.block)
            torch.cuda.synchronize()
            r["outputs_bit_identical"] = all(torch.equal(x, y) for x, y in zip(mine.out, theirs.out))
            r["this_minus_parent_ms"] = round(r["this"]["ms_median"] - r["parent"]["ms_median"], 4)
            out[str(N)] = r
        return {"off_vs_parent": out}
    out = {"field": "bench (smooth, seed 100), uniform depths", "eps": 1e-30}     # option on where nothing cuts
    for N in (128, 64):
        ln = Launch(lib, blob, rays, zs[N], white)
        r = alternate({"off": ln.off, "on": lambda: ln.on(1e-30)}, a.repeats, a.block)
        ln.cut.zero_()
        ln.on(1e-30)
        r["windows_cut"] = int(ln.cut.item())
        r["on_minus_off_ms"] = round(r["on"]["ms_median"] - r["off"]["ms_median"], 4)
        r["on_over_off"] = round(r["on"]["ms_median"] / r["off"]["ms_median"], 4)
        out[str(N)] = r
    return {"no_cut": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="another build of libnsr.so to compare the default path against")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=5, help="launches per timed block")
    ap.add_argument("--train-steps", type=int, default=4000, help="0 skips the trained fields")
    ap.add_argument("--out", default="")
    ap.add_argument("--stage", default="", help="internal: run this one step and print its part of the record")
    a = ap.parse_args()
    if a.stage:
        print("@@" + json.dumps(stage(a.stage, a)), flush=True)
        return
    # the driver touches no GPU: every step is a fresh child process under a time limit of its own, and nothing is started
    # after a step that fails, faults or runs out of time
    import subprocess
    from nerf_sr_amd import build
    res = {"source_hash": build.source_hash()[:16],
           "protocol": f"{a.repeats} alternating runs, each of {a.block} launches; whole frames of BASELINE config #2 / #3 geometry; "
                       "one process per step, alternation inside it"}
    for name in STAGES:
        if (name == "off_vs_parent" and not a.parent_lib) or (name.startswith("trained_") and a.train_steps <= 0):
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
            res.setdefault(k, {}).update(v)
        print(json.dumps({name: json.loads(part[-1][2:])}), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
