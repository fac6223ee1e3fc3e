#!/usr/bin/env python3
"""A/B of the fold of xyz_encoding_final into dir_encoding ("The fold"): the parent commit's libnsr against this
tree's, alternated on one MI355X, after the protocol of profiles/empty_skip_ab.json.

    bench       bench.py --gpus 1 --steps 20 --warmup 5: five runs each of config #2, one each of #3 and #4, the library
                chosen per run through NSR_LIB_PATH, the sides alternating; the first config #2 run of each side dumps its
                outputs (--dump-outputs) and the dumps are compared array by array
    fields      the 128-sample render launch of config #2's 190,512 rays alone (nsr_render_rays_composited through the C ABI,
                both libraries in one process, alternating blocks) on three fields: the bench's fine network, every density
                > 0 (sigma.bias = +1e3: no window is empty) and every density < 0 (sigma.bias = -1e3: every window is)
    raw_launch  scripts/ab_libs.py 5 parent=... new=...: the project's library alternator on the UNFUSED 128-sample network
                launch (nsr_render_rays, no compositing, random rays), as every earlier ladder ran it
    parity      bench.py --full --no-extras --no-config4 once per side: the `parity` block against the oracle
    kernel_stats  one bench run per side under rocprofv3 --kernel-trace --stats; the two tables, a `Side` column in front,
                become --stats-csv (profiles/fold_final_kernel_stats.csv) and the fold kernel's duration goes into the record
    isa         (no GPU) kernel metadata of every mlp_f16x3_kernel instantiation from build.compile_listing, and -- with
                --parent-csrc DIR, the parent commit's nerf_sr_amd/csrc -- the parent's, plus whether the TRAIN body is
                byte-identical once basic-block label numbers and comments are stripped

The driver itself touches no GPU: every step is a child process under a time limit of its own, and nothing is started after
a step that fails.  Every stage is recorded first; then the record is gated (--no-gate: record only): the six density-side
arrays `array_equal`, `rays_over_1e-4` 0 on both sides, the config #2 gain over three times the parent's spread.  A stage run
later (another call, --stages isa on a host with the parent's sources) adds to the record that --out already holds.

    python scripts/ab_fold_final.py --parent-lib ab/libnsr_parent.so --out profiles/fold_final_ab.json \
        [--stages bench,fields,raw_launch,parity,kernel_stats] [--parent-csrc DIR --stages isa]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PREDICTED = {"fine_launch_percent": -7.9, "coarse_launch_percent": -8.2, "source": "k-step counts, 1,184 -> 1,056 per live window"}


def child(cmd, limit, env=None):
    """One GPU step: a fresh process under its own time limit; raises on any failure (the caller starts nothing more)."""
    p = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"step failed (exit {p.returncode}): {' '.join(cmd)}")
    return p.stdout


def bench_line(lib, extra, limit=300):
    env = dict(os.environ, NSR_LIB_PATH=os.path.abspath(lib))
    out = child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"] + extra, limit, env)
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def med_spread(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "runs": v}


def stage_bench(libs, dump_root):
    import numpy as np
    res = {"config2": {}, "config3": {}, "config4": {}}
    runs = {side: {"value": [], "launch_ms": [], "coarse_launch_ms": []} for side in libs}
    for i in range(5):
        for side, lib in libs.items():
            extra = ["--dump-outputs", os.path.join(dump_root, side)] if i == 0 else []
            r = bench_line(lib, extra)
            for k in runs[side]:
                runs[side][k].append(r["value"] if k == "value" else r["roofline"][k])
            print(f"config #2 run {i} {side}: {r['value']:.0f} rays/s", flush=True)
    for side in libs:
        res["config2"][side] = {k: med_spread(v) for k, v in runs[side].items()}
    p, n = res["config2"]["parent"], res["config2"]["new"]
    res["config2"]["gain_percent"] = 100.0 * (n["value"]["median"] / p["value"]["median"] - 1.0)
    res["config2"]["three_times_parent_spread_percent"] = 300.0 * p["value"]["spread"] / p["value"]["median"]
    res["config2"]["headline_claim_holds"] = n["value"]["median"] - p["value"]["median"] > 3.0 * p["value"]["spread"]
    res["config2"]["fine_launch_percent"] = 100.0 * (n["launch_ms"]["median"] / p["launch_ms"]["median"] - 1.0)
    res["config2"]["coarse_launch_percent"] = 100.0 * (n["coarse_launch_ms"]["median"] / p["coarse_launch_ms"]["median"] - 1.0)
    res["config2"]["predicted"] = PREDICTED
    for cfg in (3, 4):
        for side, lib in libs.items():
            r = bench_line(lib, ["--config", str(cfg)], 400)
            res[f"config{cfg}"][side] = {"value": r["value"], "ms_per_step": r["ms_per_step"]}
            print(f"config #{cfg} {side}: {r['value']:.0f} rays/s", flush=True)
    cmp = {}
    for name in sorted(os.listdir(os.path.join(dump_root, "parent"))):
        a, b = (np.load(os.path.join(dump_root, s, name)).astype(np.float64) for s in ("parent", "new"))
        d = np.abs(a - b)
        cmp[name[:-4]] = {"array_equal": bool(np.array_equal(a, b)), "max_abs": float(d.max()), "p999_abs": float(np.quantile(d, 0.999))}
    res["dumped_outputs_config2"] = cmp
    return res


def stage_fields_child(libs, out_path, repeats=5, block=4):
    """(child process) the fine launch alone, both libraries in this process"""
    import numpy as np
    import torch
    from nerf_sr_amd import _lib, cameras, ops
    from nerf_sr_amd.weights import make_state_dict, STATE_DICT_SPEC
    F16X3 = _lib.NSR_F16X3
    rays = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True).reshape(-1, 8).contiguous()
    R, N = rays.shape[0], 128
    z, _ = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)
    outs = [torch.empty(s, device="cuda") for s in ((R, 3), (R,), (R,), (R, N))]
    base = make_state_dict(100)
    fields = {"smooth": base, "all_sigma_positive": dict(base, **{"sigma.bias": np.full((1,), 1e3, np.float32)}),
              "all_sigma_negative": dict(base, **{"sigma.bias": np.full((1,), -1e3, np.float32)})}
    handles = {}
    for side, path in libs.items():
        L = ctypes.CDLL(os.path.abspath(path))
        for name in ("nsr_packed_weights_bytes", "nsr_pack_weights", "nsr_render_rays_composited"):
            getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
        handles[side] = L
    res = {}
    for fname, sd in fields.items():
        dev = [torch.from_numpy(np.ascontiguousarray(sd[k])).float().cuda() for k in STATE_DICT_SPEC]
        ptrs = (ctypes.c_void_p * len(dev))(*[ctypes.c_void_p(t.data_ptr()) for t in dev])
        fns = {}
        for side, L in handles.items():
            blob = torch.zeros(L.nsr_packed_weights_bytes(F16X3), dtype=torch.uint8, device="cuda")
            t0 = time.perf_counter()
            assert L.nsr_pack_weights(ptrs, blob.data_ptr(), F16X3, None) == 0
            pack_ms = (time.perf_counter() - t0) * 1e3          # nsr_pack_weights waits for the stream (it reads the status word)

            def run(L=L, blob=blob):
                rc = L.nsr_render_rays_composited(blob.data_ptr(), F16X3, rays.data_ptr(), 8, z.data_ptr(), R, N, 0, None,
                                                  *[o.data_ptr() for o in outs], None)
                assert rc == 0, rc
            fns[side] = (run, blob, pack_ms)
        t = {side: [] for side in fns}
        for run, _, _ in fns.values():
            run(); run()
        for _ in range(repeats):
            for side, (run, _, _) in fns.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(block):
                    run()
                torch.cuda.synchronize(); t[side].append((time.perf_counter() - t0) * 1e3 / block)
        res[fname] = {side: dict(med_spread(v), pack_call_ms=fns[side][2]) for side, v in t.items()}
        res[fname]["change_percent"] = 100.0 * (res[fname]["new"]["median"] / res[fname]["parent"]["median"] - 1.0)
        print(fname, json.dumps(res[fname]), flush=True)
    json.dump(res, open(out_path, "w"))


def stage_kernel_stats(libs, scratch, csv_path):
    import csv
    rows, fold_us = [], None
    for side, lib in libs.items():
        d = os.path.join(scratch, "prof_" + side)
        env = dict(os.environ, NSR_LIB_PATH=os.path.abspath(lib))
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 300, env)
        found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
        for r in csv.DictReader(open(found[0])):
            rows.append(dict(Side=side, **r))
            if r["Name"].startswith("fold_final_kernel"):
                fold_us = float(r["AverageNs"]) / 1e3
    with open(csv_path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        w.writerows(rows)
    mlp = {side: sum(float(r["Percentage"]) for r in rows if r["Side"] == side and "mlp_f16x3_kernel" in r["Name"]) for side in libs}
    return {"csv": os.path.relpath(csv_path, REPO), "fold_kernel_us_per_network": fold_us, "mlp_f16x3_kernel_percent_of_kernel_time": mlp}


def stage_isa(parent_csrc):
    import re
    from nerf_sr_amd import build

    def listing(path):
        if path is None:
            return build.compile_listing("nsr_mlp_f16.hip")
        out = os.path.join(tempfile.mkdtemp(), "parent.s")
        subprocess.check_call([build._hipcc(), *build.ISA_FLAGS, os.path.join(path, "nsr_mlp_f16.hip"), "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()

    def meta(text):
        out = {}
        for b in text.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", b).group(1)
            if "mlp_f16x3_kernel" not in name:
                continue
            g = lambda k: int(re.search(r"\.%s:\s+(\S+)" % k, b).group(1))
            out[name.split("mlp_f16x3_kernel")[1].split("EvPKf")[0]] = {
                "vgpr_count": g("vgpr_count"), "agpr_count": int(b.split()[0]), "vgpr_spill_count": g("vgpr_spill_count"),
                "sgpr_spill_count": g("sgpr_spill_count"), "private_segment_fixed_size": g("private_segment_fixed_size")}
        return out

    def train_body(text):
        name = re.findall(r"^(_Z16mlp_f16x3_kernelILi1ELb0ELi0ELb0ELb1ELb0E\S*):", text, re.M)[0]
        i = text.index("\n" + name + ":")
        body = re.sub(r";.*", "", re.sub(r"\.LBB\d+_", ".LBB_", text[i:text.index(".Lfunc_end", i)]))
        return [l.rstrip() for l in body.splitlines()]

    new = listing(None)
    res = {"template_arguments": "<MODE, SIGMA_ONLY, NS, COMP, TRAIN, ERT> as mangled (I = int, Lb = bool)", "new": meta(new)}
    assert all(m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0 for m in res["new"].values()), res["new"]
    if parent_csrc:
        old = listing(parent_csrc)
        res["parent"] = meta(old)
        a, b = train_body(old), train_body(new)
        res["train_body_lines"] = len(b)
        res["train_body_identical_apart_from_label_numbers"] = a == b
    return res


def gate(res):
    bad = []
    for k in ("coarse_weights", "fine_weights", "coarse_depth", "fine_depth", "coarse_opacity", "fine_opacity"):
        if "dumped_outputs_config2" in res and not res["dumped_outputs_config2"][k]["array_equal"]:
            bad.append(k + " differs from the parent's")
    for side, p in res.get("parity_vs_oracle", {}).items():
        if p["rays_over_1e-4"] != 0:
            bad.append(f"{side}: rays_over_1e-4 = {p['rays_over_1e-4']}")
    if "config2" in res and not res["config2"]["headline_claim_holds"]:
        bad.append("config #2 gain within three times the parent's spread")
    if res.get("isa_metadata", {}).get("train_body_identical_apart_from_label_numbers") is False:
        bad.append("TRAIN body differs from the parent's")
    if bad:
        raise SystemExit("gate: " + "; ".join(bad))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="ab/libnsr_parent.so")
    ap.add_argument("--new-lib", default="nerf_sr_amd/libnsr.so")
    ap.add_argument("--out", default="profiles/fold_final_ab.json")
    ap.add_argument("--stages", default="bench,fields,raw_launch,parity,kernel_stats")
    ap.add_argument("--stats-csv", default="profiles/fold_final_kernel_stats.csv")
    ap.add_argument("--parent-csrc", default="", help="isa: the parent commit's nerf_sr_amd/csrc")
    ap.add_argument("--no-gate", action="store_true")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "nsr_fold_ab"), help="dumps and intermediate files")
    ap.add_argument("--fields-child", default="")
    a = ap.parse_args()
    libs = {"parent": a.parent_lib, "new": a.new_lib}
    if a.fields_child:
        return stage_fields_child(libs, a.fields_child)
    os.makedirs(os.path.join(REPO, a.scratch), exist_ok=True)
    out_path = os.path.join(REPO, a.out)
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["what"] = ("parent commit vs this build, alternated on one MI355X: bench.py --gpus 1 --steps 20 --warmup 5, five runs each of "
                   "config #2, one each of #3 and #4 (scripts/ab_fold_final.py); CPU study in front of it: profiles/fold_final_study.txt")
    for stage in a.stages.split(","):
        if stage == "bench":
            res.update(stage_bench(libs, os.path.join(REPO, a.scratch, "dump")))
        elif stage == "fields":
            tmp = os.path.join(REPO, a.scratch, "fields.json")
            print(child([sys.executable, os.path.abspath(__file__), "--parent-lib", a.parent_lib, "--new-lib", a.new_lib,
                         "--fields-child", tmp], 300), flush=True)
            res["fine_launch_alone_ms"] = json.load(open(tmp))
        elif stage == "parity":
            res["parity_vs_oracle"] = {}
            for side, lib in libs.items():
                r = bench_line(lib, ["--full", "--no-extras", "--no-config4"], 900)
                res["parity_vs_oracle"][side] = r["parity"]
                print(f"parity {side}: {json.dumps(r['parity'])}", flush=True)
        elif stage == "raw_launch":
            tmp = os.path.join(REPO, a.scratch, "ab_libs.json")
            print(child([sys.executable, "scripts/ab_libs.py", "5", f"parent={os.path.abspath(a.parent_lib)}",
                         f"new={os.path.abspath(a.new_lib)}", "--json", tmp], 300), flush=True)
            r = json.load(open(tmp))
            r["change_percent"] = 100.0 * (r["new"]["ms_median"] / r["parent"]["ms_median"] - 1.0)
            res["raw_128_sample_launch_ab_libs"] = r
        elif stage == "kernel_stats":
            res["kernel_stats"] = stage_kernel_stats(libs, os.path.join(REPO, a.scratch), os.path.join(REPO, a.stats_csv))
        elif stage == "isa":
            res["isa_metadata"] = stage_isa(a.parent_csrc)
        else:
            raise SystemExit(f"unknown stage {stage!r}")
        if "config2" in res:      # the timeline stamps of the trunk's tail are called for only when the launches miss half the prediction
            c = res["config2"]
            short = [k for k in ("fine_launch_percent", "coarse_launch_percent") if c[k] > 0.5 * PREDICTED[k]]
            res["timeline_stamps"] = (f"called for: {short} under half the prediction" if short else
                                      "not called for: both launches changed by more than half the k-step prediction")
        json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res, indent=1))
    if not a.no_gate:
        gate(res)


if __name__ == "__main__":
    main()
