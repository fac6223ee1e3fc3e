#!/usr/bin/env python3
"""A/B of the weight DMA by constant per-wave shares ("Constant shares"): the parent commit's libnsr against this
tree's, alternated on one MI355X, after the protocol of scripts/ab_fold_final.py (whose helpers this script uses).

    bench         bench.py --gpus 1 --steps 20 --warmup 5: five runs each of config #2, one each of #3 and #4, the library
                  chosen per run through NSR_LIB_PATH, the sides alternating; one run per side and config dumps its outputs
                  (--dump-outputs) and every dumped array of #2, #3 and #4 must be numpy.array_equal to the parent's
    kernel_stats  one bench run per side under rocprofv3 --kernel-trace --stats, each in a process of its own: the share of
                  the mlp_f16x3_kernel launches in the kernel time
    train         bench.py --mode train, three runs per side, alternating: the training step keeps the run-time shares and must
                  not be slower than the parent beyond its spread
    isa           (no GPU) instruction counts of the two COMP listings (64 and 128 samples) and the kernel metadata of every
                  mlp_f16x3_kernel instantiation from build.compile_listing and -- with --parent-csrc DIR, the parent commit's
                  nerf_sr_amd/csrc -- the parent's

The driver itself touches no GPU: every step is a child process under a time limit of its own, and nothing is started after
a step that fails.  Every stage is recorded first; then the record is gated (--no-gate: record only): every dumped array
equal, the config #2 gain over three times the spread of the parent's own repeats, no scratch and no VGPR spill.

    python scripts/ab_dma_shares.py --parent-lib ab/libnsr_parent.so --out profiles/dma_shares_ab.json \
        [--stages bench,kernel_stats,train] [--parent-csrc DIR --stages isa]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
import ab_fold_final as fold  # noqa: E402

# derived from the parent's listing, not measured (the issue text of this change): per wave and trunk chunk about 8 x 2 scalar
# instructions and 4 x (s_and + branch) of ~1,860 cycles, of which about half returns as wall time on this power-limited kernel
PREDICTED = {"mainloop_cycles_percent": [-6.0, -5.0], "rays_per_s_percent": [2.0, 4.0],
             "source": "instruction counts of the parent's COMP listings; the guide's DVFS give-back of about one half"}
COMP = {"64": "ILi1ELb0ELi64ELb1ELb0ELb0E", "128": "ILi1ELb0ELi128ELb1ELb0ELb0E"}


def stage_bench(libs, dump_root):
    import numpy as np
    res = {"config2": {}, "config3": {}, "config4": {}}
    runs = {side: {"value": [], "launch_ms": [], "coarse_launch_ms": []} for side in libs}
    for i in range(5):
        for side, lib in libs.items():
            extra = ["--dump-outputs", os.path.join(dump_root, "config2", side)] if i == 0 else []
            r = fold.bench_line(lib, extra)
            for k in runs[side]:
                runs[side][k].append(r["value"] if k == "value" else r["roofline"][k])
            print(f"config #2 run {i} {side}: {r['value']:.0f} rays/s", flush=True)
    for side in libs:
        res["config2"][side] = {k: fold.med_spread(v) for k, v in runs[side].items()}
    p, n = res["config2"]["parent"], res["config2"]["new"]
    res["config2"]["gain_percent"] = 100.0 * (n["value"]["median"] / p["value"]["median"] - 1.0)
    res["config2"]["three_times_parent_spread_percent"] = 300.0 * p["value"]["spread"] / p["value"]["median"]
    res["config2"]["headline_claim_holds"] = n["value"]["median"] - p["value"]["median"] > 3.0 * p["value"]["spread"]
    res["config2"]["fine_launch_percent"] = 100.0 * (n["launch_ms"]["median"] / p["launch_ms"]["median"] - 1.0)
    res["config2"]["coarse_launch_percent"] = 100.0 * (n["coarse_launch_ms"]["median"] / p["coarse_launch_ms"]["median"] - 1.0)
    res["config2"]["predicted"] = PREDICTED
    for cfg in (3, 4):
        for side, lib in libs.items():
            r = fold.bench_line(lib, ["--config", str(cfg), "--dump-outputs", os.path.join(dump_root, f"config{cfg}", side)], 400)
            res[f"config{cfg}"][side] = {"value": r["value"], "ms_per_step": r["ms_per_step"]}
            print(f"config #{cfg} {side}: {r['value']:.0f} rays/s", flush=True)
        a, b = res[f"config{cfg}"]["parent"]["value"], res[f"config{cfg}"]["new"]["value"]
        res[f"config{cfg}"]["gain_percent"] = 100.0 * (b / a - 1.0)
    cmp = {}
    for cfg in (2, 3, 4):
        root = os.path.join(dump_root, f"config{cfg}")
        names = sorted(os.listdir(os.path.join(root, "parent")))
        assert names and names == sorted(os.listdir(os.path.join(root, "new"))), (cfg, names)
        cmp[f"config{cfg}"] = {name[:-4]: bool(np.array_equal(np.load(os.path.join(root, "parent", name)), np.load(os.path.join(root, "new", name))))
                               for name in names}
    res["dumped_outputs_array_equal"] = cmp
    return res


def stage_kernel_stats(libs, scratch):
    import csv
    share = {}
    for side, lib in libs.items():
        d = os.path.join(scratch, "prof_" + side)
        env = dict(os.environ, NSR_LIB_PATH=os.path.abspath(lib))
        fold.child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
                    "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 300, env)
        found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
        rows = list(csv.DictReader(open(found[0])))
        share[side] = sum(float(r["Percentage"]) for r in rows if "mlp_f16x3_kernel" in r["Name"])
    return {"mlp_f16x3_kernel_percent_of_kernel_time": share}


def stage_train(libs):
    runs = {side: [] for side in libs}
    for i in range(3):
        for side, lib in libs.items():
            r = fold.bench_line(lib, ["--mode", "train"], 200)
            runs[side].append(r["value"])
            print(f"train run {i} {side}: {r['value']:.0f} rays/s", flush=True)
    res = {side: fold.med_spread(v) for side, v in runs.items()}
    res["gain_percent"] = 100.0 * (res["new"]["median"] / res["parent"]["median"] - 1.0)
    return res


def kernel_bodies(text):
    return {m.group(1).split("mlp_f16x3_kernel")[1].split("EvPKf")[0]: m.group(2)
            for m in re.finditer(r"^(_Z16mlp_f16x3_kernel\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)}


def count(body):
    """Static counts of one kernel body.  `scalar_in_front_of_dma_sites`: the s_* instructions among the five in front of each
    LDS-DMA instruction (each counted once); a site is `behind a branch` when one of the eight in front of it is a s_cbranch."""
    ins = [c for c in (line.split(";")[0].strip() for line in body.split("\n")) if c and not c.endswith(":") and not c.startswith(".")]
    sites = [i for i, c in enumerate(ins) if c.startswith("global_load_lds_dword")]
    front = {j for i in sites for j in range(max(0, i - 5), i) if ins[j].startswith("s_")}
    n = lambda prefix: sum(1 for c in ins if c.startswith(prefix))
    return {"instructions": len(ins), "mfma": n("v_mfma"), "instructions_per_mfma": round(len(ins) / n("v_mfma"), 3),
            "dma_sites": len(sites), "dma_sites_dword_form": sum(1 for i in sites if not ins[i].startswith("global_load_lds_dwordx4")),
            "scalar_in_front_of_dma_sites": len(front), "scalar_in_front_per_dma_site": round(len(front) / len(sites), 3),
            "dma_sites_behind_a_branch": sum(1 for i in sites if any(ins[j].startswith("s_cbranch") for j in range(max(0, i - 8), i))),
            "branches": n("s_cbranch"), "v_readlane": n("v_readlane"), "s_nop": n("s_nop")}


def stage_isa(parent_csrc):
    from nerf_sr_amd import build

    def listing(path):
        if not path:
            return build.compile_listing("nsr_mlp_f16.hip")
        out = os.path.join(tempfile.mkdtemp(), "parent.s")
        subprocess.check_call([build._hipcc(), *build.ISA_FLAGS, os.path.join(path, "nsr_mlp_f16.hip"), "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()

    def meta(text):
        out = {}
        for b in text.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", b).group(1)
            if "mlp_f16x3_kernel" in name:
                g = lambda k: int(re.search(r"\.%s:\s+(\S+)" % k, b).group(1))
                out[name.split("mlp_f16x3_kernel")[1].split("EvPKf")[0]] = {
                    "vgpr_count": g("vgpr_count"), "agpr_count": int(b.split()[0]), "vgpr_spill_count": g("vgpr_spill_count"),
                    "sgpr_spill_count": g("sgpr_spill_count"), "private_segment_fixed_size": g("private_segment_fixed_size")}
        return out

    res = {"template_arguments": "<MODE, SIGMA_ONLY, NS, COMP, TRAIN, ERT> as mangled (I = int, Lb = bool)",
           "note": ("static counts; the parent's listing runs the body of a trunk pair three times per window, this build's runs the "
                    "plain pair twice and the pair around the skip layer, a body of its own, once: the MFMA counts differ, the "
                    "per-MFMA and per-site figures compare")}
    for side, path in (("new", None), ("parent", parent_csrc)):
        if side == "parent" and not path:
            continue
        text = listing(path)
        bodies = kernel_bodies(text)
        res[side] = {"metadata": meta(text), "comp_listings": {ns: count(bodies[k]) for ns, k in COMP.items()}}
    return res


def gate(res):
    bad = []
    for cfg, arrays in res.get("dumped_outputs_array_equal", {}).items():
        bad += [f"{cfg}: {k} differs from the parent's" for k, same in arrays.items() if not same]
    if "config2" in res and not res["config2"]["headline_claim_holds"]:
        bad.append("config #2 gain within three times the parent's spread")
    for name, m in res.get("isa", {}).get("new", {}).get("metadata", {}).items():
        if m["vgpr_spill_count"] or m["private_segment_fixed_size"]:
            bad.append(f"{name}: VGPR spill or scratch")
    if bad:
        raise SystemExit("gate: " + "; ".join(bad))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="ab/libnsr_parent.so")
    ap.add_argument("--new-lib", default="nerf_sr_amd/libnsr.so")
    ap.add_argument("--out", default="profiles/dma_shares_ab.json")
    ap.add_argument("--stages", default="bench,kernel_stats")
    ap.add_argument("--parent-csrc", default="", help="isa: the parent commit's nerf_sr_amd/csrc")
    ap.add_argument("--no-gate", action="store_true")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "nsr_dma_shares_ab"), help="dumps and intermediate files")
    a = ap.parse_args()
    libs = {"parent": a.parent_lib, "new": a.new_lib}
    scratch = os.path.join(REPO, a.scratch)
    os.makedirs(scratch, exist_ok=True)
    out_path = os.path.join(REPO, a.out)
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["what"] = ("parent commit vs this build, alternated on one MI355X: bench.py --gpus 1 --steps 20 --warmup 5, five runs each of "
                   "config #2, one each of #3 and #4 (scripts/ab_dma_shares.py); prediction, static counts and measurement side by side")
    for stage in a.stages.split(","):
        if stage == "bench":
            res.update(stage_bench(libs, os.path.join(scratch, "dump")))
        elif stage == "kernel_stats":
            res["kernel_stats"] = stage_kernel_stats(libs, scratch)
        elif stage == "train":
            res["train_mode"] = stage_train(libs)
        elif stage == "isa":
            res["isa"] = stage_isa(a.parent_csrc)
        else:
            raise SystemExit(f"unknown stage {stage!r}")
        json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res, indent=1))
    if not a.no_gate:
        gate(res)


if __name__ == "__main__":
    main()
