#!/usr/bin/env python3
"""Bit-for-bit A/B of the training entry points between this tree's library and the parent commit's, for the change that made
the descriptor-driven network the only layer-by-layer implementation.

    python scripts/ab_train_unify.py --build-parent HEAD~1          # CPU box: the parent's library into ab/libnsr_parent.so
    python scripts/ab_train_unify.py --out profiles/train_unify_ab.json

Every group of cases runs in a child process per library (NSR_LIB_PATH), the two libraries alternated, each child under its
own time limit; a child that fails ends the run.  Inputs: tests/golden/train_llff_rand.npz and the four cases of
tests/golden/train_arch.npz.  Compared with numpy.array_equal:

  a) every chain precision: the eight outputs and 48 gradient tensors of the fused step and of the autograd pair, the weights
     after 4 optimize_parameters steps                                                       new == parent
  b) the four non-default cases through arch=, both layer-by-layer precisions: outputs, gradients          new == parent
  c) the default network on fp32 / f16x3_gemm through (i) the pair with arch=None, (ii) the fused step, (iii) the pair with
     arch=DEFAULT_ARCH, all under the step's own loss:  new (i) == new (iii) == parent (iii); (ii) against (i) is reported for
     both libraries (how many of the outputs / gradient tensors are bit-equal, the largest relative distance)
  d) nsr_adam_step on random state                                                                        new == parent
and the distance new (i) to parent (i) per precision (not zero, fp32 included: dir_encoding's forward sums its direction terms in
another order since its input lost the four columns in front of them).

    python scripts/ab_train_unify.py --timing profiles/train_unify_timing.json

times both libraries interleaved in one call: scripts/time_train_arch.py once per library, then five alternating runs per
library of `bench.py --mode train` at --train-precision f16x3, f16x3_gemm and fp32 (ms_per_step of its JSON line).  Per figure:
the parent's and the new median, the spread (max - min) of the parent's repeats, and whether the new median stays within the
parent's median + spread (chain path: its code is unchanged) or + 3 x spread (layer-by-layer precisions).
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
PARENT_LIB = os.path.join(ROOT, "ab", "libnsr_parent.so")
CHAIN = ("f16x3", "f16x3_bwd3", "f16x3_bwd2", "f16x3_bwd1", "f16x3_bwdm")
GEMM = ("fp32", "f16x3_gemm")
GROUPS = ("chain", "arch", "default")      # `default` also runs d)


def build_parent(rev):
    """The library of commit `rev`, built by that commit's own build script from an export of its tree."""
    tmp = tempfile.mkdtemp(prefix="nsr_parent_")
    try:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "nerf_sr_amd", "include", "tests/csrc"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        subprocess.run([sys.executable, "-c", "from nerf_sr_amd import build; build.build(verbose=False)"], cwd=tmp, check=True)
        os.makedirs(os.path.dirname(PARENT_LIB), exist_ok=True)
        shutil.copy(os.path.join(tmp, "nerf_sr_amd", "libnsr.so"), PARENT_LIB)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(PARENT_LIB)


# ---- child: one group on the library NSR_LIB_PATH selects ---------------------------------------------------------------
def child(group, out_path):
    import torch
    from nerf_sr_amd import train as tr
    from nerf_sr_amd.weights import make_state_dict
    from tests import arch_util as au
    from tests.util import train_draws

    res = {}

    def put(prefix, out=None, grads=None, **more):
        for k, v in (out or {}).items():
            res[f"{prefix}.out.{k}"] = v.detach().cpu().numpy()
        for n, gs in enumerate(grads or ()):
            for k, v in gs.items():
                res[f"{prefix}.grad{n}.{k}"] = v.detach().cpu().numpy()
        for k, v in more.items():
            res[f"{prefix}.{k}"] = v.detach().cpu().numpy()

    g = np.load(os.path.join(GOLDEN, "train_llff_rand.npz"))
    draws = {k: v for k, v in train_draws(g).items() if k != "noise_std"}

    def trainer(**kw):
        t = tr.Trainer(make_state_dict(int(g["seed_coarse"])), make_state_dict(int(g["seed_fine"])), white_bkgd=bool(g["white_bkgd"]),
                       downscale=int(round(int(g["s2"]) ** 0.5)), randomized=bool(g["randomized"]), noise_std=float(g["noise_std"]),
                       lr=float(g["lr"]), beta1=float(g["beta1"]), lambda_coarse_mse=float(g["lambda_coarse"]),
                       lambda_fine_mse=float(g["lambda_fine"]), **kw)
        t.set_input(torch.from_numpy(g["rays"]).cuda(), torch.from_numpy(g["target_lr"]).cuda())
        return t

    def pair(t, d):      # the step's own loss, written in torch over the autograd pair
        out = t.forward(d)
        s2 = t.s2
        mse = torch.nn.functional.mse_loss
        lc = mse(out["coarse_comp_rgbs"].reshape(-1, s2, 3).mean(1), t.data_rgbs) * t.lambda_coarse
        lf = mse(out["fine_comp_rgbs"].reshape(-1, s2, 3).mean(1), t.data_rgbs) * t.lambda_fine
        t.backward(lc + lf)
        return {k: out[k] for k in tr.OUT_KEYS}, torch.stack([lc.detach(), lf.detach()])

    if group == "chain":
        for prec in CHAIN:
            t = trainer(precision=prec)
            t.loss_and_grads(draws)
            put(f"a.{prec}.fused", {k: t.out[k] for k in tr.OUT_KEYS}, t.grads, losses=t.losses)
            t = trainer(precision=prec)
            out, losses = pair(t, draws)
            put(f"a.{prec}.pair", out, t.grads, losses=losses)
            t = trainer(precision=prec)
            for i in range(4):
                torch.manual_seed(100 + i)
                t.optimize_parameters()
            put(f"a.{prec}.steps4", None, t.params)
    elif group == "arch":
        for tag in au.CASES:
            c = au.load_case(GOLDEN, tag)
            for prec in GEMM:
                sds = au.state_dicts(c)
                p = [{k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in sd.items()} for sd in sds]
                out = tr.forward_rays_train(p[0], p[1], torch.from_numpy(c["rays"]).cuda(), au.draws_of(c), white_bkgd=bool(c["white_bkgd"]),
                                            noise_std=float(c["noise_std"]), precision=prec, arch=c["arch"])
                loss = sum(out[k].square().sum() for k in tr.OUT_KEYS)      # every output's upstream gradient is set
                grads = torch.autograd.grad(loss, [p[n][k] for n in range(2) for k in p[n]])
                nt = len(p[0])
                put(f"b.{tag}.{prec}", out, [dict(zip(p[0], grads[:nt])), dict(zip(p[1], grads[nt:]))])
    elif group == "default":
        for prec in GEMM:
            t = trainer(precision=prec)
            out, losses = pair(t, draws)
            put(f"c.{prec}.i", out, t.grads, losses=losses)
            t = trainer(precision=prec)
            t.loss_and_grads(draws)
            put(f"c.{prec}.ii", {k: t.out[k] for k in tr.OUT_KEYS}, t.grads, losses=t.losses)
            t = trainer(precision=prec, arch=au.DEFAULT_ARCH)
            out, losses = pair(t, draws)
            put(f"c.{prec}.iii", out, t.grads, losses=losses)
        gen = torch.Generator().manual_seed(5)
        spec = make_state_dict(1)
        p = {k: torch.randn(*v.shape, generator=gen) for k, v in spec.items()}
        t = tr.Trainer(p, p)
        for k in spec:
            t.grads[0][k].copy_(torch.randn(*spec[k].shape, generator=gen) * 1e-2)
            t.exp_avg[0][k].copy_(torch.randn(*spec[k].shape, generator=gen) * 1e-3)
            t.exp_avg_sq[0][k].copy_(torch.rand(*spec[k].shape, generator=gen) * 1e-5)
        t.step = 6
        t.optimizer_step()
        put("d.adam", None, [t.params[0], t.exp_avg[0], t.exp_avg_sq[0]])
    else:
        raise SystemExit(f"unknown group {group}")
    torch.cuda.synchronize()
    np.savez(out_path, **res)


# ---- parent process: alternate the libraries, compare ---------------------------------------------------------------------
def rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    n = float(np.linalg.norm(a))
    return float(np.linalg.norm(a - b)) / n if n > 0 else float(np.linalg.norm(b))


def compare(x, y, px, py):
    """Keys under prefix px of x against the same keys under py of y: (n, n_equal, worst relative distance, its key)."""
    keys = sorted(k[len(px):] for k in x if k.startswith(px))
    assert keys and keys == sorted(k[len(py):] for k in y if k.startswith(py)), (px, py)
    eq, worst = 0, (0.0, None)
    for k in keys:
        a, b = x[px + k], y[py + k]
        if np.array_equal(a, b):
            eq += 1
        else:
            d = rel(a, b)
            worst = max(worst, (d, k), key=lambda t: t[0])
    return {"tensors": len(keys), "bit_equal": eq, "worst_relative_distance": worst[0], "worst": worst[1]}


def last_json(text):
    return json.loads([l for l in text.strip().splitlines() if l.startswith("{")][-1])


def timing(libs, out_path, per_child):
    import statistics

    def run(cmd, path):
        r = subprocess.run([sys.executable, *cmd], env=dict(os.environ, NSR_LIB_PATH=path), cwd=ROOT, timeout=per_child,
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"{cmd} ended with status {r.returncode}: nothing more is started")
        return last_json(r.stdout)

    res = {"libraries": {k: os.path.relpath(v, ROOT) for k, v in libs.items()}, "pair": {}, "bench_train": {}}
    pair = {name: run(["scripts/time_train_arch.py"], path) for name, path in libs.items()}
    res["device"] = pair["new"]["device"]
    res["pair_shape"] = pair["new"]["shape"]
    for v, p in pair["parent"]["variants"].items():
        runs_p, runs_n = p["ms_per_step_runs"], pair["new"]["variants"][v]["ms_per_step_runs"]
        spread = max(runs_p) - min(runs_p)
        med_p, med_n = statistics.median(runs_p), statistics.median(runs_n)
        res["pair"][v] = {"parent_ms": med_p, "new_ms": med_n, "parent_runs": runs_p, "new_runs": runs_n, "parent_spread_ms": round(spread, 4),
                          "met": bool(med_n <= med_p + 3.0 * spread)}
    for prec in ("f16x3", "f16x3_gemm", "fp32"):
        runs = {"parent": [], "new": []}
        for _ in range(5):
            for name in ("parent", "new"):
                runs[name].append(run(["bench.py", "--gpus", "1", "--mode", "train", "--train-precision", prec, "--steps", "25",
                                       "--warmup", "5", "--no-cpu-baseline"], libs[name])["ms_per_step"])
        spread = max(runs["parent"]) - min(runs["parent"])
        med_p, med_n = statistics.median(runs["parent"]), statistics.median(runs["new"])
        margin = spread if prec == "f16x3" else 3.0 * spread
        res["bench_train"][prec] = {"parent_ms": med_p, "new_ms": med_n, "parent_runs": runs["parent"], "new_runs": runs["new"],
                                    "parent_spread_ms": round(spread, 4), "bound_ms": round(med_p + margin, 4), "met": bool(med_n <= med_p + margin)}
        print(prec, json.dumps(res["bench_train"][prec]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: {v: d["met"] for v, d in res[k].items()} for k in ("pair", "bench_train")}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", metavar="OUT", default="")
    ap.add_argument("--build-parent", metavar="REV", default="")
    ap.add_argument("--child", nargs=2, metavar=("GROUP", "OUT"))
    ap.add_argument("--parent-lib", default=PARENT_LIB)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_unify_ab.json"))
    a = ap.parse_args()
    if a.build_parent:
        return build_parent(a.build_parent)
    if a.child:
        return child(*a.child)
    if not os.path.exists(a.parent_lib):
        raise SystemExit(f"{a.parent_lib}: build it first (--build-parent REV)")
    from nerf_sr_amd import _lib
    libs = {"new": os.path.join(ROOT, "nerf_sr_amd", "libnsr.so"), "parent": a.parent_lib}
    if a.timing:
        return timing(libs, a.timing, a.timeout)
    data = {"new": {}, "parent": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for group in GROUPS:
            for name, path in libs.items():
                out = os.path.join(tmp, f"{name}_{group}.npz")
                env = dict(os.environ, NSR_LIB_PATH=path)
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", group, out], env=env, cwd=ROOT,
                                    timeout=a.timeout).returncode
                if rc != 0:
                    raise SystemExit(f"child {group} on {name} ended with status {rc}: nothing more is started")
                with np.load(out) as z:
                    data[name].update({k: z[k] for k in z.files})
                print(f"{group} {name}: {len(data[name])} arrays so far", flush=True)
    new, par = data["new"], data["parent"]
    res = {"libraries": {k: os.path.relpath(v, ROOT) for k, v in libs.items()}, "version": int(_lib.load().nsr_version()), "a_chain_new_vs_parent": {}, "b_arch_new_vs_parent": {},
           "c_default": {}, "d_adam_new_vs_parent": compare(new, par, "d.adam.", "d.adam.")}
    for prec in CHAIN:
        res["a_chain_new_vs_parent"][prec] = compare(new, par, f"a.{prec}.", f"a.{prec}.")
    from tests import arch_util as au
    for tag in au.CASES:
        for prec in GEMM:
            res["b_arch_new_vs_parent"][f"{tag}.{prec}"] = compare(new, par, f"b.{tag}.{prec}.", f"b.{tag}.{prec}.")
    for prec in GEMM:
        p = f"c.{prec}."
        res["c_default"][prec] = {
            "new_i_vs_new_iii": compare(new, new, p + "i.", p + "iii."),
            "new_iii_vs_parent_iii": compare(new, par, p + "iii.", p + "iii."),
            "new_ii_vs_new_i": compare(new, new, p + "i.", p + "ii."),
            "parent_ii_vs_parent_i": compare(par, par, p + "i.", p + "ii."),
            "parent_ii_vs_parent_iii": compare(par, par, p + "iii.", p + "ii."),
            "new_ii_vs_parent_ii": compare(new, par, p + "ii.", p + "ii."),
            "new_i_vs_parent_i": compare(new, par, p + "i.", p + "i."),
        }
    same = lambda d: d["bit_equal"] == d["tensors"]
    res["verdict"] = {
        "a": all(same(v) for v in res["a_chain_new_vs_parent"].values()),
        "b": all(same(v) for v in res["b_arch_new_vs_parent"].values()),
        "c": all(same(v["new_i_vs_new_iii"]) and same(v["new_iii_vs_parent_iii"]) for v in res["c_default"].values()),
        "d": same(res["d_adam_new_vs_parent"]),
    }
    print(json.dumps(res["verdict"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    return 0 if all(res["verdict"].values()) else 1


if __name__ == "__main__":
    sys.exit(main() or 0)
