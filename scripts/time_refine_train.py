#!/usr/bin/env python3
"""Cost of one training iteration of the refinement network (forward -> torch L1 -> backward -> Adam) at the reference's
batch (scripts/train_llff_refine.sh: 32 patch sets of 1 + 8 patches, 64 x 64), fp32:

    ours    nerf_sr_amd.refine.RefineTrainer.optimize_parameters (nsr_refine_train_forward / _backward, nsr_adam_step_n)
    torch   the restatement tests/refine_train_ref.py on the GPU in fp32 -- torch-ROCm's own convolutions, BatchNorm and
            autograd -- with torch.optim.Adam

`--repeats` (5) alternating runs of `--block` iterations each, every block timed by wall clock around a device
synchronisation.  Recorded, not gated: nobody had measured either number.  Prints one JSON object (also written to --out).

    python scripts/time_refine_train.py --out profiles/refine_train_timing.json
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_refine_train.py --only ours --repeats 1 --block 3

`--precision f16x3_mixed` times the trainer at that precision (forward and input gradients split-fp16, weight gradients fp32).
`--baseline-lib PATH` is the A/B against another build of the library -- the parent commit's, built beforehand as
ab/libnsr_parent.so: every timed block then runs in a CHILD process of its own (a library is chosen when the package is
imported: NSR_LIB_PATH), `--repeats` alternating rounds of

    parent_fp32   the baseline library's fp32 step      ours_fp32   this build's fp32 step
    ours_<precision>   this build at --precision        torch       the restatement

and the verdicts the project's yardstick asks for are recorded: the new precision faster than the parent's fp32 step by more
than three times the spread of the parent's repeats, this build's fp32 step within that spread of the parent's.

    python scripts/time_refine_train.py --precision f16x3_mixed --baseline-lib ab/libnsr_parent.so \
        --out profiles/refine_train_mixed_timing.json

`--weight-grad f16x3` times the trainer with the implicit split-fp16 weight gradients (RefineTrainer(weight_grad=...)).  With
`--baseline-lib` the rounds then are

    parent_fp32, parent_<precision>   the baseline library's steps      ours_fp32, ours_<precision>   this build, weight_grad fp32
    ours_<precision>_wgrad_f16x3      this build with the new route     torch                         the restatement

and the verdicts: the new route faster than the parent's step at the same precision by more than three times the spread of that
parent step's repeats; this build's fp32 and <precision> steps with weight_grad fp32 not slower than the parent's beyond its spread.

    python scripts/time_refine_train.py --precision f16x3_mixed --weight-grad f16x3 --baseline-lib ab/libnsr_parent.so \
        --out profiles/refine_train_wgrad_timing.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_sr_amd import refine  # noqa: E402
from tests import refine_train_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--refs", type=int, default=8)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=3, help="iterations per timed block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="'ours' or 'torch' (default: both, alternating)")
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32", help="'fp32' or 'f16x3_mixed': RefineTrainer(precision=...)")
    ap.add_argument("--weight-grad", default="fp32", help="'fp32' or 'f16x3': RefineTrainer(weight_grad=...)")
    ap.add_argument("--baseline-lib", default="", help="another build of libnsr.so to time the fp32 step of, in child processes")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)      # one block of one variant: what a child process runs
    a = ap.parse_args()
    if a.baseline_lib and not a.child:
        return ab_rounds(a)
    if a.child.startswith("parent_"):
        # a library from before the entry points with a precision / a weight-gradient argument (NSR_LIB_PATH): the pair it has
        # under their names (the baseline is only ever asked for weight_grad fp32, and for fp32 where it has no precision)
        from nerf_sr_amd import _lib
        new = [k for k in ("nsr_refine_train_forward_p", "nsr_refine_train_backward_p", "nsr_refine_train_backward_w") if k in _lib.SIGNATURES]
        sigs = {k: _lib.SIGNATURES.pop(k) for k in new}
        lib = _lib.load()
        for k, (res, args) in sigs.items():
            try:
                fn = getattr(lib, k)
                fn.restype, fn.argtypes = res, args
            except AttributeError:
                if k.endswith("_w"):
                    setattr(lib, k, lambda prec, wgrad, *rest, _lib=lib: _lib.nsr_refine_train_backward_p(prec, *rest))
                else:
                    old = getattr(lib, k[:-2])
                    setattr(lib, k, lambda prec, *rest, _f=old: _f(*rest))
    dev = torch.device("cuda", 0)
    B, R, P = a.batch, a.refs, a.patch
    gen = torch.Generator().manual_seed(3)
    x = (torch.rand(B, 3, P, P, generator=gen) * 2 - 1).to(dev)
    c = (torch.rand(B, R, 3, P, P, generator=gen) * 2 - 1).to(dev)
    gt = (torch.rand(B, 3, P, P, generator=gen) * 2 - 1).to(dev)
    sd = refine.make_refine_state_dict(7)
    variants = {}
    if a.only in ("", "ours"):
        tr = refine.RefineTrainer(sd, lr=5e-4, device=dev, precision=a.precision, weight_grad=a.weight_grad)
        tr.set_input({"sr_patch": x, "ref_patches": c, "gt_patch": gt})
        variants["ours"] = tr.optimize_parameters
    if a.only in ("", "torch"):
        tsd = OrderedDict((k, torch.from_numpy(v).to(dev)) for k, v in sd.items())
        leaves = [tsd[k].requires_grad_(True) for k in refine.TRAIN_PARAM_KEYS]
        opt = torch.optim.Adam(leaves, lr=5e-4, betas=(0.9, 0.999))

        def torch_step():
            y, running = ref.forward_train(tsd, x, c)
            opt.zero_grad()
            torch.nn.functional.l1_loss(y, gt).backward()
            opt.step()
            for k, v in running.items():        # the module's in-place buffer update
                tsd[k] = v
        variants["torch"] = torch_step
    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(a.repeats):
        for name, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.block):
                f()
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0) * 1e3 / a.block)
    if a.child:
        print(json.dumps({"ms": runs[a.only][0], "device": torch.cuda.get_device_name(dev),
                          "peak_memory_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}))
        return
    res = {"shape": f"B = {B} patch sets, R = {R} references, {P} x {P}, ours: {a.precision}, weight gradients {a.weight_grad}; forward -> L1 -> backward -> Adam; "
                    f"{a.repeats} alternating runs of {a.block} iterations after {a.warmup} warm-up iterations",
           "device": torch.cuda.get_device_name(dev), "conv_gmacs_forward": round(B * refine.refine_macs(P, P, R) / 1e9, 1),
           "peak_memory_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2), "variants": {}}
    for k, v in runs.items():
        res["variants"][k] = {"ms_per_iteration_median": round(statistics.median(v), 2), "ms_per_iteration_runs": [round(t, 2) for t in v],
                              "spread_ms": round(max(v) - min(v), 2)}
    if len(runs) == 2:
        res["ours_over_torch"] = round(statistics.median(runs["ours"]) / statistics.median(runs["torch"]), 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def ab_rounds(a):
    """--baseline-lib: `--repeats` alternating rounds, every block in a child process (one process, one library)."""
    here = os.path.abspath(__file__)
    base = os.path.abspath(a.baseline_lib)
    if not os.path.exists(base):
        raise SystemExit(f"{base} not found: build the parent commit's library there first")
    mixed = f"ours_{a.precision}"
    wg = a.weight_grad != "fp32"
    plan = [("parent_fp32", "ours", "fp32", "fp32", base)]
    if wg and a.precision != "fp32":
        plan.append((f"parent_{a.precision}", "ours", a.precision, "fp32", base))
    plan.append(("ours_fp32", "ours", "fp32", "fp32", ""))
    if a.precision != "fp32":
        plan.append((mixed, "ours", a.precision, "fp32", ""))
    new = f"{mixed}_wgrad_{a.weight_grad}"
    if wg:
        plan.append((new, "ours", a.precision, a.weight_grad, ""))
    plan.append(("torch", "torch", "fp32", "fp32", ""))
    runs, info = {name: [] for name, *_ in plan}, {}
    for _ in range(a.repeats):
        for name, only, prec, wgrad, lib in plan:
            env = dict(os.environ)
            env.pop("NSR_LIB_PATH", None)
            if lib:
                env["NSR_LIB_PATH"] = lib
            cmd = [sys.executable, here, "--child", name, "--only", only, "--precision", prec, "--weight-grad", wgrad, "--repeats", "1",
                   "--batch", str(a.batch), "--refs", str(a.refs), "--patch", str(a.patch), "--block", str(a.block), "--warmup", str(a.warmup)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            rec = json.loads(out.strip().splitlines()[-1])
            runs[name].append(rec["ms"])
            info[name] = rec
            print(f"{name}: {rec['ms']:.2f} ms", flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = max(runs["parent_fp32"]) - min(runs["parent_fp32"])
    res = {"shape": f"B = {a.batch} patch sets, R = {a.refs} references, {a.patch} x {a.patch}; forward -> L1 -> backward -> Adam; "
                    f"{a.repeats} alternating rounds, every block ({a.block} iterations after {a.warmup} warm-up iterations) in a "
                    "process of its own",
           "device": info["ours_fp32"]["device"], "baseline_lib": os.path.basename(base), "variants": {}}
    for k, v in runs.items():
        res["variants"][k] = {"ms_per_iteration_median": round(med[k], 2), "ms_per_iteration_runs": [round(t, 2) for t in v],
                              "spread_ms": round(max(v) - min(v), 2), "peak_memory_gb": info[k]["peak_memory_gb"]}
    res["parent_spread_ms"] = round(spread, 2)
    res["ours_fp32_minus_parent_ms"] = round(med["ours_fp32"] - med["parent_fp32"], 2)
    res["ours_fp32_within_parent_spread"] = bool(abs(med["ours_fp32"] - med["parent_fp32"]) <= spread)
    if mixed in med:
        res[f"{mixed}_gain_over_parent_ms"] = round(med["parent_fp32"] - med[mixed], 2)
        res[f"{mixed}_faster_by_more_than_3_spreads"] = bool(med["parent_fp32"] - med[mixed] > 3 * spread)
        res[f"{mixed}_over_torch"] = round(med[mixed] / med["torch"], 3)
    res["ours_fp32_over_torch"] = round(med["ours_fp32"] / med["torch"], 3)
    if wg:
        # the new route against the parent's step at the SAME precision, in units of that parent step's spread
        par = f"parent_{a.precision}"
        pspread = max(runs[par]) - min(runs[par])
        res[f"{par}_spread_ms"] = round(pspread, 2)
        res[f"{new}_gain_over_{par}_ms"] = round(med[par] - med[new], 2)
        res[f"{new}_faster_than_{par}_by_more_than_3_spreads"] = bool(med[par] - med[new] > 3 * pspread)
        res[f"{new}_over_torch"] = round(med[new] / med["torch"], 3)
        res["torch_still_ahead"] = bool(med["torch"] < med[new])
        if a.precision != "fp32":
            res[f"{mixed}_minus_{par}_ms"] = round(med[mixed] - med[par], 2)
            res[f"{mixed}_not_slower_than_{par}_beyond_its_spread"] = bool(med[mixed] - med[par] <= pspread)
        res["ours_fp32_not_slower_than_parent_beyond_its_spread"] = bool(med["ours_fp32"] - med["parent_fp32"] <= spread)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
