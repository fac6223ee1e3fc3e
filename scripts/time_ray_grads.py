"""What the gradient with respect to the rays costs (needs an MI355X): profiles/ray_grads_timing.json.

The bench's training batch -- 2,048 rays, 64 + 64 samples, one chunk -- on the default descriptor and on 6 x 192 with skips
(1, 3), under NSR_FP32 and NSR_F16X3_GEMM, through the C entry points (ctypes), timed with device events; five runs per
variant, the variants alternated inside every round, one box:
  (a) the backward WITHOUT the ray gradient -- nsr_train_arch_backward_e, and nsr_train_arch_backward_r with g_rays = NULL --
      against the same call of the parent commit's library (--parent PATH.so; each library differentiates its own forward's
      saved state).  Must lie inside the parent's figure + 3 x the spread (max - min) of the parent's repeats.
  (b) the time g_rays adds (backward_r with g_rays minus backward_e), next to the step time (forward + backward) and the count
      of added GEMM FLOPs: per pass of P points 2 P Wp Kx per layer that reads the encoded position + 2 P Hp Dp.

usage: time_ray_grads.py [--parent ab/libnsr_parent.so] [--rounds 5] [--iters 5] [--json profiles/ray_grads_timing.json]"""
import argparse
import ctypes
import json
import os
import sys
from ctypes import c_void_p

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_sr_amd import _lib  # noqa: E402
from nerf_sr_amd.weights import make_state_dict_arch, normalize_arch  # noqa: E402

ARCHS = {"default": {}, "6x192_skips_1_3": {"D": 6, "W": 192, "skips": (1, 3)}}
R, NC, NI = 2048, 64, 64
NAMES = ("nsr_train_arch_workspace_bytes_e", "nsr_train_arch_saved_bytes_e", "nsr_train_arch_forward_e", "nsr_train_arch_backward_e")


def _p(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _ptrs(ts):
    return (c_void_p * len(ts))(*[_p(t) for t in ts])


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _bind(path, with_r):
    lib = ctypes.CDLL(path)
    for n in NAMES + (("nsr_train_arch_workspace_bytes_r", "nsr_train_arch_backward_r") if with_r else ()):
        fn = getattr(lib, n)
        fn.restype, fn.argtypes = _lib.SIGNATURES[n]
    return lib


def _r32(n):
    return (n + 31) // 32 * 32


def added_gemm_flops(arch):
    a = normalize_arch(arch)
    Kx, Wp, Hp = _r32(3 + 6 * a["deg_pos"]), _r32(a["W"]), _r32(a["W"] // 2)
    Dp = 0 if a["no_dir"] else _r32(3 + 6 * a["deg_dir"])
    per_point = (1 + len(a["skips"])) * 2 * Wp * Kx + 2 * Hp * Dp
    return per_point * R * (NC + NC + NI)


class Run:
    """One library's forward on the batch, and its backward variants as closures."""

    def __init__(self, lib, arch, prec, batch, with_r):
        self.lib, self.with_r = lib, with_r
        self.arch = _lib.NsrArch.from_arch(normalize_arch(arch))
        self.lead = (ctypes.byref(self.arch), 0)
        self.prec = prec
        self.w, self.rays, self.draws, self.g_outs = batch
        size = lib.nsr_train_arch_workspace_bytes_r if with_r else lib.nsr_train_arch_workspace_bytes_e
        self.ws = torch.zeros(size(*self.lead, prec, R, NC, NI), dtype=torch.uint8, device="cuda")
        self.saved = torch.empty(lib.nsr_train_arch_saved_bytes_e(*self.lead, prec, R, NC, NI, 0), dtype=torch.uint8, device="cuda")
        shapes = [(R, 3), (R,), (R,), (R, NC), (R, 3), (R,), (R,), (R, NC + NI)]
        self.outs = [torch.empty(s, device="cuda") for s in shapes]
        self.grads = [[torch.empty_like(t) for t in n] for n in self.w]
        self.g_rays = torch.empty(R, 8, device="cuda")

    def forward(self):
        rc = self.lib.nsr_train_arch_forward_e(
            *self.lead, _ptrs(self.w[0]), _ptrs(self.w[1]), _p(self.rays), 8, R, NC, NI, 0, 0, *[_p(t) for t in self.draws], 1.0,
            self.prec, 0, _ptrs(self.outs), _p(self.ws), self.ws.numel(), _p(self.saved), self.saved.numel(), _stream())
        assert rc == 0, rc

    def backward(self, entry):
        head = (*self.lead, _ptrs(self.w[0]), _ptrs(self.w[1]), _ptrs(self.g_outs), _ptrs(self.grads[0]), _ptrs(self.grads[1]))
        tail = (_p(self.ws), self.ws.numel(), _p(self.saved), self.saved.numel(), _stream())
        if entry == "e":
            rc = self.lib.nsr_train_arch_backward_e(*head, *tail)
        else:
            rc = self.lib.nsr_train_arch_backward_r(*head, _p(self.g_rays if entry == "r" else None), 8, *tail)
        assert rc == 0, rc


def timed(fn, iters):
    """Milliseconds per call over ``iters`` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="the parent commit's libnsr.so, built beside this tree")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ray_grads.py measures on the GPU: none is visible")
    new = _bind(_lib.LIB_PATH, True)
    old = _bind(a.parent, False) if a.parent else None
    gen = torch.Generator().manual_seed(1)
    rays = torch.empty(R, 8)
    rays[:, 0:3] = torch.rand(R, 3, generator=gen) - 0.5
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=1)
    rays[:, 6], rays[:, 7] = 0.0, 1.0
    draws = [torch.rand(R, NC, generator=gen).cuda(), torch.rand(R, NI, generator=gen).cuda(), torch.randn(R, NC, generator=gen).cuda(),
             torch.randn(R, NC + NI, generator=gen).cuda()]
    g_outs = [torch.randn(R, 3, generator=gen).cuda(), None, None, None, torch.randn(R, 3, generator=gen).cuda(), None, None, None]
    report = {"batch": {"rays": R, "n_coarse": NC, "n_importance": NI, "ray_chunk": 0}, "rounds": a.rounds, "iters_per_run": a.iters,
              "protocol": "device events; variants alternated inside every round; one box", "cases": {}}
    for tag, arch in ARCHS.items():
        w = [[torch.from_numpy(v).cuda() for v in make_state_dict_arch(seed, **arch).values()] for seed in (99, 100)]
        batch = (w, rays.cuda(), draws, g_outs)
        for pname in ("fp32", "f16x3_gemm"):
            prec = _lib.TRAIN_PRECISIONS[pname]
            runs = {"new": Run(new, arch, prec, batch, True)}
            if old is not None:
                runs["parent"] = Run(old, arch, prec, batch, False)
            variants = {"backward_e": lambda: runs["new"].backward("e"), "backward_r_null": lambda: runs["new"].backward("null"),
                        "backward_r": lambda: runs["new"].backward("r"), "forward": lambda: runs["new"].forward()}
            if old is not None:
                variants["parent_backward_e"] = lambda: runs["parent"].backward("e")
            for r in runs.values():
                r.forward()
            for fn in variants.values():      # warm-up of every variant
                fn()
            torch.cuda.synchronize()
            if old is not None:               # the same bits without the ray gradient
                runs["new"].backward("null")
                runs["parent"].backward("e")
                torch.cuda.synchronize()
                same = all(torch.equal(x, y) for n in range(2) for x, y in zip(runs["new"].grads[n], runs["parent"].grads[n]))
            ms = {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    ms[k].append(timed(fn, a.iters))
            med = lambda v: sorted(v)[len(v) // 2]
            case = {k: {"ms_median": round(med(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                        "ms_all": [round(x, 4) for x in v]} for k, v in ms.items()}
            flops = added_gemm_flops(arch)
            added = med(ms["backward_r"]) - med(ms["backward_e"])
            case["added_by_g_rays"] = {"ms": round(added, 4), "step_ms": round(med(ms["forward"]) + med(ms["backward_e"]), 4),
                                       "share_of_step": round(added / (med(ms["forward"]) + med(ms["backward_e"])), 4),
                                       "added_gemm_flops": flops, "gemm_tflops_if_all_gemm": round(flops / (added * 1e-3) / 1e12, 2)}
            if old is not None:
                p = ms["parent_backward_e"]
                limit = med(p) + 3.0 * (max(p) - min(p))
                case["against_parent"] = {"limit_ms": round(limit, 4), "weight_gradients_bit_identical": bool(same),
                                          "backward_e_inside": bool(med(ms["backward_e"]) <= limit),
                                          "backward_r_null_inside": bool(med(ms["backward_r_null"]) <= limit)}
            report["cases"][f"{tag}-{pname}"] = case
            print(tag, pname, json.dumps(case["added_by_g_rays"]), json.dumps(case.get("against_parent", {})),
                  {k: case[k]["ms_median"] for k in variants}, flush=True)
            del runs
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
