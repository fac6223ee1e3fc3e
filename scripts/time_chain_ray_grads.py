"""What the gradient with respect to the rays costs on the CHAIN pair (needs an MI355X): profiles/chain_ray_grads_timing.json.

The bench's training batch -- 2,048 rays, 64 + 64 samples, one chunk, the default network -- through the C entry points (ctypes),
timed with device events; five runs per variant, the variants alternated inside every round, one box:
  (a) the UNCHANGED route under NSR_F16X3: nsr_train_backward, and nsr_train_backward_r with g_rays = NULL and flags = 0, against
      nsr_train_backward of the parent commit's library (--parent PATH.so, built with scripts/ab_train_unify.py --build-parent;
      each library differentiates its own forward's saved state).  Both medians must lie inside the parent's median + 3 x the
      spread (max - min) of the parent's repeats; the weight gradients must be bit-identical.
  (b) the time g_rays adds (backward_r with g_rays minus backward), in ms and as a share of the step (forward + backward); the
      yardstick is the layer-by-layer NSR_F16X3_GEMM step with ray gradients (nsr_train_arch_forward_e +
      nsr_train_arch_backward_r), measured in the same run: the chain step with ray gradients must be faster than it by more
      than the sum of both spreads.
  (c) the frozen field: the step with NSR_BACKWARD_NO_WEIGHT_GRADS next to the step with weight gradients, and (--refine N) the
      iterations/s of examples/refine_pose.py with and without --chain, each in a child process under its own time limit.

usage: time_chain_ray_grads.py [--parent ab/libnsr_parent.so] [--rounds 5] [--iters 5] [--refine 60]
                               [--json profiles/chain_ray_grads_timing.json]"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
from ctypes import c_void_p

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_sr_amd import _lib  # noqa: E402
from nerf_sr_amd.weights import make_state_dict, normalize_arch  # noqa: E402

R, NC, NI = 2048, 64, 64
CHAIN_NAMES = ("nsr_train_workspace_bytes_for", "nsr_train_saved_bytes", "nsr_train_forward", "nsr_train_backward")
CHAIN_R_NAMES = ("nsr_train_workspace_bytes_r", "nsr_train_backward_r")
ARCH_NAMES = ("nsr_train_arch_workspace_bytes_r", "nsr_train_arch_saved_bytes_e", "nsr_train_arch_forward_e", "nsr_train_arch_backward_e",
              "nsr_train_arch_backward_r")
# per point: 2 x 256 x 63 (layer 1) + 2 x 256 x 63 (the skip layer) + 2 x 128 x 27 (dir_encoding), the useful columns only
ADDED_FLOPS = (2 * 256 * 63 * 2 + 2 * 128 * 27) * R * (NC + NC + NI)


def _p(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _ptrs(ts):
    return (c_void_p * len(ts))(*[_p(t) for t in ts])


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _bind(path, names):
    lib = ctypes.CDLL(path)
    for n in names:
        fn = getattr(lib, n)
        fn.restype, fn.argtypes = _lib.SIGNATURES[n]
    return lib


class Base:
    def _buffers(self, batch, ws_bytes, saved_bytes):
        self.w, self.rays, self.draws, self.g_outs = batch
        self.ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        self.saved = torch.empty(saved_bytes, dtype=torch.uint8, device="cuda")
        shapes = [(R, 3), (R,), (R,), (R, NC), (R, 3), (R,), (R,), (R, NC + NI)]
        self.outs = [torch.empty(s, device="cuda") for s in shapes]
        self.grads = [[torch.empty_like(t) for t in n] for n in self.w]
        self.g_rays = torch.empty(R, 8, device="cuda")


class ChainRun(Base):
    """One library's chain forward on the batch, and its backward variants."""

    def __init__(self, lib, batch, with_r):
        self.lib, self.prec = lib, _lib.TRAIN_PRECISIONS["f16x3"]
        size = lib.nsr_train_workspace_bytes_r if with_r else lib.nsr_train_workspace_bytes_for
        self._buffers(batch, size(self.prec, R, NC, NI), lib.nsr_train_saved_bytes(self.prec, R, NC, NI, 0))

    def forward(self):
        rc = self.lib.nsr_train_forward(_ptrs(self.w[0]), _ptrs(self.w[1]), _p(self.rays), 8, R, NC, NI, 0, 0, *[_p(t) for t in self.draws],
                                        1.0, self.prec, 0, _ptrs(self.outs), _p(self.ws), self.ws.numel(), _p(self.saved),
                                        self.saved.numel(), _stream())
        assert rc == 0, rc

    def backward(self, entry):
        w = (_ptrs(self.w[0]), _ptrs(self.w[1]))
        g = (_ptrs(self.g_outs), _ptrs(self.grads[0]), _ptrs(self.grads[1]))
        tail = (_p(self.ws), self.ws.numel(), _p(self.saved), self.saved.numel(), _stream())
        if entry == "plain":
            rc = self.lib.nsr_train_backward(*w, *g, *tail)
        else:
            g_rays = None if entry == "null" else self.g_rays
            flags = _lib.NSR_BACKWARD_NO_WEIGHT_GRADS if entry == "frozen" else 0
            rc = self.lib.nsr_train_backward_r(*w, _p(self.rays), 8, *g, _p(g_rays), 8, flags, *tail)
        assert rc == 0, rc


class LayerRun(Base):
    """The layer-by-layer pair on the default descriptor under NSR_F16X3_GEMM: the yardstick."""

    def __init__(self, lib, batch):
        self.lib, self.prec = lib, _lib.TRAIN_PRECISIONS["f16x3_gemm"]
        self.arch = _lib.NsrArch.from_arch(normalize_arch({}))
        self.lead = (ctypes.byref(self.arch), 0)
        self._buffers(batch, lib.nsr_train_arch_workspace_bytes_r(*self.lead, self.prec, R, NC, NI),
                      lib.nsr_train_arch_saved_bytes_e(*self.lead, self.prec, R, NC, NI, 0))

    def forward(self):
        rc = self.lib.nsr_train_arch_forward_e(*self.lead, _ptrs(self.w[0]), _ptrs(self.w[1]), _p(self.rays), 8, R, NC, NI, 0, 0,
                                               *[_p(t) for t in self.draws], 1.0, self.prec, 0, _ptrs(self.outs), _p(self.ws),
                                               self.ws.numel(), _p(self.saved), self.saved.numel(), _stream())
        assert rc == 0, rc

    def backward(self, entry):
        head = (*self.lead, _ptrs(self.w[0]), _ptrs(self.w[1]), _ptrs(self.g_outs), _ptrs(self.grads[0]), _ptrs(self.grads[1]))
        tail = (_p(self.ws), self.ws.numel(), _p(self.saved), self.saved.numel(), _stream())
        rc = self.lib.nsr_train_arch_backward_e(*head, *tail) if entry == "e" else \
            self.lib.nsr_train_arch_backward_r(*head, _p(self.g_rays), 8, *tail)
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


def refine_rate(iters, chain, limit):
    """iterations/s of examples/refine_pose.py in a child process under its own time limit"""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "refine_pose.py"), "--iters", str(iters)] + (["--chain"] if chain else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, check=True).stdout
    rate = re.search(r"([0-9.]+) iterations/s", out)
    after = re.search(r"after:\s+rotation error ([0-9.]+) deg, translation error ([0-9.]+)", out)
    before = re.search(r"before: rotation error ([0-9.]+) deg, translation error ([0-9.]+)", out)
    return {"iterations_per_s": float(rate.group(1)), "iters": iters,
            "rotation_error_deg": [float(before.group(1)), float(after.group(1))],
            "translation_error": [float(before.group(2)), float(after.group(2))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="the parent commit's libnsr.so (scripts/ab_train_unify.py --build-parent)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--refine", type=int, default=0, help="iterations of examples/refine_pose.py per route (0: skip)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_chain_ray_grads.py measures on the GPU: none is visible")
    new = _bind(_lib.LIB_PATH, CHAIN_NAMES + CHAIN_R_NAMES + ARCH_NAMES)
    old = _bind(a.parent, CHAIN_NAMES) if a.parent else None
    gen = torch.Generator().manual_seed(1)
    rays = torch.empty(R, 8)
    rays[:, 0:3] = torch.rand(R, 3, generator=gen) - 0.5
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=1)
    rays[:, 6], rays[:, 7] = 0.0, 1.0
    draws = [torch.rand(R, NC, generator=gen).cuda(), torch.rand(R, NI, generator=gen).cuda(), torch.randn(R, NC, generator=gen).cuda(),
             torch.randn(R, NC + NI, generator=gen).cuda()]
    g_outs = [torch.randn(R, 3, generator=gen).cuda(), None, None, None, torch.randn(R, 3, generator=gen).cuda(), None, None, None]
    w = [[torch.from_numpy(v).cuda() for v in make_state_dict(seed).values()] for seed in (99, 100)]
    batch = (w, rays.cuda(), draws, g_outs)
    chain, layers = ChainRun(new, batch, True), LayerRun(new, batch)
    parent = ChainRun(old, batch, False) if old is not None else None
    variants = {"forward": chain.forward, "backward": lambda: chain.backward("plain"), "backward_r_null": lambda: chain.backward("null"),
                "backward_r": lambda: chain.backward("r"), "backward_r_frozen": lambda: chain.backward("frozen"),
                "layers_forward": layers.forward, "layers_backward_e": lambda: layers.backward("e"),
                "layers_backward_r": lambda: layers.backward("r")}
    if parent is not None:
        variants["parent_backward"] = lambda: parent.backward("plain")
    for r in (chain, layers) + ((parent,) if parent is not None else ()):
        r.forward()
    for fn in variants.values():      # warm-up of every variant
        fn()
    torch.cuda.synchronize()
    same = None
    if parent is not None:            # the same bits without the ray gradient
        chain.backward("null")
        parent.backward("plain")
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for n in range(2) for x, y in zip(chain.grads[n], parent.grads[n]))
    chain.backward("r")
    rows = chain.g_rays.clone()
    chain.backward("frozen")
    torch.cuda.synchronize()
    frozen_same = bool(torch.equal(rows, chain.g_rays))
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, a.iters))
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: max(v) - min(v)
    report = {"batch": {"rays": R, "n_coarse": NC, "n_importance": NI, "ray_chunk": 0, "precision": "f16x3"}, "rounds": a.rounds,
              "iters_per_run": a.iters, "protocol": "device events; variants alternated inside every round; one box",
              "device": torch.cuda.get_device_name(0),
              "variants": {k: {"ms_median": round(med(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                               "ms_all": [round(x, 4) for x in v]} for k, v in ms.items()}}
    step = med(ms["forward"]) + med(ms["backward"])
    added = med(ms["backward_r"]) - med(ms["backward"])
    l_step = med(ms["layers_forward"]) + med(ms["layers_backward_e"])
    l_added = med(ms["layers_backward_r"]) - med(ms["layers_backward_e"])
    chain_r_step, layers_r_step = med(ms["forward"]) + med(ms["backward_r"]), med(ms["layers_forward"]) + med(ms["layers_backward_r"])
    margin = spread(ms["forward"]) + spread(ms["backward_r"]) + spread(ms["layers_forward"]) + spread(ms["layers_backward_r"])
    report["added_by_g_rays"] = {"ms": round(added, 4), "step_ms": round(step, 4), "share_of_step": round(added / step, 4),
                                 "added_gemm_flops": ADDED_FLOPS, "gemm_tflops_if_all_gemm": round(ADDED_FLOPS / (added * 1e-3) / 1e12, 2)}
    report["yardstick_f16x3_gemm"] = {"step_ms": round(l_step, 4), "added_ms": round(l_added, 4),
                                      "step_with_g_rays_ms": round(layers_r_step, 4),
                                      "chain_step_with_g_rays_ms": round(chain_r_step, 4), "sum_of_spreads_ms": round(margin, 4),
                                      "chain_faster_by_more_than_the_spreads": bool(layers_r_step - chain_r_step > margin),
                                      "added_cost_below_the_layer_by_layer_added_cost": bool(added < l_added)}
    report["frozen_field"] = {"step_with_weight_gradients_ms": round(chain_r_step, 4),
                              "step_no_weight_grads_ms": round(med(ms["forward"]) + med(ms["backward_r_frozen"]), 4),
                              "rows_bit_identical": frozen_same}
    if parent is not None:
        p = ms["parent_backward"]
        limit = med(p) + 3.0 * spread(p)
        report["against_parent"] = {"limit_ms": round(limit, 4), "weight_gradients_bit_identical": bool(same),
                                    "backward_inside": bool(med(ms["backward"]) <= limit),
                                    "backward_r_null_inside": bool(med(ms["backward_r_null"]) <= limit)}
    print(json.dumps({k: report[k] for k in ("added_by_g_rays", "yardstick_f16x3_gemm", "frozen_field") + (("against_parent",) if parent else ())}),
          {k: v["ms_median"] for k, v in report["variants"].items()}, flush=True)
    del chain, layers, parent
    torch.cuda.empty_cache()
    if a.refine > 0:
        report["refine_pose"] = {"layer_by_layer_fp32": refine_rate(a.refine, False, 300), "chain_f16x3": refine_rate(a.refine, True, 300)}
        print(json.dumps(report["refine_pose"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
