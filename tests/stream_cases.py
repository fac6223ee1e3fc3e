"""The cases of tests/test_gpu_stream_order.py and tests/test_gpu_graph_capture.py: for every entry point of ``stream_gate.TABLE``
one or more builders ``build(ctx) -> stream_gate.Case``.  Importing this module touches no device; a builder does.

Every case owns its buffers: two valid input sets A and B, the state the call updates in place, the outputs and the scratch.
Calls go through ctypes with the argument lists the Python wrappers pass (nerf_sr_amd/ops.py, train.py, refine.py, metrics.py,
losses.py), so that the outputs and workspaces are buffers the protocol can make stale; the wrappers' own plumbing (``_stream()``,
temporaries) is covered by the ``wrapper`` cases, which call the wrapper itself and compare what it returns.

``WRAPPER_WAITS``: host waits of the Python layer itself, each with the words of INTEGRATION.md that document it; a wrapper case
that waits names one (``Case.documented``), and tests/test_stream_contract_cpu.py checks that the words stand there."""
import ctypes
from collections import OrderedDict
from ctypes import c_void_p

import numpy as np
import torch

from tests.stream_gate import Case, TABLE, WAITS

DEV = "cuda"
WRAPPER_WAITS = {
    "Trainer far": "`Trainer.loss_and_grads` with a depth-variance loss reads the far bound of one ray back",
    "GenericMLP fused load": "`GenericMLP(fused=True).load_state_dict` reads the pack's range verdict back",
    "RefinePatchSet": "`RefinePatchSet(...)` of the 'train' split reads the bounding boxes back",
}
CASES: "OrderedDict[str, list]" = OrderedDict()        # entry -> [(case name, builder)]

def case(entry: str, tag: str = ""):
    assert entry in TABLE, entry

    def deco(fn):
        CASES.setdefault(entry, []).append((entry + (f"[{tag}]" if tag else ""), fn))
        return fn
    return deco


def all_cases():
    return [(name, entry, fn) for entry, lst in CASES.items() for name, fn in lst]


# ----------------------------------------------------------------------------------------------------------------- helpers
def P(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def ptrs(ts):
    return (c_void_p * len(ts))(*[P(t) for t in ts])


def S():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def lib():
    from nerf_sr_amd import _lib
    return _lib.load()


def ok(rc, what):
    from nerf_sr_amd import _lib
    _lib.check(rc, what)


def rnd(seed, *shape, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(DEV)


def randn(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def empty_like_all(ts):
    return [torch.empty_like(t) for t in ts]


def named(prefix, ts):
    return OrderedDict((f"{prefix}{i}", t) for i, t in enumerate(ts))


def out_buf(shape, dtype=torch.float32):
    """An output buffer; what it holds first never matters (the serial runs overwrite it)."""
    return torch.zeros(shape, dtype=dtype, device=DEV)


class Ctx:
    """Inputs shared by the cases of one module, made on first use and never changed."""

    def __init__(self):
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    # -- 96 rays, twice: two poses of the same camera
    def rays(self, which):
        def make():
            from nerf_sr_amd import cameras, ops
            lo = 252 * 95 + 100
            pose = cameras.spiral_pose(0.4 if which == "A" else 0.7)
            r = ops.subpixel_rays(pose, (504, 378), cameras.llff_focal(504), 2, True, 0.0, 1.0, device=DEV, lr_range=(lo, lo + 24))
            return r.view(-1, 8)[:96].contiguous()
        return self.memo(("rays", which), make)

    def z(self, which, n):
        lo, hi = (0.0, 1.0) if which == "A" else (0.02, 0.98)
        return self.memo(("z", which, n), lambda: torch.linspace(lo, hi, n, device=DEV).repeat(96, 1).contiguous())

    # -- the default network: seeds (coarse, fine) of the scratch-state tests, swapped for B
    def weights(self, which, net):
        def make():
            from nerf_sr_amd.weights import make_state_dict
            from tests.scratch_state import RENDER_SEEDS
            seed = RENDER_SEEDS[net if which == "A" else 1 - net]
            return [torch.from_numpy(v).to(DEV) for v in make_state_dict(seed, "smooth").values()]
        return self.memo(("w", which, net), make)

    def blob(self, which, net, prec):
        """The packed network (uint8) of ``weights(which, net)`` at ``prec``, status word clear."""
        def make():
            from nerf_sr_amd import _lib
            p = _lib.PRECISIONS[prec]
            b = torch.empty(lib().nsr_packed_weights_bytes(p), dtype=torch.uint8, device=DEV)
            ok(lib().nsr_pack_weights(ptrs(self.weights(which, net)), P(b), p, S()), "nsr_pack_weights")
            return b
        return self.memo(("blob", which, net, prec), make)

    def draws(self, which):
        def make():
            s = 50 if which == "A" else 60
            g = torch.Generator().manual_seed(s)
            return {"u_coarse": torch.rand(96, 64, generator=g).to(DEV), "u_fine": torch.rand(96, 64, generator=g).to(DEV),
                    "noise_coarse": torch.randn(96, 64, generator=g).to(DEV), "noise_fine": torch.randn(96, 128, generator=g).to(DEV)}
        return self.memo(("draws", which), make)

    # -- a non-default architecture (the exact-input case of tests/test_gpu_arch_fused.py) and the training one of the
    # scratch-state tests
    FUSED_ARCH = {"D": 2, "W": 64, "skips": (1,), "deg_pos": 2, "deg_dir": 1, "no_dir": False}

    def arch_weights(self, which, net, arch_items, embed):
        def make():
            from nerf_sr_amd.weights import make_state_dict_arch
            seed = (3, 6)[net if which == "A" else 1 - net]
            return [torch.from_numpy(v).to(DEV) for v in make_state_dict_arch(seed, no_xyz=bool(embed & 1), **dict(arch_items)).values()]
        return self.memo(("aw", which, net, arch_items, embed), make)

    def refine_sd(self, which):
        def make():
            from nerf_sr_amd import refine as rf
            sd = rf.make_refine_state_dict(5 if which == "A" else 6)
            return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(sd[k])).to(DEV).float().contiguous()) for k in rf.REFINE_SPEC)
        return self.memo(("refine_sd", which), make)


def blob_status(bufs_and_prec):
    """status(host) of a case whose packed networks are input buffers: the words, cleared."""
    def status(_host):
        out = []
        for b, p in bufs_and_prec:
            f = ctypes.c_uint(0)
            ok(lib().nsr_weights_status(P(b), p, 1, ctypes.byref(f), S()), "nsr_weights_status")
            out.append(int(f.value))
        return tuple(out)
    return status


def wire(items):
    """items: name -> (A, B) tensors.  Returns bufs, A, B dicts with a fresh buffer per name."""
    bufs, A, B = OrderedDict(), OrderedDict(), OrderedDict()
    for k, (a, b) in items.items():
        bufs[k], A[k], B[k] = torch.empty_like(a), a, b
    return bufs, A, B


# ============================================================================================== include/nsr.h: small stages
def _simple(entry, tag, items, outs, call, **kw):
    """Registers a case whose builder is ``items(ctx) -> name -> (A, B)``, ``outs() -> name -> buffer`` and
    ``call(bufs, outs, host)``."""
    @case(entry, tag)
    def build(ctx, _name=entry + (f"[{tag}]" if tag else "")):
        bufs, A, B = wire(items(ctx))
        o = outs()
        return Case(_name, entry, lambda host: call(bufs, o, host), bufs=bufs, A=A, B=B, outs=o, waits=TABLE[entry].kind == WAITS, **kw)
    return build


_simple("nsr_posenc", "", lambda c: {"x": (rnd(1, 300, 3, lo=-1, hi=1), rnd(2, 300, 3, lo=-1, hi=1))},
        lambda: {"out": out_buf((300, 63))},
        lambda b, o, h: ok(lib().nsr_posenc(P(b["x"]), 300, 10, P(o["out"]), S()), "nsr_posenc"))
_simple("nsr_posenc_e", "no_xyz+linear", lambda c: {"x": (rnd(1, 300, 3, lo=-1, hi=1), rnd(2, 300, 3, lo=-1, hi=1))},
        lambda: {"out": out_buf((300, 60))},
        lambda b, o, h: ok(lib().nsr_posenc_e(P(b["x"]), 300, 10, 3, P(o["out"]), S()), "nsr_posenc_e"))
_simple("nsr_sample_along_rays", "", lambda c: {"rays": (c.rays("A"), c.rays("B"))},
        lambda: {"z": out_buf((96, 64)), "pts": out_buf((96, 64, 3))},
        lambda b, o, h: ok(lib().nsr_sample_along_rays(P(b["rays"]), 8, 96, 64, 0, None, P(o["z"]), P(o["pts"]), S()), "nsr_sample_along_rays"))
_simple("nsr_sample_along_rays", "randomized", lambda c: {"rays": (c.rays("A"), c.rays("B")), "u": (rnd(3, 96, 64), rnd(4, 96, 64))},
        lambda: {"z": out_buf((96, 64)), "pts": out_buf((96, 64, 3))},
        lambda b, o, h: ok(lib().nsr_sample_along_rays(P(b["rays"]), 8, 96, 64, 0, P(b["u"]), P(o["z"]), P(o["pts"]), S()), "nsr_sample_along_rays"))
_simple("nsr_resample_along_rays", "", lambda c: {"rays": (c.rays("A"), c.rays("B")), "z": (c.z("A", 64), c.z("B", 64)),
                                                   "w": (rnd(5, 96, 64), rnd(6, 96, 64))},
        lambda: {"z_out": out_buf((96, 128)), "pts": out_buf((96, 128, 3))},
        lambda b, o, h: ok(lib().nsr_resample_along_rays(P(b["rays"]), 8, P(b["z"]), P(b["w"]), 96, 64, 64, None, P(o["z_out"]), P(o["pts"]),
                                                         S()), "nsr_resample_along_rays"))
_simple("nsr_composite", "", lambda c: {"rgb": (rnd(7, 96, 64, 3), rnd(8, 96, 64, 3)), "sigma": (randn(9, 96, 64, scale=20), randn(10, 96, 64, scale=20)),
                                         "z": (c.z("A", 64), c.z("B", 64))},
        lambda: {"comp": out_buf((96, 3)), "depth": out_buf((96,)), "opac": out_buf((96,)), "w": out_buf((96, 64))},
        lambda b, o, h: ok(lib().nsr_composite(P(b["rgb"]), 3, P(b["sigma"]), 1, P(b["z"]), 96, 64, 1, P(o["comp"]), P(o["depth"]), P(o["opac"]),
                                               P(o["w"]), S()), "nsr_composite"))
_simple("nsr_sr_mean", "", lambda c: {"hr": (rnd(11, 120 * 4, 3), rnd(12, 120 * 4, 3))}, lambda: {"lr": out_buf((120, 3))},
        lambda b, o, h: ok(lib().nsr_sr_mean(P(b["hr"]), 120, 4, 3, P(o["lr"]), S()), "nsr_sr_mean"))
_simple("nsr_unflatten", "", lambda c: {"x": (rnd(13, 20 * 24, 3), rnd(14, 20 * 24, 3))}, lambda: {"img": out_buf((20, 24, 3))},
        lambda b, o, h: ok(lib().nsr_unflatten(P(b["x"]), 20, 24, 2, 3, P(o["img"]), S()), "nsr_unflatten"))


def _pose(t):
    from nerf_sr_amd import cameras
    c = np.ascontiguousarray(np.asarray(cameras.spiral_pose(t), dtype=np.float32).reshape(12))
    return c, c.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _gen_rays_case(entry, call):
    @case(entry)
    def build(ctx):
        from nerf_sr_amd import cameras
        focal = float(cameras.llff_focal(24))
        o = {"rays": out_buf((480, 8))}
        return Case(entry, entry, lambda host: ok(call(host[1], focal, o["rays"]), entry), outs=o, host_A=_pose(0.3), host_B=_pose(0.8))


_gen_rays_case("nsr_gen_rays", lambda c2w, f, r: lib().nsr_gen_rays(c2w, 20, 24, f, 2, 1, 0.0, 1.0, P(r), S()))
_gen_rays_case("nsr_gen_rays_range", lambda c2w, f, r: lib().nsr_gen_rays_range(c2w, 20, 24, f, 2, 1, 0.0, 1.0, 0, 120, P(r), S()))
_gen_rays_case("nsr_gen_rays_opt", lambda c2w, f, r: lib().nsr_gen_rays_opt(c2w, 20, 24, f, 2, 1, 0.0, 1.0, 1, 0, 120, P(r), S()))


# ============================================================================================ include/nsr.h: packed networks
def _prec(name):
    from nerf_sr_amd import _lib
    return _lib.PRECISIONS[name]


def _pack_case(entry, prec):
    @case(entry, prec)
    def build(ctx):
        p = _prec(prec)
        wa = [t.clone() for t in ctx.weights("A", 0)]
        wb = ctx.weights("B", 0)
        if TABLE[entry].kind == WAITS:       # the verdict of the GATED work: A is finite but outside the split-fp16 range
            wa[0][0, 0] = 2000.0
        bufs, A, B = wire(OrderedDict((f"w{i}", (a, b)) for i, (a, b) in enumerate(zip(wa, wb))))
        o = {"packed": torch.zeros(lib().nsr_packed_weights_bytes(p), dtype=torch.uint8, device=DEV)}
        rc = []

        def call(_host):
            rc.append(getattr(lib(), entry)(ptrs(list(bufs.values())), P(o["packed"]), p, S()))
        return Case(f"{entry}[{prec}]", entry, call, bufs=bufs, A=A, B=B, outs=o, status=lambda h: (rc[-1],), waits=TABLE[entry].kind == WAITS)


_pack_case("nsr_pack_weights", "f16x3")
_pack_case("nsr_pack_weights_async", "f16x3")
_pack_case("nsr_pack_weights_async", "fp32")


@case("nsr_weights_status")
def _weights_status(ctx):
    """The flag a GATED launch raises: A's rows hold a finite value beyond fp16 (NSR_FLAG_INPUT_RANGE), B's do not."""
    p = _prec("f16x3")
    xa, xb = rnd(20, 200, 90, lo=-1, hi=1), rnd(21, 200, 90, lo=-1, hi=1)
    xa[7, 3] = 1.0e5
    bufs, A, B = wire({"x": (xa, xb)})
    st = {"packed": ctx.blob("A", 0, "f16x3").clone()}
    o = {"out": out_buf((200, 4))}
    flags = []

    def call(_host):
        ok(lib().nsr_mlp_forward(P(st["packed"]), p, P(bufs["x"]), 200, 0, P(o["out"]), S()), "nsr_mlp_forward")
        f = ctypes.c_uint(0)
        ok(lib().nsr_weights_status(P(st["packed"]), p, 1, ctypes.byref(f), S()), "nsr_weights_status")
        flags.append(int(f.value))
    return Case("nsr_weights_status", "nsr_weights_status", call, bufs=bufs, A=A, B=B, state=st, outs=o, status=lambda h: (flags[-1],), waits=True)


def _options_case(entry, a, b):
    @case(entry)
    def build(ctx):
        p = _prec("f16x3")
        st = {"packed": ctx.blob("A", 0, "f16x3").clone()}
        return Case(entry, entry, lambda host: ok(getattr(lib(), entry)(P(st["packed"]), p, host, S()), entry), state=st, host_A=a, host_B=b)


_options_case("nsr_weights_set_options", 1, 2)
_options_case("nsr_weights_set_gamma", 1, 0)


def _net_inputs(ctx, prec, nets=(0,)):
    items = OrderedDict()
    for n in nets:
        items[f"packed{n}"] = (ctx.blob("A", n, prec), ctx.blob("B", n, prec))
    return items


def _mlp_case(prec, sigma_only):
    @case("nsr_mlp_forward", f"{prec}{'-sigma' if sigma_only else ''}")
    def build(ctx):
        p = _prec(prec)
        items = _net_inputs(ctx, prec)
        items["x"] = (rnd(22, 200, 90, lo=-1, hi=1), rnd(23, 200, 90, lo=-1, hi=1))
        bufs, A, B = wire(items)
        o = {"out": out_buf((200, 1 if sigma_only else 4))}
        return Case(f"nsr_mlp_forward[{prec}]", "nsr_mlp_forward",
                    lambda h: ok(lib().nsr_mlp_forward(P(bufs["packed0"]), p, P(bufs["x"]), 200, int(sigma_only), P(o["out"]), S()), "nsr_mlp_forward"),
                    bufs=bufs, A=A, B=B, outs=o, status=blob_status([(bufs["packed0"], p)]))


for _p_ in ("fp32", "f16x3", "f16", "bf16"):
    _mlp_case(_p_, False)
_mlp_case("f16x3", True)


def _rays_z_inputs(ctx, prec, n):
    items = _net_inputs(ctx, prec)
    items["rays"] = (ctx.rays("A"), ctx.rays("B"))
    items["z"] = (ctx.z("A", n), ctx.z("B", n))
    return items


def _render_rays_case(prec, n):
    @case("nsr_render_rays", f"{prec}-{n}")
    def build(ctx):
        p = _prec(prec)
        bufs, A, B = wire(_rays_z_inputs(ctx, prec, n))
        o = {"raw": out_buf((96 * n, 4))}
        return Case(f"nsr_render_rays[{prec}-{n}]", "nsr_render_rays",
                    lambda h: ok(lib().nsr_render_rays(P(bufs["packed0"]), p, P(bufs["rays"]), 8, P(bufs["z"]), 96, n, P(o["raw"]), S()), "nsr_render_rays"),
                    bufs=bufs, A=A, B=B, outs=o, status=blob_status([(bufs["packed0"], p)]))


_render_rays_case("f16x3", 64)
_render_rays_case("fp32", 64)


def _comp_outs(n, raw=False):
    o = OrderedDict([("comp", out_buf((96, 3))), ("depth", out_buf((96,))), ("opac", out_buf((96,))), ("w", out_buf((96, n)))])
    if raw:
        o["raw"] = out_buf((96 * n, 4))
    return o


def _composited_case(prec, n, raw=False):
    @case("nsr_render_rays_composited", f"{prec}-{n}{'-raw' if raw else ''}")
    def build(ctx):
        p = _prec(prec)
        bufs, A, B = wire(_rays_z_inputs(ctx, prec, n))
        o = _comp_outs(n, raw)
        return Case(f"nsr_render_rays_composited[{prec}-{n}]", "nsr_render_rays_composited",
                    lambda h: ok(lib().nsr_render_rays_composited(P(bufs["packed0"]), p, P(bufs["rays"]), 8, P(bufs["z"]), 96, n, 0, P(o.get("raw")),
                                                                  P(o["comp"]), P(o["depth"]), P(o["opac"]), P(o["w"]), S()), "nsr_render_rays_composited"),
                    bufs=bufs, A=A, B=B, outs=o, status=blob_status([(bufs["packed0"], p)]))


for _n_ in (64, 128, 192, 256):
    _composited_case("f16x3", _n_)
_composited_case("f16x3", 64, raw=True)
_composited_case("fp32", 128)


@case("nsr_render_rays_composited_ert", "f16x3-128")
def _composited_ert(ctx):
    p, n = _prec("f16x3"), 128
    bufs, A, B = wire(_rays_z_inputs(ctx, "f16x3", n))
    o = _comp_outs(n)
    st = {"cut": torch.zeros(1, dtype=torch.int32, device=DEV)}
    return Case("nsr_render_rays_composited_ert[f16x3-128]", "nsr_render_rays_composited_ert",
                lambda h: ok(lib().nsr_render_rays_composited_ert(P(bufs["packed0"]), p, P(bufs["rays"]), 8, P(bufs["z"]), 96, n, 0, 1e-3, P(o["comp"]),
                                                                  P(o["depth"]), P(o["opac"]), P(o["w"]), P(st["cut"]), S()), "nsr_render_rays_composited_ert"),
                bufs=bufs, A=A, B=B, outs=o, state=st, status=blob_status([(bufs["packed0"], p)]))


def _density_case(n):
    @case("nsr_render_rays_density", f"f16x3-{n}")
    def build(ctx):
        p = _prec("f16x3")
        bufs, A, B = wire(_rays_z_inputs(ctx, "f16x3", n))
        o = _comp_outs(n)
        del o["comp"]
        return Case(f"nsr_render_rays_density[{n}]", "nsr_render_rays_density",
                    lambda h: ok(lib().nsr_render_rays_density(P(bufs["packed0"]), p, P(bufs["rays"]), 8, P(bufs["z"]), 96, n, 0, P(o["depth"]),
                                                               P(o["opac"]), P(o["w"]), S()), "nsr_render_rays_density"),
                    bufs=bufs, A=A, B=B, outs=o, status=blob_status([(bufs["packed0"], p)]))


_density_case(64)
_density_case(256)


def _forward_rays_case(entry, prec, ni, eps=0.0):
    tag = f"{prec}-64+{ni}" + ("-early_stop" if eps > 0.0 else "")

    @case(entry, tag)
    def build(ctx):
        p, nc = _prec(prec), 64
        items = _net_inputs(ctx, prec, (0, 1))
        items["rays"] = (ctx.rays("A"), ctx.rays("B"))
        bufs, A, B = wire(items)
        shapes = [(96, 3), (96,), (96,), (96, nc), (96, 3), (96,), (96,), (96, nc + ni)]
        o = OrderedDict((f"o{i}", out_buf(s)) for i, s in enumerate(shapes))
        if entry == "nsr_forward_rays_density_coarse":
            del o["o0"]                                  # coarse_comp_rgbs must be NULL
        st = {"cut": torch.zeros(1, dtype=torch.int32, device=DEV)} if eps > 0.0 else {}
        ws = torch.zeros(max(lib().nsr_forward_rays_workspace_bytes_for(p, 96, nc, ni), 256), dtype=torch.uint8, device=DEV)
        fn = getattr(lib(), entry)

        def call(_host):
            args = (P(bufs["packed0"]), P(bufs["packed1"]), p, P(bufs["rays"]), 8, 96, nc, ni, 0, 0, ptrs([o.get(f"o{i}") for i in range(8)]),
                    P(ws), ws.numel(), S())
            if entry == "nsr_forward_rays":
                ok(fn(*args), entry)
            elif entry == "nsr_forward_rays_profiled":
                ok(fn(*args, None), entry)
            else:
                ok(fn(*args, None, eps, P(st.get("cut"))), entry)
        return Case(f"{entry}[{tag}]", entry, call, bufs=bufs, A=A, B=B, outs=o, state=st, scratch={"ws": ws},
                    status=blob_status([(bufs["packed0"], p), (bufs["packed1"], p)]))


_forward_rays_case("nsr_forward_rays", "f16x3", 64)
_forward_rays_case("nsr_forward_rays", "fp32", 64)
_forward_rays_case("nsr_forward_rays", "f16", 128)          # 192 fine samples: the unfused route (render + composite)
_forward_rays_case("nsr_forward_rays_profiled", "f16x3", 128)
_forward_rays_case("nsr_forward_rays_ert", "f16x3", 64, eps=1e-3)
_forward_rays_case("nsr_forward_rays_density_coarse", "f16x3", 64)
_forward_rays_case("nsr_forward_rays_density_coarse", "f16x3", 64, eps=1e-3)


# ===================================================================================================== include/nsr_train.h
def _status_block(ws):
    return {"status block": ws[:64]}, {"ws": ws[64:]}


def _train_status(ws):
    def status(_host):
        f = ctypes.c_uint(0)
        ok(lib().nsr_train_status(P(ws), 1, ctypes.byref(f), S()), "nsr_train_status")
        return (int(f.value),)
    return status


def _train_inputs(ctx, wa, wb):
    """Weights of both networks, rays and the four draws as input buffers.  wa / wb: ([coarse], [fine]) for A and B."""
    items = OrderedDict()
    for n in range(2):
        for i, (a, b) in enumerate(zip(wa[n], wb[n])):
            items[f"w{n}_{i}"] = (a, b)
    items["rays"] = (ctx.rays("A"), ctx.rays("B"))
    for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine"):
        items[k] = (ctx.draws("A")[k], ctx.draws("B")[k])
    return items


def _w_lists(bufs, nt):
    return [[bufs[f"w{n}_{i}"] for i in range(nt)] for n in range(2)]


def _out8(nc, ni):
    shapes = [(96, 3), (96,), (96,), (96, nc), (96, 3), (96,), (96,), (96, nc + ni)]
    return OrderedDict((f"o{i}", out_buf(s)) for i, s in enumerate(shapes))


def _fused_train_case(entry, prec, chunk):
    @case(entry, f"{prec}-chunk{chunk}")
    def build(ctx):
        from nerf_sr_amd import _lib
        p, R, nc, ni, s2 = _lib.TRAIN_PRECISIONS[prec], 96, 64, 64, 4
        wa, wb = (ctx.weights("A", 0), ctx.weights("A", 1)), (ctx.weights("B", 0), ctx.weights("B", 1))
        items = _train_inputs(ctx, wa, wb)
        items["target"] = (rnd(30, R // s2, 3), rnd(31, R // s2, 3))
        bufs, A, B = wire(items)
        w = _w_lists(bufs, 24)
        grads = [empty_like_all(w[0]), empty_like_all(w[1])]
        o = _out8(nc, ni)
        extra = OrderedDict([("lr_c", out_buf((R // s2, 3))), ("lr_f", out_buf((R // s2, 3))), ("losses", out_buf((2,)))])
        var = entry == "nsr_train_loss_and_grads_var"
        if var:
            extra["var_losses"] = out_buf((4,))
        ws = torch.zeros(lib().nsr_train_workspace_bytes_for(p, chunk if 0 < chunk < R else R, nc, ni), dtype=torch.uint8, device=DEV)
        st, scratch = _status_block(ws)
        fn = getattr(lib(), entry)
        var_host = (ctypes.c_float * 5)(0.1, 0.1, 0.05, 0.05, 1.0)

        def call(_host):
            args = (ptrs(w[0]), ptrs(w[1]), ptrs(grads[0]), ptrs(grads[1]), P(bufs["rays"]), 8, R, s2, P(bufs["target"]), nc, ni, 0, 0,
                    P(bufs["u_coarse"]), P(bufs["u_fine"]), P(bufs["noise_coarse"]), P(bufs["noise_fine"]), 1.0, 1.0, 1.0, p, chunk,
                    ptrs(list(o.values())), P(extra["lr_c"]), P(extra["lr_f"]), P(extra["losses"]), P(ws), ws.numel(), S())
            if var:
                args += (ctypes.cast(var_host, c_void_p), P(extra["var_losses"]))
            ok(fn(*args), entry)
        outs = OrderedDict(o)
        outs.update(extra)
        outs.update(named("g0_", grads[0]))
        outs.update(named("g1_", grads[1]))
        return Case(f"{entry}[{prec}-chunk{chunk}]", entry, call, bufs=bufs, A=A, B=B, outs=outs, state=st, scratch=scratch, status=_train_status(ws))


for _p_ in ("f16x3", "f16x3_gemm", "fp32"):
    _fused_train_case("nsr_train_loss_and_grads", _p_, 64)
_fused_train_case("nsr_train_loss_and_grads_var", "f16x3", 64)
_fused_train_case("nsr_train_loss_and_grads_var", "fp32", 64)

TRAIN_ARCH = {"D": 3, "W": 48, "skips": (1,), "deg_pos": 4, "deg_dir": 2, "no_dir": False}      # tests/scratch_state.py ARCH


def _pair(ctx, prec, arch, embed, ray_grad, chain_ray_grad, chunk=64):
    """The pieces the forward and the backward cases of one pair share: the run, the inputs, the sizes."""
    from nerf_sr_amd import _lib
    from nerf_sr_amd.train import _TrainRun
    from nerf_sr_amd.weights import normalize_arch
    c_arch = None if arch is None else _lib.NsrArch.from_arch(normalize_arch(dict(arch)))
    run = _TrainRun(64, 64, 0, 0, 1.0, _lib.TRAIN_PRECISIONS[prec], chunk, None, c_arch, embed, ray_grad, chain_ray_grad)
    if arch is None:
        wa, wb = (ctx.weights("A", 0), ctx.weights("A", 1)), (ctx.weights("B", 0), ctx.weights("B", 1))
    else:
        key = tuple(sorted(arch.items()))
        wa = tuple(ctx.arch_weights("A", n, key, embed) for n in range(2))
        wb = tuple(ctx.arch_weights("B", n, key, embed) for n in range(2))
    what, need = run.call("workspace_bytes", run.prec, chunk, 64, 64)
    what_s, nsaved = run.call("saved_bytes", run.prec, 96, 64, 64, chunk)
    assert need > 0 and nsaved > 0, (what, need, what_s, nsaved)
    return run, wa, wb, need, nsaved


def _forward_call(run, w, bufs, o, ws, saved):
    what, rc = run.call("forward", ptrs(w[0]), ptrs(w[1]), P(bufs["rays"]), 8, 96, 64, 64, run.flags, run.lindisp, P(bufs["u_coarse"]),
                        P(bufs["u_fine"]), P(bufs["noise_coarse"]), P(bufs["noise_fine"]), run.noise_std, run.prec, run.chunk,
                        ptrs(list(o.values())), P(ws), ws.numel(), P(saved), saved.numel(), S())
    ok(rc, what)


def _pair_forward_case(entry, prec, arch=None, embed=0):
    @case(entry, prec + (f"-embed{embed}" if embed else ""))
    def build(ctx):
        run, wa, wb, need, nsaved = _pair(ctx, prec, arch, embed, False, False)
        assert run.names["forward"] == entry, (run.names, entry)
        bufs, A, B = wire(_train_inputs(ctx, wa, wb))
        w = _w_lists(bufs, len(wa[0]))
        o = _out8(64, 64)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        saved = torch.zeros(nsaved, dtype=torch.uint8, device=DEV)
        st, scratch = _status_block(ws)
        scratch["saved"] = saved          # opaque (include/nsr_train.h): the backward cases check what it carries
        return Case(f"{entry}[{prec}]", entry, lambda h: _forward_call(run, w, bufs, o, ws, saved), bufs=bufs, A=A, B=B, outs=o, state=st,
                    scratch=scratch, status=_train_status(ws))


def _pair_backward_case(entry, prec, arch=None, embed=0, ray_grad=False, chain_ray_grad=False, no_weight_grads=False):
    tag = prec + (f"-embed{embed}" if embed else "") + ("-g_rays" if (ray_grad or chain_ray_grad) else "") + ("-frozen" if no_weight_grads else "")

    @case(entry, tag)
    def build(ctx):
        from nerf_sr_amd import _lib
        run, wa, wb, need, nsaved = _pair(ctx, prec, arch, embed, ray_grad, chain_ray_grad)
        assert run.names["backward"] == entry, (run.names, entry)
        items = _train_inputs(ctx, wa, wb)
        # the saved state of the forward of A and of B, made here on the default stream
        fb, fA, fB = wire(items)
        fw = _w_lists(fb, len(wa[0]))
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        ok(lib().nsr_train_status_reset(P(ws), S()), "nsr_train_status_reset")
        saved_ab = []
        for src in (fA, fB):
            for k, b in fb.items():
                b.copy_(src[k])
            saved = torch.zeros(nsaved, dtype=torch.uint8, device=DEV)
            _forward_call(run, fw, fb, _out8(64, 64), ws, saved)
            saved_ab.append(saved)
        torch.cuda.synchronize()
        items["saved"] = tuple(saved_ab)
        bufs, A, B = wire(items)
        w = _w_lists(bufs, len(wa[0]))
        g_outs = [randn(40 + i, *s, scale=0.1) for i, s in enumerate([(96, 3), (96,), (96,), (96, 64), (96, 3), (96,), (96,), (96, 128)])]
        grads = [empty_like_all(w[0]), empty_like_all(w[1])]
        outs = OrderedDict()
        if not no_weight_grads:
            outs.update(named("g0_", grads[0]))
            outs.update(named("g1_", grads[1]))
        g_rays = out_buf((96, 8)) if (ray_grad or chain_ray_grad) else None
        if g_rays is not None:
            outs["g_rays"] = g_rays
        st, scratch = _status_block(ws)

        def call(_host):
            gp = (None, None) if no_weight_grads else (ptrs(grads[0]), ptrs(grads[1]))
            tail = (P(ws), ws.numel(), P(bufs["saved"]), nsaved, S())
            if chain_ray_grad:
                args = (ptrs(w[0]), ptrs(w[1]), P(bufs["rays"]), 8, ptrs(g_outs), gp[0], gp[1], P(g_rays), 8,
                        _lib.NSR_BACKWARD_NO_WEIGHT_GRADS if no_weight_grads else 0) + tail
            elif ray_grad:
                args = (ptrs(w[0]), ptrs(w[1]), ptrs(g_outs), gp[0], gp[1], P(g_rays), 8) + tail
            else:
                args = (ptrs(w[0]), ptrs(w[1]), ptrs(g_outs), gp[0], gp[1]) + tail
            what, rc = run.call("backward", *args)
            ok(rc, what)
        return Case(f"{entry}[{tag}]", entry, call, bufs=bufs, A=A, B=B, outs=outs, state=st, scratch=scratch, status=_train_status(ws), waits=True)


for _p_ in ("f16x3", "f16x3_gemm", "fp32", "f16x3_gemm_bwd"):
    _pair_forward_case("nsr_train_forward", _p_)
    _pair_backward_case("nsr_train_backward", _p_)
_pair_backward_case("nsr_train_backward_r", "f16x3", chain_ray_grad=True)
_pair_backward_case("nsr_train_backward_r", "f16x3", chain_ray_grad=True, no_weight_grads=True)
for _p_ in ("fp32", "f16x3_gemm"):
    _pair_forward_case("nsr_train_arch_forward", _p_, TRAIN_ARCH)
    _pair_backward_case("nsr_train_arch_backward", _p_, TRAIN_ARCH)
_pair_forward_case("nsr_train_arch_forward_e", "f16x3_gemm", TRAIN_ARCH, embed=1)
_pair_backward_case("nsr_train_arch_backward_e", "f16x3_gemm", TRAIN_ARCH, embed=1)
_pair_backward_case("nsr_train_arch_backward_e", "f16x3_gemm_bwd", TRAIN_ARCH, embed=1)
for _p_ in ("fp32", "f16x3_gemm_bwd"):
    _pair_backward_case("nsr_train_arch_backward_r", _p_, TRAIN_ARCH, ray_grad=True)


@case("nsr_train_status_reset")
def _status_reset(ctx):
    """The reset lands BEHIND the flags a gated copy puts into the block: stale content 0xFF.., A = 5, B = 9, result 0 either
    way -- so the word next to the block (which the reset must leave alone) carries the A / B difference."""
    a = torch.zeros(128, dtype=torch.uint8, device=DEV)
    a[0], a[64] = 5, 1
    b = torch.zeros(128, dtype=torch.uint8, device=DEV)
    b[0], b[64] = 9, 2
    bufs, A, B = wire({"ws": (a, b)})

    def call(_host):
        ok(lib().nsr_train_status_reset(P(bufs["ws"]), S()), "nsr_train_status_reset")
        return {"ws after": bufs["ws"]}
    return Case("nsr_train_status_reset", "nsr_train_status_reset", call, bufs=bufs, A=A, B=B)


@case("nsr_train_status")
def _train_status_case(ctx):
    """The word a GATED copy puts into the block: A = 6, B = 0 (and a byte behind the block that the call leaves alone)."""
    a = torch.zeros(128, dtype=torch.uint8, device=DEV)
    a[0], a[64] = 6, 1
    b = torch.zeros(128, dtype=torch.uint8, device=DEV)
    b[64] = 2
    bufs, A, B = wire({"ws": (a, b)})
    flags = []

    def call(_host):
        f = ctypes.c_uint(0)
        ok(lib().nsr_train_status(P(bufs["ws"]), 1, ctypes.byref(f), S()), "nsr_train_status")
        flags.append(int(f.value))
        return {"ws after": bufs["ws"]}
    return Case("nsr_train_status", "nsr_train_status", call, bufs=bufs, A=A, B=B, status=lambda h: (flags[-1],), waits=True)


def _adam_case(entry):
    @case(entry)
    def build(ctx):
        if entry == "nsr_adam_step":
            w0 = [t.clone() for t in ctx.weights("A", 0)]
        else:
            w0 = [rnd(70, 1000, lo=-1, hi=1), rnd(71, 37, lo=-1, hi=1), rnd(72, 64, 64, lo=-1, hi=1)]
        n = len(w0)
        bufs, A, B = wire(OrderedDict((f"g{i}", (randn(80 + i, *t.shape, scale=0.01), randn(180 + i, *t.shape, scale=0.01))) for i, t in enumerate(w0)))
        m = [rnd(280 + i, *t.shape, lo=-0.01, hi=0.01) for i, t in enumerate(w0)]
        v = [rnd(380 + i, *t.shape, lo=0.0, hi=1e-4) for i, t in enumerate(w0)]
        st = OrderedDict()
        st.update(named("w", w0))
        st.update(named("m", m))
        st.update(named("v", v))
        g = list(bufs.values())
        numel = (ctypes.c_int64 * n)(*[t.numel() for t in w0])

        def call(_host):
            if entry == "nsr_adam_step":
                ok(lib().nsr_adam_step(ptrs(w0), ptrs(g), ptrs(m), ptrs(v), 3, 5e-4, 0.9, 0.999, 1e-8, S()), entry)
            else:
                ok(lib().nsr_adam_step_n(n, numel, ptrs(w0), ptrs(g), ptrs(m), ptrs(v), 3, 5e-4, 0.9, 0.999, 1e-8, S()), entry)
        return Case(entry, entry, call, bufs=bufs, A=A, B=B, state=st)


_adam_case("nsr_adam_step")
_adam_case("nsr_adam_step_n")


def _fused_arch(ctx, embed):
    from nerf_sr_amd import _lib
    from nerf_sr_amd.weights import normalize_arch
    arch = normalize_arch(dict(Ctx.FUSED_ARCH))
    key = tuple(sorted(Ctx.FUSED_ARCH.items()))
    return _lib.NsrArch.from_arch(arch), ctx.arch_weights("A", 0, key, embed), ctx.arch_weights("B", 0, key, embed)


def _lead(c_arch, e_form, embed):
    return (ctypes.byref(c_arch), embed) if e_form else (ctypes.byref(c_arch),)


def _fused_blob(ctx, which, embed):
    def make():
        c_arch, wa, wb = _fused_arch(ctx, embed)
        b = torch.zeros(lib().nsr_arch_fused_packed_bytes_e(ctypes.byref(c_arch), embed), dtype=torch.uint8, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        ok(lib().nsr_arch_fused_pack_e(ctypes.byref(c_arch), embed, ptrs(wa if which == "A" else wb), P(b), P(st), S()), "nsr_arch_fused_pack_e")
        assert int(st.item()) == 0
        return b
    return ctx.memo(("fused blob", which, embed), make)


def _fused_pack_case(entry, e_form, embed):
    @case(entry)
    def build(ctx):
        c_arch, wa, wb = _fused_arch(ctx, embed)
        bufs, A, B = wire(OrderedDict((f"w{i}", (a, b)) for i, (a, b) in enumerate(zip(wa, wb))))
        o = {"packed": torch.zeros(lib().nsr_arch_fused_packed_bytes_e(ctypes.byref(c_arch), embed), dtype=torch.uint8, device=DEV)}
        st = {"status": torch.zeros(1, dtype=torch.int32, device=DEV)}
        return Case(entry, entry, lambda h: ok(getattr(lib(), entry)(*_lead(c_arch, e_form, embed), ptrs(list(bufs.values())), P(o["packed"]),
                                                                      P(st["status"]), S()), entry), bufs=bufs, A=A, B=B, outs=o, state=st)


_fused_pack_case("nsr_arch_fused_pack", False, 0)
_fused_pack_case("nsr_arch_fused_pack_e", True, 1)


def _fused_forward_case(entry, e_form, embed):
    @case(entry)
    def build(ctx):
        c_arch, _, _ = _fused_arch(ctx, embed)
        first = 0 if embed & 1 else 3
        width = (first + 12) + (first + 6)
        bufs, A, B = wire({"packed": (_fused_blob(ctx, "A", embed), _fused_blob(ctx, "B", embed)),
                           "x": (rnd(90, 300, width, lo=-1, hi=1), rnd(91, 300, width, lo=-1, hi=1))})
        o = {"out": out_buf((300, 4))}
        st = {"status": torch.zeros(1, dtype=torch.int32, device=DEV)}
        return Case(entry, entry, lambda h: ok(getattr(lib(), entry)(*_lead(c_arch, e_form, embed), P(bufs["packed"]), P(bufs["x"]), width, 300, 0,
                                                                      P(o["out"]), 4, P(st["status"]), S()), entry), bufs=bufs, A=A, B=B, outs=o, state=st)


_fused_forward_case("nsr_arch_fused_forward", False, 0)
_fused_forward_case("nsr_arch_fused_forward_e", True, 1)


def _fused_rays_case(entry, e_form, embed):
    @case(entry)
    def build(ctx):
        c_arch, _, _ = _fused_arch(ctx, embed)
        bufs, A, B = wire({"packed": (_fused_blob(ctx, "A", embed), _fused_blob(ctx, "B", embed)), "rays": (ctx.rays("A"), ctx.rays("B")),
                           "z": (ctx.z("A", 64), ctx.z("B", 64))})
        o = {"out": out_buf((96 * 64, 4))}
        st = {"status": torch.zeros(1, dtype=torch.int32, device=DEV)}
        return Case(entry, entry, lambda h: ok(getattr(lib(), entry)(*_lead(c_arch, e_form, embed), P(bufs["packed"]), P(bufs["rays"]), 8, P(bufs["z"]),
                                                                      96, 64, 0, P(o["out"]), 4, P(st["status"]), S()), entry),
                    bufs=bufs, A=A, B=B, outs=o, state=st)


_fused_rays_case("nsr_arch_fused_render_rays", False, 0)
_fused_rays_case("nsr_arch_fused_render_rays_e", True, 1)


# one 65 x 90 -> 64 product; K is padded to 96 (K % 32 == 0), the pad columns of w are zero
def _lin_inputs():
    def w(seed):
        t = rnd(seed, 64, 96, lo=-0.5, hi=0.5)
        t[:, 90:] = 0
        return t
    return OrderedDict([("x", (rnd(100, 65, 96, lo=-1, hi=1), rnd(101, 65, 96, lo=-1, hi=1))), ("w", (w(102), w(103))),
                        ("b", (rnd(104, 64, lo=-1, hi=1), rnd(105, 64, lo=-1, hi=1)))])


_simple("nsr_linear", "65x90->64", lambda c: _lin_inputs(), lambda: {"y": out_buf((65, 64)), "yt": out_buf((64, 65 + 3))},
        lambda b, o, h: ok(lib().nsr_linear(P(b["x"]), 96, P(b["w"]), 96, P(b["b"]), 1, P(o["y"]), 64, P(o["yt"]), 68, 65, 96, 64, S()), "nsr_linear"))
_simple("nsr_split_weights", "", lambda c: {"w": _lin_inputs()["w"]},
        lambda: {"hi": out_buf((64 * 96,), torch.int16), "lo": out_buf((64 * 96,), torch.int16)},
        lambda b, o, h: ok(lib().nsr_split_weights(P(b["w"]), 64 * 96, P(o["hi"]), P(o["lo"]), S()), "nsr_split_weights"))


@case("nsr_linear_f16x3", "65x90->64")
def _linear_f16x3(ctx):
    items = _lin_inputs()
    halves = []
    for w in items.pop("w"):
        hi, lo = torch.zeros(2, 64 * 96, dtype=torch.int16, device=DEV)
        ok(lib().nsr_split_weights(P(w), 64 * 96, P(hi), P(lo), S()), "nsr_split_weights")
        halves.append((hi.clone(), lo.clone()))
    items["hi"] = (halves[0][0], halves[1][0])
    items["lo"] = (halves[0][1], halves[1][1])
    bufs, A, B = wire(items)
    o = {"y": out_buf((65, 64))}
    return Case("nsr_linear_f16x3", "nsr_linear_f16x3",
                lambda h: ok(lib().nsr_linear_f16x3(P(bufs["x"]), 96, P(bufs["hi"]), P(bufs["lo"]), 96, P(bufs["b"]), 2, P(o["y"]), 64, 65, 96, 64, S()),
                             "nsr_linear_f16x3"), bufs=bufs, A=A, B=B, outs=o)


# ============================================================================= include/nsr_metrics.h, include/nsr_losses.h
IMG = (2, 3, 24, 20)


def _images(c):
    return OrderedDict([("x", (rnd(110, *IMG), rnd(111, *IMG))), ("y", (rnd(112, *IMG), rnd(113, *IMG)))])


def _ssim_obj():
    from nerf_sr_amd import metrics
    return metrics.SSIM()


@case("nsr_ssim", "values+map")
def _ssim(ctx):
    s = _ssim_obj()
    win = s._window(torch.device(DEV, torch.cuda.current_device()))
    B, C, H, W = IMG
    bufs, A, Bv = wire(_images(ctx))
    o = {"vals": out_buf((B,), torch.float64), "map": out_buf(IMG)}
    ws = torch.zeros(lib().nsr_ssim_workspace_bytes(B, C, H, W), dtype=torch.uint8, device=DEV)
    return Case("nsr_ssim", "nsr_ssim",
                lambda h: ok(lib().nsr_ssim(P(bufs["x"]), P(bufs["y"]), B, C, H, W, 0, P(win), s.kernel_size[0], s.kernel_size[1], s.c1, s.c2,
                                            P(o["vals"]), P(o["map"]), P(ws), ws.numel(), S()), "nsr_ssim"),
                bufs=bufs, A=A, B=Bv, outs=o, scratch={"ws": ws})


@case("nsr_ssim_backward", "values+map")
def _ssim_backward(ctx):
    s = _ssim_obj()
    win = s._window(torch.device(DEV, torch.cuda.current_device()))
    B, C, H, W = IMG
    items = _images(ctx)
    items["g_ssim"] = (rnd(114, B), rnd(115, B))
    items["g_map"] = (rnd(116, *IMG), rnd(117, *IMG))
    bufs, A, Bv = wire(items)
    o = {"gx": out_buf(IMG), "gy": out_buf(IMG)}
    return Case("nsr_ssim_backward", "nsr_ssim_backward",
                lambda h: ok(lib().nsr_ssim_backward(P(bufs["x"]), P(bufs["y"]), B, C, H, W, 0, P(win), s.kernel_size[0], s.kernel_size[1], s.c1, s.c2,
                                                     P(bufs["g_ssim"]), P(bufs["g_map"]), P(o["gx"]), P(o["gy"]), S()), "nsr_ssim_backward"),
                bufs=bufs, A=A, B=Bv, outs=o)


def _psnr_case(masked):
    @case("nsr_psnr", "mask" if masked else "no mask")
    def build(ctx):
        B, n = IMG[0], IMG[1] * IMG[2] * IMG[3]
        items = _images(ctx)
        if masked:
            m = lambda seed: (rnd(seed, B, n) < 0.7).to(torch.uint8)
            items["mask"] = (m(118), m(119))
        bufs, A, Bv = wire(items)
        o = {"mse": out_buf((B,), torch.float64), "psnr": out_buf((B,), torch.float64)}
        ws = torch.zeros(lib().nsr_psnr_workspace_bytes(B, n), dtype=torch.uint8, device=DEV)
        return Case(f"nsr_psnr[{'mask' if masked else 'no mask'}]", "nsr_psnr",
                    lambda h: ok(lib().nsr_psnr(P(bufs["x"]), P(bufs["y"]), B, n, P(bufs.get("mask")), 1, P(o["mse"]), P(o["psnr"]), P(ws), ws.numel(),
                                                S()), "nsr_psnr"), bufs=bufs, A=A, B=Bv, outs=o, scratch={"ws": ws})


_psnr_case(False)
_psnr_case(True)


def _loss_ws(kind, n, C, H, W):
    return torch.zeros(max(lib().nsr_loss_workspace_bytes(kind, n, C, H, W), 8), dtype=torch.uint8, device=DEV)


@case("nsr_tv_loss")
def _tv(ctx):
    from nerf_sr_amd import _lib
    H, W, C = 24, 20, 3
    bufs, A, B = wire({"x": (rnd(120, H, W, C), rnd(121, H, W, C))})
    o = {"loss": out_buf((1,), torch.float64)}
    ws = _loss_ws(_lib.NSR_LOSS_TV, 1, C, H, W)
    return Case("nsr_tv_loss", "nsr_tv_loss", lambda h: ok(lib().nsr_tv_loss(P(bufs["x"]), H, W, C, P(o["loss"]), P(ws), ws.numel(), S()), "nsr_tv_loss"),
                bufs=bufs, A=A, B=B, outs=o, scratch={"ws": ws})


@case("nsr_tv_loss_backward")
def _tv_backward(ctx):
    H, W, C = 24, 20, 3
    bufs, A, B = wire({"x": (rnd(120, H, W, C), rnd(121, H, W, C)), "g": (rnd(122, 1), rnd(123, 1))})
    o = {"grad": out_buf((H, W, C))}
    return Case("nsr_tv_loss_backward", "nsr_tv_loss_backward",
                lambda h: ok(lib().nsr_tv_loss_backward(P(bufs["x"]), H, W, C, P(bufs["g"]), P(o["grad"]), S()), "nsr_tv_loss_backward"),
                bufs=bufs, A=A, B=B, outs=o)


@case("nsr_gradient_loss")
def _gradient(ctx):
    from nerf_sr_amd import _lib
    B_, C, H, W = IMG
    bufs, A, B = wire(_images(ctx))
    o = {"loss": out_buf((1,), torch.float64)}
    ws = _loss_ws(_lib.NSR_LOSS_GRADIENT, B_, C, H, W)
    return Case("nsr_gradient_loss", "nsr_gradient_loss",
                lambda h: ok(lib().nsr_gradient_loss(P(bufs["x"]), P(bufs["y"]), B_, C, H, W, P(o["loss"]), P(ws), ws.numel(), S()), "nsr_gradient_loss"),
                bufs=bufs, A=A, B=B, outs=o, scratch={"ws": ws})


@case("nsr_gradient_loss_backward")
def _gradient_backward(ctx):
    B_, C, H, W = IMG
    items = _images(ctx)
    items["g"] = (rnd(122, 1), rnd(123, 1))
    bufs, A, B = wire(items)
    o = {"ga": out_buf(IMG), "gb": out_buf(IMG)}
    return Case("nsr_gradient_loss_backward", "nsr_gradient_loss_backward",
                lambda h: ok(lib().nsr_gradient_loss_backward(P(bufs["x"]), P(bufs["y"]), B_, C, H, W, P(bufs["g"]), P(o["ga"]), P(o["gb"]), S()),
                             "nsr_gradient_loss_backward"), bufs=bufs, A=A, B=B, outs=o)


def _lap_inputs():
    return OrderedDict([("d", (rnd(124, 2, 24, 20), rnd(125, 2, 24, 20))), ("guide", (rnd(126, 2, 24, 20, 3), rnd(127, 2, 24, 20, 3)))])


@case("nsr_laplacian_loss", "bilateral")
def _laplacian(ctx):
    from nerf_sr_amd import _lib
    bufs, A, B = wire(_lap_inputs())
    o = {"loss": out_buf((1,), torch.float64)}
    ws = _loss_ws(_lib.NSR_LOSS_LAPLACIAN, 2, 3, 24, 20)
    return Case("nsr_laplacian_loss", "nsr_laplacian_loss",
                lambda h: ok(lib().nsr_laplacian_loss(P(bufs["d"]), P(bufs["guide"]), 2, 24, 20, 3, 0.1, P(o["loss"]), P(ws), ws.numel(), S()),
                             "nsr_laplacian_loss"), bufs=bufs, A=A, B=B, outs=o, scratch={"ws": ws})


@case("nsr_laplacian_loss_backward", "bilateral")
def _laplacian_backward(ctx):
    items = _lap_inputs()
    items["g"] = (rnd(122, 1), rnd(123, 1))
    bufs, A, B = wire(items)
    o = {"grad": out_buf((2, 24, 20))}
    return Case("nsr_laplacian_loss_backward", "nsr_laplacian_loss_backward",
                lambda h: ok(lib().nsr_laplacian_loss_backward(P(bufs["d"]), P(bufs["guide"]), 2, 24, 20, 3, 0.1, P(bufs["g"]), P(o["grad"]), S()),
                             "nsr_laplacian_loss_backward"), bufs=bufs, A=A, B=B, outs=o)


# ===================================================================================================== include/nsr_refine.h
RSHAPE = (2, 2, 16, 24)      # B, R, H, W: fixture case A of tests/golden/refine_train.npz, the smallest the unit tests use


def _refine_images():
    B, R, H, W = RSHAPE
    return OrderedDict([("x", (rnd(130, B, 3, H, W, lo=-1, hi=1), rnd(131, B, 3, H, W, lo=-1, hi=1))),
                        ("c", (rnd(132, B, R, 3, H, W, lo=-1, hi=1), rnd(133, B, R, 3, H, W, lo=-1, hi=1)))])


def _refine_noref_sd(ctx, which):
    def make():
        from nerf_sr_amd import refine as rf
        sd = rf.make_refine_state_dict(5 if which == "A" else 6, not_use_ref=True)
        return [torch.from_numpy(np.ascontiguousarray(sd[k])).to(DEV).float().contiguous() for k in rf.REFINE_SPEC_NOREF]
    return ctx.memo(("refine noref", which), make)


def _refine_tensors(ctx, which, noref):
    return _refine_noref_sd(ctx, which) if noref else list(ctx.refine_sd(which).values())


def _refine_pack_case(entry, noref, prec):
    @case(entry, prec)
    def build(ctx):
        p = _prec(prec)
        ta, tb = _refine_tensors(ctx, "A", noref), _refine_tensors(ctx, "B", noref)
        bufs, A, B = wire(OrderedDict((f"t{i}", (a, b)) for i, (a, b) in enumerate(zip(ta, tb))))
        size = (lib().nsr_refine_packed_bytes_noref if noref else lib().nsr_refine_packed_bytes)(p)
        o = {"packed": torch.zeros(size, dtype=torch.uint8, device=DEV)}
        return Case(f"{entry}[{prec}]", entry, lambda h: ok(getattr(lib(), entry)(ptrs(list(bufs.values())), P(o["packed"]), p, S()), entry),
                    bufs=bufs, A=A, B=B, outs=o)


for _p_ in ("fp32", "f16x3"):
    _refine_pack_case("nsr_refine_pack_weights", False, _p_)
_refine_pack_case("nsr_refine_pack_weights_noref", True, "f16x3")


def _refine_blob(ctx, which, noref, prec):
    def make():
        p = _prec(prec)
        size = (lib().nsr_refine_packed_bytes_noref if noref else lib().nsr_refine_packed_bytes)(p)
        b = torch.zeros(size, dtype=torch.uint8, device=DEV)
        fn = lib().nsr_refine_pack_weights_noref if noref else lib().nsr_refine_pack_weights
        ok(fn(ptrs(_refine_tensors(ctx, which, noref)), P(b), p, S()), "nsr_refine_pack_weights")
        torch.cuda.synchronize()
        return b
    return ctx.memo(("refine blob", which, noref, prec), make)


def _refine_forward_case(noref, prec):
    entry = "nsr_refine_forward_noref" if noref else "nsr_refine_forward"

    @case(entry, prec)
    def build(ctx):
        p = _prec(prec)
        B, R, H, W = RSHAPE
        items = _refine_images()
        if noref:
            del items["c"]
        items["packed"] = (_refine_blob(ctx, "A", noref, prec), _refine_blob(ctx, "B", noref, prec))
        bufs, A, Bv = wire(items)
        o = {"out": out_buf((B, 3, H, W))}
        ws = torch.zeros(lib().nsr_refine_workspace_bytes_for(p, B, 1 if noref else R, H, W), dtype=torch.uint8, device=DEV)

        def call(_host):
            if noref:
                ok(lib().nsr_refine_forward_noref(P(bufs["packed"]), p, P(bufs["x"]), B, H, W, P(o["out"]), P(ws), ws.numel(), S()), entry)
            else:
                ok(lib().nsr_refine_forward(P(bufs["packed"]), p, P(bufs["x"]), P(bufs["c"]), B, R, H, W, P(o["out"]), P(ws), ws.numel(), S()), entry)
        return Case(f"{entry}[{prec}]", entry, call, bufs=bufs, A=A, B=Bv, outs=o, scratch={"ws": ws})


for _p_ in ("fp32", "f16x3"):
    _refine_forward_case(False, _p_)
    _refine_forward_case(True, _p_)


def _refine_train_parts(ctx):
    """The 72 parameters as input buffers (A / B), the 34 running statistics as in-place state, the 106-pointer array."""
    from nerf_sr_amd import refine as rf
    sa, sb = ctx.refine_sd("A"), ctx.refine_sd("B")
    items = OrderedDict((k, (sa[k], sb[k])) for k in rf.TRAIN_PARAM_KEYS)
    items.update(_refine_images())
    bufs, A, B = wire(items)
    running = OrderedDict((k, sa[k].clone()) for k in rf.RUNNING_KEYS)
    by_name = dict(bufs)
    by_name.update(running)
    t106 = [by_name[k] for k in rf.REFINE_SPEC]
    return rf, bufs, A, B, running, t106


def _refine_train_forward_call(entry, prec, t106, running, bufs, y, ws, saved):
    B, R, H, W = RSHAPE
    common = (ptrs(t106), ptrs(list(running.values())), 0.1, P(bufs["x"]), P(bufs["c"]), B, R, H, W, 1, P(y), P(ws), ws.numel(), P(saved), saved.numel(), S())
    if entry == "nsr_refine_train_forward":
        ok(lib().nsr_refine_train_forward(*common), entry)
    else:
        ok(lib().nsr_refine_train_forward_p(prec, *common), entry)


def _refine_train_sizes():
    B, R, H, W = RSHAPE
    return lib().nsr_refine_train_workspace_bytes(B, R, H, W, 1), lib().nsr_refine_train_saved_bytes(B, R, H, W)


def _refine_train_forward_case(entry, precision):
    @case(entry, precision)
    def build(ctx):
        rf, bufs, A, Bv, running, t106 = _refine_train_parts(ctx)
        prec = rf.TRAIN_PRECISIONS[precision]
        need, nsaved = _refine_train_sizes()
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        saved = torch.zeros(nsaved, dtype=torch.uint8, device=DEV)
        o = {"y": out_buf((RSHAPE[0], 3, RSHAPE[2], RSHAPE[3]))}
        return Case(f"{entry}[{precision}]", entry, lambda h: _refine_train_forward_call(entry, prec, t106, running, bufs, o["y"], ws, saved),
                    bufs=bufs, A=A, B=Bv, outs=o, state=running, scratch={"ws": ws, "saved": saved})


_refine_train_forward_case("nsr_refine_train_forward", "fp32")
_refine_train_forward_case("nsr_refine_train_forward_p", "fp32")
_refine_train_forward_case("nsr_refine_train_forward_p", "f16x3_mixed")


def _refine_train_backward_case(entry, precision, weight_grad="fp32"):
    @case(entry, f"{precision}-wgrad_{weight_grad}")
    def build(ctx):
        rf, fb, fA, fB, running, t106f = _refine_train_parts(ctx)
        prec, wg = rf.TRAIN_PRECISIONS[precision], rf.WEIGHT_GRADS[weight_grad]
        need, nsaved = _refine_train_sizes()
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        saved_ab = []
        for src in (fA, fB):
            for k, b in fb.items():
                b.copy_(src[k])
            saved = torch.zeros(nsaved, dtype=torch.uint8, device=DEV)
            _refine_train_forward_call("nsr_refine_train_forward_p", prec, t106f, running, fb, out_buf((RSHAPE[0], 3, RSHAPE[2], RSHAPE[3])), ws, saved)
            saved_ab.append(saved)
        torch.cuda.synchronize()
        # the backward's own buffers: the 72 parameters again (the backward reads the weights), g_out and the saved state
        items = OrderedDict((k, (fA[k], fB[k])) for k in rf.TRAIN_PARAM_KEYS)
        shape = (RSHAPE[0], 3, RSHAPE[2], RSHAPE[3])
        items["g_out"] = (randn(140, *shape, scale=1e-3), randn(141, *shape, scale=1e-3))
        items["saved"] = tuple(saved_ab)
        bufs, A, Bv = wire(items)
        by_name = dict(bufs)
        by_name.update(running)
        t106 = [by_name[k] for k in rf.REFINE_SPEC]
        grads = [torch.zeros_like(bufs[k]) for k in rf.TRAIN_PARAM_KEYS]

        def call(_host):
            tail = (ptrs(t106), P(bufs["g_out"]), ptrs(grads), P(ws), ws.numel(), P(bufs["saved"]), nsaved, S())
            if entry == "nsr_refine_train_backward":
                ok(lib().nsr_refine_train_backward(*tail), entry)
            elif entry == "nsr_refine_train_backward_p":
                ok(lib().nsr_refine_train_backward_p(prec, *tail), entry)
            else:
                ok(lib().nsr_refine_train_backward_w(prec, wg, *tail), entry)
        return Case(f"{entry}[{precision}-wgrad_{weight_grad}]", entry, call, bufs=bufs, A=A, B=Bv, outs=named("g", grads), scratch={"ws": ws}, waits=True)


_refine_train_backward_case("nsr_refine_train_backward", "fp32")
_refine_train_backward_case("nsr_refine_train_backward_p", "f16x3_mixed")
_refine_train_backward_case("nsr_refine_train_backward_w", "fp32", "f16x3")
_refine_train_backward_case("nsr_refine_train_backward_w", "f16x3_mixed", "f16x3")


# the tiler on a 2 x 2 grid of 16 x 16 tiles; warp targets inside and outside the image
TILE_H, TILE_W, TILE_P, TILE_R = 32, 32, 16, 2


def _locs(seed):
    return (rnd(seed, TILE_H, TILE_W, 3, lo=-8.0, hi=40.0)).double().contiguous()


def _tiles(ctx, which):
    def make():
        starts = torch.zeros(4, 2, dtype=torch.int32, device=DEV)
        refs = torch.zeros(4, TILE_R, 2, dtype=torch.int32, device=DEV)
        ok(lib().nsr_refine_tile(P(_locs(150 if which == "A" else 151)), TILE_H, TILE_W, TILE_P, TILE_R, P(starts), P(refs), S()), "nsr_refine_tile")
        torch.cuda.synchronize()
        return starts, refs
    return ctx.memo(("tiles", which), make)


_simple("nsr_refine_tile", "2x2", lambda c: {"locs": (_locs(150), _locs(151))},
        lambda: {"starts": out_buf((4, 2), torch.int32), "refs": out_buf((4, TILE_R, 2), torch.int32)},
        lambda b, o, h: ok(lib().nsr_refine_tile(P(b["locs"]), TILE_H, TILE_W, TILE_P, TILE_R, P(o["starts"]), P(o["refs"]), S()), "nsr_refine_tile"))
_simple("nsr_refine_gather", "2x2",
        lambda c: OrderedDict([("sr", (rnd(152, 3, TILE_H, TILE_W), rnd(153, 3, TILE_H, TILE_W))), ("ref", (rnd(154, 3, TILE_H, TILE_W), rnd(155, 3, TILE_H, TILE_W))),
                               ("starts", (_tiles(c, "A")[0], _tiles(c, "B")[0])), ("refs", (_tiles(c, "A")[1], _tiles(c, "B")[1]))]),
        lambda: {"sr_patch": out_buf((4, 3, TILE_P, TILE_P)), "ref_patches": out_buf((4, TILE_R, 3, TILE_P, TILE_P))},
        lambda b, o, h: ok(lib().nsr_refine_gather(P(b["sr"]), P(b["ref"]), TILE_H, TILE_W, TILE_P, TILE_R, P(b["starts"]), P(b["refs"]), 4,
                                                   P(o["sr_patch"]), P(o["ref_patches"]), S()), "nsr_refine_gather"))
_simple("nsr_refine_stitch", "2x2",
        lambda c: OrderedDict([("patches", (rnd(156, 4, 3, TILE_P, TILE_P), rnd(157, 4, 3, TILE_P, TILE_P))), ("starts", (_tiles(c, "A")[0], _tiles(c, "A")[0].clone()))]),
        lambda: {"img": out_buf((3, TILE_H, TILE_W))},
        lambda b, o, h: ok(lib().nsr_refine_stitch(P(b["patches"]), P(b["starts"]), 4, TILE_P, TILE_H, TILE_W, P(o["img"]), S()), "nsr_refine_stitch"))


# ========================================= include/nsr_image.h, nsr_warp.h, nsr_data.h, nsr_refine_data.h: images and batches
IH, IW = 24, 20


def u8(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(DEV)


@case("nsr_resample_pass_u8", "24x20->24x10")
def _resample_pass(ctx):
    from nerf_sr_amd import io as nsr_io
    bounds, kk = nsr_io.lanczos_tables(IW, 10)
    b_dev, k_dev = torch.from_numpy(bounds).to(DEV), torch.from_numpy(kk).to(DEV)
    bufs, A, B = wire({"src": (u8(160, IH, IW, 3), u8(161, IH, IW, 3))})
    o = {"dst": out_buf((IH, 10, 3), torch.uint8)}
    return Case("nsr_resample_pass_u8", "nsr_resample_pass_u8",
                lambda h: ok(lib().nsr_resample_pass_u8(P(bufs["src"]), IH, IW, 3, 1, 10, P(b_dev), P(k_dev), kk.shape[1], P(o["dst"]), S()),
                             "nsr_resample_pass_u8"), bufs=bufs, A=A, B=B, outs=o)


_simple("nsr_image_to_targets", "24x20", lambda c: {"img": (u8(162, IH, IW, 3), u8(163, IH, IW, 3))},
        lambda: {"out": out_buf((IH // 2 * IW // 2, 4, 3))},
        lambda b, o, h: ok(lib().nsr_image_to_targets(P(b["img"]), IH, IW, 2, P(o["out"]), S()), "nsr_image_to_targets"))
_simple("nsr_image_to_targets_rgba", "24x20", lambda c: {"img": (u8(164, IH, IW, 4), u8(165, IH, IW, 4))},
        lambda: {"out": out_buf((IH // 2 * IW // 2, 4, 3))},
        lambda b, o, h: ok(lib().nsr_image_to_targets_rgba(P(b["img"]), IH, IW, 2, P(o["out"]), S()), "nsr_image_to_targets_rgba"))
_simple("nsr_rgba_premultiply_u8", "24x20", lambda c: {"src": (u8(166, IH, IW, 4), u8(167, IH, IW, 4))},
        lambda: {"dst": out_buf((IH, IW, 4), torch.uint8)},
        lambda b, o, h: ok(lib().nsr_rgba_premultiply_u8(P(b["src"]), IH * IW, 0, P(o["dst"]), S()), "nsr_rgba_premultiply_u8"))


@case("nsr_depth_warp", "24x20")
def _depth_warp(ctx):
    from nerf_sr_amd import cameras
    c2w = (ctypes.c_float * 12)(*np.asarray(cameras.spiral_pose(0.2), dtype=np.float32).reshape(12).tolist())
    w2c = (ctypes.c_double * 12)(1, 0, 0, 0.05, 0, 1, 0, -0.02, 0, 0, 1, 0.01)
    bufs, A, B = wire({"depth": (rnd(168, IH, IW, lo=0.1, hi=0.9), rnd(169, IH, IW, lo=0.1, hi=0.9)),
                       "ref_rgb": (rnd(170, 3, IH, IW), rnd(171, 3, IH, IW))})
    o = {"locs": out_buf((IH, IW, 3), torch.float64), "warped": out_buf((3, IH, IW))}
    return Case("nsr_depth_warp", "nsr_depth_warp",
                lambda h: ok(lib().nsr_depth_warp(P(bufs["depth"]), IH, IW, 20.0, c2w, w2c, 1, P(bufs["ref_rgb"]), P(o["locs"]), P(o["warped"]), S()),
                             "nsr_depth_warp"), bufs=bufs, A=A, B=B, outs=o)


@case("nsr_rayset_batch", "64 indices")
def _rayset_batch(ctx):
    from nerf_sr_amd import _lib, cameras
    poses = lambda ts: torch.from_numpy(np.stack([np.asarray(cameras.spiral_pose(t), dtype=np.float32).reshape(12) for t in ts])).to(DEV)
    g = torch.Generator().manual_seed(172)
    idx = lambda: torch.randint(0, 2 * 10 * 12, (64,), generator=g, dtype=torch.int64).to(DEV)
    bufs, A, B = wire(OrderedDict([("poses", (poses((0.1, 0.6)), poses((0.3, 0.9)))), ("hr", (u8(173, 2, IH, IW, 3), u8(174, 2, IH, IW, 3))),
                                   ("lr", (u8(175, 2, IH // 2, IW // 2, 3), u8(176, 2, IH // 2, IW // 2, 3))), ("idx", (idx(), idx()))]))
    d = _lib.NsrRayset(poses=bufs["poses"].data_ptr(), n_views=2, H=IH, W=IW, s=2, focal=float(cameras.llff_focal(IW)), ndc=1, near_=0.0, far_=1.0,
                       options=0, x0=0, y0=0, w=IW // 2, h=IH // 2, hr=bufs["hr"].data_ptr(), lr=bufs["lr"].data_ptr(), C=3,
                       lr_mode=_lib.NSR_LR_FROM_IMAGES, patch_w=0)
    o = {"rays": out_buf((64, 4, 8)), "rgbs": out_buf((64, 3)), "rgbs_ori": out_buf((64, 4, 3))}
    st = {"status": torch.zeros(1, dtype=torch.int32, device=DEV)}
    return Case("nsr_rayset_batch", "nsr_rayset_batch",
                lambda h: ok(lib().nsr_rayset_batch(ctypes.byref(d), P(bufs["idx"]), 64, 0, P(o["rays"]), P(o["rgbs"]), P(o["rgbs_ori"]), P(st["status"]),
                                                    S()), "nsr_rayset_batch"), bufs=bufs, A=A, B=B, outs=o, state=st)


PATCH_W, PATCH_H, PATCH_P, PATCH_R = 64, 48, 16, 2


def _patch_sets(ctx):
    """Two train-split patch sets (three augmentations each: the identity and two drawn perspectives) and a descriptor over
    input BUFFERS of their tables, so that a case can swap one set for the other."""
    def make():
        from nerf_sr_amd.refine_data import RefinePatchSet
        sets = []
        for n, seed in enumerate((180, 190)):
            sets.append(RefinePatchSet(u8(seed, PATCH_H, PATCH_W, 3).cpu().numpy(), u8(seed + 1, PATCH_H, PATCH_W, 3).cpu().numpy(), patch_len=PATCH_P,
                                       num_ref_patches=PATCH_R, ref_offset=8, aug_num=3, generator=torch.Generator().manual_seed(seed + 2), device=DEV))
        torch.cuda.synchronize()
        return sets
    return ctx.memo("patch sets", make)


def _patch_desc(ctx):
    from nerf_sr_amd import _lib
    a, b = _patch_sets(ctx)
    bufs, A, B = wire(OrderedDict((k, (getattr(a, k).contiguous(), getattr(b, k).contiguous())) for k in ("gt", "sr", "coeffs", "bboxs")))
    d = _lib.NsrRefinePatchset(gt=bufs["gt"].data_ptr(), sr=bufs["sr"].data_ptr(), ref=bufs["gt"].data_ptr(), coeffs=bufs["coeffs"].data_ptr(),
                               bboxs=bufs["bboxs"].data_ptr(), n_img=1, n_aug=3, H=PATCH_H, W=PATCH_W, patch_len=PATCH_P, num_ref_patches=PATCH_R,
                               ref_offset=8, with_gt_patch=0, mode=_lib.NSR_PATCHES_TRAIN)
    return d, bufs, A, B


@case("nsr_refine_aug_bbox")
def _aug_bbox(ctx):
    d, bufs, A, B = _patch_desc(ctx)
    o = {"bboxs": out_buf((3, 4), torch.int32)}
    return Case("nsr_refine_aug_bbox", "nsr_refine_aug_bbox", lambda h: ok(lib().nsr_refine_aug_bbox(ctypes.byref(d), P(o["bboxs"]), S()), "nsr_refine_aug_bbox"),
                bufs=bufs, A=A, B=B, outs=o)


@case("nsr_refine_warp_image")
def _warp_image(ctx):
    d, bufs, A, B = _patch_desc(ctx)
    o = {"img": out_buf((3, PATCH_H, PATCH_W))}
    return Case("nsr_refine_warp_image", "nsr_refine_warp_image",
                lambda h: ok(lib().nsr_refine_warp_image(ctypes.byref(d), 1, 0, P(o["img"]), S()), "nsr_refine_warp_image"), bufs=bufs, A=A, B=B, outs=o)


@case("nsr_refine_patch_batch", "batch 2")
def _patch_batch(ctx):
    """Positions drawn on the device: raw words the kernel maps into the reference's ranges, so every draw is a valid sample."""
    d, bufs, A, B = _patch_desc(ctx)
    n_words = 2 + 2 * PATCH_R + 1
    g = torch.Generator().manual_seed(195)
    words = lambda: torch.randint(0, 2 ** 31 - 1, (2, n_words), generator=g, dtype=torch.int32).to(DEV)
    more, mA, mB = wire({"aug_idx": (torch.tensor([1, 2], dtype=torch.int32, device=DEV), torch.tensor([2, 0], dtype=torch.int32, device=DEV)),
                         "draws": (words(), words())})
    bufs.update(more)
    A.update(mA)
    B.update(mB)
    o = {"sr_patch": out_buf((2, 3, PATCH_P, PATCH_P)), "gt_patch": out_buf((2, 3, PATCH_P, PATCH_P)),
         "ref_patches": out_buf((2, PATCH_R, 3, PATCH_P, PATCH_P)), "starts": out_buf((2, n_words), torch.int32)}
    st = {"status": torch.zeros(1, dtype=torch.int32, device=DEV)}
    return Case("nsr_refine_patch_batch", "nsr_refine_patch_batch",
                lambda h: ok(lib().nsr_refine_patch_batch(ctypes.byref(d), P(bufs["aug_idx"]), None, P(bufs["draws"]), 2, P(o["sr_patch"]), P(o["gt_patch"]),
                                                          P(o["ref_patches"]), P(o["starts"]), P(st["status"]), S()), "nsr_refine_patch_batch"),
                bufs=bufs, A=A, B=B, outs=o, state=st, status=lambda h: (int(st["status"].item()),))


# =========================================================================================== the Python wrappers themselves
def _wrapper(entry, tag):
    return case(entry, f"wrapper {tag}")


@_wrapper("nsr_forward_rays_profiled", "ops.forward_rays")
def _w_forward_rays(ctx):
    from nerf_sr_amd import ops
    nets = ctx.memo("wrapper nets", lambda: tuple(ops.VanillaMLP(None, precision="f16x3").load_state_dict(
        OrderedDict(zip(ops.STATE_DICT_SPEC, ctx.weights("A", n)))) for n in range(2)))
    bufs, A, B = wire({"rays": (ctx.rays("A"), ctx.rays("B"))})
    return Case("ops.forward_rays", "nsr_forward_rays_profiled", lambda h: dict(ops.forward_rays(nets[0], nets[1], bufs["rays"], 64, 64, False)),
                bufs=bufs, A=A, B=B)


@_wrapper("nsr_ssim", "metrics.SSIM")
def _w_ssim(ctx):
    s = _ssim_obj()
    bufs, A, B = wire(_images(ctx))
    return Case("metrics.SSIM", "nsr_ssim", lambda h: dict(zip(("ssim", "map"), s(bufs["x"], bufs["y"], reduction="none", return_map=True))),
                bufs=bufs, A=A, B=B)


@_wrapper("nsr_psnr", "metrics.mse_psnr")
def _w_psnr(ctx):
    from nerf_sr_amd import metrics
    bufs, A, B = wire(_images(ctx))
    return Case("metrics.mse_psnr", "nsr_psnr", lambda h: dict(zip(("mse", "psnr"), metrics.mse_psnr(bufs["x"], bufs["y"], per_image=True))),
                bufs=bufs, A=A, B=B)


@_wrapper("nsr_gradient_loss", "losses.GradientLoss")
def _w_gradient(ctx):
    from nerf_sr_amd import losses
    bufs, A, B = wire(_images(ctx))
    return Case("losses.GradientLoss", "nsr_gradient_loss", lambda h: {"loss": losses.GradientLoss()(bufs["x"], bufs["y"])}, bufs=bufs, A=A, B=B)


@_wrapper("nsr_ssim_backward", "autograd 1 - SSIM")
def _w_ssim_autograd(ctx):
    s = _ssim_obj()
    bufs, A, B = wire(_images(ctx))

    def call(_host):
        x = bufs["x"].detach().requires_grad_(True)
        loss = 1.0 - s(x, bufs["y"])
        loss.backward()
        return {"loss": loss.detach(), "grad": x.grad}
    return Case("autograd 1 - SSIM", "nsr_ssim_backward", call, bufs=bufs, A=A, B=B)


@_wrapper("nsr_refine_forward", "MaxPoolingModel")
def _w_refine(ctx):
    from nerf_sr_amd import refine as rf
    net = ctx.memo("wrapper refine net", lambda: rf.MaxPoolingModel(precision="f16x3", device=DEV).load_state_dict(ctx.refine_sd("A")))
    bufs, A, B = wire(_refine_images())
    return Case("MaxPoolingModel.forward", "nsr_refine_forward", lambda h: {"y": net(bufs["x"], bufs["c"])}, bufs=bufs, A=A, B=B)


@_wrapper("nsr_refine_pack_weights", "MaxPoolingModel.load_state_dict")
def _w_refine_load(ctx):
    """Loading a network enqueues the pack and returns: the tensors it read are kept alive by the allocator's stream order."""
    from nerf_sr_amd import refine as rf
    sa, sb = ctx.refine_sd("A"), ctx.refine_sd("B")
    bufs, A, B = wire(OrderedDict((k, (sa[k], sb[k])) for k in rf.REFINE_SPEC))
    net = rf.MaxPoolingModel(precision="f16x3", device=DEV)

    def call(_host):
        net.load_state_dict(bufs)
        return {"packed": net.packed}
    return Case("MaxPoolingModel.load_state_dict", "nsr_refine_pack_weights", call, bufs=bufs, A=A, B=B)


def _sd(ctx, which, net):
    from nerf_sr_amd.weights import STATE_DICT_SPEC
    return OrderedDict(zip(STATE_DICT_SPEC, ctx.weights(which, net)))


@_wrapper("nsr_train_loss_and_grads", "Trainer.loss_and_grads")
def _w_trainer(ctx):
    """A Trainer inside a caller's side stream: its own workspace, outputs and flat gradient buffers."""
    from nerf_sr_amd import train
    t = train.Trainer(_sd(ctx, "A", 0), _sd(ctx, "A", 1), downscale=2, randomized=True, noise_std=1.0, precision="f16x3", lr=0.0, ray_chunk=64,
                      device=DEV)
    items = OrderedDict([("rays", (ctx.rays("A"), ctx.rays("B"))), ("target", (rnd(30, 24, 3), rnd(31, 24, 3)))])
    for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine"):
        items[k] = (ctx.draws("A")[k], ctx.draws("B")[k])
    bufs, A, B = wire(items)

    def call(_host):
        t.set_input(bufs["rays"], bufs["target"])
        t.loss_and_grads({k: bufs[k] for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine")})
        res = OrderedDict(t.out)
        res["losses"] = t.losses
        for n in range(2):
            res.update((f"grad{n} {k}", v) for k, v in t.grads[n].items())
        return res
    return Case("Trainer.loss_and_grads", "nsr_train_loss_and_grads", call, bufs=bufs, A=A, B=B)


@_wrapper("nsr_train_forward", "train.forward_rays_train")
def _w_forward_rays_train(ctx):
    from nerf_sr_amd import train
    params = [[t.clone() for t in ctx.weights("A", n)] for n in range(2)]
    items = OrderedDict([("rays", (ctx.rays("A"), ctx.rays("B")))])
    for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine"):
        items[k] = (ctx.draws("A")[k], ctx.draws("B")[k])
    bufs, A, B = wire(items)
    ws = train.TrainWorkspace()

    def call(_host):
        with torch.no_grad():
            return dict(train.forward_rays_train(params[0], params[1], bufs["rays"], {k: bufs[k] for k in list(bufs)[1:]}, noise_std=1.0,
                                                 precision="f16x3", ray_chunk=64, workspace=ws))
    return Case("train.forward_rays_train", "nsr_train_forward", call, bufs=bufs, A=A, B=B)


@_wrapper("nsr_refine_train_forward_p", "refine.forward_train")
def _w_refine_forward_train(ctx):
    from nerf_sr_amd import refine as rf
    sa = ctx.refine_sd("A")
    params = OrderedDict((k, sa[k].clone()) for k in rf.TRAIN_PARAM_KEYS)
    running = OrderedDict((k, sa[k].clone()) for k in rf.RUNNING_KEYS)
    bufs, A, B = wire(_refine_images())

    def call(_host):
        with torch.no_grad():
            return {"y": rf.forward_train(params, running, bufs["x"], bufs["c"], img_chunk=1, precision="f16x3_mixed")}
    return Case("refine.forward_train", "nsr_refine_train_forward_p", call, bufs=bufs, A=A, B=B, state=running)


# the thin wrappers of nerf_sr_amd/ops.py, refine.py, warp.py, io.py and losses.py: `_stream()`, their temporaries, their outputs
def _w_simple(entry, tag, items, fn):
    """``items(ctx) -> name -> (A, B)``; ``fn(ctx, bufs) -> dict of tensors`` calls the wrapper."""
    @_wrapper(entry, tag)
    def build(ctx):
        bufs, A, B = wire(items(ctx))
        return Case(tag, entry, lambda h: fn(ctx, bufs), bufs=bufs, A=A, B=B)


def _ops():
    from nerf_sr_amd import ops
    return ops


def _tup(names, values):
    return OrderedDict(zip(names, values))


def _vanilla(ctx, prec="f16x3"):
    return ctx.memo(("wrapper net", prec), lambda: _ops().VanillaMLP(None, precision=prec).load_state_dict(_sd(ctx, "A", 0)))


def _generic(ctx, fused):
    def make():
        from nerf_sr_amd.weights import arch_spec
        key = tuple(sorted(Ctx.FUSED_ARCH.items()))
        sd = OrderedDict(zip(arch_spec(**Ctx.FUSED_ARCH), ctx.arch_weights("A", 0, key, 0)))
        return _ops().GenericMLP(None, device=DEV, precision="f16x3", fused=fused, **Ctx.FUSED_ARCH).load_state_dict(sd)
    return ctx.memo(("wrapper generic", fused), make)


_X3 = lambda c: {"x": (rnd(1, 300, 3, lo=-1, hi=1), rnd(2, 300, 3, lo=-1, hi=1))}
_RAYS = lambda c: {"rays": (c.rays("A"), c.rays("B"))}
_RAYS_Z = lambda c: {"rays": (c.rays("A"), c.rays("B")), "z": (c.z("A", 64), c.z("B", 64))}
_w_simple("nsr_posenc_e", "ops.PositionalEncoding", _X3, lambda c, b: {"out": _ops().PositionalEncoding(3, 10)(b["x"])})
_w_simple("nsr_sample_along_rays", "ops.sample_along_rays", _RAYS,
          lambda c, b: _tup(("z", "pts"), _ops().sample_along_rays(b["rays"][:, :3], b["rays"][:, 3:6], b["rays"][:, 6], b["rays"][:, 7], 64, False, False)))
_w_simple("nsr_resample_along_rays", "ops.resample_along_rays", lambda c: dict(_RAYS_Z(c), w=(rnd(5, 96, 64), rnd(6, 96, 64))),
          lambda c, b: _tup(("z", "pts"), _ops().resample_along_rays(b["rays"][:, :3], b["rays"][:, 3:6], b["z"], b["w"], 64, False)))
_w_simple("nsr_composite", "ops.VolumetricRenderer",
          lambda c: {"rgb": (rnd(7, 96, 64, 3), rnd(8, 96, 64, 3)), "sigma": (randn(9, 96, 64, scale=20), randn(10, 96, 64, scale=20)), "z": (c.z("A", 64), c.z("B", 64))},
          lambda c, b: _tup(("comp", "depth", "opac", "w"), _ops().VolumetricRenderer()(b["rgb"], b["sigma"], b["z"], True)))
_w_simple("nsr_mlp_forward", "ops.VanillaMLP", lambda c: {"x": (rnd(22, 200, 90, lo=-1, hi=1), rnd(23, 200, 90, lo=-1, hi=1))},
          lambda c, b: {"out": _vanilla(c)(b["x"])})
_w_simple("nsr_render_rays", "ops.render_rays", _RAYS_Z, lambda c, b: _tup(("rgb", "sigma"), _ops().render_rays(_vanilla(c), b["rays"], b["z"])))
_w_simple("nsr_render_rays_composited", "ops.render_rays_composited", _RAYS_Z,
          lambda c, b: _tup(("comp", "depth", "opac", "w"), _ops().render_rays_composited(_vanilla(c), b["rays"], b["z"], False)))
_w_simple("nsr_render_rays_composited_ert", "ops.render_rays_composited early_stop", _RAYS_Z,
          lambda c, b: _tup(("comp", "depth", "opac", "w", "cut"), _ops().render_rays_composited(_vanilla(c), b["rays"], b["z"], False, early_stop=1e-3, want_cut_count=True)))
_w_simple("nsr_render_rays_density", "ops.render_rays_density", _RAYS_Z,
          lambda c, b: _tup(("depth", "opac", "w"), _ops().render_rays_density(_vanilla(c), b["rays"], b["z"])))
_w_simple("nsr_sr_mean", "ops.sr_mean", lambda c: {"hr": (rnd(11, 480, 3), rnd(12, 480, 3))}, lambda c, b: {"lr": _ops().sr_mean(b["hr"], 120, 4)})
_w_simple("nsr_unflatten", "ops.unflatten_reshape", lambda c: {"x": (rnd(13, 480, 3), rnd(14, 480, 3))},
          lambda c, b: {"img": _ops().unflatten_reshape(b["x"], (24, 20), 2)})
_w_simple("nsr_linear_f16x3", "ops.GenericMLP f16x3", lambda c: {"x": (rnd(90, 300, 24, lo=-1, hi=1), rnd(91, 300, 24, lo=-1, hi=1))},
          lambda c, b: {"out": _generic(c, False)(b["x"])})
_w_simple("nsr_arch_fused_forward_e", "ops.GenericMLP fused", lambda c: {"x": (rnd(90, 300, 24, lo=-1, hi=1), rnd(91, 300, 24, lo=-1, hi=1))},
          lambda c, b: {"out": _generic(c, True)(b["x"])})
_w_simple("nsr_arch_fused_render_rays_e", "ops.render_rays fused GenericMLP", _RAYS_Z,
          lambda c, b: _tup(("rgb", "sigma"), _ops().render_rays(_generic(c, True), b["rays"], b["z"])))


def _rf():
    from nerf_sr_amd import refine
    return refine


_w_simple("nsr_refine_tile", "refine.tile_refs", lambda c: {"locs": (_locs(150), _locs(151))},
          lambda c, b: _tup(("starts", "refs"), _rf().tile_refs(b["locs"], TILE_P, TILE_R)))
_w_simple("nsr_refine_gather", "refine.gather_patches",
          lambda c: OrderedDict([("sr", (rnd(152, 3, TILE_H, TILE_W), rnd(153, 3, TILE_H, TILE_W))), ("ref", (rnd(154, 3, TILE_H, TILE_W), rnd(155, 3, TILE_H, TILE_W))),
                                 ("starts", (_tiles(c, "A")[0], _tiles(c, "B")[0])), ("refs", (_tiles(c, "A")[1], _tiles(c, "B")[1]))]),
          lambda c, b: _tup(("sr", "ref"), _rf().gather_patches(b["sr"], b["ref"], b["starts"], b["refs"], TILE_P)))
_w_simple("nsr_refine_stitch", "refine.stitch_patches",
          lambda c: OrderedDict([("patches", (rnd(156, 4, 3, TILE_P, TILE_P), rnd(157, 4, 3, TILE_P, TILE_P))), ("starts", (_tiles(c, "A")[0], _tiles(c, "A")[0].clone()))]),
          lambda c, b: {"img": _rf().stitch_patches(b["patches"], b["starts"], (TILE_W, TILE_H))})


def _depth_warp_wrapper(c, b):
    from nerf_sr_amd import cameras, warp
    w2c = np.array([[1, 0, 0, 0.05], [0, 1, 0, -0.02], [0, 0, 1, 0.01]], dtype=np.float64)
    return _tup(("locs", "warped"), warp.depth_warp(b["depth"], cameras.spiral_pose(0.2), w2c, 20.0, True, b["ref_rgb"]))


_w_simple("nsr_depth_warp", "warp.depth_warp",
          lambda c: {"depth": (rnd(168, IH, IW, lo=0.1, hi=0.9), rnd(169, IH, IW, lo=0.1, hi=0.9)), "ref_rgb": (rnd(170, 3, IH, IW), rnd(171, 3, IH, IW))},
          _depth_warp_wrapper)


def _tv_wrapper(c, b):
    from nerf_sr_amd import losses
    return {"loss": losses.TVLoss()(b["x"])}


def _lap_wrapper(c, b):
    from nerf_sr_amd import losses
    return {"loss": losses.BilateralLaplacianLoss(gamma=0.1)(b["d"], b["guide"])}


_w_simple("nsr_tv_loss", "losses.TVLoss", lambda c: {"x": (rnd(120, 24, 20, 3), rnd(121, 24, 20, 3))}, _tv_wrapper)
_w_simple("nsr_laplacian_loss", "losses.BilateralLaplacianLoss", lambda c: _lap_inputs(), _lap_wrapper)


# ------------------------------------------------------------------ io.py, data.py, refine_data.py: images, scenes, patch sets
def _nio():
    from nerf_sr_amd import io as nsr_io
    return nsr_io


_w_simple("nsr_resample_pass_u8", "io.resize_lanczos_u8 RGB", lambda c: {"img": (u8(200, IH, IW, 3), u8(201, IH, IW, 3))},
          lambda c, b: {"out": _nio().resize_lanczos_u8(b["img"], (IW // 2, IH // 2))})
_w_simple("nsr_rgba_premultiply_u8", "io.resize_lanczos_u8 RGBA", lambda c: {"img": (u8(202, IH, IW, 4), u8(203, IH, IW, 4))},
          lambda c, b: {"out": _nio().resize_lanczos_u8(b["img"], (IW // 2, IH // 2))})
_w_simple("nsr_image_to_targets", "io.lr_targets RGB", lambda c: {"img": (u8(204, IH, IW, 3), u8(205, IH, IW, 3))},
          lambda c, b: _tup(("rgbs", "ori"), _nio().lr_targets(b["img"], (IW, IH), 2)))
_w_simple("nsr_image_to_targets_rgba", "io.lr_targets RGBA", lambda c: {"img": (u8(206, IH, IW, 4), u8(207, IH, IW, 4))},
          lambda c, b: _tup(("rgbs", "ori"), _nio().lr_targets(b["img"], (IW, IH), 2)))


def _cold_tables(c, b):
    """A size pair the process has not resampled yet: the tables are staged inside the call."""
    nio = _nio()
    nio._DEVICE_TABLES.clear()
    return {"out": nio.resize_lanczos_u8(b["img"], (IW // 2, IH // 2))}


_w_simple("nsr_resample_pass_u8", "io.resize_lanczos_u8 new tables", lambda c: {"img": (u8(200, IH, IW, 3), u8(201, IH, IW, 3))}, _cold_tables)


def _raysets(ctx):
    """Two scenes of two 24 x 20 views each.  The cases run the FIRST object with its device tensors as the input buffers."""
    def make():
        from nerf_sr_amd import cameras
        from nerf_sr_amd.data import RaySet
        sets = []
        for ts, seed in (((0.1, 0.6), 210), ((0.3, 0.9), 220)):
            poses = np.stack([np.asarray(cameras.spiral_pose(t), dtype=np.float64)[:3, :4] for t in ts])
            imgs = [u8(seed + i, IH, IW, 3).cpu().numpy() for i in range(2)]
            sets.append(RaySet(poses, imgs, (IW, IH), 2, True, 0.0, 1.0, focal=float(cameras.llff_focal(IW)), device=DEV))
        torch.cuda.synchronize()
        return sets
    return ctx.memo("raysets", make)


def _rayset_case(entry, tag, fn, host=(None, None), idx=None):
    @_wrapper(entry, tag)
    def build(ctx):
        a, b = _raysets(ctx)
        bufs = OrderedDict((k, getattr(a, k)) for k in ("poses", "hr", "lr"))
        A = OrderedDict((k, v.clone()) for k, v in bufs.items())
        B = OrderedDict((k, getattr(b, k).clone()) for k in bufs)
        if idx is not None:
            bufs["idx"], A["idx"], B["idx"] = torch.empty_like(idx[0]).to(DEV), idx[0].to(DEV), idx[1].to(DEV)
        return Case(tag, entry, lambda h: fn(a, bufs, h), bufs=bufs, A=A, B=B, host_A=host[0], host_B=host[1])


_G = torch.Generator().manual_seed(230)
_rayset_case("nsr_rayset_batch", "RaySet.batch", lambda rs, b, h: dict(rs.batch(b["idx"])),
             idx=(torch.randint(0, 240, (64,), generator=_G), torch.randint(0, 240, (64,), generator=_G)))
_rayset_case("nsr_rayset_batch", "RaySet.patch", lambda rs, b, h: dict(rs.patch(h, 1, 2, 4)), host=(0, 1))
_rayset_case("nsr_gen_rays_opt", "RaySet.view_rays", lambda rs, b, h: {"rays": rs.view_rays(h)}, host=(0, 1))
_rayset_case("nsr_gen_rays_opt", "RaySet.view", lambda rs, b, h: dict(rs.view(h)), host=(0, 1))


@_wrapper("nsr_gen_rays_range", "ops.subpixel_rays")
def _w_subpixel_rays(ctx):
    from nerf_sr_amd import cameras
    focal = float(cameras.llff_focal(24))
    return Case("ops.subpixel_rays", "nsr_gen_rays_range", lambda h: {"rays": _ops().subpixel_rays(h, (24, 20), focal, 2, True, device=DEV)},
                host_A=cameras.spiral_pose(0.3), host_B=cameras.spiral_pose(0.8))


def _patch_images(seed):
    return u8(seed, PATCH_H, PATCH_W, 3).cpu().numpy(), u8(seed + 1, PATCH_H, PATCH_W, 3).cpu().numpy()


@_wrapper("nsr_refine_aug_bbox", "RefinePatchSet()")
def _w_patchset_init(ctx):
    """Building a 'train' set reads the boxes back to validate them: a documented wait of the Python layer."""
    from nerf_sr_amd.refine_data import RefinePatchSet

    def call(host):
        gt, sr, seed = host
        s = RefinePatchSet(gt, sr, patch_len=PATCH_P, num_ref_patches=PATCH_R, ref_offset=8, aug_num=3, generator=torch.Generator().manual_seed(seed),
                           device=DEV)
        return {"gt": s.gt, "sr": s.sr, "coeffs": s.coeffs, "bboxs": s.bboxs}
    c = Case("RefinePatchSet()", "nsr_refine_aug_bbox", call, host_A=_patch_images(180) + (182,), host_B=_patch_images(190) + (192,), waits=True)
    c.documented = "RefinePatchSet"
    return c


def _patchset_case(entry, tag, fn, extra=None):
    @_wrapper(entry, tag)
    def build(ctx):
        a, b = _patch_sets(ctx)
        bufs = OrderedDict((k, getattr(a, k)) for k in ("gt", "sr", "coeffs", "bboxs"))
        A = OrderedDict((k, v.clone()) for k, v in bufs.items())
        B = OrderedDict((k, getattr(b, k).clone()) for k in bufs)
        if extra is not None:
            for k, (va, vb) in extra(a, b).items():
                bufs[k], A[k], B[k] = torch.empty_like(va), va, vb
        return Case(tag, entry, lambda h: fn(a, bufs), bufs=bufs, A=A, B=B, status=lambda h: (a.status(clear=True),))


def _dev_gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _drawn(a, b):
    """Positions the sets drew themselves: valid by construction."""
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    sa, sb = a.sample(i32([1, 2]), _dev_gen(7)), b.sample(i32([2, 0]), _dev_gen(8))
    torch.cuda.synchronize()
    return {"aug_idx": (sa["aug_idx"].clone(), sb["aug_idx"].clone()), "starts": (sa["starts"].clone(), sb["starts"].clone())}


_patchset_case("nsr_refine_patch_batch", "RefinePatchSet.sample", lambda s, b: dict(s.sample(b["idx"], _dev_gen(9))),
               extra=lambda a, b: {"idx": (torch.tensor([1, 5], dtype=torch.int32, device=DEV), torch.tensor([2, 3], dtype=torch.int32, device=DEV))})
_patchset_case("nsr_refine_patch_batch", "RefinePatchSet.batch", lambda s, b: dict(s.batch(b["aug_idx"], b["starts"])), extra=_drawn)
_patchset_case("nsr_refine_warp_image", "RefinePatchSet.warped_image", lambda s, b: {"img": s.warped_image(1, "gt")})


@_wrapper("nsr_refine_forward_noref", "MaxPoolingModel not_use_ref")
def _w_refine_noref(ctx):
    from nerf_sr_amd import refine as rf

    def make():
        sd = OrderedDict(zip(rf.REFINE_SPEC_NOREF, _refine_noref_sd(ctx, "A")))
        return rf.MaxPoolingModel(precision="f16x3", device=DEV, not_use_ref=True).load_state_dict(sd)
    net = ctx.memo("wrapper refine noref net", make)
    items = _refine_images()
    del items["c"]
    bufs, A, B = wire(items)
    return Case("MaxPoolingModel not_use_ref", "nsr_refine_forward_noref", lambda h: {"y": net(bufs["x"])}, bufs=bufs, A=A, B=B)


@_wrapper("nsr_refine_pack_weights", "MaxPoolingModel.load_state_dict fp16 state dict")
def _w_refine_load_half(ctx):
    """A state dict that is not fp32: the loader makes fp32 temporaries, packs from them and drops them while the pack is still
    queued behind the gate.  The allocator hands their blocks to later work of the same stream only."""
    from nerf_sr_amd import refine as rf
    sa, sb = ctx.refine_sd("A"), ctx.refine_sd("B")
    bufs, A, B = wire(OrderedDict((k, (sa[k].half(), sb[k].half())) for k in rf.REFINE_SPEC))
    net = rf.MaxPoolingModel(precision="f16x3", device=DEV)

    def call(_host):
        net.load_state_dict(bufs)
        churn = [torch.full((1 << 20,), 3.0, device=DEV) for _ in range(8)]     # takes the freed blocks and overwrites them
        del churn
        return {"packed": net.packed}
    return Case("MaxPoolingModel.load_state_dict fp16", "nsr_refine_pack_weights", call, bufs=bufs, A=A, B=B)


def _refine_trainer(ctx):
    from nerf_sr_amd import refine as rf
    t = rf.RefineTrainer(ctx.refine_sd("A"), device=DEV, img_chunk=1)
    state = OrderedDict()
    for name, d in (("p", t.params), ("run", t.running), ("m", t.exp_avg), ("v", t.exp_avg_sq)):
        state.update((f"{name} {k}", v.detach()) for k, v in d.items())
    return t, state


@_wrapper("nsr_refine_train_backward_w", "RefineTrainer.optimize_parameters")
def _w_refine_trainer(ctx):
    """forward, L1 loss in torch, backward (which reads the saved header back: the documented wait of its row) and Adam."""
    t, state = _refine_trainer(ctx)
    items = _refine_images()
    items["gt"] = (rnd(134, RSHAPE[0], 3, RSHAPE[2], RSHAPE[3], lo=-1, hi=1), rnd(135, RSHAPE[0], 3, RSHAPE[2], RSHAPE[3], lo=-1, hi=1))
    bufs, A, B = wire(items)

    def call(_host):
        t.step = 0
        t.set_input({"sr_patch": bufs["x"], "ref_patches": bufs["c"], "gt_patch": bufs["gt"]})
        return {"loss": t.optimize_parameters(), "pred": t.pred.detach()}
    return Case("RefineTrainer.optimize_parameters", "nsr_refine_train_backward_w", call, bufs=bufs, A=A, B=B, state=state, waits=True)


@_wrapper("nsr_adam_step_n", "RefineTrainer.optimizer_step")
def _w_refine_adam(ctx):
    t, state = _refine_trainer(ctx)
    bufs, A, B = OrderedDict(), OrderedDict(), OrderedDict()
    for i, (k, p) in enumerate(t.params.items()):
        bufs[k], A[k], B[k] = torch.empty_like(p.detach()), randn(300 + i, *p.shape, scale=0.01), randn(400 + i, *p.shape, scale=0.01)
        p.grad = bufs[k]

    def call(_host):
        t.step = 0
        t.optimizer_step()
    return Case("RefineTrainer.optimizer_step", "nsr_adam_step_n", call, bufs=bufs, A=A, B=B, state=state)


def _trainer_case(entry, tag, documented=None, **kw):
    @_wrapper(entry, tag)
    def build(ctx):
        from nerf_sr_amd import train
        t = train.Trainer(_sd(ctx, "A", 0), _sd(ctx, "A", 1), downscale=2, randomized=True, noise_std=1.0, precision="f16x3", lr=5e-4, ray_chunk=64,
                          device=DEV, **kw)
        rays_b = ctx.rays("B")
        if documented is not None:           # the value read back differs between the sets: an early read would take B's far bound
            rays_b = rays_b.clone()
            rays_b[:, 7] = 0.9
        items = OrderedDict([("rays", (ctx.rays("A"), rays_b)), ("target", (rnd(30, 24, 3), rnd(31, 24, 3)))])
        for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine"):
            items[k] = (ctx.draws("A")[k], ctx.draws("B")[k])
        bufs, A, B = wire(items)
        state = OrderedDict()
        for name in ("params", "exp_avg", "exp_avg_sq"):
            for n in range(2):
                state.update((f"{name}{n} {k}", v) for k, v in getattr(t, name)[n].items())

        def call(_host):
            t.step = 0
            t.set_input(bufs["rays"], bufs["target"])
            losses = t.optimize_parameters({k: bufs[k] for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine")})
            res = OrderedDict(t.out)
            res["losses"], res["var_losses"] = losses, t.var_losses
            return res
        c = Case(tag, entry, call, bufs=bufs, A=A, B=B, state=state, waits=documented is not None, status=lambda h: (t.status(clear=True),))
        c.documented = documented
        return c


_trainer_case("nsr_adam_step_n", "Trainer.optimize_parameters")
_trainer_case("nsr_train_loss_and_grads_var", "Trainer.optimize_parameters colour variance", use_var_loss=True)
_trainer_case("nsr_train_loss_and_grads_var", "Trainer.optimize_parameters depth variance", documented="Trainer far", use_depth_var_loss=True)


def _loss_autograd(entry, tag, items, loss_of):
    @_wrapper(entry, tag)
    def build(ctx):
        bufs, A, B = wire(items(ctx))

        def call(_host):
            x = next(iter(bufs.values())).detach().requires_grad_(True)
            loss = loss_of(x, bufs)
            loss.backward()
            return {"loss": loss.detach(), "grad": x.grad}
        return Case(tag, entry, call, bufs=bufs, A=A, B=B)


def _losses():
    from nerf_sr_amd import losses
    return losses


_loss_autograd("nsr_tv_loss_backward", "autograd TVLoss", lambda c: {"x": (rnd(120, 24, 20, 3), rnd(121, 24, 20, 3))},
               lambda x, b: _losses().TVLoss()(x))
_loss_autograd("nsr_gradient_loss_backward", "autograd GradientLoss", _images, lambda x, b: _losses().GradientLoss()(x, b["y"]))
_loss_autograd("nsr_laplacian_loss_backward", "autograd BilateralLaplacianLoss", lambda c: _lap_inputs(),
               lambda x, b: _losses().BilateralLaplacianLoss(gamma=0.1)(x, b["guide"]))


@_wrapper("nsr_arch_fused_pack_e", "GenericMLP(fused=True).load_state_dict")
def _w_generic_fused_load(ctx):
    """Loading reads the pack's range verdict back (a load-time wait of the Python layer, documented): the blob must still be the
    one of the weights copied in behind the gate."""
    from nerf_sr_amd.weights import arch_spec
    key = tuple(sorted(Ctx.FUSED_ARCH.items()))
    names = list(arch_spec(**Ctx.FUSED_ARCH))
    bufs, A, B = wire(OrderedDict(zip(names, zip(ctx.arch_weights("A", 0, key, 0), ctx.arch_weights("B", 0, key, 0)))))
    net = _ops().GenericMLP(None, device=DEV, precision="f16x3", fused=True, **Ctx.FUSED_ARCH)

    def call(_host):
        net.load_state_dict(bufs)
        return {"packed": net._route._packed}
    c = Case("GenericMLP(fused=True).load_state_dict", "nsr_arch_fused_pack_e", call, bufs=bufs, A=A, B=B, waits=True)
    c.documented = "GenericMLP fused load"
    return c


def _autograd_pair_case(entry, tag, precision, rays_grad):
    """train.forward_rays_train under autograd: the forward, a loss written in torch over all eight outputs, and the backward
    through the Function (its own gradient tensors and saved state), which reads the saved header back: its row's wait."""
    @_wrapper(entry, tag)
    def build(ctx):
        from nerf_sr_amd import train
        params = [[t.clone().requires_grad_(True) for t in ctx.weights("A", n)] for n in range(2)]
        items = OrderedDict([("rays", (ctx.rays("A"), ctx.rays("B")))])
        for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine"):
            items[k] = (ctx.draws("A")[k], ctx.draws("B")[k])
        bufs, A, B = wire(items)
        ws = train.TrainWorkspace()
        g_outs = [randn(40 + i, *s, scale=0.1) for i, s in enumerate([(96, 3), (96,), (96,), (96, 64), (96, 3), (96,), (96,), (96, 128)])]

        def call(_host):
            for p in params[0] + params[1]:
                p.grad = None
            rays = bufs["rays"].detach().requires_grad_(rays_grad)
            out = train.forward_rays_train(params[0], params[1], rays, {k: bufs[k] for k in list(bufs)[1:]}, noise_std=1.0, precision=precision,
                                           ray_chunk=64, workspace=ws)
            sum((o * g).sum() for o, g in zip(out.values(), g_outs)).backward()
            res = OrderedDict((k, v.detach()) for k, v in out.items())
            for n in range(2):
                res.update((f"grad{n}_{i}", p.grad) for i, p in enumerate(params[n]))
            if rays_grad:
                res["g_rays"] = rays.grad
            return res
        return Case(tag, entry, call, bufs=bufs, A=A, B=B, waits=True, status=lambda h: (ws.status(clear=True),))


_autograd_pair_case("nsr_train_backward", "autograd train.forward_rays_train f16x3", "f16x3", False)
_autograd_pair_case("nsr_train_arch_backward_r", "autograd train.forward_rays_train fp32 rays", "fp32", True)
