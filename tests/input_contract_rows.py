"""The rows of tests/input_contract.py: one per public callable of nerf_sr_amd that reaches libnsr.so with a tensor pointer, and
one per autograd binding (``BINDINGS``).  Importing this module touches no device; a builder does.

Shapes: 67 rays (no multiple of the 32-point tile) in 8 and 11 columns, 64 + 64 samples, images 16 x 24, SSIM with its 11 x 11
window, refinement patches 8 x 16 with two references, ``stream_cases.Ctx.FUSED_ARCH`` for the architecture routes.  A state
dict is one argument of many tensors: a row varies one tensor of each rank it holds (a matrix and a bias; a convolution
weight), the others plain.  Networks are packed once per module (``Ctx.memo``)."""
from collections import OrderedDict
from types import SimpleNamespace
from typing import Callable, NamedTuple

import numpy as np
import torch

from tests import stream_cases as sc
from tests.input_contract import Arg, Call, row, both16, RAISES, CONVERTS, FLOAT, INDEX, U8, MASK

DEV = sc.DEV
R, NC, NI = 67, 64, 64
IH, IW = 16, 24
PB, PR, PH, PW = 2, 2, 8, 16          # refinement patches: batch, references, 8 x 16
VIEWS = "as views of one (R,N,4) buffer"


class Binding(NamedTuple):
    entries: frozenset              # the entry points the forward and the backward reach
    run: Callable                   # run(ctx) -> the lines that say what is wrong


BINDINGS: "OrderedDict[str, Binding]" = OrderedDict()      # the autograd bindings (tests/test_gpu_input_contract.py, one test each)


def binding(name: str, entries):
    def deco(fn):
        BINDINGS[name] = Binding(frozenset(entries), fn)
        return fn
    return deco


def _o():
    from nerf_sr_amd import ops
    return ops


def rays8(ctx, which):
    return ctx.memo(("ic rays8", which), lambda: ctx.rays(which)[:R].contiguous())


def rays11(ctx, which):
    def make():
        r = rays8(ctx, which)
        d = r[:, 3:6] / r[:, 3:6].norm(dim=1, keepdim=True)
        return torch.cat([r, d], 1).contiguous()
    return ctx.memo(("ic rays11", which), make)


def zv(ctx, which, n=NC):
    return ctx.memo(("ic z", which, n), lambda: ctx.z(which, n)[:R].contiguous())


def f(A, B, **kw):
    return Arg(A, B, FLOAT, **kw)


def rays_arg(ctx, cols=8, **kw):
    g = rays8 if cols == 8 else rays11
    return f(g(ctx, "A"), g(ctx, "B"), ties=(0, 1), **kw)


def z_arg(ctx, n=NC):
    return f(zv(ctx, "A", n), zv(ctx, "B", n), ties=(0,), repeat=0)


def tup(names, values):
    return OrderedDict(zip(names, values))


def img(seed, *shape, lo=0.0, hi=1.0):
    return both16(sc.rnd(seed, *shape, lo=lo, hi=hi))


# ================================================================================================================ ops.py
@row("ops.PositionalEncoding.__call__", {"nsr_posenc_e"})
def _posenc(ctx):
    pe = _o().PositionalEncoding(3, 10)
    return Call("PositionalEncoding", lambda t: {"out": pe(t["x"])},
                {"x": f(sc.rnd(1, R, 3, lo=-1, hi=1), sc.rnd(2, R, 3, lo=-1, hi=1), ties=(1,))})


def _bounds(ctx):
    return OrderedDict([("near", f(torch.full((R, 1), 0.05, device=DEV), torch.full((R, 1), 0.08, device=DEV), ties=(0,), repeat=0)),
                        ("far", f(sc.rnd(3, R, 1, lo=0.9, hi=1.0), sc.rnd(4, R, 1, lo=0.8, hi=0.9), ties=(0,)))])


def _ori_dir(ctx):
    a, b = rays8(ctx, "A"), rays8(ctx, "B")
    return OrderedDict([("ori", f(a[:, :3].contiguous(), b[:, :3].contiguous(), ties=(0, 1))),
                        ("dir", f(a[:, 3:6].contiguous(), b[:, 3:6].contiguous(), ties=(0, 1)))])


@row("ops.sample_along_rays", {"nsr_sample_along_rays"})
def _sample(ctx):
    args = _ori_dir(ctx)
    args.update(_bounds(ctx))
    args["u"] = f(sc.rnd(5, R, NC), sc.rnd(6, R, NC), ties=(0, 1))
    return Call("sample_along_rays", lambda t: tup(("z", "pts"), _o().sample_along_rays(t["ori"], t["dir"], t["near"], t["far"], NC, True, False, t["u"])), args)


@row("ops.resample_along_rays", {"nsr_resample_along_rays"})
def _resample(ctx):
    args = _ori_dir(ctx)
    args["z_vals"] = z_arg(ctx)
    args["weights"] = f(sc.rnd(7, R, NC), sc.rnd(8, R, NC), ties=(0, 1))
    args["u"] = f(sc.rnd(9, R, NI), sc.rnd(10, R, NI), ties=(0, 1))
    return Call("resample_along_rays",
                lambda t: tup(("z", "pts"), _o().resample_along_rays(t["ori"], t["dir"], t["z_vals"], t["weights"], NI, True, t["u"])), args)


def _sd_args(names, wa, wb, picks, **kw):
    """The state dict as a call: ``picks`` are the tensors that are varied, the rest stays A's."""
    base = OrderedDict(zip(names, wa))
    other = OrderedDict(zip(names, wb))
    args = OrderedDict((k, f(both16(base[k]), both16(other[k]), policy=CONVERTS, host_ok=True,
                             ties=tuple(range(base[k].ndim)), **kw)) for k in picks)
    return base, args


def _load_call(name, names, wa, wb, picks, make, packed_of):
    base, args = _sd_args(names, wa, wb, picks)

    def fn(t):
        sd = OrderedDict(base)
        sd.update(t)
        net = make().load_state_dict(sd)
        return {"packed": packed_of(net)}
    return Call(name, fn, args)


@row("ops.VanillaMLP.load_state_dict", {"nsr_pack_weights", "nsr_weights_set_options"})
def _vanilla_load(ctx):
    from nerf_sr_amd.weights import STATE_DICT_SPEC
    opt = SimpleNamespace(gamma_correct=True)
    return _load_call("VanillaMLP.load_state_dict", list(STATE_DICT_SPEC), ctx.weights("A", 0), ctx.weights("B", 0),
                      ("xyz_encoding_1.0.weight", "xyz_encoding_1.0.bias"), lambda: _o().VanillaMLP(opt, precision="f16x3"), lambda n: n.packed)


@row("ops.VanillaMLP.forward", {"nsr_mlp_forward"})
def _vanilla_forward(ctx):
    net = sc._vanilla(ctx)
    return Call("VanillaMLP.forward", lambda t: {"out": net(t["x"])},
                {"x": f(sc.rnd(22, R, 90, lo=-1, hi=1), sc.rnd(23, R, 90, lo=-1, hi=1), ties=(1,))})


def _arch_names():
    from nerf_sr_amd.weights import arch_spec
    return list(arch_spec(**sc.Ctx.FUSED_ARCH))


def _arch_w(ctx, which):
    return ctx.arch_weights(which, 0, tuple(sorted(sc.Ctx.FUSED_ARCH.items())), 0)


def _generic_load(name, precision, fused, packed_of):
    def build(ctx):
        make = lambda: _o().GenericMLP(None, device=DEV, precision=precision, fused=fused, **sc.Ctx.FUSED_ARCH)
        return _load_call(name, _arch_names(), _arch_w(ctx, "A"), _arch_w(ctx, "B"), ("xyz_encoding_1.0.weight", "xyz_encoding_1.0.bias"), make, packed_of)
    return build


row("ops.GenericMLP.load_state_dict fused", {"nsr_arch_fused_pack_e"})(
    _generic_load("GenericMLP(fused=True).load_state_dict", "f16x3", True, lambda n: n._route._packed))
row("ops.GenericMLP.load_state_dict layers", {"nsr_split_weights"})(
    _generic_load("GenericMLP.load_state_dict", "f16x3", False, lambda n: torch.cat([n._route.linears[0][2].float(), n._route.linears[0][3].float(), n._route.linears[0][1]])))


def _generic_net(ctx, precision, fused):
    def make():
        sd = OrderedDict(zip(_arch_names(), _arch_w(ctx, "A")))
        return _o().GenericMLP(None, device=DEV, precision=precision, fused=fused, **sc.Ctx.FUSED_ARCH).load_state_dict(sd)
    return ctx.memo(("ic generic", precision, fused), make)


def _generic_forward(name, precision, fused):
    def build(ctx):
        net = _generic_net(ctx, precision, fused)
        return Call(name, lambda t: {"out": net(t["x"]), "sigma": net(t["x"], sigma_only=True)},
                    {"x": f(sc.rnd(90, R, 24, lo=-1, hi=1), sc.rnd(91, R, 24, lo=-1, hi=1), ties=(1,))})
    return build


row("ops.GenericMLP.forward fused", {"nsr_arch_fused_forward_e"})(_generic_forward("GenericMLP(fused=True).forward", "f16x3", True))
row("ops.GenericMLP.forward layers f16x3", {"nsr_linear_f16x3"})(_generic_forward("GenericMLP.forward f16x3", "f16x3", False))
row("ops.GenericMLP.forward layers fp32", {"nsr_linear"})(_generic_forward("GenericMLP.forward fp32", "fp32", False))


@row("ops.VolumetricRenderer.forward", {"nsr_composite"})
def _composite(ctx):
    rend = _o().VolumetricRenderer()
    args = OrderedDict([("rgb", f(sc.rnd(7, R, NC, 3), sc.rnd(8, R, NC, 3), ties=(0, 1, 2))),
                        ("sigma", f(sc.randn(9, R, NC, scale=20), sc.randn(10, R, NC, scale=20), ties=(0, 1))), ("z_vals", z_arg(ctx))])
    return Call("VolumetricRenderer.forward", lambda t: tup(("comp", "depth", "opac", "w"), rend(t["rgb"], t["sigma"], t["z_vals"], True)), args)


def _rays_z_row(name, entries, fn, cols=8, declared=None, net=None):
    @row(name, entries, declared)
    def build(ctx):
        model = (net or sc._vanilla)(ctx)
        return Call(name, lambda t: fn(model, t["rays"], t["z_vals"]), {"rays": rays_arg(ctx, cols), "z_vals": z_arg(ctx)}, declared)


_VIEWS = {"returns_views": ("nerf_sr_amd/ops.py", VIEWS)}
_rays_z_row("ops.render_rays VanillaMLP", {"nsr_render_rays"}, lambda m, r, z: tup(("rgb", "sigma"), _o().render_rays(m, r, z)), declared=_VIEWS)
_rays_z_row("ops.render_rays VanillaMLP 11 columns", {"nsr_render_rays"}, lambda m, r, z: tup(("rgb", "sigma"), _o().render_rays(m, r, z)), cols=11,
            declared=_VIEWS)
_rays_z_row("ops.render_rays GenericMLP", {"nsr_arch_fused_render_rays_e"}, lambda m, r, z: tup(("rgb", "sigma"), _o().render_rays(m, r, z)),
            declared=_VIEWS, net=lambda c: _generic_net(c, "f16x3", True))
_rays_z_row("ops.render_rays_sigma", {"nsr_arch_fused_render_rays_e"}, lambda m, r, z: {"sigma": _o().render_rays_sigma(m, r, z)},
            declared=_VIEWS, net=lambda c: _generic_net(c, "f16x3", True))
_rays_z_row("ops.render_rays_composited", {"nsr_render_rays_composited"},
            lambda m, r, z: tup(("comp", "depth", "opac", "w", "raw"), _o().render_rays_composited(m, r, z, False, want_raw=True)))
_rays_z_row("ops.render_rays_composited early_stop", {"nsr_render_rays_composited_ert"},
            lambda m, r, z: tup(("comp", "depth", "opac", "w", "cut"), _o().render_rays_composited(m, r, z, False, early_stop=1e-3, want_cut_count=True)))
_rays_z_row("ops.render_rays_density", {"nsr_render_rays_density"}, lambda m, r, z: tup(("depth", "opac", "w"), _o().render_rays_density(m, r, z)))


def _nets(ctx):
    return ctx.memo("ic nets", lambda: tuple(_o().VanillaMLP(None, precision="f16x3").load_state_dict(sc._sd(ctx, "A", n)) for n in range(2)))


def _forward_rays_row(name, entries, cols=8, **kw):
    @row(name, entries)
    def build(ctx):
        nets = _nets(ctx)
        # ops.forward_rays flattens leading dimensions (its docstring: "rays.reshape(-1, rays.shape[-1])"): the column count is the relation
        return Call(name, lambda t: dict(_o().forward_rays(nets[0], nets[1], t["rays"], NC, NI, False, check=True, **kw)),
                    {"rays": f((rays8 if cols == 8 else rays11)(ctx, "A"), (rays8 if cols == 8 else rays11)(ctx, "B"), ties=(1,), ndim_tied=False)})


_forward_rays_row("ops.forward_rays", {"nsr_forward_rays_profiled", "nsr_weights_status"})
_forward_rays_row("ops.forward_rays 11 columns", {"nsr_forward_rays_profiled", "nsr_weights_status"}, cols=11)
_forward_rays_row("ops.forward_rays early_stop", {"nsr_forward_rays_ert", "nsr_weights_status"}, early_stop=1e-3)
_forward_rays_row("ops.forward_rays coarse_rgb=False", {"nsr_forward_rays_density_coarse", "nsr_weights_status"}, coarse_rgb=False)


@row("ops.sr_mean", {"nsr_sr_mean"})
def _sr_mean(ctx):
    return Call("sr_mean", lambda t: {"lr": _o().sr_mean(t["hr"], IH * IW // 4, 4)}, {"hr": f(sc.rnd(11, IH * IW, 3), sc.rnd(12, IH * IW, 3), ties=(0,))})


@row("ops.unflatten_reshape", {"nsr_unflatten"})
def _unflatten(ctx):
    return Call("unflatten_reshape", lambda t: {"img": _o().unflatten_reshape(t["x"], (IW, IH), 2)},
                {"x": f(sc.rnd(13, IH * IW, 3), sc.rnd(14, IH * IW, 3), ties=(0,))})


# ============================================================================================================ metrics.py
def _m():
    from nerf_sr_amd import metrics
    return metrics


def _pair(seed, *shape, **kw):
    return OrderedDict([("a", f(sc.rnd(seed, *shape), sc.rnd(seed + 1, *shape), ties=tuple(range(len(shape))), **kw)),
                        ("b", f(sc.rnd(seed + 2, *shape), sc.rnd(seed + 3, *shape), ties=tuple(range(len(shape))), **kw))])


@row("metrics.SSIM.__call__", {"nsr_ssim"})
def _ssim(ctx):
    s = _m().SSIM(kernel_size=(11, 11))
    return Call("SSIM", lambda t: tup(("ssim", "map"), s(t["a"], t["b"], reduction="none", return_map=True)), _pair(100, 2, 3, IH, IW, differentiable=True))


def _mask(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g).to(DEV) > 0.4


def _psnr_row(name, fn, mask_shape):
    @row(name, {"nsr_psnr"})
    def build(ctx):
        args = _pair(110, 2, IH, IW, 3)
        args["mask"] = Arg(_mask(114, *mask_shape), _mask(115, *mask_shape), MASK, RAISES, ties=tuple(range(len(mask_shape))), ndim_tied=True,
                           as_is=(torch.uint8, torch.bool))
        return Call(name, lambda t: fn(t["a"], t["b"], t["mask"]), args)


_psnr_row("metrics.mse_psnr", lambda a, b, m: tup(("mse", "psnr"), _m().mse_psnr(a, b, m)), (2, IH, IW, 3))
_psnr_row("metrics.PSNR", lambda a, b, m: {"psnr": _m().PSNR()(a, b, m)}, (2, IH, IW))
_psnr_row("metrics.psnr_per_image", lambda a, b, m: {"psnr": _m().psnr_per_image(a, b, m)}, (2, IH, IW))


# ============================================================================================================= losses.py
def _l():
    from nerf_sr_amd import losses
    return losses


def _lc(A, B, **kw):
    return f(both16(A), both16(B), policy=CONVERTS, differentiable=True, **kw)


@row("losses.TVLoss", {"nsr_tv_loss"})
def _tv(ctx):
    return Call("TVLoss", lambda t: {"loss": _l().TVLoss()(t["x"])}, {"x": _lc(sc.rnd(120, IH, IW, 3), sc.rnd(121, IH, IW, 3))})


@row("losses.GradientLoss", {"nsr_gradient_loss"})
def _gradient(ctx):
    sh = (2, 3, IH, IW)
    return Call("GradientLoss", lambda t: {"loss": _l().GradientLoss()(t["a"], t["b"])},
                {"a": _lc(sc.rnd(122, *sh), sc.rnd(123, *sh), ties=(0, 1, 2, 3)), "b": _lc(sc.rnd(124, *sh), sc.rnd(125, *sh), ties=(0, 1, 2, 3))})


@row("losses.LaplacianLoss", {"nsr_laplacian_loss"})
def _laplacian(ctx):
    return Call("LaplacianLoss", lambda t: {"loss": _l().LaplacianLoss()(t["d"])}, {"d": _lc(sc.rnd(126, 2, IH, IW), sc.rnd(127, 2, IH, IW))})


@row("losses.BilateralLaplacianLoss", {"nsr_laplacian_loss"})
def _bilateral(ctx):
    guide = f(both16(sc.rnd(130, 2, IH, IW, 3)), both16(sc.rnd(131, 2, IH, IW, 3)), policy=CONVERTS, ties=(0, 1, 2))
    return Call("BilateralLaplacianLoss", lambda t: {"loss": _l().BilateralLaplacianLoss(gamma=0.1)(t["d"], t["guide"])},
                {"d": _lc(sc.rnd(128, 2, IH, IW), sc.rnd(129, 2, IH, IW), ties=(0, 1, 2)), "guide": guide})


# ============================================================================================================= refine.py
def _rf():
    from nerf_sr_amd import refine
    return refine


def _refine_load_row(name, entry, noref):
    @row(name, {entry})
    def build(ctx):
        rf = _rf()
        spec = rf.REFINE_SPEC_NOREF if noref else rf.REFINE_SPEC
        wa = sc._refine_noref_sd(ctx, "A") if noref else list(ctx.refine_sd("A").values())
        wb = sc._refine_noref_sd(ctx, "B") if noref else list(ctx.refine_sd("B").values())
        return _load_call(name, list(spec), wa, wb, ("E.conv1.weight", "E.conv2_bnorm.running_var"),
                          lambda: rf.MaxPoolingModel(precision="f16x3", device=DEV, not_use_ref=noref), lambda n: n.packed)


_refine_load_row("refine.MaxPoolingModel.load_state_dict", "nsr_refine_pack_weights", False)
_refine_load_row("refine.MaxPoolingModel.load_state_dict not_use_ref", "nsr_refine_pack_weights_noref", True)


def _patches(ctx):
    return OrderedDict([("x", f(sc.rnd(132, PB, 3, PH, PW, lo=-1, hi=1), sc.rnd(133, PB, 3, PH, PW, lo=-1, hi=1), ties=(0, 1, 2, 3))),
                        ("c", f(sc.rnd(134, PB, PR, 3, PH, PW, lo=-1, hi=1), sc.rnd(135, PB, PR, 3, PH, PW, lo=-1, hi=1), ties=(0, 2, 3, 4)))])


def _refine_net(ctx, noref=False):
    def make():
        rf = _rf()
        sd = OrderedDict(zip(rf.REFINE_SPEC_NOREF, sc._refine_noref_sd(ctx, "A"))) if noref else ctx.refine_sd("A")
        return rf.MaxPoolingModel(precision="f16x3", device=DEV, not_use_ref=noref).load_state_dict(sd)
    return ctx.memo(("ic refine net", noref), make)


@row("refine.MaxPoolingModel.forward", {"nsr_refine_forward"})
def _refine_forward(ctx):
    net = _refine_net(ctx)
    return Call("MaxPoolingModel.forward", lambda t: {"y": net(t["x"], t["c"])}, _patches(ctx))


@row("refine.MaxPoolingModel.forward not_use_ref", {"nsr_refine_forward_noref"})
def _refine_forward_noref(ctx):
    net = _refine_net(ctx, True)
    args = _patches(ctx)
    del args["c"]
    args["x"].ties = (1,)
    return Call("MaxPoolingModel(not_use_ref).forward", lambda t: {"y": net(t["x"])}, args)


def _locs(seed):
    return sc.rnd(seed, IH, IW, 3, lo=-4.0, hi=28.0).double().contiguous()


@row("refine.tile_refs", {"nsr_refine_tile"})
def _tile(ctx):
    return Call("tile_refs", lambda t: tup(("starts", "refs"), _rf().tile_refs(t["locs"], PH, PR)), {"locs": f(_locs(150), _locs(151), ties=(2,))})


def _tiles(ctx, which):
    def make():
        out = _rf().tile_refs(_locs(150 if which == "A" else 151), PH, PR)
        torch.cuda.synchronize()
        return out
    return ctx.memo(("ic tiles", which), make)


def _index(A, B, **kw):
    return Arg(A, B, INDEX, CONVERTS, **kw)


@row("refine.gather_patches", {"nsr_refine_gather"})
def _gather(ctx):
    (sa, ra), (sb, rb) = _tiles(ctx, "A"), _tiles(ctx, "B")
    args = OrderedDict([("sr", f(sc.rnd(152, 3, IH, IW), sc.rnd(153, 3, IH, IW), ties=(0, 1, 2))), ("ref", f(sc.rnd(154, 3, IH, IW), sc.rnd(155, 3, IH, IW), ties=(0, 1, 2))),
                        ("starts", _index(sa, sb, ties=(0, 1))), ("ref_starts", _index(ra, rb, ties=(0, 2)))])
    return Call("gather_patches", lambda t: tup(("sr", "ref"), _rf().gather_patches(t["sr"], t["ref"], t["starts"], t["ref_starts"], PH)), args)


@row("refine.stitch_patches", {"nsr_refine_stitch"})
def _stitch(ctx):
    sa = _tiles(ctx, "A")[0]
    n = sa.shape[0]
    sb = sa.flip(0).contiguous()           # the same tiles in another order: valid, and another image
    args = OrderedDict([("patches", f(sc.rnd(156, n, 3, PH, PH), sc.rnd(157, n, 3, PH, PH), ties=(0, 1, 2, 3))), ("starts", _index(sa, sb, ties=(0, 1)))])
    return Call("stitch_patches", lambda t: {"img": _rf().stitch_patches(t["patches"], t["starts"], (IW, IH))}, args)


def _frame_args():
    return OrderedDict([("sr", f(sc.rnd(152, 3, IH, IW, lo=-1, hi=1), sc.rnd(153, 3, IH, IW, lo=-1, hi=1), ties=(0, 1, 2))),
                        ("ref", f(sc.rnd(154, 3, IH, IW, lo=-1, hi=1), sc.rnd(155, 3, IH, IW, lo=-1, hi=1), ties=(0, 1, 2))),
                        ("locs", f(_locs(150), _locs(151), ties=(0, 1, 2)))])


_REFINE_IMAGE = {"nsr_refine_tile", "nsr_refine_gather", "nsr_refine_forward", "nsr_refine_stitch"}


@row("refine.refine_image", _REFINE_IMAGE)
def _refine_image(ctx):
    net = _refine_net(ctx)
    return Call("refine_image", lambda t: {"img": _rf().refine_image(net, t["sr"], t["ref"], t["locs"], PH, PR, batch=4)}, _frame_args())


@row("refine.evaluate_image", _REFINE_IMAGE | {"nsr_ssim", "nsr_psnr"})
def _evaluate_image(ctx):
    net = _refine_net(ctx)
    args = _frame_args()
    args["gt"] = f(sc.rnd(158, 3, IH, IW, lo=-1, hi=1), sc.rnd(159, 3, IH, IW, lo=-1, hi=1), ties=(0, 1, 2))
    return Call("evaluate_image", lambda t: dict(_rf().evaluate_image(net, t["sr"], t["ref"], t["locs"], t["gt"], PH, PR, batch=4)), args)


def _train_parts(ctx):
    rf = _rf()
    sa = ctx.refine_sd("A")
    return (OrderedDict((k, sa[k].clone()) for k in rf.TRAIN_PARAM_KEYS), OrderedDict((k, sa[k].clone()) for k in rf.RUNNING_KEYS))


@row("refine.forward_train", {"nsr_refine_train_forward_p"})
def _forward_train(ctx):
    rf = _rf()
    params, running = _train_parts(ctx)
    pristine = OrderedDict((k, v.clone()) for k, v in running.items())
    sb = ctx.refine_sd("B")
    args = _patches(ctx)
    for k in ("E.conv1.weight", "E.conv1.bias"):
        args[k] = f(params[k], sb[k], ties=tuple(range(params[k].ndim)))

    def fn(t):
        for k, v in running.items():
            v.copy_(pristine[k])
        p = OrderedDict(params)
        p.update((k, t[k]) for k in t if k in p)
        with torch.no_grad():
            return {"y": rf.forward_train(p, running, t["x"], t["c"], img_chunk=1), "running_mean": running["E.conv2_bnorm.running_mean"].clone()}
    return Call("forward_train", fn, args)


@row("refine.RefineTrainer", {"nsr_refine_train_forward_p", "nsr_refine_train_backward_w", "nsr_adam_step_n"})
def _refine_trainer(ctx):
    rf = _rf()
    t = rf.RefineTrainer(ctx.refine_sd("A"), device=DEV, img_chunk=1)
    state = [v.detach() for d in (t.params, t.running, t.exp_avg, t.exp_avg_sq) for v in d.values()]
    pristine = [v.clone() for v in state]
    src = _patches(ctx)
    conv = lambda a: f(both16(a.A), both16(a.B), policy=CONVERTS, host_ok=True, ties=a.ties)
    args = OrderedDict([("sr_patch", conv(src["x"])), ("ref_patches", conv(src["c"])),
                        ("gt_patch", f(img(136, PB, 3, PH, PW, lo=-1, hi=1), img(137, PB, 3, PH, PW, lo=-1, hi=1), policy=CONVERTS, host_ok=True, ties=(0, 1, 2, 3)))])

    def fn(tn):
        with torch.no_grad():
            for v, p in zip(state, pristine):
                v.copy_(p)
        t.step = 0
        t.set_input(tn)
        t.forward()
        t.backward()
        t.optimizer_step()
        return {"loss": t.loss_tot.detach(), "pred": t.pred.detach(), "w": t.params["D.conv9.weight"].detach().clone()}
    return Call("RefineTrainer set_input / forward / backward / optimizer_step", fn, args)


# ============================================================================================== warp.py, io.py, data.py
@row("warp.depth_warp", {"nsr_depth_warp"})
def _depth_warp(ctx):
    from nerf_sr_amd import cameras, warp
    w2c = np.array([[1, 0, 0, 0.05], [0, 1, 0, -0.02], [0, 0, 1, 0.01]], dtype=np.float64)
    pose = cameras.spiral_pose(0.2)
    args = OrderedDict([("depth", f(sc.rnd(168, IH, IW, lo=0.1, hi=0.9), sc.rnd(169, IH, IW, lo=0.1, hi=0.9), ties=(0, 1))),
                        ("ref_rgb", f(sc.rnd(170, 3, IH, IW), sc.rnd(171, 3, IH, IW), ties=(0, 1, 2)))])
    return Call("depth_warp", lambda t: tup(("locs", "warped"), warp.depth_warp(t["depth"], pose, w2c, 20.0, True, t["ref_rgb"])), args)


def _u8(A, B, **kw):
    return Arg(A, B, U8, RAISES, **kw)


def _io_row(name, entries, C, fn):
    @row(name, entries)
    def build(ctx):
        from nerf_sr_amd import io as nio
        return Call(name, lambda t: fn(nio, t["img"]), {"img": _u8(sc.u8(200 + C, IH, IW, C), sc.u8(210 + C, IH, IW, C), ties=(2,) if C == 3 else ())})   # RGBA less one channel is RGB


_io_row("io.resize_lanczos_u8 RGB", {"nsr_resample_pass_u8"}, 3, lambda nio, x: {"out": nio.resize_lanczos_u8(x, (IW // 2, IH // 2))})
_io_row("io.resize_lanczos_u8 RGBA", {"nsr_resample_pass_u8", "nsr_rgba_premultiply_u8"}, 4, lambda nio, x: {"out": nio.resize_lanczos_u8(x, (IW // 2, IH // 2))})
_io_row("io.lr_targets RGB", {"nsr_resample_pass_u8", "nsr_image_to_targets"}, 3, lambda nio, x: tup(("rgbs", "ori"), nio.lr_targets(x, (IW, IH), 2)))
_io_row("io.lr_targets RGBA", {"nsr_resample_pass_u8", "nsr_rgba_premultiply_u8", "nsr_image_to_targets_rgba"}, 4,
        lambda nio, x: tup(("rgbs", "ori"), nio.lr_targets(x, (IW, IH), 2)))


def _scene():
    from nerf_sr_amd import cameras
    poses = np.stack([np.asarray(cameras.spiral_pose(t), dtype=np.float64)[:3, :4] for t in (0.1, 0.6)])
    return poses, float(cameras.llff_focal(IW))


@row("data.RaySet(...)", {"nsr_resample_pass_u8"})
def _rayset_init(ctx):
    """The constructor on images of another size than img_wh: resized on the device, image by image."""
    from nerf_sr_amd.data import RaySet
    poses, focal = _scene()

    def fn(t):
        rs = RaySet(poses, t["images"], (IW, IH), 2, True, 0.0, 1.0, focal=focal, device=DEV)
        return {"hr": rs.hr, "lr": rs.lr}
    return Call("RaySet(...)", fn, {"images": _u8(sc.u8(220, 2, 2 * IH, 2 * IW, 3), sc.u8(221, 2, 2 * IH, 2 * IW, 3), host_ok=True, ties=(3,), per_item=True)})


@row("data.RaySet.batch / patch / view_rays", {"nsr_rayset_batch", "nsr_gen_rays_opt"})
def _rayset(ctx):
    from nerf_sr_amd.data import RaySet
    poses, focal = _scene()
    rs = RaySet(poses, sc.u8(222, 2, IH, IW, 3), (IW, IH), 2, True, 0.0, 1.0, focal=focal, device=DEV)
    n = len(rs)
    g = torch.Generator().manual_seed(230)
    idx = lambda: torch.randint(0, n, (R,), generator=g).to(DEV)

    def fn(t):
        out = OrderedDict(rs.batch(t["idx"]))
        out.update(rs.patch(1, 1, 2, 4))
        out["view_rays"] = rs.view_rays(0)
        return out
    return Call("RaySet.batch, patch, view_rays", fn, {"idx": _index(idx(), idx(), ndim_tied=False)})


def _patchset_make():
    from nerf_sr_amd.refine_data import RefinePatchSet
    return lambda gt, sr: RefinePatchSet(gt, sr, patch_len=sc.PATCH_P, num_ref_patches=sc.PATCH_R, ref_offset=8, aug_num=3,
                                         generator=torch.Generator().manual_seed(182), device=DEV)


@row("refine_data.RefinePatchSet(...)", {"nsr_refine_aug_bbox", "nsr_refine_warp_image"})
def _patchset_init(ctx):
    """The constructor (and ``warped_image``, which shows what it kept)."""
    make = _patchset_make()
    H, W = sc.PATCH_H, sc.PATCH_W
    gta, sra, gtb, srb = (sc.u8(s, H, W, 3) for s in (180, 181, 190, 191))
    args = OrderedDict([("gt_u8", _u8(gta, gtb, host_ok=True, ties=(0, 1, 2), ndim_tied=False)), ("sr_u8", _u8(sra, srb, host_ok=True, ties=(0, 1, 2), ndim_tied=False))])

    def fn(t):
        s = make(t["gt_u8"], t["sr_u8"])
        # s.gt / s.sr are no results: the set KEEPS a dense uint8 device image it is given (its docstring), it does not copy it
        return {"bboxs": s.bboxs, "warped gt": s.warped_image(1, "gt"), "warped sr": s.warped_image(1, "sr")}
    return Call("RefinePatchSet(...), warped_image", fn, args)


@row("refine_data.RefinePatchSet.batch", {"nsr_refine_patch_batch"})
def _patchset_batch(ctx):
    """``batch`` at positions the set drew itself (valid by construction)."""
    s = _patchset_make()(sc.u8(180, sc.PATCH_H, sc.PATCH_W, 3), sc.u8(181, sc.PATCH_H, sc.PATCH_W, 3))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    da, db = s.sample(i32([1, 2, 0]), sc._dev_gen(7)), s.sample(i32([2, 0, 1]), sc._dev_gen(8))
    torch.cuda.synchronize()
    args = OrderedDict([("aug_idx", _index(da["aug_idx"].clone(), db["aug_idx"].clone(), ties=(0,), ndim_tied=False)),
                        ("starts", _index(da["starts"].clone(), db["starts"].clone(), ties=(0, 1), ndim_tied=False))])
    return Call("RefinePatchSet.batch", lambda t: OrderedDict((k, v) for k, v in s.batch(t["aug_idx"], t["starts"]).items() if k != "aug_idx"), args)


# ============================================================================================================== train.py
def _draw_args(ctx, n=R):
    da, db = ctx.draws("A"), ctx.draws("B")
    # forward_rays_train / Trainer copy host draws to the device (``torch.as_tensor(..., device=)``): no `cpu` variant
    return OrderedDict((k, f(da[k][:n].contiguous(), db[k][:n].contiguous(), ties=(0, 1), host_ok=True)) for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine"))


def _tr():
    from nerf_sr_amd import train
    return train


@row("train.forward_rays_train", {"nsr_train_forward", "nsr_train_status_reset", "nsr_train_status"})
def _forward_rays_train(ctx):
    train = _tr()
    params = [[t.clone() for t in ctx.weights("A", n)] for n in range(2)]
    wb = ctx.weights("B", 0)
    args = OrderedDict([("rays", rays_arg(ctx))])
    args.update(_draw_args(ctx))
    args["w0"] = f(params[0][0], wb[0], ties=(0, 1))
    args["b0"] = f(params[0][1], wb[1], ties=(0,))

    def fn(t):
        ws = train.TrainWorkspace()
        pc = list(params[0])
        pc[0], pc[1] = t["w0"], t["b0"]
        with torch.no_grad():
            out = dict(train.forward_rays_train(pc, params[1], t["rays"], {k: t[k] for k in train.DRAW_KEYS}, noise_std=1.0, precision="f16x3",
                                                workspace=ws))
        assert ws.status() == 0
        return out
    return Call("forward_rays_train", fn, args)


def _trainer_row(name, entries, call, declared, sds=None, n=R, downscale=1, **kw):
    @row(name, entries, declared)
    def build(ctx):
        train = _tr()
        sd_c, sd_f = sds(ctx) if sds else (sc._sd(ctx, "A", 0), sc._sd(ctx, "A", 1))
        t = train.Trainer(sd_c, sd_f, downscale=downscale, randomized=True, noise_std=1.0, lr=5e-4, ray_chunk=0, device=DEV, **kw)
        state = [v for name_ in ("params", "exp_avg", "exp_avg_sq") for i in range(2) for v in getattr(t, name_)[i].values()]
        pristine = [v.clone() for v in state]
        # Trainer.set_input flattens leading dimensions ("rays (N_lr, s2, 8 | 11) or (N_lr * s2, 8 | 11)")
        n_lr = n // downscale ** 2
        args = OrderedDict([("rays", f(rays8(ctx, "A")[:n].contiguous(), rays8(ctx, "B")[:n].contiguous(), ties=(0, 1), ndim_tied=False)),
                            ("rgbs", f(sc.rnd(30, n_lr, 3), sc.rnd(31, n_lr, 3), ties=(0, 1), ndim_tied=False))])
        args.update(_draw_args(ctx, n))

        def fn(tn):
            for v, p in zip(state, pristine):
                v.copy_(p)
            t.step = 0
            t._leaves = None
            t._workspace = train.TrainWorkspace()      # afresh: behind the proxy a regrown workspace's status block is never reset
            t.set_input(tn["rays"], tn["rgbs"])
            return call(t, {k: tn[k] for k in train.DRAW_KEYS})
        return Call(name, fn, args, declared)


def _fused_step(t, draws):
    t.loss_and_grads(draws)
    res = OrderedDict(t.out)
    res["losses"], res["var"] = t.losses, t.var_losses.clone()
    res["g"] = t.grads[1]["rgb.0.weight"]
    return res


def _pair_step(t, draws):
    out = t.forward(draws)
    loss = torch.nn.functional.mse_loss(out["fine_comp_rgbs"], t.data_rgbs) + out["coarse_comp_rgbs"].mean()
    t.backward(loss)
    t.optimizer_step()
    res = OrderedDict((k, v.detach()) for k, v in out.items())
    res["g"], res["w"] = t.grads[1]["rgb.0.weight"], t.params[1]["rgb.0.weight"].clone()
    res["status"] = torch.tensor([t.status()], device=DEV)
    return res


_FILLS = {"reuses_output": ("nerf_sr_amd/train.py", "fills ``self.out``, ``self.losses``")}
_OVERWRITTEN = {"reuses_output": ("nerf_sr_amd/train.py", "into ``self.grads`` / ``self.flat_grads`` (OVERWRITTEN")}
_PAIR = {"nsr_adam_step_n", "nsr_train_status_reset", "nsr_train_status"}
_trainer_row("train.Trainer.loss_and_grads", {"nsr_train_loss_and_grads", "nsr_train_status_reset"}, _fused_step, _FILLS, precision="f16x3")
_trainer_row("train.Trainer.loss_and_grads variance losses", {"nsr_train_loss_and_grads_var", "nsr_train_status_reset"}, _fused_step, _FILLS,
             precision="f16x3", use_var_loss=True, n=64, downscale=2)       # a variance needs s^2 > 1 sub-rays per pixel
_trainer_row("train.Trainer.forward / backward / optimizer_step", _PAIR | {"nsr_train_forward", "nsr_train_backward"}, _pair_step, _OVERWRITTEN,
             precision="f16x3")


def _arch_sds(embed):
    def make(ctx):
        from nerf_sr_amd.weights import arch_spec
        key = tuple(sorted(sc.TRAIN_ARCH.items()))
        names = list(arch_spec(no_xyz=bool(embed & 1), **sc.TRAIN_ARCH))
        return tuple(OrderedDict(zip(names, ctx.arch_weights("A", n, key, embed))) for n in range(2))
    return make


_trainer_row("train.Trainer(arch=) forward / backward / optimizer_step", _PAIR | {"nsr_train_arch_forward", "nsr_train_arch_backward"}, _pair_step,
             _OVERWRITTEN, sds=_arch_sds(0), precision="fp32", arch=sc.TRAIN_ARCH)
_trainer_row("train.Trainer(arch=, embed=) forward / backward / optimizer_step", _PAIR | {"nsr_train_arch_forward_e", "nsr_train_arch_backward_e"},
             _pair_step, _OVERWRITTEN, sds=_arch_sds(2), precision="fp32", arch=sc.TRAIN_ARCH, embed=2)


@row("train.Trainer.regularize_patch", {"nsr_train_forward", "nsr_train_backward", "nsr_adam_step_n", "nsr_train_status_reset", "nsr_tv_loss",
                                        "nsr_tv_loss_backward"}, _OVERWRITTEN)
def _regularize_patch(ctx):
    train = _tr()
    t = train.Trainer(sc._sd(ctx, "A", 0), sc._sd(ctx, "A", 1), downscale=1, randomized=False, lr=5e-4, ray_chunk=0, precision="f16x3", device=DEV)
    state = [v for name_ in ("params", "exp_avg", "exp_avg_sq") for n in range(2) for v in getattr(t, name_)[n].values()]
    pristine = [v.clone() for v in state]
    patch = lambda w: ctx.rays(w)[:64].reshape(8, 8, 8).contiguous()

    def fn(tn):
        for v, p in zip(state, pristine):
            v.copy_(p)
        t.step = 0
        t._leaves = None
        t._workspace = train.TrainWorkspace()
        tv = t.regularize_patch(tn["patch_rays"], 8, fused_tv=True)
        return {"tv": tv, "g": t.grads[1]["rgb.0.weight"], "w": t.params[1]["rgb.0.weight"].clone(), "fine": t.out_patch["fine_comp_rgbs"].detach()}
    return Call("Trainer.regularize_patch", fn, {"patch_rays": f(patch("A"), patch("B"), ties=(0, 1, 2), ndim_tied=False)}, _OVERWRITTEN)


@row("train.linear", {"nsr_linear"})
def _linear(ctx):
    train = _tr()
    args = OrderedDict([("x", f(sc.rnd(60, R, 64, lo=-1, hi=1), sc.rnd(61, R, 64, lo=-1, hi=1), ties=(1,))),
                        ("w", f(sc.randn(62, 48, 64, scale=0.1), sc.randn(63, 48, 64, scale=0.1), ties=(0, 1))),
                        ("b", f(sc.randn(64, 48, scale=0.1), sc.randn(65, 48, scale=0.1), ties=(0,)))])
    return Call("train.linear", lambda t: tup(("y",), (train.linear(t["x"], t["w"], t["b"], act=1),)), args)


# ================================================================================================= model.py, pipeline.py
def _model_row(name, entries, make_model):
    @row(name, entries)
    def build(ctx):
        model = ctx.memo(("ic model", name), lambda: make_model(ctx))
        keys = ("out_coarse_comp_rgbs", "out_fine_comp_rgbs", "out_fine_depth", "out_fine_weights")

        def fn(t):
            model.set_input({"rays": t["rays"]})
            model.forward()
            return {k: getattr(model, k) for k in keys}
        # set_input squeezes a leading batch dimension of 1 and flattens (the reference's collated batches); it moves host tensors
        return Call(name, fn, {"rays": f(rays8(ctx, "A"), rays8(ctx, "B"), ties=(1,), ndim_tied=False, host_ok=True)})


def _default_model(ctx):
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    opt = default_options(img_wh=(IW, IH), downscale=2, precision="f16x3")
    return NeRFDownXModel(opt, device=DEV).load_networks(sc._sd(ctx, "A", 0), sc._sd(ctx, "A", 1)).eval()


def _generic_model(ctx):
    import warnings
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    a = sc.Ctx.FUSED_ARCH
    opt = default_options(img_wh=(IW, IH), downscale=2, precision="fp32", D=a["D"], W=a["W"], skips=list(a["skips"]), deg_pos=a["deg_pos"],
                          deg_dir=a["deg_dir"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # "running the layer-by-layer GEMM path": that is the route of this row
        m = NeRFDownXModel(opt, device=DEV)
    sd = OrderedDict(zip(_arch_names(), _arch_w(ctx, "A")))
    return m.load_networks(sd, OrderedDict(zip(_arch_names(), _arch_w(ctx, "B")))).eval()


_model_row("model.NeRFDownXModel set_input / forward_rays", {"nsr_forward_rays_profiled", "nsr_weights_status"}, _default_model)
_model_row("model.NeRFDownXModel set_input / forward_rays GenericMLP", {"nsr_sample_along_rays", "nsr_posenc_e", "nsr_linear", "nsr_composite",
                                                                         "nsr_resample_along_rays"}, _generic_model)


@row("pipeline.render_warp_refine", {"nsr_gen_rays_range", "nsr_forward_rays_profiled", "nsr_weights_status", "nsr_unflatten", "nsr_sr_mean",
                                     "nsr_depth_warp"} | _REFINE_IMAGE)
def _render_warp_refine(ctx):
    from nerf_sr_amd import cameras, pipeline
    model = ctx.memo(("ic model", "pipeline"), lambda: _default_model(ctx))
    net = _refine_net(ctx)
    c2w, ref_c2w, focal = cameras.spiral_pose(0.4), cameras.spiral_pose(0.0), float(cameras.llff_focal(IW))
    return Call("render_warp_refine", lambda t: dict(pipeline.render_warp_refine(model, net, c2w, ref_c2w, t["ref_img"], focal, True, patch_len=PH,
                                                                                 num_ref_patches=PR, batch=4)),
                {"ref_img": f(sc.rnd(170, 3, IH, IW), sc.rnd(171, 3, IH, IW), ties=(0, 1, 2))})


# ============================================================================================== the autograd bindings
def upstream(out: torch.Tensor, seed: int, zero: bool = False) -> torch.Tensor:
    """A contiguous fp32 upstream gradient whose values repeat along dimension 0 (so that an expanded tensor can hold them)."""
    if zero:
        return torch.zeros_like(out)
    g = torch.Generator().manual_seed(seed)
    if out.ndim == 0:
        return torch.tensor(0.75, device=out.device)
    first = both16(torch.randn(1, *out.shape[1:], generator=g) * 0.25).to(out.device)
    return first.expand(out.shape).contiguous()


def _as_expanded(G: torch.Tensor) -> torch.Tensor:
    return G if G.ndim == 0 else G[:1].contiguous().expand(G.shape)


def _grads(outs, G, leaves, how, unused=()):
    """The leaves' gradients with the upstream gradients ``G`` delivered in the form ``how``."""
    names = list(outs)
    o = [outs[k] for k in names]
    g = [G[k] for k in names]
    if how in ("reference", "expanded grad_outputs"):
        gs = g if how == "reference" else [_as_expanded(x) for x in g]
        return torch.autograd.grad(o, list(leaves.values()), grad_outputs=gs, allow_unused=True)
    if how == "(out * expanded G).sum()":
        loss = sum((a * _as_expanded(b)).sum() for a, b in zip(o, g))
    elif how == "transposed consumer":
        loss = sum((a.t() * b.t().contiguous()).sum() if a.ndim == 2 else (a.movedim(-1, 0) * b.movedim(-1, 0).contiguous()).sum() if a.ndim > 2
                   else (a * b).sum() for a, b in zip(o, g))
    elif how == "float64 consumer":
        loss = sum((a.double() * b.double()).sum() for a, b in zip(o, g))
    elif how == "unused outputs":
        loss = sum((a * b).sum() for k, a, b in zip(names, o, g) if k not in unused)
    else:
        raise ValueError(how)
    return torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)


FORMS = ("expanded grad_outputs", "(out * expanded G).sum()", "transposed consumer", "float64 consumer", "unused outputs")


def check_binding(name, make, unused=(), leaf_views=None):
    """``make(leaves or None) -> (outs, leaves)`` runs the forward on fresh leaves (or on the given ones).  One reference
    backward from explicit contiguous fp32 upstream gradients; the same gradients in every form of ``FORMS`` give the same
    bits; behind the recording proxy no backward is handed a pointer into an expanded gradient's storage; leaves that are
    non-contiguous views get gradients of their shape with the plain run's values (or the wrapper refuses them)."""
    from tests import input_contract as ic
    from tests import scratch_state as ss
    p, lines = ic.Protocol(), []
    outs, leaves = make(None)
    G = OrderedDict((k, upstream(v, 500 + i, zero=k in unused)) for i, (k, v) in enumerate(outs.items()))
    want = _grads(outs, G, leaves, "reference")
    want_out = OrderedDict((k, v.detach().clone()) for k, v in outs.items())
    if all(g is None or not bool(g.any()) for g in want):
        lines.append(f"{name}: degenerate binding: every reference gradient is zero")
    for how in FORMS:
        if how == "unused outputs" and not unused:
            continue
        if how == "expanded grad_outputs":          # phase 1 of this form first: the backward behind the proxy
            outs, leaves = make(None)
            exp = [_as_expanded(G[k]) for k in outs]
            calls, exc = p.record(lambda _t: torch.autograd.grad(list(outs.values()), list(leaves.values()), grad_outputs=exp, allow_unused=True), None)
            bad = False
            for e in exp:
                if e.ndim == 0 or e.is_contiguous():
                    continue
                lo, hi = ic._span(e)
                for entry, ptrs in calls:
                    if any(lo <= q < hi for q in ptrs):
                        lines.append(f"phase 1: {name}: {entry} was handed a pointer into an expanded upstream gradient's storage")
                        bad = True
            if bad:
                continue
        outs, leaves = make(None)
        lines += [f"{name}: forward not reproducible: {l}" for l in ss.diff_all("", OrderedDict((k, v.detach()) for k, v in outs.items()), want_out)]
        got = _grads(outs, G, leaves, how, unused)
        torch.cuda.synchronize()
        for k, a, b in zip(leaves, got, want):
            if (a is None) != (b is None):
                lines.append(f"{name}: [{how}] gradient of {k}: {'None' if a is None else 'a tensor'}, the reference backward gave {'None' if b is None else 'a tensor'}")
            elif a is not None:
                line = ss.diff(f"gradient of {k}", a, b)
                if line:
                    lines.append(f"{name}: [{how}] {line}")
    if leaf_views is not None:
        _, plain = make(None)
        view = lambda v: v.detach().t().contiguous().t() if v.ndim == 2 else \
            v.detach().contiguous(memory_format=torch.channels_last) if v.ndim == 4 else v.detach().clone()
        views = OrderedDict((k, torch.nn.Parameter(view(v))) for k, v in plain.items())
        assert any(not v.is_contiguous() for v in views.values()), f"{name}: no leaf is a matrix or a convolution weight"
        try:
            outs, leaves = make(views)
        except (TypeError, ValueError):
            return lines                # refused before anything ran: the other accepted outcome
        got = _grads(outs, G, leaves, "reference")
        torch.cuda.synchronize()
        for k, a, b in zip(leaves, got, want):
            if a is not None and b is not None:
                if a.shape != leaves[k].shape:
                    lines.append(f"{name}: non-contiguous leaf {k}: gradient of shape {tuple(a.shape)}, the leaf has {tuple(leaves[k].shape)}")
                line = ss.diff(f"gradient of non-contiguous leaf {k}", a.contiguous(), b)
                if line:
                    lines.append(f"{name}: {line}")
    return lines


def _train_binding(name, entries, precision, rays_grad, **kw):
    @binding(name, entries)
    def run(ctx):
        train = _tr()
        ws = train.TrainWorkspace()
        draws = {k: ctx.draws("A")[k][:R].contiguous() for k in train.DRAW_KEYS}

        def make(given):
            if given is None:
                given = OrderedDict((f"net{n} {i}", t.clone().requires_grad_(True)) for n in range(2) for i, t in enumerate(ctx.weights("A", n)))
                if rays_grad:
                    given["rays"] = rays8(ctx, "A").clone().requires_grad_(True)
            ws_ = list(v for k, v in given.items() if k != "rays")
            rays = given["rays"] if rays_grad else rays8(ctx, "A")
            out = train.forward_rays_train(ws_[:24], ws_[24:], rays, draws, noise_std=1.0, precision=precision, workspace=ws, **kw)
            return OrderedDict(out), given
        return check_binding(name, make, unused=("coarse_depth", "coarse_opacity"), leaf_views=True)


_train_binding("train._ForwardRaysTrain chain", {"nsr_train_forward", "nsr_train_backward", "nsr_train_status_reset"}, "f16x3", False)
_train_binding("train._ForwardRaysTrain layer by layer, rays.requires_grad", {"nsr_train_arch_forward_e", "nsr_train_arch_backward_r", "nsr_train_status_reset"},
               "fp32", True)
_train_binding("train._ForwardRaysTrain chain_ray_grad", {"nsr_train_forward", "nsr_train_backward_r", "nsr_train_status_reset"}, "f16x3", True,
               chain_ray_grad=True)


def _image_binding(name, entries, shapes, forward, unused=()):
    @binding(name, entries)
    def run(ctx):
        def make(given):
            if given is None:
                given = OrderedDict((k, img(700 + i, *sh).requires_grad_(True)) for i, (k, sh) in enumerate(shapes.items()))
            return OrderedDict(forward(given)), given
        return check_binding(name, make, unused=unused)


_image_binding("metrics._SSIMFunction", {"nsr_ssim", "nsr_ssim_backward"}, {"output": (2, 3, IH, IW), "target": (2, 3, IH, IW)},
               lambda t: tup(("ssim", "map"), _m().SSIM(kernel_size=(11, 11))(t["output"], t["target"], reduction="none", return_map=True)), unused=("map",))
_image_binding("losses._TVFunction", {"nsr_tv_loss", "nsr_tv_loss_backward"}, {"x": (IH, IW, 3)}, lambda t: {"loss": _l().TVLoss()(t["x"])})
_image_binding("losses._GradientFunction", {"nsr_gradient_loss", "nsr_gradient_loss_backward"}, {"a": (2, 3, IH, IW), "b": (2, 3, IH, IW)},
               lambda t: {"loss": _l().GradientLoss()(t["a"], t["b"])})
_image_binding("losses._LaplacianFunction", {"nsr_laplacian_loss", "nsr_laplacian_loss_backward"}, {"d": (2, IH, IW)},
               lambda t: {"loss": _l().LaplacianLoss()(t["d"])})


@binding("refine._ForwardTrain", {"nsr_refine_train_forward_p", "nsr_refine_train_backward_w"})
def _refine_binding(ctx):
    rf = _rf()
    params0, running = _train_parts(ctx)
    pristine = OrderedDict((k, v.clone()) for k, v in running.items())
    x, c = sc.rnd(132, PB, 3, PH, PW, lo=-1, hi=1), sc.rnd(134, PB, PR, 3, PH, PW, lo=-1, hi=1)

    def make(given):
        if given is None:
            given = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in params0.items())
        for k, v in running.items():
            v.copy_(pristine[k])
        return OrderedDict(y=rf.forward_train(given, running, x, c, img_chunk=1)), given
    return check_binding("refine._ForwardTrain", make, leaf_views=True)
