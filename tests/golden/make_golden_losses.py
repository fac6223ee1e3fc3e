#!/usr/bin/env python3
"""Golden vectors of the reference's image-space regularisers (``models/criterions.py``: ``TVLoss`` :56-69, ``GradientLoss``
:71-101, ``LaplacianLoss`` :103-115, ``BilateralLaplacianLoss`` :118-137) on the smallest shapes at which a tiled stencil
kernel can go wrong.  Per case: the fp32 inputs, the class's loss on ``.double()`` inputs (``loss64``), the class's own fp32
loss (``loss32``, informational: the reference's own gap) and the fp64 autograd gradients of ``0.7 * loss`` with respect to
every differentiable input.  Random inputs are ``rand * 2 - 1`` from a seeded generator; "quantised" inputs are multiples of
1 / 8, so that many differences are exactly 0 (``sign(0) = 0``).  Development container only; data only.

    python tests/golden/make_golden_losses.py      # rewrites tests/golden/losses.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

UPSTREAM = 0.7

# tag -> (shape, kind of values)
TV_CASES = {"2x2x3": ((2, 2, 3), "rand"), "3x5x1": ((3, 5, 1), "rand"), "8x8x3": ((8, 8, 3), "rand"),
            "33x35x3": ((33, 35, 3), "rand"), "const": ((4, 4, 3), "const")}
GRADIENT_CASES = {"3d": ((3, 1, 4), "rand"), "2x3x2x2": ((2, 3, 2, 2), "rand"), "1x1x1x1": ((1, 1, 1, 1), "rand"),
                  "1x3x33x34": ((1, 3, 33, 34), "rand"), "half": ((3, 3, 16, 16), "half"), "quant": ((2, 3, 8, 8), "quant")}
LAPLACIAN_CASES = {"1x3x3": ((1, 3, 3), "rand"), "2x3x5": ((2, 3, 5), "rand"), "3x4x4": ((3, 4, 4), "rand"),
                   "1x33x35": ((1, 33, 35), "rand"), "ramp": ((1, 6, 6), "ramp"), "quant": ((2, 8, 8), "quant")}
# tag -> (Laplacian case, guide channels, gamma)
BILATERAL_CASES = {"1x3x3": ("1x3x3", 3, 0.1), "2x3x5": ("2x3x5", 3, 0.1), "3x4x4": ("3x4x4", 3, 0.1), "1x33x35": ("1x33x35", 3, 0.1),
                   "ramp": ("ramp", 3, 0.1), "quant": ("quant", 3, 0.1), "3x4x4_c1": ("3x4x4", 1, 1.0),
                   "1x33x35_g1": ("1x33x35", 3, 1.0), "quant_g1": ("quant", 3, 1.0)}


def _values(shape, kind, gen):
    if kind == "const":
        return torch.full(shape, 0.3)
    if kind == "ramp":                       # integers, linear in both indices: every second difference is exactly 0
        h, w = torch.meshgrid(torch.arange(shape[-2], dtype=torch.float32), torch.arange(shape[-1], dtype=torch.float32), indexing="ij")
        return (2 * h + 3 * w - 7).expand(shape).contiguous()
    x = torch.rand(shape, generator=gen) * 2 - 1
    if kind == "quant":
        x = torch.round(x * 8) / 8
    return x.float()


def _run(module, inputs, wrt):
    """(loss64, loss32, [fp64 gradient of 0.7 * loss for each differentiable input])."""
    with torch.no_grad():
        loss32 = module(*inputs)
    dbl = [t.double().requires_grad_(i in wrt) for i, t in enumerate(inputs)]
    loss64 = module(*dbl)
    assert loss64.dtype == torch.float64 and loss32.dtype == torch.float32
    grads = torch.autograd.grad(UPSTREAM * loss64, [dbl[i] for i in wrt])
    return loss64.detach().numpy(), mg.np32(loss32), [g.numpy() for g in grads]


def main():
    mg.install_shim()
    from models.criterions import BilateralLaplacianLoss, GradientLoss, LaplacianLoss, TVLoss
    gen = torch.Generator().manual_seed(41)
    out = {"upstream": np.float64(UPSTREAM), "tv_tags": np.array(list(TV_CASES)), "gradient_tags": np.array(list(GRADIENT_CASES)),
           "laplacian_tags": np.array(list(LAPLACIAN_CASES)), "bilateral_tags": np.array(list(BILATERAL_CASES))}

    def put(prefix, loss64, loss32, **arrays):
        out[f"{prefix}_loss64"], out[f"{prefix}_loss32"] = loss64, loss32
        for k, v in arrays.items():
            out[f"{prefix}_{k}"] = v
        print(prefix, f"loss64 {float(loss64):.12g}  fp32 gap {abs(float(loss32) - float(loss64)):.1e}")

    for tag, (shape, kind) in TV_CASES.items():
        x = _values(shape, kind, gen)
        l64, l32, (gx,) = _run(TVLoss(None), [x], (0,))
        put(f"tv_{tag}", l64, l32, x=mg.np32(x), gx64=gx)

    for tag, (shape, kind) in GRADIENT_CASES.items():
        a = _values(shape, kind, gen)
        b = _values(shape, kind, gen)
        if kind == "half":                   # targets == inputs on the left half: differences of exactly 0 there
            b = b.clone()
            b[..., : shape[-1] // 2] = a[..., : shape[-1] // 2]
        l64, l32, (ga, gb) = _run(GradientLoss(None), [a, b], (0, 1))
        put(f"gradient_{tag}", l64, l32, a=mg.np32(a), b=mg.np32(b), ga64=ga, gb64=gb)

    lap_inputs = {}
    opt = types.SimpleNamespace(patch_size=8, bilateral_gamma=0.1)
    for tag, (shape, kind) in LAPLACIAN_CASES.items():
        d = lap_inputs[tag] = _values(shape, kind, gen)
        l64, l32, (gd,) = _run(LaplacianLoss(opt), [d], (0,))
        put(f"laplacian_{tag}", l64, l32, d=mg.np32(d), gd64=gd)

    for tag, (lap_tag, C, gamma) in BILATERAL_CASES.items():
        d = lap_inputs[lap_tag]
        guide = _values(tuple(d.shape) + (C,), "quant" if LAPLACIAN_CASES[lap_tag][1] == "quant" else "rand", gen)
        module = BilateralLaplacianLoss(types.SimpleNamespace(patch_size=8, bilateral_gamma=gamma))
        l64, l32, (gd,) = _run(module, [d, guide], (0,))
        put(f"bilateral_{tag}", l64, l32, d=mg.np32(d), guide=mg.np32(guide), gamma=np.float64(gamma), gd64=gd)

    path = os.path.join(HERE, "losses.npz")
    np.savez_compressed(path, **out)
    print("->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
