#!/usr/bin/env python3
"""Golden gradients of the reference's ``SSIM`` class (``models/criterions.py:190-284``) under autograd, on the ``tiny``,
``gray`` and ``box`` images of tests/golden/metrics.npz (both reflected aliases of a row at once; kh != kw and C = 1; the
uniform window).  The upstream is sum_b v_b * ssim_b over ``reduction='none'`` with a seeded, fp32-representable vector v.
Per case: ``v``, the gradients with respect to ``output`` and ``target`` of the class run on ``.double()`` inputs with its
``_kernel`` cast to double (``gx64``, ``gy64``), the class's own fp32 gradients (``gx32``, ``gy32``) and ``gap`` = the largest
distance of the two as a fraction of the fp64 gradient's largest magnitude: the reference's own fp32 error.  Development
container only; data only.

    python tests/golden/make_golden_metrics_grad.py      # rewrites tests/golden/metrics_grad.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

TAGS = ("tiny", "gray", "box")


def _options(g, tag):
    return dict(data_range=tuple(float(v) for v in g[f"range_{tag}"]), kernel_size=tuple(int(v) for v in g[f"kernel_size_{tag}"]),
                sigma=tuple(float(v) for v in g[f"sigma_{tag}"]), gaussian=bool(g[f"gaussian_{tag}"]))


def _grads(ssim, x, y, v):
    x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (ssim(x, y, reduction="none") * v.to(x.dtype)).sum().backward()
    return x.grad, y.grad


def main():
    mg.install_shim()
    from models.criterions import SSIM
    g = np.load(os.path.join(HERE, "metrics.npz"))
    gen = torch.Generator().manual_seed(23)
    out = {"tags": np.array(TAGS)}
    for tag in TAGS:
        x, y = torch.from_numpy(g[f"x_{tag}"]), torch.from_numpy(g[f"y_{tag}"])
        v = (torch.rand(x.shape[0], generator=gen) + 0.5).float()           # fp32 values: the GPU side is fed the same bits
        gx32, gy32 = _grads(SSIM(**_options(g, tag)), x, y, v)
        m64 = SSIM(**_options(g, tag))
        m64._kernel = m64._kernel.double()
        gx64, gy64 = _grads(m64, x.double(), y.double(), v)
        assert gx64.dtype == torch.float64 and gx32.dtype == torch.float32 and tuple(gx64.shape) == tuple(x.shape)
        gap = max(float((gx32.double() - gx64).abs().max() / gx64.abs().max()), float((gy32.double() - gy64).abs().max() / gy64.abs().max()))
        out[f"v_{tag}"] = mg.np32(v)
        out[f"gx64_{tag}"], out[f"gy64_{tag}"] = gx64.numpy(), gy64.numpy()
        out[f"gx32_{tag}"], out[f"gy32_{tag}"] = mg.np32(gx32), mg.np32(gy32)
        out[f"gap_{tag}"] = np.float64(gap)
        print(tag, tuple(x.shape), "v", v.numpy(), f"max |gx64| {float(gx64.abs().max()):.3e}  fp32 gap {gap:.1e}")
    path = os.path.join(HERE, "metrics_grad.npz")
    np.savez_compressed(path, **out)
    print("->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
