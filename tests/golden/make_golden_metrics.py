#!/usr/bin/env python3
"""Golden vectors of the reference's evaluation metrics (``models/criterions.py``: ``SSIM``, ``PSNR``) on the smallest
shapes at which a tiled SSIM kernel can go wrong.  Per SSIM case: the two images, the class's own fp32 result
(``ref32``, ``reduction='none'``), the result of the same class on ``.double()`` inputs with its ``_kernel`` cast to double
(``ref64``), the fp64 map its mean is taken over (``map64``) and ``gap`` = max |ref32 - ref64|, the reference's own fp32
error.  Per PSNR case: the class's fp32 and fp64 values.  Image values are 8-bit levels (k / 255, as decoded frames are),
which also keeps the compressed file small.  Development container only; data only.

    python tests/golden/make_golden_metrics.py      # rewrites tests/golden/metrics.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

# tag -> ((B, C, H, W), data_range, SSIM options)
SSIM_CASES = {
    "tiny": ((2, 3, 6, 7), (-1, 1), {}),                 # H = pad + 1: every row is halo, reflection at both edges of one tile
    "ragged": ((2, 3, 45, 70), (0, 1), {}),              # several tiles, ragged in both directions, B > 1
    "gray": ((1, 1, 19, 33), (0, 1), {"kernel_size": (7, 11), "sigma": (1.0, 2.0)}),    # C = 1, kh != kw
    "box": ((1, 3, 24, 24), (0, 1), {"gaussian": False}),                               # uniform window: zero rows in the table
    "flat": ((1, 3, 32, 32), (0, 1), {}),                # constant background: the E[x^2] - mu^2 cancellation
}
PSNR_SIZES = {"big": (4096, 3), "small": (5, 3)}


def _levels(x, lo, hi):
    """Round to the 256 levels of an 8-bit frame scaled to [lo, hi]; fp32."""
    k = torch.round((x.clamp(lo, hi) - lo) / (hi - lo) * 255.0)
    return (k / 255.0 * (hi - lo) + lo).float()


def _images(tag, shape, rng, gen):
    B, C, H, W = shape
    lo, hi = rng
    if tag == "flat":
        x = torch.full(shape, 0.7)
        x[..., 8:20, 10:22] = 0.2
        return x.float(), (x + 0.01 * torch.randn(shape, generator=gen)).float()
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    phase = torch.rand(B, C, 1, 1, generator=gen) * 6.28
    base = 0.5 + 0.25 * torch.sin(0.37 * xx + phase) * torch.cos(0.23 * yy - phase) + 0.15 * torch.randn(shape, generator=gen)
    other = base + 0.08 * torch.randn(shape, generator=gen)
    scale = lambda t: t * (hi - lo) + lo
    return _levels(scale(base), lo, hi), _levels(scale(other), lo, hi)


def main():
    mg.install_shim()
    torch.set_grad_enabled(False)
    from models.criterions import PSNR, SSIM
    gen = torch.Generator().manual_seed(11)
    out = {"ssim_tags": np.array(list(SSIM_CASES)), "psnr_tags": np.array(list(PSNR_SIZES))}
    for tag, (shape, rng, kw) in SSIM_CASES.items():
        x, y = _images(tag, shape, rng, gen)
        ref32 = SSIM(data_range=rng, **kw)(x, y, reduction="none")
        m64 = SSIM(data_range=rng, **kw)
        m64._kernel = m64._kernel.double()
        seen, mean = {}, torch.mean

        def spy(t, *a, **k):            # the class keeps its map to itself: look at what it hands to torch.mean
            seen["map"] = t.clone()
            return mean(t, *a, **k)
        torch.mean = spy
        try:
            ref64 = m64(x.double(), y.double(), reduction="none")
        finally:
            torch.mean = mean
        assert ref64.dtype == torch.float64 and seen["map"].dtype == torch.float64 and tuple(seen["map"].shape) == shape
        gap = float((ref32.double() - ref64).abs().max())
        out[f"x_{tag}"], out[f"y_{tag}"] = mg.np32(x), mg.np32(y)
        out[f"ref32_{tag}"], out[f"ref64_{tag}"] = mg.np32(ref32), ref64.numpy()
        out[f"map64_{tag}"], out[f"gap_{tag}"] = seen["map"].numpy(), np.float64(gap)
        out[f"range_{tag}"] = np.array(rng, dtype=np.float64)
        out[f"kernel_size_{tag}"] = np.array(kw.get("kernel_size", (11, 11)))
        out[f"sigma_{tag}"] = np.array(kw.get("sigma", (1.5, 1.5)), dtype=np.float64)
        out[f"gaussian_{tag}"] = np.bool_(kw.get("gaussian", True))
        print(tag, shape, "ssim", ref64.numpy(), f"fp32 gap {gap:.1e}")
    psnr = PSNR(None)
    for tag, (N, C) in PSNR_SIZES.items():
        a = _levels(torch.rand(N, C, generator=gen), 0, 1)
        b = _levels(a + 0.05 * torch.randn(N, C, generator=gen), 0, 1)
        masks = {"none": None, "row": torch.rand(N, generator=gen) < 0.6, "elem": torch.rand(N, C, generator=gen) < 0.4,
                 "empty": torch.zeros(N, dtype=torch.bool)}
        for kind in ("row", "elem"):          # both values occur, whatever the draw
            masks[kind][0], masks[kind][1] = True, False
        out[f"psnr_a_{tag}"], out[f"psnr_b_{tag}"] = mg.np32(a), mg.np32(b)
        for kind, m in masks.items():
            if m is not None:
                out[f"psnr_mask_{kind}_{tag}"] = m.numpy()
            r32, r64 = psnr(a, b, m), psnr(a.double(), b.double(), m)
            out[f"psnr_ref32_{kind}_{tag}"], out[f"psnr_ref64_{kind}_{tag}"] = mg.np32(r32), r64.numpy()
            print("psnr", tag, kind, float(r64))
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print("->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
