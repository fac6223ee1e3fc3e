"""Evaluation metrics on the device over ``include/nsr_metrics.h``: ``SSIM`` and ``PSNR``.

``SSIM`` mirrors ``models/criterions.py:190-284`` (same constructor, same argument checks and exception types, same window
table) and ``PSNR`` ``:27-36`` (``value[valid_mask]`` with an element mask or a row mask).  Both run as one kernel plus a
fixed-order reduction with every product and sum in double, so the values agree with the reference evaluated in fp64 and
a frame gives the same bits whatever batch it is part of.  ``SSIM`` is differentiable as the reference's is: with an input
that requires grad it back-propagates through ``nsr_ssim_backward``.  All arithmetic runs in libnsr.so; there is no CPU path.

Inputs ("Inputs"): images are float32 on the current device -- another dtype raises ``TypeError``, nothing is
converted (so "the inputs' dtype" of a result is float32) --, in any memory form (a view is read through a dense copy); a mask
is bool or uint8.  Results are fresh tensors.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .ops import _check_device, _f32, _p, _stream

LAYOUTS = {"BCHW": _lib.NSR_LAYOUT_BCHW, "BHWC": _lib.NSR_LAYOUT_BHWC}
REDUCTIONS = ("mean", "sum", "none")

_WS: Dict[torch.device, torch.Tensor] = {}     # partial sums of the two-stage reductions, one per device (grows, never shrinks)


def _workspace(need: int, dev) -> torch.Tensor:
    ws = _WS.get(dev)
    if ws is None or ws.numel() < need:
        _WS[dev] = ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=dev)
    return ws


def _window_1d(size: int, sigma: float, gaussian: bool) -> torch.Tensor:
    """One axis of the window, fp32, by the reference's torch ops (criterions.py:208-224): taps at linspace(-h, h) with
    h = (size - 1) / 2; a normalised Gaussian, or 1 / 5 on the taps inside [-2.5, 2.5] and 0 outside (for sizes above 5 the
    uniform table therefore has zero rows and columns and does not sum to 1)."""
    half = (size - 1) * 0.5
    t = torch.linspace(-half, half, steps=size)
    if gaussian:
        g = torch.exp(-0.5 * (t / sigma).pow(2))
        return g / g.sum()
    return torch.where((t >= -2.5) & (t <= 2.5), torch.tensor(1 / 5.0), torch.tensor(0.0))


def window_table(kernel_size=(11, 11), sigma=(1.5, 1.5), gaussian: bool = True) -> torch.Tensor:
    """The reference's ``_kernel`` (kh, kw): the fp32 outer product of the two 1-D windows, built with the same torch ops
    on the host (criterions.py:226-234), so the table the kernel reads is the reference's table, rounding included."""
    rows = _window_1d(kernel_size[0], sigma[0], gaussian)
    cols = _window_1d(kernel_size[1], sigma[1], gaussian)
    return torch.matmul(rows.unsqueeze(1), cols.unsqueeze(0)).contiguous()


class SSIM:
    """``SSIM(data_range, kernel_size, sigma, k1, k2, gaussian)(output, target, reduction)`` of the reference, on the GPU.

    ``layout='BHWC'`` reads (B, H, W, C) frames (the NeRF side's images) without a permute; ``return_map=True`` also returns
    the (B, C, H, W) fp32 map the means are taken over.  Returns a tensor of the inputs' dtype (float32: any other raises
    ``TypeError``): the per-image values for
    ``reduction='none'``, their mean or sum otherwise.

    As the reference's chain of torch ops does, the result back-propagates: when ``output`` or ``target`` requires grad, the
    values (and the map) carry a ``grad_fn`` whose backward is ``nsr_ssim_backward`` (double arithmetic, fp32 gradients in the
    inputs' layout, only those autograd asks for; not differentiable twice), so ``1 - ssim(pred, gt)`` is a loss.  The forward
    values are the same bits with and without grad."""

    def __init__(self, data_range=(0, 1), kernel_size=(11, 11), sigma=(1.5, 1.5), k1=0.01, k2=0.03, gaussian=True):
        self.kernel_size = tuple(kernel_size)
        self.sigma = tuple(sigma)
        self.gaussian = gaussian
        if len(self.kernel_size) != 2 or len(self.sigma) != 2:
            raise ValueError(f"SSIM: kernel_size and sigma take two entries each, got {kernel_size} and {sigma}")
        if any(x % 2 == 0 or x <= 0 for x in self.kernel_size):
            raise ValueError(f"SSIM: both window sizes must be odd and positive, got kernel_size={kernel_size}")
        if any(y <= 0 for y in self.sigma):
            raise ValueError(f"SSIM: both sigmas must be positive, got sigma={sigma}")
        data_scale = data_range[1] - data_range[0]
        self.c1 = (k1 * data_scale) ** 2
        self.c2 = (k2 * data_scale) ** 2
        self.pad_h = (self.kernel_size[0] - 1) // 2
        self.pad_w = (self.kernel_size[1] - 1) // 2
        self._kernel = window_table(self.kernel_size, self.sigma, gaussian)       # host, fp32
        self._dev_kernel: Dict[torch.device, torch.Tensor] = {}

    def _window(self, dev) -> torch.Tensor:
        w = self._dev_kernel.get(dev)
        if w is None:
            self._dev_kernel[dev] = w = self._kernel.to(dev)
        return w

    def __call__(self, output: torch.Tensor, target: torch.Tensor, reduction: str = "mean", layout: str = "BCHW",
                 return_map: bool = False):
        # every option is checked before a device is touched
        if output.dtype != target.dtype:
            raise TypeError(f"SSIM: output is {output.dtype} but target is {target.dtype}: the two must have one dtype")
        if output.shape != target.shape:
            raise ValueError(f"SSIM: output {tuple(output.shape)} and target {tuple(target.shape)} differ in shape")
        if len(output.shape) != 4:
            raise ValueError(f"SSIM: images must be 4-D ({layout}), got {tuple(output.shape)}")
        if reduction not in REDUCTIONS:
            raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be 'BCHW' or 'BHWC', got {layout!r}")
        B, C, H, W = output.shape if layout == "BCHW" else (output.shape[0], output.shape[3], output.shape[1], output.shape[2])
        if C == 0 or self.pad_h >= H or self.pad_w >= W:
            raise ValueError(f"SSIM: a {H} x {W} image with {C} channels is not larger than the reflect padding "
                             f"({self.pad_h}, {self.pad_w}) of the window")
        output, target = _f32(output, "output"), _f32(target, "target")
        if torch.is_grad_enabled() and (output.requires_grad or target.requires_grad):
            # the same launches under a torch.autograd.Function whose backward is nsr_ssim_backward; mean / sum stay torch ops
            outs = _SSIMFunction.apply(self, (B, C, H, W), layout, return_map, output, target)
            _ssim, smap = outs if return_map else (outs, None)
        else:
            _ssim, smap = self._forward(output, target, (B, C, H, W), layout, return_map)
        res = _ssim if reduction == "none" else (_ssim.mean() if reduction == "mean" else _ssim.sum())
        return (res, smap) if return_map else res

    def _forward(self, output, target, dims, layout, return_map):
        """The per-image values (B,) in the inputs' dtype and the map (or None): nsr_ssim."""
        B, C, H, W = dims
        dev = output.device
        lib = _lib.load()
        vals = torch.empty(B, dtype=torch.float64, device=dev)
        smap = torch.empty(B, C, H, W, dtype=torch.float32, device=dev) if return_map else None
        if B > 0:
            need = lib.nsr_ssim_workspace_bytes(B, C, H, W)
            ws = _workspace(need, dev)
            _lib.check(lib.nsr_ssim(_p(output), _p(target), B, C, H, W, LAYOUTS[layout], _p(self._window(dev)), self.kernel_size[0],
                                    self.kernel_size[1], self.c1, self.c2, _p(vals), _p(smap), _p(ws), ws.numel(), _stream()),
                       "nsr_ssim")
        return vals.to(output.dtype), smap

    def _backward(self, output, target, dims, layout, g_ssim, g_map, want_output, want_target):
        """(grad_output, grad_target) in the inputs' memory order, None where not wanted: nsr_ssim_backward."""
        B, C, H, W = dims
        grads = [torch.empty_like(output) if want_output else None, torch.empty_like(target) if want_target else None]
        if g_ssim is None and g_map is None:
            return [None if g is None else g.zero_() for g in grads]
        if B > 0:
            g_ssim = None if g_ssim is None else g_ssim.to(torch.float32).contiguous()
            g_map = None if g_map is None else g_map.to(torch.float32).contiguous()
            dev = output.device
            _lib.check(_lib.load().nsr_ssim_backward(_p(output), _p(target), B, C, H, W, LAYOUTS[layout], _p(self._window(dev)),
                                                     self.kernel_size[0], self.kernel_size[1], self.c1, self.c2, _p(g_ssim), _p(g_map),
                                                     _p(grads[0]), _p(grads[1]), _stream()), "nsr_ssim_backward")
        return grads


class _SSIMFunction(torch.autograd.Function):
    """Outputs: the per-image values (B,), and the map (B, C, H, W) with ``return_map``.  Saves the two images only: the
    backward recomputes the window sums.  Not differentiable twice."""

    @staticmethod
    def forward(ctx, ssim, dims, layout, return_map, output, target):
        vals, smap = ssim._forward(output, target, dims, layout, return_map)
        ctx.save_for_backward(output, target)
        ctx.ssim, ctx.dims, ctx.layout = ssim, dims, layout
        ctx.set_materialize_grads(False)           # an output nothing was computed from arrives as None: a null pointer
        return (vals, smap) if return_map else vals

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ssim, g_map=None):
        output, target = ctx.saved_tensors
        grads = ctx.ssim._backward(output, target, ctx.dims, ctx.layout, g_ssim, g_map, ctx.needs_input_grad[4], ctx.needs_input_grad[5])
        return (None, None, None, None) + tuple(grads)


def _mask_bytes(valid_mask: Optional[torch.Tensor], shape, lead: int) -> Tuple[Optional[torch.Tensor], int]:
    """``value[valid_mask]`` as (uint8 flags, elements per flag): the mask covers the leading dimensions of ``shape`` that
    follow the first ``lead`` (segment) ones -- all of them: an element mask; all but the last: a row mask."""
    if valid_mask is None:
        return None, 1
    if valid_mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"valid_mask must be a bool (or uint8) tensor, got {valid_mask.dtype}")
    if valid_mask.ndim < lead or tuple(valid_mask.shape) != tuple(shape[:valid_mask.ndim]):
        raise ValueError(f"valid_mask of shape {tuple(valid_mask.shape)} does not index values of shape {tuple(shape)}")
    group = 1
    for d in shape[valid_mask.ndim:]:
        group *= int(d)
    if not valid_mask.is_cuda:
        raise ValueError("valid_mask must live on the GPU (nerf_sr_amd has no CPU path)")
    _check_device(valid_mask.device, "valid_mask")
    m = valid_mask.contiguous()
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), group


def mse_psnr(inputs: torch.Tensor, targets: torch.Tensor, valid_mask: Optional[torch.Tensor] = None, per_image: bool = False):
    """(mse, psnr) as float64 device tensors through ``nsr_psnr``: 0-d over everything, or (B,) over each ``inputs[i]`` with
    ``per_image``.  No host synchronisation."""
    if inputs.dtype != targets.dtype:
        raise TypeError(f"PSNR: inputs are {inputs.dtype} but targets are {targets.dtype}")
    if inputs.shape != targets.shape:
        raise ValueError(f"PSNR: inputs {tuple(inputs.shape)} and targets {tuple(targets.shape)} differ in shape")
    if per_image and inputs.ndim < 1:
        raise ValueError("psnr_per_image needs a leading image dimension")
    lead = 1 if per_image else 0
    mask, group = _mask_bytes(valid_mask, tuple(inputs.shape), lead)
    a, b = _f32(inputs, "inputs"), _f32(targets, "targets")
    n_seg = int(a.shape[0]) if per_image else 1
    n = a.numel() // n_seg if n_seg > 0 else 0
    lib = _lib.load()
    out = torch.empty(2, n_seg, dtype=torch.float64, device=a.device)
    if n_seg > 0:
        if n == 0:
            group = 1
        need = lib.nsr_psnr_workspace_bytes(n_seg, n)
        ws = _workspace(need, a.device)
        _lib.check(lib.nsr_psnr(_p(a), _p(b), n_seg, n, _p(mask), group, _p(out[0]), _p(out[1]), _p(ws), ws.numel(), _stream()), "nsr_psnr")
    return (out[0], out[1]) if per_image else (out[0, 0], out[1, 0])


class PSNR:
    """``PSNR(opt)(inputs, targets, valid_mask=None)`` of the reference: -10 log10 of the mean squared difference over the
    selected elements, a 0-d tensor of the inputs' dtype (NaN for an empty selection)."""

    def __init__(self, opt=None):
        self.opt = opt

    def __call__(self, inputs: torch.Tensor, targets: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        return mse_psnr(inputs, targets, valid_mask)[1].to(inputs.dtype)

    forward = __call__


def psnr_per_image(inputs: torch.Tensor, targets: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The batched form: one PSNR per ``inputs[i]`` -> (B,), in one launch; each value is what ``PSNR()`` gives for that image
    alone, bit for bit."""
    return mse_psnr(inputs, targets, valid_mask, per_image=True)[1].to(inputs.dtype)
