"""Image-space regularisers on the device over ``include/nsr_losses.h``: ``TVLoss``, ``GradientLoss``, ``LaplacianLoss`` and
``BilateralLaplacianLoss``.

The classes mirror ``models/criterions.py:56-137`` (same names, same call signatures; the constructor's ``opt`` is optional).
Each loss is one tile launch plus a fixed-order finishing launch, and its gradient one launch in gather form, with every
difference, product and sum in double: the values agree with the reference's classes evaluated on ``.double()`` inputs, and
identical calls give identical bits.  Each call returns a 0-d fp32 tensor on the inputs' device that back-propagates to every
input that requires grad (``|.|`` differentiates to ``sign`` with ``sign(0) = 0``, as ``torch.abs`` does).  All arithmetic runs
in libnsr.so; there is no CPU path.

Inputs ("Inputs"): device tensors of any floating dtype and memory form; they are CONVERTED to dense float32
(``.to(torch.float32).contiguous()``, as the reference's torch ops would promote them), never written, and the gradient comes
back in the input's dtype and shape through that conversion.  The host or another GPU raises ``ValueError``, a shape that does
not fit ``ValueError``, both before anything is enqueued.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .metrics import _workspace      # the per-device grow-only buffer of the two-stage reductions: one for metrics and losses
from .ops import _check_device, _p, _stream


def _device_tensor(t, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (nerf_sr_amd has no CPU path)")
    _check_device(t.device, name)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


def _upstream(g: torch.Tensor) -> torch.Tensor:
    """The upstream gradient as the one-element fp32 device scalar the backward kernels read."""
    return g.to(torch.float32).reshape(1).contiguous()


def _run_forward(kind: int, n_img: int, C: int, H: int, W: int, dev, call, what: str) -> torch.Tensor:
    """``call(lib, loss, workspace)`` -> status; returns the device double rounded to a 0-d fp32 tensor."""
    lib = _lib.load()
    ws = _workspace(lib.nsr_loss_workspace_bytes(kind, n_img, C, H, W), dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    _lib.check(call(lib, loss, ws), what)
    return loss[0].to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------- TV
def _tv_forward(x: torch.Tensor) -> torch.Tensor:
    H, W, C = x.shape
    return _run_forward(_lib.NSR_LOSS_TV, 1, C, H, W, x.device,
                        lambda lib, loss, ws: lib.nsr_tv_loss(_p(x), H, W, C, _p(loss), _p(ws), ws.numel(), _stream()), "nsr_tv_loss")


class _TVFunction(torch.autograd.Function):
    """Saves the image only; the backward recomputes the differences.  Not differentiable twice."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _tv_forward(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        H, W, C = x.shape
        grad = torch.empty_like(x)
        _lib.check(_lib.load().nsr_tv_loss_backward(_p(x), H, W, C, _p(_upstream(g)), _p(grad), _stream()), "nsr_tv_loss_backward")
        return grad


class TVLoss:
    """``TVLoss(opt)(inputs)`` of the reference (criterions.py:56-69): ``inputs`` (H, W, C); the mean squared difference of
    vertically adjacent pixels plus that of horizontally adjacent ones."""

    def __init__(self, opt=None):
        self.opt = opt

    def __call__(self, inputs: torch.Tensor) -> torch.Tensor:
        _device_tensor(inputs, "inputs")
        if inputs.ndim != 3:
            raise ValueError(f"TVLoss: inputs must be (H, W, C), got {tuple(inputs.shape)}")
        H, W, C = inputs.shape
        if H < 2 or W < 2 or C < 1:
            raise ValueError(f"TVLoss: an image of {H} x {W} x {C} has no adjacent pixels along one axis (the reference divides 0 by 0)")
        x = _f32c(inputs)
        if torch.is_grad_enabled() and x.requires_grad:
            return _TVFunction.apply(x)
        return _tv_forward(x)

    forward = __call__


# ---------------------------------------------------------------------------------------------------------- gradient
def _gradient_forward(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    B, C, H, W = a.shape
    return _run_forward(_lib.NSR_LOSS_GRADIENT, B, C, H, W, a.device,
                        lambda lib, loss, ws: lib.nsr_gradient_loss(_p(a), _p(b), B, C, H, W, _p(loss), _p(ws), ws.numel(), _stream()),
                        "nsr_gradient_loss")


class _GradientFunction(torch.autograd.Function):
    """Saves the two images only.  Computes the gradients autograd asks for.  Not differentiable twice."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _gradient_forward(a, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        B, C, H, W = a.shape
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if ga is None and gb is None:
            return None, None
        _lib.check(_lib.load().nsr_gradient_loss_backward(_p(a), _p(b), B, C, H, W, _p(_upstream(g)), _p(ga), _p(gb), _stream()),
                   "nsr_gradient_loss_backward")
        return ga, gb


class GradientLoss:
    """``GradientLoss(opt)(inputs, targets)`` of the reference (criterions.py:71-101): (B, C, H, W) images, or (C, H, W), which
    is read as a batch of one; the L1 distance of the forward differences along columns and along rows (zero in the last
    column / row, which still counts in the mean), averaged over the two axes.  Back-propagates to ``inputs``, ``targets``,
    or both."""

    def __init__(self, opt=None):
        self.opt = opt

    def __call__(self, inputs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        _device_tensor(inputs, "inputs")
        _device_tensor(targets, "targets")
        if inputs.ndim == 3:
            inputs = inputs.unsqueeze(0)
        if targets.ndim == 3:
            targets = targets.unsqueeze(0)
        if inputs.ndim != 4:
            raise ValueError(f"GradientLoss: images must be (B, C, H, W) or (C, H, W), got {tuple(inputs.shape)}")
        if inputs.shape != targets.shape:
            raise ValueError(f"GradientLoss: inputs {tuple(inputs.shape)} and targets {tuple(targets.shape)} differ in shape")
        if inputs.numel() == 0:
            raise ValueError(f"GradientLoss: empty images {tuple(inputs.shape)}")
        a, b = _f32c(inputs), _f32c(targets)
        if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
            return _GradientFunction.apply(a, b)
        return _gradient_forward(a, b)

    forward = __call__


# --------------------------------------------------------------------------------------------------------- Laplacian
def _laplacian_forward(d: torch.Tensor, guide: Optional[torch.Tensor], gamma: float) -> torch.Tensor:
    N, H, W = d.shape
    C = 1 if guide is None else int(guide.shape[3])
    return _run_forward(_lib.NSR_LOSS_LAPLACIAN, N, C, H, W, d.device,
                        lambda lib, loss, ws: lib.nsr_laplacian_loss(_p(d), _p(guide), N, H, W, C, gamma, _p(loss), _p(ws), ws.numel(),
                                                                     _stream()), "nsr_laplacian_loss")


class _LaplacianFunction(torch.autograd.Function):
    """Saves the map (and the guide) only.  The guide gets no gradient.  Not differentiable twice."""

    @staticmethod
    def forward(ctx, d, guide, gamma):
        if guide is None:
            ctx.save_for_backward(d)
        else:
            ctx.save_for_backward(d, guide)
        ctx.gamma = gamma
        return _laplacian_forward(d, guide, gamma)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        d = ctx.saved_tensors[0]
        guide = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
        N, H, W = d.shape
        C = 1 if guide is None else int(guide.shape[3])
        grad = torch.empty_like(d)
        _lib.check(_lib.load().nsr_laplacian_loss_backward(_p(d), _p(guide), N, H, W, C, ctx.gamma, _p(_upstream(g)), _p(grad), _stream()),
                   "nsr_laplacian_loss_backward")
        return grad, None, None


def _laplacian(name: str, inputs: torch.Tensor, weights: Optional[torch.Tensor], gamma: float) -> torch.Tensor:
    if isinstance(weights, torch.Tensor) and weights.requires_grad:
        raise ValueError(f"{name}: weights (the guide image) get no gradient; pass weights.detach()")
    _device_tensor(inputs, "inputs")
    if inputs.ndim != 3:
        raise ValueError(f"{name}: inputs must be (N, H, W), got {tuple(inputs.shape)}")
    N, H, W = inputs.shape
    if N < 1 or H < 3 or W < 3:
        raise ValueError(f"{name}: a second difference needs at least 3 x 3 pixels and one image, got {tuple(inputs.shape)}")
    guide = None
    if weights is not None:
        _device_tensor(weights, "weights")
        if weights.ndim != 4 or tuple(weights.shape[:3]) != (N, H, W) or weights.shape[3] < 1:
            raise ValueError(f"{name}: weights must be (N, H, W, C) over inputs {tuple(inputs.shape)}, got {tuple(weights.shape)}")
        if weights.device != inputs.device:
            raise ValueError(f"{name}: inputs live on {inputs.device} but weights on {weights.device}")
        if not gamma > 0:
            raise ValueError(f"{name}: gamma must be positive, got {gamma}")
        guide = _f32c(weights)
    d = _f32c(inputs)
    if torch.is_grad_enabled() and d.requires_grad:
        return _LaplacianFunction.apply(d, guide, float(gamma))
    return _laplacian_forward(d, guide, float(gamma))


class LaplacianLoss:
    """``LaplacianLoss(opt)(inputs)`` of the reference (criterions.py:103-115): ``inputs`` (N, H, W), e.g. rendered depth
    patches; the mean absolute second difference along columns, rows and the two diagonals, averaged over the four."""

    def __init__(self, opt=None):
        self.opt = opt

    def __call__(self, inputs: torch.Tensor) -> torch.Tensor:
        return _laplacian("LaplacianLoss", inputs, None, 1.0)

    forward = __call__


class BilateralLaplacianLoss:
    """``BilateralLaplacianLoss(opt)(inputs, weights)`` of the reference (criterions.py:118-137): the Laplacian loss with every
    second difference of ``inputs`` (N, H, W) weighted by ``exp(-sum_c |second difference of weights| / gamma)``; ``weights``
    (N, H, W, C) is the guide (the target image) and gets no gradient.  ``gamma``: the argument, else ``opt.bilateral_gamma``,
    else 0.1 (the reference's default)."""

    def __init__(self, opt=None, gamma: Optional[float] = None):
        self.opt = opt
        self.gamma = float(gamma if gamma is not None else getattr(opt, "bilateral_gamma", 0.1))
        if not self.gamma > 0:
            raise ValueError(f"BilateralLaplacianLoss: gamma must be positive, got {self.gamma}")

    def __call__(self, inputs: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
        if weights is None:
            raise ValueError("BilateralLaplacianLoss: weights (the guide image) are required; LaplacianLoss is the plain form")
        return _laplacian("BilateralLaplacianLoss", inputs, weights, self.gamma)

    forward = __call__
