"""The four image-space regularisers of include/nsr_losses.h restated in plain torch ops, differentiable by autograd, in the
dtype of their inputs (fp64 inputs: the oracle of the device kernels; fp32 inputs: the chain of torch ops the kernels replace).
tests/test_losses_cpu.py ties them to the reference's own classes through tests/golden/losses.npz."""
import torch


def tv(x):
    """x (H, W, C): mean squared difference of vertical neighbours plus that of horizontal neighbours."""
    dh = x[1:] - x[:-1]
    dw = x[:, 1:] - x[:, :-1]
    return (dh * dh).sum() / dh.numel() + (dw * dw).sum() / dw.numel()


def _forward_differences(x):
    """(dx, dy) of x (B, C, H, W): the difference to the right / lower neighbour, zero in the last column / row."""
    dx, dy = torch.zeros_like(x), torch.zeros_like(x)
    dx[..., :, :-1] = x[..., :, 1:] - x[..., :, :-1]
    dy[..., :-1, :] = x[..., 1:, :] - x[..., :-1, :]
    return dx, dy


def gradient(a, b):
    """a, b (B, C, H, W) or (C, H, W): L1 distance of the forward differences, averaged over all elements and the two axes."""
    if a.ndim == 3:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    ax, ay = _forward_differences(a)
    bx, by = _forward_differences(b)
    return ((ax - bx).abs().mean() + (ay - by).abs().mean()) / 2


def _second_differences(x):
    """The four second differences of x (N, H, W, ...) along columns, rows, the main diagonal and the anti-diagonal."""
    c = x[:, 1:-1, 1:-1]
    return (x[:, :, :-2] + x[:, :, 2:] - 2 * x[:, :, 1:-1],
            x[:, :-2, :] + x[:, 2:, :] - 2 * x[:, 1:-1, :],
            x[:, :-2, :-2] + x[:, 2:, 2:] - 2 * c,
            x[:, 2:, :-2] + x[:, :-2, 2:] - 2 * c)


def laplacian(d, guide=None, gamma=0.1):
    """d (N, H, W): the mean absolute second difference along each of four directions, averaged over the four; with
    ``guide`` (N, H, W, C) each second difference is first weighted by exp(-sum_c |second difference of guide| / gamma)."""
    terms = _second_differences(d)
    if guide is not None:
        terms = [torch.exp(-g.abs().sum(-1) / gamma) * t for g, t in zip(_second_differences(guide), terms)]
    total = terms[0].abs().mean()
    for t in terms[1:]:
        total = total + t.abs().mean()
    return total / 4
