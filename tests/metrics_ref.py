"""Plain-torch restatement of the reference's two evaluation metrics (models/criterions.py:190-284 ``SSIM``, :27-36
``PSNR``): reflect pad, five-way cat, depthwise ``F.conv2d`` with the fp32 outer-product window, the elementwise SSIM map.
It runs in whatever dtype / device its tensors have: in fp64 on the CPU it is the reference of tests/test_gpu_metrics.py
(tests/golden/metrics.npz pins it to the reference's own classes: tests/test_metrics_cpu.py), in fp32 on the GPU it is the
torch baseline of scripts/time_metrics.py."""
import torch
import torch.nn.functional as F


def _window_1d(size, sigma, gaussian):
    half = (size - 1) * 0.5
    t = torch.linspace(-half, half, steps=size)
    if gaussian:
        g = torch.exp(-0.5 * (t / sigma).pow(2))
        return g / g.sum()
    return torch.where((t >= -2.5) & (t <= 2.5), torch.tensor(1 / 5.0), torch.tensor(0.0))      # 1 / 5 inside [-2.5, 2.5]


def window(kernel_size=(11, 11), sigma=(1.5, 1.5), gaussian=True):
    """(kh, kw) fp32: the outer product of the two fp32 1-D windows, rounded as the reference rounds it."""
    return torch.matmul(_window_1d(kernel_size[0], sigma[0], gaussian).unsqueeze(1),
                        _window_1d(kernel_size[1], sigma[1], gaussian).unsqueeze(0))


def ssim_map(output, target, data_range=(0, 1), kernel_size=(11, 11), sigma=(1.5, 1.5), k1=0.01, k2=0.03, gaussian=True):
    """The (B, C, H, W) map of (a1 a2) / (b1 b2) in the dtype of ``output``; the fp32 window table is cast to it."""
    scale = data_range[1] - data_range[0]
    c1, c2 = (k1 * scale) ** 2, (k2 * scale) ** 2
    pad_h, pad_w = (kernel_size[0] - 1) // 2, (kernel_size[1] - 1) // 2
    B, C = output.shape[:2]
    kernel = window(kernel_size, sigma, gaussian).to(device=output.device, dtype=output.dtype).expand(C, 1, -1, -1)
    output = F.pad(output, [pad_w, pad_w, pad_h, pad_h], mode="reflect")
    target = F.pad(target, [pad_w, pad_w, pad_h, pad_h], mode="reflect")
    outs = F.conv2d(torch.cat([output, target, output * output, target * target, output * target]), kernel, groups=C)
    mu_x, mu_y, e_xx, e_yy, e_xy = (outs[i * B:(i + 1) * B] for i in range(5))
    mu_xx, mu_yy, mu_xy = mu_x.pow(2), mu_y.pow(2), mu_x * mu_y
    s_xx, s_yy, s_xy = e_xx - mu_xx, e_yy - mu_yy, e_xy - mu_xy
    a1, a2 = 2 * mu_xy + c1, 2 * s_xy + c2
    b1, b2 = mu_xx + mu_yy + c1, s_xx + s_yy + c2
    return (a1 * a2) / (b1 * b2)


def ssim(output, target, reduction="none", **kw):
    """Per-image SSIM (B,), or its mean / sum."""
    v = torch.mean(ssim_map(output, target, **kw), (1, 2, 3))
    return v if reduction == "none" else (v.mean() if reduction == "mean" else v.sum())


def psnr(inputs, targets, valid_mask=None):
    value = (inputs - targets) ** 2
    if valid_mask is not None:
        value = value[valid_mask]
    return -10 * torch.log10(torch.mean(value))


# ---- tests/golden/metrics.npz (tests/golden/make_golden_metrics.py)
PSNR_KINDS = ("none", "row", "elem", "empty")


def ssim_options(g, tag):
    """The SSIM options of fixture case ``tag`` as keyword arguments."""
    return dict(data_range=tuple(float(v) for v in g[f"range_{tag}"]), kernel_size=tuple(int(v) for v in g[f"kernel_size_{tag}"]),
                sigma=tuple(float(v) for v in g[f"sigma_{tag}"]), gaussian=bool(g[f"gaussian_{tag}"]))
