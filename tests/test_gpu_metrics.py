"""Evaluation metrics on the device (include/nsr_metrics.h, nerf_sr_amd/metrics.py) against the fixture produced by the
reference's own ``SSIM`` / ``PSNR`` classes (tests/golden/metrics.npz) and against tests/metrics_ref.py in fp64.

Bounds.  SSIM per image: |ssim - ref64| <= max(1e-6, 2 |ref32 - ref64|) -- the project's bound for scalar losses, or twice the
reference's own fp32-vs-fp64 distance; the map within 2.4e-7 of the fp64 map (two fp32 spacings at 1: the arithmetic is
double, only the store rounds).  PSNR within two fp32 spacings of the fp64 value (the sum is double, only the final fp32 store
rounds).  Bit-equality where the fixed-order reduction promises it."""
import os

import numpy as np
import pytest
import torch

from nerf_sr_amd.refine import make_refine_state_dict
from nerf_sr_amd.weights import make_state_dict
from . import metrics_ref as ref
from .metrics_ref import PSNR_KINDS, ssim_options

pytestmark = pytest.mark.gpu
SSIM_TAGS = ["tiny", "ragged", "gray", "box", "flat"]
MAP_TOL = 2.4e-7


@pytest.fixture(scope="module")
def g(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return np.load(os.path.join(golden_dir, "metrics.npz"))


def psnr_tol(value):
    return 2.0 * float(np.spacing(np.float32(value)))


def bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("tag", SSIM_TAGS)
def test_ssim_vs_reference_fixture(g, tag):
    from nerf_sr_amd.metrics import SSIM
    x, y = torch.from_numpy(g[f"x_{tag}"]).cuda(), torch.from_numpy(g[f"y_{tag}"]).cuda()
    got, smap = SSIM(**ssim_options(g, tag))(x, y, reduction="none", return_map=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0],) and tuple(smap.shape) == tuple(x.shape)
    ref64, ref32 = g[f"ref64_{tag}"], g[f"ref32_{tag}"].astype(np.float64)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref64)
    bound = np.maximum(1e-6, 2.0 * np.abs(ref32 - ref64))
    map_err = float(np.abs(smap.cpu().numpy().astype(np.float64) - g[f"map64_{tag}"]).max())
    print(f"{tag}: |ssim - ref64| {err}, bound {bound}, reference's own fp32 gap {float(g[f'gap_{tag}']):.1e}, map err {map_err:.2e}")
    assert (err <= bound).all(), (tag, err, bound)
    assert map_err <= MAP_TOL, (tag, map_err)


def test_ssim_invariances(g):
    from nerf_sr_amd.metrics import SSIM
    s = SSIM()
    x, y = torch.from_numpy(g["x_ragged"]).cuda(), torch.from_numpy(g["y_ragged"]).cuda()
    assert float((s(x, x, reduction="none") - 1.0).abs().max()) <= 1e-6
    none, smap = s(x, y, reduction="none", return_map=True)
    # (B, H, W, C) frames read in place give the bits of the permuted tensor
    hwc, hwc_map = s(x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous(), reduction="none", layout="BHWC", return_map=True)
    assert bits(hwc) == bits(none) and bits(hwc_map) == bits(smap)
    # fixed-order reduction: an image gives the same bits alone, at B = 3 in any slot, and on a second call
    alone = s(x[:1], y[:1], reduction="none")
    assert bits(alone) == bits(none[:1]) == bits(s(x[:1], y[:1], reduction="none"))
    fx, fy = torch.flip(x[1:], dims=(3,)), torch.flip(y[1:], dims=(2,))
    for slot in range(3):
        order = [1, 2]
        order.insert(slot, 0)
        bx, by = torch.cat([x, fx])[order].contiguous(), torch.cat([y, fy])[order].contiguous()
        assert bits(s(bx, by, reduction="none")[slot:slot + 1]) == bits(alone), slot
    # 'mean' / 'sum' are the mean / sum of 'none'
    assert bits(s(x, y)) == bits(none.mean()) == bits(s(x, y, reduction="mean")) and bits(s(x, y, reduction="sum")) == bits(none.sum())


@pytest.mark.parametrize("tag", ["big", "small"])
def test_psnr_vs_reference_fixture(g, tag):
    from nerf_sr_amd.metrics import PSNR, mse_psnr, psnr_per_image
    a, b = torch.from_numpy(g[f"psnr_a_{tag}"]).cuda(), torch.from_numpy(g[f"psnr_b_{tag}"]).cuda()
    p = PSNR()
    for kind in PSNR_KINDS:
        m = None if kind == "none" else torch.from_numpy(g[f"psnr_mask_{kind}_{tag}"]).cuda()
        got = p(a, b, m)
        assert got.dtype == torch.float32 and got.ndim == 0 and got.is_cuda
        want = float(g[f"psnr_ref64_{kind}_{tag}"])
        if kind == "empty":
            assert np.isnan(want) and bool(torch.isnan(got))
            continue
        print(f"psnr {tag}/{kind}: {float(got):.7f} vs {want:.9f} (tolerance {psnr_tol(want):.1e})")
        assert abs(float(got) - want) <= psnr_tol(want), (kind, float(got), want)
        mse, _ = mse_psnr(a, b, m)
        assert abs(float(mse) - 10.0 ** (-want / 10.0)) <= 1e-12
    # per-segment results do not depend on the number of segments: each image of a batch gives the bits it gives alone
    a4 = torch.stack([a, b, torch.flip(a, dims=(0,)), a * 0.5])
    b4 = torch.stack([b, a * 0.5, a, b])
    rows = torch.from_numpy(g[f"psnr_mask_row_{tag}"]).cuda()
    m4 = torch.stack([rows, ~rows, rows, torch.zeros_like(rows)])
    both = psnr_per_image(a4, b4)
    masked = psnr_per_image(a4, b4, m4)
    assert tuple(both.shape) == (4,) and bool(torch.isnan(masked[3])) and not bool(torch.isnan(masked[:3]).any())
    for i in range(4):
        assert bits(both[i]) == bits(p(a4[i], b4[i])) == bits(psnr_per_image(a4[i:i + 1], b4[i:i + 1])[0]), i
        if i < 3:
            assert bits(masked[i]) == bits(p(a4[i], b4[i], m4[i])), i
    assert abs(float(both[0]) - float(g[f"psnr_ref64_none_{tag}"])) <= psnr_tol(float(both[0]))


# ------------------------------------------------------------------------------------------------------ model layer
W_HR, H_HR, S = 16, 12, 2


@pytest.fixture(scope="module")
def frames(g):
    """Three validation dicts of a 16 x 12 <- 8 x 6 frame: rays of three poses, random ``rgbs`` (LR) and ``rgbs_ori`` (HR, ray
    order), and a model with synthetic weights."""
    from nerf_sr_amd import cameras, ops
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    opt = default_options(img_wh=(W_HR, H_HR), downscale=S, white_bkgd=False)
    model = NeRFDownXModel(opt, device="cuda:0").load_networks(make_state_dict(11), make_state_dict(12)).eval()
    gen = torch.Generator().manual_seed(21)
    n_lr = (W_HR // S) * (H_HR // S)
    dicts = []
    for t in (0.1, 0.5, 0.9):
        rays = ops.subpixel_rays(cameras.spiral_pose(t), opt.img_wh, cameras.llff_focal(W_HR), S, True, 0.0, 1.0, "cuda:0")
        dicts.append({"rays": rays, "rgbs": torch.rand(n_lr, 3, generator=gen), "rgbs_ori": torch.rand(n_lr * S * S, 3, generator=gen)})
    return model, dicts


def expected_scores(model, d):
    """metrics_ref in fp64 on the model's own out_* tensors (after calculate_losses)."""
    f64 = lambda t: t.detach().cpu().double()
    rgbs, ori = f64(d["rgbs"]), f64(d["rgbs_ori"])
    want = {"loss_coarse_psnr": ref.psnr(f64(model.out_coarse_comp_rgbs), rgbs), "loss_fine_psnr": ref.psnr(f64(model.out_fine_comp_rgbs), rgbs),
            "loss_coarse_psnr_ori": ref.psnr(f64(model.out_coarse_comp_rgbs_ori), ori),
            "loss_fine_psnr_ori": ref.psnr(f64(model.out_fine_comp_rgbs_ori), ori)}
    chw = lambda t, h, w: f64(t).reshape(1, h, w, 3).permute(0, 3, 1, 2)
    h1, w1 = H_HR // S, W_HR // S
    want["loss_fine_ssim"] = ref.ssim(chw(model.out_fine_comp_rgbs, h1, w1), chw(d["rgbs"], h1, w1))[0]
    unflat = lambda t: model.unflatten_reshape(t.cuda().float().contiguous())
    want["loss_fine_ssim_ori"] = ref.ssim(chw(unflat(model.out_fine_comp_rgbs_ori), H_HR, W_HR), chw(unflat(d["rgbs_ori"]), H_HR, W_HR))[0]
    want["mse_coarse"] = torch.mean((f64(model.out_coarse_comp_rgbs) - rgbs) ** 2)
    want["mse_fine"] = torch.mean((f64(model.out_fine_comp_rgbs) - rgbs) ** 2)
    return {k: float(v) for k, v in want.items()}


def test_model_calculate_losses_and_validate(frames):
    model, dicts = frames
    per_image = []
    for d in dicts:
        model.set_input(d)
        model.forward()
        model.calculate_losses()
        assert model.calculate_ssim()
        want = expected_scores(model, d)
        for k in ("loss_coarse_psnr", "loss_fine_psnr", "loss_coarse_psnr_ori", "loss_fine_psnr_ori"):
            v = getattr(model, k)
            assert isinstance(v, torch.Tensor) and v.is_cuda and v.ndim == 0 and v.dtype == torch.float32
            assert abs(float(v) - want[k]) <= psnr_tol(want[k]), (k, float(v), want[k])
        for k in ("loss_fine_ssim", "loss_fine_ssim_ori"):
            assert abs(float(getattr(model, k)) - want[k]) <= 1e-6, (k, float(getattr(model, k)), want[k])
        assert abs(float(model.loss_coarse_mse) - want["mse_coarse"]) <= 1e-6 and abs(float(model.loss_fine_mse) - want["mse_fine"]) <= 1e-6
        assert abs(float(model.loss_tot) - (want["mse_coarse"] + want["mse_fine"])) <= 1e-6
        per_image.append(want)
    res = model.validate(dicts)
    assert sorted(res) == sorted(k for k in per_image[0] if k.startswith("loss_"))
    for k, v in res.items():
        mean = float(np.mean([w[k] for w in per_image]))
        tol = 1e-6 if "ssim" in k else max(psnr_tol(w[k]) for w in per_image)
        assert isinstance(v, float) and getattr(model, k) == v and abs(v - mean) <= tol, (k, v, mean)
    # lambda_*_mse are read from the options
    model.opt.lambda_coarse_mse, model.opt.lambda_fine_mse = 2.0, 0.5
    try:
        model.set_input(dicts[0])
        model.forward()
        model.calculate_losses()
        w = per_image[0]
        assert abs(float(model.loss_tot) - (2.0 * w["mse_coarse"] + 0.5 * w["mse_fine"])) <= 1e-6
    finally:
        del model.opt.lambda_coarse_mse, model.opt.lambda_fine_mse


def test_refine_evaluate_image():
    """tile -> network -> stitch -> scores on one 64 x 64-tile pair of frames: the four numbers are those of metrics_ref on
    refine_image's own output."""
    from nerf_sr_amd import refine as r
    net = r.MaxPoolingModel(precision="f16x3").load_state_dict(make_refine_state_dict(7)).eval()
    rng = np.random.default_rng(4)
    W, H, P, NR = 64, 64, 64, 4
    sr = (rng.random((3, H, W)) * 2 - 1).astype(np.float32)
    refimg = (rng.random((3, H, W)) * 2 - 1).astype(np.float32)
    gt = np.clip(sr + 0.1 * rng.standard_normal((3, H, W)), -1, 1).astype(np.float32)
    locs = np.stack([rng.integers(-20, W + 20, (H, W)), rng.integers(-20, H + 20, (H, W)), -np.ones((H, W))], -1).astype(np.float64)
    args = (net, torch.from_numpy(sr).cuda(), torch.from_numpy(refimg).cuda(), torch.from_numpy(locs).cuda())
    res = r.evaluate_image(*args, torch.from_numpy(gt).cuda(), P, NR, batch=4)
    refined = r.refine_image(*args, P, NR, batch=4)
    assert bits(res["refined"]) == bits(refined) and tuple(refined.shape) == (3, H, W)
    f64 = lambda t: (torch.from_numpy(t) if isinstance(t, np.ndarray) else t.cpu()).double().unsqueeze(0)
    for name, img in (("input", sr), ("refine", refined)):
        want_psnr = float(ref.psnr(f64(img), f64(gt)))
        want_ssim = float(ref.ssim(f64(img), f64(gt), data_range=(-1, 1))[0])
        got_psnr, got_ssim = res[f"psnr_{name}"], res[f"ssim_{name}"]
        assert got_psnr.ndim == 0 and got_ssim.ndim == 0 and got_psnr.is_cuda and got_ssim.is_cuda
        assert abs(float(got_psnr) - want_psnr) <= psnr_tol(want_psnr), (name, float(got_psnr), want_psnr)
        assert abs(float(got_ssim) - want_ssim) <= 1e-6, (name, float(got_ssim), want_ssim)
