"""CPU-side checks of the evaluation metrics (include/nsr_metrics.h, nerf_sr_amd/metrics.py):

* tests/metrics_ref.py -- the plain-torch restatement the GPU tests and scripts/time_metrics.py use -- is pinned to the
  fixture the reference's own ``SSIM`` / ``PSNR`` classes produced (tests/golden/metrics.npz): in fp64 within 1e-12 of the
  class run in fp64 (values and map), in fp32 within 1e-6 of the class's fp32 values;
* ``metrics.SSIM`` / ``metrics.PSNR`` raise the reference's exception types for bad options and bad arguments before any
  device is touched;
* ``nsr_ssim`` / ``nsr_psnr`` reject bad arguments before any launch;
* the new header is pedantic C99 next to the five existing ones.
"""
import os
import shutil
import subprocess
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib, build as nsr_build
from . import metrics_ref as ref
from .metrics_ref import PSNR_KINDS, ssim_options

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


def test_fixture_has_the_cases(g):
    assert list(g["ssim_tags"]) == ["tiny", "ragged", "gray", "box", "flat"] and list(g["psnr_tags"]) == ["big", "small"]
    assert g["x_tiny"].shape == (2, 3, 6, 7) and g["x_ragged"].shape == (2, 3, 45, 70) and g["x_gray"].shape == (1, 1, 19, 33)
    assert g["x_box"].shape == (1, 3, 24, 24) and g["x_flat"].shape == (1, 3, 32, 32)
    assert g["psnr_a_big"].shape == (4096, 3) and g["psnr_a_small"].shape == (5, 3)
    for tag in g["ssim_tags"]:
        assert g[f"map64_{tag}"].dtype == np.float64 and g[f"map64_{tag}"].shape == g[f"x_{tag}"].shape
        assert float(g[f"gap_{tag}"]) == float(np.abs(g[f"ref32_{tag}"].astype(np.float64) - g[f"ref64_{tag}"]).max())
    # the flat frame is where the reference's fp32 E[x^2] - mu^2 loses digits
    assert float(g["gap_flat"]) > 1e-5 > float(g["gap_tiny"])


@pytest.mark.parametrize("tag", ["tiny", "ragged", "gray", "box", "flat"])
def test_restatement_matches_the_reference_classes(g, tag):
    kw = ssim_options(g, tag)
    x, y = torch.from_numpy(g[f"x_{tag}"]), torch.from_numpy(g[f"y_{tag}"])
    m64 = ref.ssim_map(x.double(), y.double(), **kw)
    assert float((m64 - torch.from_numpy(g[f"map64_{tag}"])).abs().max()) <= 1e-12
    assert float((ref.ssim(x.double(), y.double(), **kw) - torch.from_numpy(g[f"ref64_{tag}"])).abs().max()) <= 1e-12
    v32 = ref.ssim(x, y, **kw)
    assert v32.dtype == torch.float32
    assert float((v32 - torch.from_numpy(g[f"ref32_{tag}"])).abs().max()) <= 1e-6


@pytest.mark.parametrize("tag", ["big", "small"])
def test_psnr_restatement_matches_the_reference_class(g, tag):
    a, b = torch.from_numpy(g[f"psnr_a_{tag}"]), torch.from_numpy(g[f"psnr_b_{tag}"])
    for kind in PSNR_KINDS:
        m = None if kind == "none" else torch.from_numpy(g[f"psnr_mask_{kind}_{tag}"])
        want64, want32 = float(g[f"psnr_ref64_{kind}_{tag}"]), float(g[f"psnr_ref32_{kind}_{tag}"])
        got64, got32 = float(ref.psnr(a.double(), b.double(), m)), float(ref.psnr(a, b, m))
        if kind == "empty":
            assert np.isnan(want64) and np.isnan(got64) and np.isnan(got32)
        else:
            assert abs(got64 - want64) <= 1e-12 and abs(got32 - want32) <= 1e-6
    assert bool(g[f"psnr_mask_row_{tag}"].any()) and not bool(g[f"psnr_mask_row_{tag}"].all())


def test_window_table_is_the_reference_table():
    """metrics.window_table and the restatement's window are the same fp32 outer product; the uniform table has zero rows."""
    from nerf_sr_amd import metrics
    for ks, sg, ga in (((11, 11), (1.5, 1.5), True), ((7, 11), (1.0, 2.0), True), ((11, 11), (1.5, 1.5), False), ((3, 5), (0.5, 3.0), False)):
        w = metrics.window_table(ks, sg, ga)
        assert w.dtype == torch.float32 and tuple(w.shape) == ks and torch.equal(w, ref.window(ks, sg, ga))
    box = metrics.window_table((11, 11), (1.5, 1.5), False)
    assert float(box[0].abs().max()) == 0.0 and float(box[5, 5]) == float(np.float32(0.2) * np.float32(0.2))


def test_ssim_argument_checks_raise_the_reference_types_without_a_gpu():
    from nerf_sr_amd.metrics import PSNR, SSIM
    for bad in ({"kernel_size": (10, 11)}, {"kernel_size": (11, 0)}, {"kernel_size": (-3, 3)}, {"sigma": (0.0, 1.5)}, {"sigma": (1.5, -1.0)}):
        with pytest.raises(ValueError):
            SSIM(**bad)
    s = SSIM()
    assert s.c1 == (0.01 * 1) ** 2 and s.c2 == (0.03 * 1) ** 2 and (s.pad_h, s.pad_w) == (5, 5)
    assert SSIM(data_range=(-1, 1)).c2 == (0.03 * 2) ** 2
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(TypeError):
        s(x, x.double())
    with pytest.raises(ValueError):
        s(x, torch.zeros(1, 3, 16, 17))
    with pytest.raises(ValueError):
        s(x[0], x[0])                                    # rank
    with pytest.raises(ValueError):
        s(x, x, reduction="median")
    with pytest.raises(ValueError):
        s(x, x, layout="CHWB")
    with pytest.raises(ValueError):
        s(torch.zeros(1, 3, 5, 16), torch.zeros(1, 3, 5, 16))      # pad_h = 5 >= H: torch's reflect condition
    with pytest.raises(ValueError):
        s(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, 3))    # W = 3 in BCHW ...
    with pytest.raises(ValueError, match="no CPU path"):
        s(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, 3), layout="BHWC")     # ... a valid frame in BHWC: only the device is missing
    with pytest.raises(ValueError, match="no CPU path"):
        s(x, x)
    p = PSNR()
    with pytest.raises(TypeError):
        p(x, x.double())
    with pytest.raises(ValueError):
        p(x, torch.zeros(1, 3, 16, 17))
    with pytest.raises(ValueError):
        p(x, x, valid_mask=torch.ones(2, 3, dtype=torch.bool))
    with pytest.raises(TypeError):
        p(x, x, valid_mask=torch.ones(1, 3, 16, 16))


def test_metric_entry_points_validate_before_any_launch(lib):
    null, one = c_void_p(0), c_void_p(256)
    big = 1 << 30
    ok = lambda **kw: {**dict(o=one, t=one, B=1, C=3, H=16, W=16, layout=0, w=one, kh=11, kw=11, out=one, ws=one, wsb=big), **kw}
    call = lambda a: lib.nsr_ssim(a["o"], a["t"], a["B"], a["C"], a["H"], a["W"], a["layout"], a["w"], a["kh"], a["kw"], 1e-4, 9e-4,
                                  a["out"], null, a["ws"], a["wsb"], null)
    for bad in (dict(o=null), dict(t=null), dict(w=null), dict(out=null), dict(ws=null),        # null pointers
                dict(kh=10), dict(kw=4), dict(kh=0), dict(kw=-3),                                # even / non-positive windows
                dict(H=5), dict(W=5), dict(H=1, kh=3),                                           # pad >= H or W
                dict(B=-1), dict(C=0), dict(C=-3), dict(H=-16), dict(W=0), dict(layout=2)):      # sizes, layout
        assert call(ok(**bad)) == -1, bad
    assert call(ok(wsb=0)) == -4                                    # workspace too small
    assert call(ok(kh=61, kw=61, H=64, W=64)) == -2                 # the staged tiles of a 61 x 61 window exceed the LDS
    assert call(ok(B=0, o=null, t=null)) == 0                       # empty batch: no-op
    assert lib.nsr_ssim_workspace_bytes(2, 3, 45, 70) == 2 * 3 * 2 * 3 * 8 and lib.nsr_ssim_workspace_bytes(1, 3, 32, 32) == 3 * 8
    assert lib.nsr_ssim_workspace_bytes(0, 3, 8, 8) == 0 and lib.nsr_ssim_workspace_bytes(1, 3, -8, 8) == 0
    # PSNR
    assert lib.nsr_psnr(null, one, 1, 12, null, 1, one, one, one, big, null) == -1
    assert lib.nsr_psnr(one, null, 1, 12, null, 1, one, one, one, big, null) == -1
    assert lib.nsr_psnr(one, one, 1, 12, null, 1, null, null, one, big, null) == -1       # nowhere to write
    assert lib.nsr_psnr(one, one, 1, 12, null, 1, one, one, null, big, null) == -1
    assert lib.nsr_psnr(one, one, -1, 12, null, 1, one, one, one, big, null) == -1
    assert lib.nsr_psnr(one, one, 1, -12, null, 1, one, one, one, big, null) == -1
    assert lib.nsr_psnr(one, one, 1, 12, one, 0, one, one, one, big, null) == -1          # mask_group
    assert lib.nsr_psnr(one, one, 1, 13, one, 3, one, one, one, big, null) == -1          # n % mask_group
    assert lib.nsr_psnr(one, one, 1, 12, null, 1, one, one, one, 8, null) == -4
    assert lib.nsr_psnr(one, one, 0, 12, null, 1, one, one, one, 0, null) == 0
    assert lib.nsr_psnr_workspace_bytes(4, 4096 * 3) == 4 * 3 * 16 and lib.nsr_psnr_workspace_bytes(1, 0) == 16
    assert lib.nsr_psnr_workspace_bytes(0, 8) == 0 and lib.nsr_psnr_workspace_bytes(1, -1) == 0


def test_metrics_header_is_plain_c99_with_the_others(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc not available: the C99 check of include/nsr_metrics.h cannot run")
    headers = ("nsr.h", "nsr_train.h", "nsr_warp.h", "nsr_refine.h", "nsr_image.h", "nsr_metrics.h")
    src = tmp_path / "metrics_abi.c"
    src.write_text("".join(f'#include "{h}"\n' for h in headers)
                   + "int main(void) {\n"
                     "  return nsr_ssim(0, 0, 1, 3, 16, 16, NSR_LAYOUT_BHWC, 0, 11, 11, 1e-4, 9e-4, 0, 0, 0, 0, 0) == NSR_ERR_INVALID_ARG\n"
                     "      && nsr_psnr_workspace_bytes(1, 4096) == 2 * sizeof(double) ? 0 : 1;\n}\n")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c", str(src),
                           "-o", str(tmp_path / "metrics_abi.o")])
