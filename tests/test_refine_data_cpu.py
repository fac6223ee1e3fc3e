"""CPU-side checks of the refinement patch batches (include/nsr_refine_data.h, nerf_sr_amd/refine_data.py): the numpy
restatement (tests/refine_data_ref.py) equals Pillow's own transform byte for byte and reproduces every array the reference's
dataset class wrote into tests/golden/refine_data.npz; the mapping of raw words follows the ranges the reference handed to
``np.random.randint``; the new C-ABI symbols are exported, bound and reject bad arguments before any launch."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_void_p

import numpy as np
import pytest

from nerf_sr_amd import _lib, build as nsr_build
from tests import refine_data_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "refine_data.npz")))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


def random_coeffs(rng, W, H, d=0.3):
    dw, dh = int(d * (W // 2)), int(d * (H // 2))
    ends = [[rng.integers(0, dw + 1), rng.integers(0, dh + 1)], [rng.integers(W - dw - 1, W), rng.integers(0, dh + 1)],
            [rng.integers(W - dw - 1, W), rng.integers(H - dh - 1, H)], [rng.integers(0, dw + 1), rng.integers(H - dh - 1, H)]]
    return rr.perspective_coeffs([[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]], ends)


# ------------------------------------------------------------------------------------------------ the warp rule
@pytest.mark.parametrize("W, H, n", [(40, 28, 20), (37, 23, 20), (41, 30, 15), (18, 11, 15)])
def test_restatement_is_pillows_transform_byte_for_byte(W, H, n):
    """70 random perspectives, three of the four sizes with W % 4 != 0; distortions up to 0.6 so that large parts fall outside."""
    from PIL import Image
    rng = np.random.default_rng(W * 100 + H)
    for k in range(n):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        co = random_coeffs(rng, W, H, d=(0.3, 0.6)[k % 2])
        want = np.asarray(Image.fromarray(img).transform((W, H), Image.PERSPECTIVE, [float(c) for c in co], Image.BILINEAR, fillcolor=0))
        got = rr.warp_u8(img, co)
        assert np.array_equal(got, want), f"warp {k} at {W} x {H}: {int((got != want).sum())} bytes differ"


def test_identity_row_returns_the_source():
    img = np.random.default_rng(1).integers(0, 256, (13, 19, 3), dtype=np.uint8)
    assert np.array_equal(rr.warp_u8(img, rr.IDENTITY), img)
    assert np.array_equal(rr.aug_bbox(np.maximum(img, 1), rr.IDENTITY), [0, 0, 19, 13])


# ------------------------------------------------------------------------------------------------ against the reference
def test_fixture_boxes_and_image_stacks(fx):
    i = int(fx["ref_idx"])
    gt, sr = fx["gt_u8"][i], fx["sr_u8"][i]
    assert gt.min() >= 16 and fx["coeffs"].shape == (int(fx["aug_num"]), 8) and np.array_equal(fx["coeffs"][0], rr.IDENTITY)
    for a, co in enumerate(fx["coeffs"]):
        assert np.array_equal(rr.aug_bbox(gt, co), fx["bboxs"][a]), a
        assert np.array_equal(rr.normalize(rr.warp_u8(gt, co)), fx["gt_pspc_imgs"][a]), a
        assert np.array_equal(rr.normalize(rr.warp_u8(sr, co)), fx["sr_pspc_imgs"][a]), a
    assert len({tuple(b) for b in fx["bboxs"]}) > 3          # the boxes are not all the whole image


def case_setup(fx, tag):
    m = re.fullmatch(r"(train|val)_R(\d+)_gt(\d)", tag)
    mode, R, with_gt = (rr.TRAIN if m.group(1) == "train" else rr.VAL), int(m.group(2)), bool(int(m.group(3)))
    return mode, R, with_gt


def test_fixture_samples(fx):
    P, off, W, H, ri = int(fx["patch_len"]), int(fx["ref_offset"]), int(fx["W"]), int(fx["H"]), int(fx["ref_idx"])
    n = 0
    for tag in fx["cases"]:
        mode, R, with_gt = case_setup(fx, str(tag))
        for k, a in enumerate(fx[f"{tag}_aug"]):
            if mode == rr.TRAIN:
                gt, sr, ref, co, box = fx["gt_u8"][ri], fx["sr_u8"][ri], fx["gt_u8"][ri], fx["coeffs"][a], fx["bboxs"][a]
            else:
                gt, sr, ref, co, box = fx["gt_u8"][a], fx["sr_u8"][a], fx["gt_u8"][ri], rr.IDENTITY, (0, 0, W, H)
            starts = fx[f"{tag}_starts"][k]
            assert rr.starts_valid(starts, box, P, R, off, mode, with_gt, W, H)
            s, g, r = rr.sample(gt, sr, ref, co, starts, P, R, with_gt)
            assert np.array_equal(s, fx[f"{tag}_sr_patch"][k]) and np.array_equal(g, fx[f"{tag}_gt_patch"][k])
            assert np.array_equal(r, fx[f"{tag}_ref_patches"][k])
            n += 1
    assert n >= 12


def test_draw_ranges_are_the_references(fx):
    """The ranges the restatement maps words onto are the (low, high) pairs the reference gave np.random.randint, and the
    mapping is lo + word % (hi - lo): both ends are reached, nothing outside is."""
    P, off, W, H = int(fx["patch_len"]), int(fx["ref_offset"]), int(fx["W"]), int(fx["H"])
    rng = np.random.default_rng(2)
    for tag in fx["cases"]:
        mode, R, with_gt = case_setup(fx, str(tag))
        for k, a in enumerate(fx[f"{tag}_aug"]):
            box = fx["bboxs"][a] if mode == rr.TRAIN else (0, 0, W, H)
            starts, recorded = fx[f"{tag}_starts"][k], fx[f"{tag}_ranges"][k]
            mine = rr.all_ranges(box, int(starts[0]), int(starts[1]), P, R, off, mode, with_gt)
            for j, rg in enumerate(mine):
                assert (tuple(recorded[j]) == (-1, -1)) if rg is None else (tuple(recorded[j]) == rg), (tag, k, j)
            # words that reproduce the recorded positions, shifted by random multiples of the range lengths
            words = [0 if rg is None else int(starts[j]) - rg[0] + (rg[1] - rg[0]) * int(rng.integers(0, 1000)) for j, rg in enumerate(mine)]
            got = rr.positions_from_draws(words, box, P, R, off, mode, with_gt)
            assert np.array_equal(got, starts)
    box = (3, 0, 38, 27)
    xs = {int(rr.positions_from_draws([w] + [0] * 18, box, 8, 8, 8, rr.TRAIN, True)[0]) for w in range(100)}
    assert xs == set(range(3, 30))
    assert rr.positions_from_draws([-1] + [0] * 18, box, 8, 8, 8, rr.TRAIN, True) is None
    assert rr.positions_from_draws([0] * 19, (0, 0, 40, 28), 8, 8, 8, rr.VAL, False) is None      # x = 0: the reference's empty range
    assert rr.positions_from_draws([1, 1] + [0] * 17, (0, 0, 40, 28), 8, 8, 8, rr.VAL, False) is not None


def test_package_coefficients_follow_the_law():
    """draw_coeffs: row 0 the identity, every other row takes its four end points to the image corners; offsets within
    int(d * (W // 2)) x int(d * (H // 2)); the package's solver is the restatement's."""
    import torch
    from nerf_sr_amd import refine_data as rd
    W, H, d = 40, 28, 0.3
    g = torch.Generator().manual_seed(4)
    c = rd.draw_coeffs(W, H, 9, d, g)
    assert c.shape == (9, 8) and c.dtype == np.float64 and tuple(c[0]) == rd.IDENTITY
    g = torch.Generator().manual_seed(4)
    seen = set()
    for row in c[1:]:
        start, end = rd.perspective_params(W, H, d, g)
        assert start == [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]]
        assert np.array_equal(row, rr.perspective_coeffs(start, end))
        for (sx, sy), (ex, ey) in zip(start, end):
            den = row[6] * ex + row[7] * ey + 1
            assert abs((row[0] * ex + row[1] * ey + row[2]) / den - sx) < 1e-9 and abs((row[3] * ex + row[4] * ey + row[5]) / den - sy) < 1e-9
            assert abs(ex - sx) <= 6 and abs(ey - sy) <= 4
            seen.add((abs(ex - sx), abs(ey - sy)))
    assert len(seen) > 8


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "nsr_refine_data.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(nsr_[a-z_0-9]+)\s*\(", text)))
    assert names == ["nsr_refine_aug_bbox", "nsr_refine_patch_batch", "nsr_refine_warp_image"]
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert ("nsr_refine_data.hip", ["-ffp-contract=off"]) in nsr_build.UNITS


def test_struct_layout_matches_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    fields = [f[0] for f in _lib.NsrRefinePatchset._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nsr.h"\n#include "nsr_refine_data.h"\nint main(void) {\n'
                   '  printf("%lu", (unsigned long)sizeof(struct nsr_refine_patchset));\n'
                   + "".join(f'  printf(" %lu", (unsigned long)offsetof(struct nsr_refine_patchset, {f}));\n' for f in fields)
                   + '  printf(" %d %d %d", NSR_PATCHES_TRAIN, NSR_PATCHES_VAL, NSR_REFINE_MAX_REF_PATCHES);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.NsrRefinePatchset)
    assert got[1:-3] == [getattr(_lib.NsrRefinePatchset, f).offset for f in fields]
    assert got[-3:] == [_lib.NSR_PATCHES_TRAIN, _lib.NSR_PATCHES_VAL, _lib.NSR_REFINE_MAX_REF_PATCHES]


def _desc(**kw):
    d = dict(gt=256, sr=256, ref=256, coeffs=256, bboxs=256, n_img=1, n_aug=6, H=28, W=40, patch_len=8, num_ref_patches=8,
             ref_offset=8, with_gt_patch=0, mode=0)
    d.update(kw)
    return _lib.NsrRefinePatchset(**d)


def test_arguments_are_checked_before_any_launch(lib):
    null, one, odd = c_void_p(0), c_void_p(256), c_void_p(258)

    def call(d, B=4, aug=one, starts=one, draws=null, sr=one, gt=one, ref=one, so=one, status=null):
        return lib.nsr_refine_patch_batch(ctypes.byref(d), aug, starts, draws, B, sr, gt, ref, so, status, null)

    assert lib.nsr_refine_patch_batch(None, one, one, null, 4, one, one, one, one, null, null) == -1
    for bad in (dict(gt=0), dict(sr=0), dict(ref=0), dict(coeffs=0), dict(bboxs=0), dict(coeffs=260), dict(bboxs=258), dict(n_img=2),
                dict(n_img=0), dict(n_aug=0), dict(H=0), dict(W=-1), dict(patch_len=0), dict(patch_len=29), dict(num_ref_patches=0),
                dict(num_ref_patches=65), dict(ref_offset=0), dict(mode=2), dict(mode=1, with_gt_patch=1)):
        assert call(_desc(**bad)) == -1, bad
    assert call(_desc(), B=-1) == -1 and call(_desc(), aug=null) == -1
    assert call(_desc(), starts=null) == -1 and call(_desc(), draws=one) == -1                # exactly one of starts / draws
    assert call(_desc(), starts=null, draws=one, so=null) == -1                               # draws need starts_out
    assert call(_desc(), sr=null) == -1 and call(_desc(), gt=null) == -1 and call(_desc(), ref=null) == -1
    assert call(_desc(), starts=odd) == -1 and call(_desc(), status=odd) == -1                # misaligned words
    # empty batch: fine whatever the pointers; 'val' needs no tables
    assert call(_desc(), B=0, aug=null, starts=null, sr=null, gt=null, ref=null, so=null) == 0
    assert call(_desc(mode=1, coeffs=0, bboxs=0, n_img=3), B=0) == 0
    # the two setup / inspection entry points
    assert lib.nsr_refine_aug_bbox(ctypes.byref(_desc()), null, null) == -1
    assert lib.nsr_refine_aug_bbox(None, one, null) == -1 and lib.nsr_refine_aug_bbox(ctypes.byref(_desc(mode=1)), one, null) == -1
    assert lib.nsr_refine_aug_bbox(ctypes.byref(_desc(coeffs=0)), one, null) == -1
    assert lib.nsr_refine_warp_image(ctypes.byref(_desc()), 6, 0, one, null) == -1            # row outside the table
    assert lib.nsr_refine_warp_image(ctypes.byref(_desc()), 0, 2, one, null) == -1
    assert lib.nsr_refine_warp_image(ctypes.byref(_desc()), 0, 0, null, null) == -1
    assert lib.nsr_refine_warp_image(ctypes.byref(_desc(mode=1)), 0, 0, one, null) == -1


def test_header_is_pedantic_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "hdr.c"
    src.write_text('#include "nsr.h"\n#include "nsr_refine_data.h"\n'
                   'int main(void) { struct nsr_refine_patchset d; d.mode = NSR_PATCHES_VAL; d.num_ref_patches = NSR_REFINE_MAX_REF_PATCHES;\n'
                   '  return (d.mode == 1 && d.num_ref_patches == 64 && nsr_refine_patch_batch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == NSR_ERR_INVALID_ARG\n'
                   '          && nsr_refine_aug_bbox(0, 0, 0) == NSR_ERR_INVALID_ARG && nsr_refine_warp_image(0, 0, 0, 0, 0) == NSR_ERR_INVALID_ARG) ? 0 : 1; }\n')
    libdir = os.path.join(REPO, "nerf_sr_amd")
    exe = tmp_path / "hdr"
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libnsr.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_options_are_checked_before_a_device_is_touched():
    from nerf_sr_amd import refine_data as rd
    img = np.zeros((28, 40, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="split"):
        rd.RefinePatchSet(img, img, split="test")
    with pytest.raises(ValueError, match="num_ref_patches"):
        rd.RefinePatchSet(img, img, num_ref_patches=0)
    with pytest.raises(ValueError, match="with_gt_patch"):
        rd.RefinePatchSet(img, img, split="val", with_gt_patch=True)
    with pytest.raises(ValueError, match="no CPU path"):
        rd.RefinePatchSet(img, img, patch_len=8, device="cpu")
