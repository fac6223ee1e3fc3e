"""CPU-side checks of the ray-batch feature (include/nsr_data.h, nerf_sr_amd/data.py): the numpy restatement of the
index / window / patch / layout rules (tests/dataset_ref.py) reproduces every array the reference's own dataset classes
wrote into tests/golden/dataset.npz; the new C-ABI symbols are exported, bound and reject bad arguments before any launch."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_float, c_void_p

import numpy as np
import pytest

from nerf_sr_amd import _lib, build as nsr_build, io as nsr_io
from tests import dataset_ref as dr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_TOL = 2e-6       # the bound of test_subpixel_rays_vs_golden (oracle vs reference rays)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "dataset.npz")))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        nsr_build.build(verbose=False)
    return _lib.load()


def llff_views(fx, include_val=False):
    val = int(fx["llff_val_idx"])
    return [i for i in range(len(fx["llff_poses"])) if include_val or i != val]


def llff_set(fx, s=2, include_val=False, spheric=False, **kw):
    views = llff_views(fx, include_val)
    near, far = (float(fx["llff_bounds"].min()), float(min(8 * fx["llff_bounds"].min(), fx["llff_bounds"].max()))) if spheric else (0.0, 1.0)
    return dr.RefSet([fx["llff_poses"][i] for i in views], [fx[f"llff_px_{i}"] for i in views], 16, 12, s, float(fx["llff_focal"]),
                     not spheric, near, far, **kw)


def check_set(ref, fx, prefix, targets_prefix=None):
    t = targets_prefix or prefix
    assert ref.rays.shape == fx[f"{prefix}_rays"].shape
    assert np.abs(ref.rays - fx[f"{prefix}_rays"]).max() <= RAY_TOL
    assert np.array_equal(ref.rgbs, fx[f"{t}_rgbs"])
    assert np.array_equal(ref.rgbs_ori, fx[f"{t}_rgbs_ori"])


@pytest.mark.parametrize("prefix, kw", [
    ("llff_s2", {}), ("llff_s4", {"s": 4}), ("llff_unified", {"unified_dir": True}), ("llff_nocentre", {"use_pixel_centers": False}),
    ("llff_spheric", {"spheric": True}), ("llff_avgvar", {"ds_method": "avg", "include_val": True})])
def test_llff_train_buffers(fx, prefix, kw):
    own_targets = prefix in ("llff_s2", "llff_s4", "llff_avgvar")     # the direction options leave the targets alone (stored once)
    check_set(llff_set(fx, **kw), fx, prefix, None if own_targets else "llff_s2")


def test_llff_patches(fx):
    ref = llff_set(fx)
    for k in range(3):
        i_img, row, col = (int(v) for v in fx[f"llff_patch{k}_loc"])
        _, rays, rgbs = ref.patch(i_img, row, col, 2)
        assert rays.shape == fx[f"llff_patch{k}_rays"].shape == (4, 4, 8)
        assert np.abs(rays - fx[f"llff_patch{k}_rays"]).max() <= RAY_TOL
        assert np.array_equal(rgbs, fx[f"llff_patch{k}_rgbs"])


def test_llff_validation_sample(fx):
    val = int(fx["llff_val_idx"])
    got = dr.validation_sample(fx["llff_poses"][val], fx[f"llff_px_{val}"], 16, 12, 2, float(fx["llff_focal"]), True, 0.0, 1.0)
    for k in ("rays", "rays_ori", "c2w"):
        assert np.abs(got[k] - fx[f"llff_val_{k}"]).max() <= RAY_TOL, k
    assert np.array_equal(got["rgbs"], fx["llff_val_rgbs"]) and np.array_equal(got["rgbs_ori"], fx["llff_val_rgbs_ori"])


def blender_set(fx, window=None):
    return dr.RefSet(list(fx["blender_poses"]), [fx[f"blender_train_px_{i}"] for i in range(3)], 16, 16, 2, float(fx["blender_focal"]),
                     False, 2.0, 6.0, window=window)


def test_blender_train_and_crop(fx):
    check_set(blender_set(fx), fx, "blender_train")
    win = dr.crop_window(16, 16, 2, 0.5)
    assert win == (2, 2, 4, 4)
    check_set(blender_set(fx, win), fx, "blender_crop")
    with pytest.raises(ValueError):
        dr.crop_window(20, 20, 4, 0.5)      # HR crop 10 +- 5, LR crop 2 +- 1 = HR 8 +- 4


def test_blender_validation_sample(fx):
    import json
    meta = json.loads(bytes(fx["blender_val_json"]).decode())
    pose = np.array(meta["frames"][0]["transform_matrix"])[:3, :4]
    got = dr.validation_sample(pose, fx["blender_val_px_0"], 16, 16, 2, float(fx["blender_focal"]), False, 2.0, 6.0)
    for k in ("rays", "rays_ori", "c2w"):
        assert np.abs(got[k] - fx[f"blender_val_{k}"]).max() <= RAY_TOL, k
    for k in ("rgbs", "rgbs_ori", "valid_mask", "valid_mask_ori"):
        assert np.array_equal(got[k], fx[f"blender_val_{k}"]), k
    assert 0 < got["valid_mask"].sum() < got["valid_mask"].size


def test_test_path_mirrors(fx):
    assert np.abs(nsr_io.spiral_path(fx["path_radii"], float(fx["path_focus"]), 8) - fx["path_spiral"]).max() <= 1e-12
    assert np.abs(nsr_io.spheric_path(float(fx["path_radius"]), 8) - fx["path_spheric"]).max() <= 1e-12
    assert fx["path_spiral"].shape == fx["path_spheric"].shape == (8, 3, 4)


def test_crop_rule_matches_the_package():
    from nerf_sr_amd import data
    for (W, H, s, frac) in ((16, 16, 2, 0.5), (800, 800, 2, 0.5), (800, 800, 4, 0.5), (400, 400, 2, 0.3), (20, 20, 4, 0.5), (18, 18, 2, 0.5)):
        try:
            want = dr.crop_window(W, H, s, frac)
        except ValueError:
            with pytest.raises(ValueError):
                data.crop_window((W, H), s, frac)
        else:
            assert data.crop_window((W, H), s, frac) == want


# ------------------------------------------------------------------------------------------------ C ABI


def test_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "nsr_data.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(nsr_[a-z_0-9]+)\s*\(", text)))
    assert names == ["nsr_gen_rays_opt", "nsr_rayset_batch"]
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.nsr_version() == 131


def test_struct_layout_matches_the_header(tmp_path):
    """ctypes' NsrRayset and the C struct agree on size and on the offset of every field."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    fields = [f[0] for f in _lib.NsrRayset._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nsr.h"\n#include "nsr_data.h"\nint main(void) {\n'
                   '  printf("%lu", (unsigned long)sizeof(struct nsr_rayset));\n'
                   + "".join(f'  printf(" %lu", (unsigned long)offsetof(struct nsr_rayset, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.NsrRayset)
    assert got[1:] == [getattr(_lib.NsrRayset, f).offset for f in fields]


def _desc(**kw):
    d = dict(poses=256, n_views=2, H=12, W=16, s=2, focal=33.6, ndc=1, near_=0.0, far_=1.0, options=0, x0=0, y0=0, w=8, h=6,
             hr=256, lr=256, C=3, lr_mode=0, patch_w=0)
    d.update(kw)
    return _lib.NsrRayset(**d)


def test_batch_arguments_are_checked_before_any_launch(lib):
    null, one, odd = c_void_p(0), c_void_p(256), c_void_p(260)
    call = lambda d, B=4, layout=0, idx=one, rays=one: lib.nsr_rayset_batch(ctypes.byref(d), idx, B, layout, rays, one, one, null, null)
    assert lib.nsr_rayset_batch(None, one, 4, 0, one, one, one, null, null) == -1
    assert call(_desc(poses=0)) == -1 and call(_desc(hr=0)) == -1 and call(_desc(), idx=null) == -1
    assert call(_desc(H=13)) == -1 and call(_desc(W=15)) == -1                       # H % s, W % s
    assert call(_desc(x0=1)) == -1 and call(_desc(y0=-1)) == -1 and call(_desc(h=7)) == -1 and call(_desc(w=0)) == -1    # window
    assert call(_desc(C=2)) == -1 and call(_desc(C=5)) == -1
    assert call(_desc(lr=0)) == -1 and call(_desc(lr_mode=2)) == -1
    assert call(_desc(), rays=odd) == -1                                              # misaligned rays
    assert call(_desc(), B=-1) == -1
    assert call(_desc(options=4)) == -1 and call(_desc(focal=0.0)) == -1 and call(_desc(n_views=0)) == -1
    assert call(_desc(options=2, focal=1.5)) == -1                                    # unified direction: focal // s == 0
    assert call(_desc(), layout=2) == -1 and call(_desc(patch_w=3), layout=1) == -1 and call(_desc(), layout=1) == -1
    # empty batch: fine, null outputs allowed; a NULL lr is fine when the targets are pooled from the HR images
    assert lib.nsr_rayset_batch(ctypes.byref(_desc()), null, 0, 0, null, null, null, null, null) == 0
    assert lib.nsr_rayset_batch(ctypes.byref(_desc(lr=0, lr_mode=1)), null, 0, 0, null, null, null, null, null) == 0


def test_gen_rays_opt_arguments(lib):
    null, one = c_void_p(0), c_void_p(256)
    c2w = (c_float * 12)()
    assert lib.nsr_gen_rays_opt(c2w, 8, 8, 10.0, 2, 0, 2.0, 6.0, 0, 3, 17, one, null) == -1      # 16 LR pixels only
    assert lib.nsr_gen_rays_opt(c2w, 8, 8, 10.0, 2, 0, 2.0, 6.0, 4, 0, 16, one, null) == -1      # unknown option bit
    assert lib.nsr_gen_rays_opt(c2w, 8, 8, 10.0, 3, 0, 2.0, 6.0, 1, 0, 4, one, null) == -1       # H % s
    assert lib.nsr_gen_rays_opt(None, 8, 8, 10.0, 2, 0, 2.0, 6.0, 1, 0, 4, one, null) == -1
    assert lib.nsr_gen_rays_opt(c2w, 8, 8, 10.0, 2, 0, 2.0, 6.0, 3, 0, 4, c_void_p(260), null) == -1
    assert lib.nsr_gen_rays_opt(c2w, 8, 8, 10.0, 2, 0, 2.0, 6.0, 3, 5, 5, null, null) == 0        # empty shard


def test_data_header_is_pedantic_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "hdr.c"
    src.write_text('#include "nsr.h"\n#include "nsr_data.h"\n'
                   'int main(void) { struct nsr_rayset d; d.options = NSR_RAYS_NO_PIXEL_CENTERS | NSR_RAYS_UNIFIED_DIR; d.lr_mode = NSR_LR_MEAN_OF_HR;\n'
                   '  return (d.options == 3u && d.lr_mode == 1 && nsr_rayset_batch(0, 0, 0, 0, 0, 0, 0, 0, 0) == NSR_ERR_INVALID_ARG\n'
                   '          && nsr_gen_rays_opt(0, 8, 8, 10.0, 2, 0, 2.0f, 6.0f, 0u, 0, 4, 0, 0) == NSR_ERR_INVALID_ARG) ? 0 : 1; }\n')
    libdir = os.path.join(REPO, "nerf_sr_amd")
    exe = tmp_path / "hdr"
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libnsr.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0
