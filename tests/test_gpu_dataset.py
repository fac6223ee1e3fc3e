"""Ray batches generated on the device (include/nsr_data.h, nerf_sr_amd/data.py) against the library's own full grids (bit
identity) and against the buffers the reference's dataset classes built (tests/golden/dataset.npz; rays within the bound of
test_subpixel_rays_vs_golden, targets equal).  Everything at the fixture's sizes: 16 x 12 / 16 x 16 frames, 3 - 5 views."""
import json
import os

import numpy as np
import pytest
import torch

from tests import colmap_writer, dataset_ref as dr

pytestmark = pytest.mark.gpu
RAY_TOL = 2e-6


@pytest.fixture(scope="module")
def fx(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return dict(np.load(os.path.join(golden_dir, "dataset.npz")))


@pytest.fixture(scope="module")
def data():
    from nerf_sr_amd import data as _data
    return _data


def train_views(fx, include_val=False):
    val = int(fx["llff_val_idx"])
    return [i for i in range(len(fx["llff_poses"])) if include_val or i != val]


def spheric_near_far(fx):
    return float(fx["llff_bounds"].min()), float(min(8 * fx["llff_bounds"].min(), fx["llff_bounds"].max()))


def llff_set(data, fx, s=2, include_val=False, spheric=False, **kw):
    views = train_views(fx, include_val)
    near, far = spheric_near_far(fx) if spheric else (0.0, 1.0)
    return data.RaySet(fx["llff_poses"][views], [fx[f"llff_px_{i}"] for i in views], (16, 12), s, not spheric, near, far,
                       focal=float(fx["llff_focal"]), **kw)


def blender_set(data, fx, **kw):
    return data.RaySet(fx["blender_poses"], [fx[f"blender_train_px_{i}"] for i in range(3)], (16, 16), 2, False, 2.0, 6.0,
                       focal=float(fx["blender_focal"]), **kw)


def all_rows(rs):
    return rs.batch(torch.arange(len(rs), device="cuda"))


def check_against(got, fx, prefix, targets=None, rows=None):
    t = targets or prefix
    sel = slice(None) if rows is None else rows
    err = np.abs(got["rays"].cpu().numpy() - fx[f"{prefix}_rays"][sel]).max()
    print(f"{prefix}: max |d ray| {err:.2e}")
    assert err <= RAY_TOL
    assert np.array_equal(got["rgbs"].cpu().numpy(), fx[f"{t}_rgbs"][sel])
    assert np.array_equal(got["rgbs_ori"].cpu().numpy(), fx[f"{t}_rgbs_ori"][sel])


# ---- 1. bit identity against the library's own full grids
@pytest.mark.parametrize("case", ["ndc", "spheric", "rgba"])
def test_batch_rows_are_the_librarys_own_grids(data, fx, case):
    from nerf_sr_amd import io as nio, ops
    if case == "rgba":
        rs, px, poses, wh = blender_set(data, fx), [fx[f"blender_train_px_{i}"] for i in range(3)], fx["blender_poses"], (16, 16)
    else:
        rs = llff_set(data, fx, spheric=case == "spheric")
        px, poses, wh = [fx[f"llff_px_{i}"] for i in train_views(fx)], fx["llff_poses"][train_views(fx)], (16, 12)
    n = len(rs) // rs.n_views
    for v in range(rs.n_views):
        got = rs.batch(torch.arange(v * n, (v + 1) * n, device="cuda"))
        assert torch.equal(got["rays"], ops.subpixel_rays(poses[v], wh, rs.focal, 2, rs.ndc, rs.near, rs.far))
        rgbs, ori = nio.lr_targets(torch.from_numpy(px[v]).cuda(), wh, 2)
        assert torch.equal(got["rgbs"], rgbs) and torch.equal(got["rgbs_ori"], ori)


# ---- 2. against the reference
@pytest.mark.parametrize("ds_method", ["lanc", "avg"])
def test_shuffled_batches_vs_reference(data, fx, ds_method):
    prefix = "llff_s2" if ds_method == "lanc" else "llff_avgvar"
    rs = llff_set(data, fx, ds_method=ds_method, include_val=ds_method == "avg")
    n = len(rs)
    assert n == fx[f"{prefix}_rays"].shape[0]
    rng = np.random.default_rng(5)
    for B in (1, 63, 64, 65, n):
        idx = rng.integers(0, n, B)
        idx[-1] = n - 1                       # the last pixel of the last view
        if B >= 63:
            idx[10] = idx[3]                  # duplicates
        got = rs.batch(torch.from_numpy(idx).cuda())
        assert got["rays"].shape == (B, 4, 8) and got["rgbs"].shape == (B, 3) and got["rgbs_ori"].shape == (B, 4, 3)
        check_against(got, fx, prefix, rows=idx)
    check_against(all_rows(rs), fx, prefix)
    assert rs.status() == 0
    only = rs._launch(torch.arange(5, device="cuda"), want=("rgbs",))        # null outputs are simply not produced
    assert list(only) == ["rgbs"] and np.array_equal(only["rgbs"].cpu().numpy(), fx[f"{prefix}_rgbs"][:5])


def test_downscale_4_vs_reference(data, fx):
    got = all_rows(llff_set(data, fx, s=4))
    assert got["rays"].shape == (4 * 12, 16, 8)
    check_against(got, fx, "llff_s4")


# ---- 3. options
def test_direction_options_vs_reference(data, fx):
    check_against(all_rows(llff_set(data, fx, unified_dir=True)), fx, "llff_unified", "llff_s2")
    check_against(all_rows(llff_set(data, fx, use_pixel_centers=False)), fx, "llff_nocentre", "llff_s2")
    check_against(all_rows(llff_set(data, fx, spheric=True)), fx, "llff_spheric", "llff_s2")
    both = llff_set(data, fx, unified_dir=True, use_pixel_centers=False)      # no recorded buffer: the restated rule
    want = np.concatenate([dr.view_rays(p, 12, 16, float(fx["llff_focal"]), 2, True, 0, 1, use_pixel_centers=False, unified_dir=True)
                           for p in fx["llff_poses"][train_views(fx)]])
    assert np.abs(all_rows(both)["rays"].cpu().numpy() - want).max() <= RAY_TOL


def test_gen_rays_opt_word_zero_is_gen_rays_range(data, fx):
    import ctypes
    from nerf_sr_amd import _lib
    lib = _lib.load()
    pose = np.ascontiguousarray(fx["llff_poses"][1].astype(np.float32).reshape(12))
    cp = pose.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for ndc, (lo, hi) in ((1, (0, 48)), (0, (5, 37))):
        a = torch.zeros(hi - lo, 4, 8, device="cuda")
        b = torch.zeros_like(a)
        _lib.check(lib.nsr_gen_rays_range(cp, 12, 16, float(fx["llff_focal"]), 2, ndc, 2.0, 6.0, lo, hi, a.data_ptr(), None), "range")
        _lib.check(lib.nsr_gen_rays_opt(cp, 12, 16, float(fx["llff_focal"]), 2, ndc, 2.0, 6.0, 0, lo, hi, b.data_ptr(), None), "opt")
        torch.cuda.synchronize()
        assert torch.equal(a, b) and float(a.abs().sum()) > 0
    # ... and with the options it is the rows of the batch kernel, bit for bit
    rs = llff_set(data, fx, unified_dir=True, use_pixel_centers=False)
    assert torch.equal(rs.view_rays(2), rs.batch(torch.arange(2 * 48, 3 * 48, device="cuda"))["rays"])


# ---- 4. precrop
def test_precrop_vs_train_crop(data, fx):
    full = blender_set(data, fx)
    crop = full.precrop(0.5)
    assert crop.window == (2, 2, 4, 4) and len(crop) == 3 * 16 and len(full) == 3 * 64
    assert crop.hr.data_ptr() == full.hr.data_ptr() and crop.poses.data_ptr() == full.poses.data_ptr()
    check_against(all_rows(crop), fx, "blender_crop")
    check_against(all_rows(full), fx, "blender_train")
    with pytest.raises(ValueError, match="do not cover the same pixels"):
        data.crop_window((20, 20), 4, 0.5)


# ---- 5. patches
def test_patches(data, fx):
    rs = llff_set(data, fx)
    ref = dr.RefSet(fx["llff_poses"][train_views(fx)], [fx[f"llff_px_{i}"] for i in train_views(fx)], 16, 12, 2, float(fx["llff_focal"]),
                    True, 0.0, 1.0)
    for k in range(3):
        i_img, row, col = (int(v) for v in fx[f"llff_patch{k}_loc"])
        got = rs.patch(i_img, row, col, 2)
        assert got["patch_rays"].shape == (4, 4, 8) and got["patch_rgbs"].shape == (4, 3)
        assert np.abs(got["patch_rays"].cpu().numpy() - fx[f"llff_patch{k}_rays"]).max() <= RAY_TOL
        assert np.array_equal(got["patch_rgbs"].cpu().numpy(), fx[f"llff_patch{k}_rgbs"])
    for view, row, col, length in ((0, 0, 0, 3), (1, 0, 5, 3), (2, 3, 0, 3), (3, 3, 5, 3), (3, 4, 6, 2), (0, 2, 1, 1)):   # corners
        got = rs.patch(view, row, col, length)
        _, rays, rgbs = ref.patch(view, row, col, length)
        assert np.abs(got["patch_rays"].cpu().numpy() - rays).max() <= RAY_TOL
        assert np.array_equal(got["patch_rgbs"].cpu().numpy(), rgbs)
    with pytest.raises(ValueError):
        rs.patch(0, 4, 6, 3)
    assert rs.n_patches(2) == 4 * 7 * 5
    g = torch.Generator().manual_seed(17)          # the reference's draw: seed 17 is recorded patch 1
    assert torch.equal(rs.random_patch(2, g)["patch_rays"], rs.patch(*(int(v) for v in fx["llff_patch1_loc"]), 2)["patch_rays"])


def test_regularize_patch_accepts_a_patch(data, fx):
    from nerf_sr_amd import train
    from nerf_sr_amd.weights import make_state_dict
    rs = llff_set(data, fx)
    t = train.Trainer(make_state_dict(11), make_state_dict(12), randomized=False, noise_std=0.0)
    tv = t.regularize_patch(rs.patch(1, 1, 2, 4)["patch_rays"], 4)       # 8 x 8 HR pixels: 64 rays
    assert tv.shape == (2,) and bool(torch.isfinite(tv).all())


# ---- 6. validation samples
def test_view_vs_validation_samples(data, fx):
    val = int(fx["llff_val_idx"])
    rs = data.RaySet(fx["llff_poses"][[val]], [fx[f"llff_px_{val}"]], (16, 12), 2, True, focal=float(fx["llff_focal"]))
    got = rs.view(0)
    for k in ("rays", "rays_ori", "c2w"):
        assert got[k].shape == fx[f"llff_val_{k}"].shape and np.abs(got[k].cpu().numpy() - fx[f"llff_val_{k}"]).max() <= RAY_TOL, k
    for k in ("rgbs", "rgbs_ori"):          # rgbs: pooled from the HR image although the set's ds_method is 'lanc'
        assert np.array_equal(got[k].cpu().numpy(), fx[f"llff_val_{k}"]), k
    assert "valid_mask" not in got
    meta = json.loads(bytes(fx["blender_val_json"]).decode())
    pose = np.array(meta["frames"][0]["transform_matrix"])[None, :3, :4]
    got = data.RaySet(pose, [fx["blender_val_px_0"]], (16, 16), 2, False, 2.0, 6.0, focal=float(fx["blender_focal"])).view(0)
    for k in ("rays", "rays_ori", "c2w"):
        assert np.abs(got[k].cpu().numpy() - fx[f"blender_val_{k}"]).max() <= RAY_TOL, k
    for k in ("rgbs", "rgbs_ori", "valid_mask", "valid_mask_ori"):
        assert got[k].shape == fx[f"blender_val_{k}"].shape and np.array_equal(got[k].cpu().numpy(), fx[f"blender_val_{k}"]), k
    # Blender with --ds_method avg: all four channels are pooled, then blended (the restated rule)
    avg = data.RaySet(pose, [fx["blender_val_px_0"]], (16, 16), 2, False, 2.0, 6.0, focal=float(fx["blender_focal"]), ds_method="avg")
    want = dr.validation_sample(pose[0], fx["blender_val_px_0"], 16, 16, 2, float(fx["blender_focal"]), False, 2.0, 6.0, ds_method="avg")
    got = avg.view(0)
    assert np.array_equal(got["rgbs"].cpu().numpy(), want["rgbs"]) and np.array_equal(got["valid_mask"].cpu().numpy(), want["valid_mask"])
    assert np.array_equal(all_rows(avg)["rgbs"].cpu().numpy(), want["rgbs"])


# ---- 7. out-of-range indices
def test_out_of_range_indices(data, fx):
    from nerf_sr_amd import _lib
    rs = llff_set(data, fx)
    n = len(rs)
    idx = torch.tensor([3, -1, 7, n, n - 1, 2 ** 40, -2 ** 40, 0], device="cuda")
    good = [0, 2, 4, 7]
    got = rs.batch(idx)
    want = rs.batch(idx[good])
    assert rs.status() == _lib.NSR_FLAG_INPUT_RANGE
    for k in ("rays", "rgbs", "rgbs_ori"):
        assert torch.equal(got[k][good], want[k]), k
        assert float(got[k][[1, 3, 5, 6]].abs().sum()) == 0.0, k
        assert float(want[k].abs().sum()) > 0.0
    assert rs.status(clear=True) == _lib.NSR_FLAG_INPUT_RANGE and rs.status() == 0
    rs.batch(idx[good])
    assert rs.status() == 0
    empty = rs.batch(torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert empty["rays"].shape == (0, 4, 8) and empty["rgbs"].shape == (0, 3)


# ---- 8. epochs
def test_epoch(data, fx):
    rs = llff_set(data, fx)
    n = len(rs)                                    # 192
    seen = []
    full = all_rows(rs)
    key = lambda rays: rays.reshape(rays.shape[0], -1)
    batches = list(rs.epoch(50, torch.Generator(device="cuda").manual_seed(3), keep_last=True))
    assert [b["rgbs"].shape[0] for b in batches] == [50, 50, 50, 42]
    # rays of different rows differ, so matching every produced row against the full buffer recovers its index
    for b in batches:
        eq = (key(b["rays"])[:, None, :] == key(full["rays"])[None, :, :]).all(-1)
        assert bool((eq.sum(1) == 1).all())
        rows = eq.float().argmax(1)
        assert torch.equal(b["rgbs"], full["rgbs"][rows]) and torch.equal(b["rgbs_ori"], full["rgbs_ori"][rows])
        seen.append(rows)
    assert torch.equal(torch.sort(torch.cat(seen))[0], torch.arange(n, device="cuda"))
    dropped = list(rs.epoch(50, torch.Generator(device="cuda").manual_seed(3)))
    assert len(dropped) == 3 and all(torch.equal(a["rays"], b["rays"]) for a, b in zip(dropped, batches))     # same seed, same batches
    other = list(rs.epoch(50, torch.Generator(device="cuda").manual_seed(4)))
    assert not torch.equal(other[0]["rays"], batches[0]["rays"])


# ---- 9. scenes on disk, training through the set
def write_llff(fx, root):
    os.makedirs(os.path.join(root, "images"))
    names = [str(n) for n in fx["llff_names"]]
    for i, n in enumerate(names):
        with open(os.path.join(root, "images", n), "wb") as f:
            f.write(fx[f"llff_png_{i}"].tobytes())
    W0, H0 = (int(v) for v in fx["llff_src_wh"])
    pts = fx["llff_points"]
    colmap_writer.write_reconstruction(os.path.join(root, "sparse", "0"), W0, H0, float(fx["llff_src_focal"]), names, fx["llff_c2ws"], pts,
                                       [[1, 2, 3, 4, 5] for _ in range(len(pts))])
    return root


def write_blender(fx, root):
    for split, n in (("train", 3), ("val", 1)):
        os.makedirs(os.path.join(root, split))
        for i in range(n):
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(fx[f"blender_{split}_png_{i}"].tobytes())
        with open(os.path.join(root, f"transforms_{split}.json"), "wb") as f:
            f.write(fx[f"blender_{split}_json"].tobytes())
    return root


def test_scenes_on_disk_reproduce_the_fixture(data, fx, tmp_path):
    root = write_llff(fx, str(tmp_path / "llff"))
    rs = data.RaySet.from_llff(root, (16, 12), 2, "train")
    assert rs.n_views == 4 and abs(rs.focal - float(fx["llff_focal"])) < 1e-9
    check_against(all_rows(rs), fx, "llff_s2")
    check_against(all_rows(data.RaySet.from_llff(root, (16, 12), 2, "train", include_var=True, ds_method="avg")), fx, "llff_avgvar")
    sph = data.RaySet.from_llff(root, (16, 12), 2, "train", spheric_poses=True)
    assert abs(sph.near - spheric_near_far(fx)[0]) < 1e-9 and abs(sph.far - spheric_near_far(fx)[1]) < 1e-9
    check_against(all_rows(sph), fx, "llff_spheric", "llff_s2")
    val = data.RaySet.from_llff(root, (16, 12), 2, "val").view(0)
    assert np.abs(val["rays"].cpu().numpy() - fx["llff_val_rays"]).max() <= RAY_TOL
    assert np.array_equal(val["rgbs"].cpu().numpy(), fx["llff_val_rgbs"])
    test = data.RaySet.from_llff(root, (16, 12), 2, "test", n_test_poses=8)
    assert np.abs(test.poses_host - fx["path_spiral"].astype(np.float32)).max() <= 1e-6 and set(test.view(3)) == {"rays", "rays_ori", "c2w"}
    broot = write_blender(fx, str(tmp_path / "blender"))
    check_against(all_rows(data.RaySet.from_blender(broot, (16, 16), 2, "train")), fx, "blender_train")
    check_against(all_rows(data.RaySet.from_blender(broot, (16, 16), 2, "train_crop", precrop_frac=0.5)), fx, "blender_crop")
    bval = data.RaySet.from_blender(broot, (16, 16), 2, "val").view(0)
    assert np.array_equal(bval["rgbs"].cpu().numpy(), fx["blender_val_rgbs"])
    assert np.array_equal(bval["valid_mask"].cpu().numpy(), fx["blender_val_valid_mask"])


def test_training_through_the_set_matches_materialised_buffers(data, fx):
    """Three optimisation steps fed by RaySet.batch against the same rows gathered from the materialised buffers (the
    reference's way): the inputs are the same bits, so the losses are."""
    from nerf_sr_amd import train
    from nerf_sr_amd.weights import make_state_dict
    rs = llff_set(data, fx)
    full = all_rows(rs)
    gen = torch.Generator().manual_seed(9)
    steps = [torch.randint(0, len(rs), (16,), generator=gen).cuda() for _ in range(3)]
    draws = [{"u_coarse": torch.rand(64, 64, generator=gen).cuda(), "u_fine": torch.rand(64, 64, generator=gen).cuda()} for _ in range(3)]
    losses = []
    for route in ("set", "buffers"):
        t = train.Trainer(make_state_dict(11), make_state_dict(12), randomized=True, noise_std=0.0)
        out = []
        for idx, d in zip(steps, draws):
            if route == "set":
                b = rs.batch(idx)
                t.set_input(b["rays"], b["rgbs"])
            else:
                t.set_input(full["rays"].index_select(0, idx), full["rgbs"].index_select(0, idx))
            out.append(t.optimize_parameters(d).clone())
        losses.append(torch.stack(out))
    assert torch.equal(losses[0], losses[1]) and bool(torch.isfinite(losses[0]).all()) and float(losses[0].abs().sum()) > 0
    assert not torch.equal(losses[0][0], losses[0][1])
