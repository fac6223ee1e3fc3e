"""Refinement patch batches generated on the device (include/nsr_refine_data.h, nerf_sr_amd/refine_data.py) against what the
reference's own dataset class produced (tests/golden/refine_data.npz) and against the numpy restatement
(tests/refine_data_ref.py, pinned to Pillow and to the same fixture by tests/test_refine_data_cpu.py).  Every comparison is
exact equality.  Sizes: the fixture's 40 x 28 images with 8-pixel patches; the trainer run uses 16-pixel patches of a 96 x 64
image."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from tests import refine_data_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return dict(np.load(os.path.join(golden_dir, "refine_data.npz")))


@pytest.fixture(scope="module")
def rd():
    from nerf_sr_amd import refine_data
    return refine_data


def make_set(rd, fx, tag):
    m = re.fullmatch(r"(train|val)_R(\d+)_gt(\d)", tag)
    return rd.RefinePatchSet(fx["gt_u8"], fx["sr_u8"], patch_len=int(fx["patch_len"]), num_ref_patches=int(m.group(2)),
                             ref_offset=int(fx["ref_offset"]), with_gt_patch=bool(int(m.group(3))), coeffs=fx["coeffs"],
                             split=m.group(1), ref_idx=int(fx["ref_idx"]))


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def ref_batch(fx, ps, aug, starts):
    """The restatement's batch for a 'train' set at explicit positions."""
    i = int(fx["ref_idx"])
    gt, sr = fx["gt_u8"][i], fx["sr_u8"][i]
    rows = [rr.sample(gt, sr, gt, fx["coeffs"][a], s, ps.patch_len, ps.num_ref_patches, ps.with_gt_patch) for a, s in zip(aug, starts)]
    return [np.stack([r[k] for r in rows]) for k in range(3)]


def valid_positions(fx, ps, n, seed):
    """n samples' (aug, starts) drawn through the restatement's mapping of random words."""
    rng = np.random.default_rng(seed)
    aug = rng.integers(0, ps.aug_num, n).astype(np.int32)
    words = rng.integers(0, 2 ** 31 - 1, (n, ps.n_words)).astype(np.int32)
    starts = np.stack([rr.positions_from_draws(w, fx["bboxs"][a], ps.patch_len, ps.num_ref_patches, ps.ref_offset, rr.TRAIN, ps.with_gt_patch)
                       for a, w in zip(aug, words)])
    return aug, words, starts


def test_boxes_are_the_references(rd, fx):
    ps = make_set(rd, fx, "train_R8_gt0")
    assert ps.bboxs.dtype == torch.int32 and np.array_equal(ps.bboxs.cpu().numpy(), fx["bboxs"])
    # the kernel's own row 0 (the constructor overwrites the identity row with the whole image, as the reference hard-codes it)
    raw = torch.full((ps.aug_num, 4), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().nsr_refine_aug_bbox(ctypes.byref(ps._d), raw.data_ptr(), None), "nsr_refine_aug_bbox")
    assert np.array_equal(raw.cpu().numpy(), fx["bboxs"])
    assert ps.resident_bytes() == 2 * 28 * 40 * 3 + 6 * 8 * 8 + 6 * 4 * 4
    # a box that is not wider and taller than the patch is refused
    with pytest.raises(ValueError, match="not wider and taller"):
        rd.RefinePatchSet(fx["gt_u8"], fx["sr_u8"], patch_len=27, coeffs=fx["coeffs"], ref_idx=1)


@pytest.mark.parametrize("tag", ["train_R8_gt0", "train_R8_gt1", "train_R3_gt0", "train_R3_gt1", "val_R8_gt0"])
def test_recorded_positions_give_the_references_samples(rd, fx, tag):
    ps = make_set(rd, fx, tag)
    got = host(ps.batch(fx[f"{tag}_aug"], fx[f"{tag}_starts"]))
    for k in ("sr_patch", "gt_patch", "ref_patches"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], fx[f"{tag}_{k}"]), k
    assert np.array_equal(got["starts"], fx[f"{tag}_starts"]) and ps.status() == 0


def test_whole_images_are_the_references_stacks(rd, fx):
    ps = make_set(rd, fx, "train_R8_gt0")
    for a in range(ps.aug_num):
        assert np.array_equal(ps.warped_image(a, "gt").cpu().numpy(), fx["gt_pspc_imgs"][a]), a
        assert np.array_equal(ps.warped_image(a, "sr").cpu().numpy(), fx["sr_pspc_imgs"][a]), a


def test_identity_row_returns_the_source_bytes(rd):
    """Values over the whole byte range, 0 included, at a size that is no multiple of anything."""
    rng = np.random.default_rng(8)
    gt, sr = rng.integers(0, 256, (21, 37, 3), dtype=np.uint8), rng.integers(0, 256, (21, 37, 3), dtype=np.uint8)
    gt[0, 0] = gt[20, 36] = 255
    ps = rd.RefinePatchSet(gt, sr, patch_len=5, num_ref_patches=2, ref_offset=4, coeffs=[rr.IDENTITY])
    assert np.array_equal(ps.warped_image(0, "gt").cpu().numpy(), rr.normalize(gt))
    assert np.array_equal(ps.warped_image(0, "sr").cpu().numpy(), rr.normalize(sr))
    starts = np.array([[31, 15, 30, 14, 28, 12, -1], [0, 0, 0, 0, 3, 3, -1]], dtype=np.int32)      # both ends of every range
    got = host(ps.batch([0, 0], starts))
    for b, s in enumerate(starts):
        assert np.array_equal(got["sr_patch"][b], rr.normalize(sr[s[1]:s[1] + 5, s[0]:s[0] + 5]))
        assert np.array_equal(got["gt_patch"][b], rr.normalize(gt[s[1]:s[1] + 5, s[0]:s[0] + 5]))
        assert np.array_equal(got["ref_patches"][b, 1], rr.normalize(gt[s[5]:s[5] + 5, s[4]:s[4] + 5]))
    assert ps.status() == 0


@pytest.mark.parametrize("tag", ["train_R8_gt1", "train_R3_gt0"])
def test_draws_follow_the_range_law(rd, fx, tag):
    ps = make_set(rd, fx, tag)
    aug, words, starts = valid_positions(fx, ps, 40, 11)
    got = ps._launch(aug, draws=words)
    assert np.array_equal(got["starts"].cpu().numpy(), starts)
    explicit = ps.batch(aug, starts)
    want = ref_batch(fx, ps, aug, starts)
    for k, w in zip(("sr_patch", "gt_patch", "ref_patches"), want):
        assert torch.equal(got[k], explicit[k]) and np.array_equal(got[k].cpu().numpy(), w), k
    assert ps.status() == 0
    if ps.with_gt_patch:
        assert len(set(starts[:, -1])) > 3 and all(np.array_equal(want[2][b, s[-1]], want[1][b]) for b, s in enumerate(starts))
    # sample(): the same law from words drawn on the device, reproducible from the generator
    g = torch.Generator(device="cuda").manual_seed(3)
    s1 = ps.sample(torch.arange(100, 113, device="cuda"), g)
    g = torch.Generator(device="cuda").manual_seed(3)
    words = torch.randint(0, 2 ** 31 - 1, (13, ps.n_words), dtype=torch.int32, device="cuda", generator=g).cpu().numpy()
    a1 = np.arange(100, 113) % ps.aug_num
    assert np.array_equal(s1["aug_idx"].cpu().numpy(), a1)
    want = np.stack([rr.positions_from_draws(w, fx["bboxs"][a], ps.patch_len, ps.num_ref_patches, ps.ref_offset, rr.TRAIN, ps.with_gt_patch)
                     for a, w in zip(a1, words)])
    assert np.array_equal(s1["starts"].cpu().numpy(), want) and ps.status() == 0
    assert sum(int(b["sr_patch"].shape[0]) for b in ps.epoch(5, 23, g)) == 20


def test_val_draws_and_the_references_empty_ranges(rd, fx):
    """'val': the window law with get_start_pos's second patch_len; a word that lands on x = 0 leaves the reference's range
    empty (np.random.randint raises there): that sample is zeros and flagged, its neighbours are untouched."""
    ps = make_set(rd, fx, "val_R8_gt0")
    rng = np.random.default_rng(12)
    n, W, H, P = 9, 40, 28, 8
    view = rng.integers(0, 3, n).astype(np.int32)
    words = rng.integers(0, 2 ** 31 - 1, (n, ps.n_words)).astype(np.int32)
    words[:, 0] = words[:, 0] // 32 * 32 + 1 + np.arange(n)          # x = 1 + b, never 0
    words[:, 1] = words[:, 1] // 20 * 20 + 2 + np.arange(n)
    words[4, 0] -= 5                                                    # ... but for sample 4: x = 0
    want = [rr.positions_from_draws(w, (0, 0, W, H), P, 8, 8, rr.VAL, False) for w in words]
    assert [w is None for w in want] == [b == 4 for b in range(n)]
    got = host(ps._launch(view, draws=words))
    ri = int(fx["ref_idx"])
    for b in range(n):
        if b == 4:
            assert not got["starts"][b].any() and not got["sr_patch"][b].any() and not got["gt_patch"][b].any() and not got["ref_patches"][b].any()
            continue
        assert np.array_equal(got["starts"][b], want[b])
        s, g, r = rr.sample(fx["gt_u8"][view[b]], fx["sr_u8"][view[b]], fx["gt_u8"][ri], rr.IDENTITY, want[b], P, 8, False)
        assert np.array_equal(got["sr_patch"][b], s) and np.array_equal(got["gt_patch"][b], g) and np.array_equal(got["ref_patches"][b], r)
    assert ps.status(clear=True) == _lib.NSR_FLAG_INPUT_RANGE and ps.status() == 0


def test_a_sample_does_not_depend_on_its_batch(rd, fx):
    ps = make_set(rd, fx, "train_R8_gt1")
    aug, _, starts = valid_positions(fx, ps, 67, 13)
    big = ps.batch(aug, starts)
    want = ref_batch(fx, ps, aug, starts)
    for k, w in zip(("sr_patch", "gt_patch", "ref_patches"), want):
        assert np.array_equal(big[k].cpu().numpy(), w), k
    for B, at in ((1, 0), (5, 3)):          # sample 66 of the large batch, alone and in the middle of five
        idx = np.arange(B)
        idx[at] = 66
        small = ps.batch(aug[idx], starts[idx])
        for k in ("sr_patch", "gt_patch", "ref_patches"):
            assert torch.equal(small[k][at], big[k][66]), (B, k)
    empty = ps.batch(np.zeros(0, dtype=np.int32), np.zeros((0, ps.n_words), dtype=np.int32))
    assert tuple(empty["ref_patches"].shape) == (0, 8, 3, 8, 8)


@pytest.mark.parametrize("P", [16, 20])
def test_patches_larger_than_one_workgroup(rd, fx, P):
    """256 pixels fill one workgroup exactly; 400 take two, the second partly empty."""
    ps = rd.RefinePatchSet(fx["gt_u8"], fx["sr_u8"], patch_len=P, num_ref_patches=3, ref_offset=5, with_gt_patch=True, coeffs=fx["coeffs"],
                           ref_idx=int(fx["ref_idx"]))
    aug, words, starts = valid_positions(fx, ps, 9, 16 + P)
    got = ps._launch(aug, draws=words)
    assert np.array_equal(got["starts"].cpu().numpy(), starts)
    for k, w in zip(("sr_patch", "gt_patch", "ref_patches"), ref_batch(fx, ps, aug, starts)):
        assert np.array_equal(got[k].cpu().numpy(), w), k
    assert ps.status() == 0


def test_out_of_range_positions_never_reach_memory(rd, fx):
    """Every kind of bad value in a batch of good ones: the bad samples are zeros, the flag is raised, the rest is intact."""
    ps = make_set(rd, fx, "train_R8_gt1")
    aug, _, starts = valid_positions(fx, ps, 12, 14)
    aug, starts = aug.copy(), starts.copy()
    good = host(ps.batch(aug, starts))
    assert ps.status() == 0
    box = fx["bboxs"][aug[1]]
    starts[1, 0] = box[2] - 8                      # x = wh - P: one past the reference's range
    starts[3, 1] = -1                              # y negative
    starts[5, 2 + 2 * 7] = 10 ** 9                 # a reference patch far outside
    starts[7, -1] = 8                              # gt_slot = R
    aug[9] = 6                                     # augmentation outside the table
    starts[10, 3] = starts[10, 1] + 8              # ref_y = y + ref_offset: one past the window
    bad = {1, 3, 5, 7, 9, 10}
    got = host(ps.batch(aug, starts))
    for b in range(12):
        for k in ("sr_patch", "gt_patch", "ref_patches"):
            assert (not got[k][b].any()) if b in bad else np.array_equal(got[k][b], good[k][b]), (b, k)
    assert ps.status(clear=True) == _lib.NSR_FLAG_INPUT_RANGE and ps.status() == 0


def test_from_files_reads_like_the_reference(rd, tmp_path):
    """:115-119: the ground truth resized to img_wh with LANCZOS (Pillow's bytes), the synthesised image cropped from its corner."""
    from PIL import Image
    rng = np.random.default_rng(17)
    gts, srs = [], []
    for k in range(2):
        g, s = rng.integers(16, 256, (56, 80, 3), dtype=np.uint8), rng.integers(16, 256, (30, 44, 3), dtype=np.uint8)
        Image.fromarray(g).save(tmp_path / f"gt{k}.png")
        Image.fromarray(s).save(tmp_path / f"{k}-fine-ori.png")
        gts.append(np.asarray(Image.fromarray(g).resize((40, 28), Image.LANCZOS)))
        srs.append(s[:28, :40])
    ps = rd.RefinePatchSet.from_files(str(tmp_path / "gt1.png"), str(tmp_path / "1-fine-ori.png"), (40, 28), patch_len=8, aug_num=3,
                                      generator=torch.Generator().manual_seed(0))
    assert np.array_equal(ps.gt.cpu().numpy(), gts[1][None]) and np.array_equal(ps.sr.cpu().numpy(), srs[1][None])
    assert ps.aug_num == 3 and tuple(ps.bboxs_host[0]) == (0, 0, 40, 28)
    val = rd.RefinePatchSet.from_files([str(tmp_path / f"gt{k}.png") for k in range(2)], [str(tmp_path / f"{k}-fine-ori.png") for k in range(2)],
                                       (40, 28), patch_len=8, split="val", ref_idx=1)
    assert np.array_equal(val.gt.cpu().numpy(), np.stack(gts)) and np.array_equal(val.ref.cpu().numpy(), gts[1]) and val.aug_num == 2


def test_trainer_learns_from_sampled_batches(rd):
    """24 Adam steps of RefineTrainer on batches of 4 from sample() at patch_len 16.  The bound needs no measurement: the
    randomly initialised network starts far from the target, every batch comes from the same image pair, and the existing
    trainer test already requires 20 steps on a fixed batch to fall below the reference's 10-step loss -- so the mean L1 of
    the last four steps must lie below the first step's."""
    from PIL import Image, ImageFilter
    from nerf_sr_amd import refine
    rng = np.random.default_rng(15)
    small = Image.fromarray(rng.integers(16, 256, (8, 12, 3), dtype=np.uint8))
    gt = small.resize((96, 64), Image.BICUBIC)
    sr = np.asarray(gt.filter(ImageFilter.GaussianBlur(1.5)), dtype=np.int16) + rng.integers(-6, 7, (64, 96, 3))
    gt, sr = np.maximum(np.asarray(gt, dtype=np.uint8), 16), np.clip(sr, 16, 255).astype(np.uint8)
    ps = rd.RefinePatchSet(gt, sr, patch_len=16, num_ref_patches=8, ref_offset=16, aug_num=10, generator=torch.Generator().manual_seed(1))
    tr = refine.RefineTrainer(refine.make_refine_state_dict(7), lr=5e-4)
    g = torch.Generator(device="cuda").manual_seed(2)
    l1 = []
    for it in range(24):
        tr.set_input(ps.sample(torch.arange(4 * it, 4 * it + 4, device="cuda"), g))
        tr.optimize_parameters()
        l1.append(float(tr.loss_l1.detach()))
    print("L1 per step:", " ".join(f"{v:.4f}" for v in l1))
    assert ps.status() == 0 and np.isfinite(l1).all()
    assert np.mean(l1[-4:]) < l1[0]
