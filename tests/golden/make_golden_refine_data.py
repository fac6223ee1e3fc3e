#!/usr/bin/env python3
"""Golden vectors of the reference's refinement training data: ``LLFFRefineDataset`` in its 'train' and 'val' splits
(data/llff_refine_dataset.py:113-159, 214-254): the perspective-warped image stacks ``gt_pspc_imgs`` / ``sr_pspc_imgs``, their
bounding boxes, and a dozen ``__getitem__`` samples together with the positions their ``np.random.randint`` calls returned
(the function is wrapped; arguments and results are recorded).  Development container only; data only.

The reference's own dataset class is instantiated on a fabricated scene (COLMAP binaries written by tests/colmap_writer.py,
random PNGs with pixel values >= 16): 40 x 28 images, 8-pixel patches, ref_offset 8, 6 augmentations.

torchvision and OpenCV are not installed in the development container.  Like the earlier generators do for ``ToTensor``, this
one supplies stand-ins written from the documented behaviour of the calls the dataset makes:
  * ``T.RandomPerspective.get_params(width, height, distortion_scale)``: the four corners move inwards by ``torch.randint``
    offsets in ``[0, int(d * (width // 2))]`` x ``[0, int(d * (height // 2))]``, drawn in the order top-left, top-right,
    bottom-right, bottom-left, x before y; start points (0, 0), (W-1, 0), (W-1, H-1), (0, H-1);
  * ``TF.perspective(pil_img, startpoints, endpoints)``: solves the 8 x 8 system for the coefficients of the map end point ->
    start point (in double here) and calls Pillow's own ``img.transform(img.size, Image.PERSPECTIVE, coeffs, Image.BILINEAR,
    fillcolor=0)`` -- the pixels are Pillow's, not a restatement;
  * ``cv2.cvtColor(a, COLOR_BGR2GRAY)``: the 14-bit fixed-point luma (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 of channel
    order B, G, R;  ``cv2.threshold(g, 0, 255, THRESH_BINARY)``: 255 where g > 0;  ``cv2.findContours(t, RETR_EXTERNAL,
    CHAIN_APPROX_SIMPLE)``: the outer contour of each 8-connected component -- the stand-in asserts there is exactly ONE
    component and returns its pixels;  ``cv2.boundingRect(points)``: x_min, y_min, x_max - x_min + 1, y_max - y_min + 1.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_warp as mw  # noqa: E402
from make_golden_tiler import Compose, Normalize  # noqa: E402
from colmap_writer import write_reconstruction  # noqa: E402

W, H, P, OFF, AUG = 40, 28, 8, 8, 6
COEFFS = []          # one row per TF.perspective call on the ground-truth image


class RandomPerspective:
    @staticmethod
    def get_params(width, height, distortion_scale):
        hh, hw = height // 2, width // 2
        r = lambda lo, hi: int(torch.randint(lo, hi, size=(1,)).item())
        dw, dh = int(distortion_scale * hw), int(distortion_scale * hh)
        topleft = [r(0, dw + 1), r(0, dh + 1)]
        topright = [r(width - dw - 1, width), r(0, dh + 1)]
        botright = [r(width - dw - 1, width), r(height - dh - 1, height)]
        botleft = [r(0, dw + 1), r(height - dh - 1, height)]
        return [[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]], [topleft, topright, botright, botleft]


def perspective(img, startpoints, endpoints):
    a = np.zeros((8, 8), dtype=np.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i] = [p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]]
        a[2 * i + 1] = [0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]]
    coeffs = np.linalg.solve(a, np.asarray(startpoints, dtype=np.float64).reshape(8))
    if not COEFFS or not np.array_equal(COEFFS[-1], coeffs):       # called for the gt and the sr image with the same points
        COEFFS.append(coeffs)
    return img.transform(img.size, Image.PERSPECTIVE, [float(c) for c in coeffs], Image.BILINEAR, fillcolor=0)


def cvt_color(a, code):
    a = a.astype(np.int64)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def threshold(g, thresh, maxval, kind):
    return float(thresh), np.where(g > thresh, maxval, 0).astype(np.uint8)


def find_contours(t, mode, method):
    ys, xs = np.nonzero(t)
    todo, seen = [(int(ys[0]), int(xs[0]))], {(int(ys[0]), int(xs[0]))}
    while todo:                                   # flood fill, 8-connected
        y, x = todo.pop()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = (y + dy, x + dx)
                if 0 <= q[0] < t.shape[0] and 0 <= q[1] < t.shape[1] and t[q] and q not in seen:
                    seen.add(q)
                    todo.append(q)
    assert len(seen) == len(ys), "the warped image is not one connected region"
    return [np.array([[x, y] for y, x in sorted(seen)])], None


def bounding_rect(pts):
    x0, y0, x1, y1 = pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()
    return int(x0), int(y0), int(x1 - x0 + 1), int(y1 - y0 + 1)


class RecordedRandint:
    """np.random.randint with its (low, high, result) triples kept."""

    def __init__(self):
        self.orig, self.calls = np.random.randint, []

    def __call__(self, low, high=None):
        v = self.orig(int(low), None if high is None else int(high))
        self.calls.append((0 if high is None else int(low), int(low) if high is None else int(high), int(v)))
        return v

    def take(self):
        c, self.calls = self.calls, []
        return c


def main():
    mg.install_shim()
    import cv2
    import torchvision.transforms as T
    import torchvision.transforms.functional as TF
    T.ToTensor, T.Normalize, T.Compose, T.RandomPerspective = mw.ToTensor, Normalize, Compose, RandomPerspective
    TF.perspective = perspective
    cv2.cvtColor, cv2.threshold, cv2.findContours, cv2.boundingRect = cvt_color, threshold, find_contours, bounding_rect
    cv2.COLOR_BGR2GRAY, cv2.THRESH_BINARY, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE = 6, 0, 0, 2
    rec = RecordedRandint()
    np.random.randint = rec

    rng = np.random.default_rng(33)
    root = tempfile.mkdtemp(prefix="nsr_rdata_root_")
    syn = tempfile.mkdtemp(prefix="nsr_rdata_syn_")
    os.makedirs(os.path.join(root, "images"))
    names = ["a.png", "b.png", "c.png"]
    gt_u8, sr_u8 = [], []
    for i, n in enumerate(names):
        gt_u8.append(rng.integers(16, 256, (H, W, 3), dtype=np.uint8))
        sr_u8.append(rng.integers(16, 256, (H, W, 3), dtype=np.uint8))
        Image.fromarray(gt_u8[-1]).save(os.path.join(root, "images", n))
        Image.fromarray(sr_u8[-1]).save(os.path.join(syn, f"{i}-fine-ori.png"))
    c2ws = [mw.look_at_colmap(np.array([0.3 * i, 0.0, 0.0]), np.array([0.0, 0.0, 4.0])) for i in range(3)]
    pts = rng.normal(0, 0.5, (20, 3)) + np.array([0.0, 0.0, 4.0])
    write_reconstruction(os.path.join(root, "sparse", "0"), W, H, 2.0 * W, names, c2ws, pts, [[1, 2, 3]] * len(pts))
    from data.llff_refine_dataset import LLFFRefineDataset

    def options(R, with_gt):
        return types.SimpleNamespace(dataset_root=root, img_wh=(W, H), ref_idx=1, syn_dataroot=syn, patch_len=P, num_ref_patches=R,
                                     aug_num=AUG, distort_scale=0.3, with_gt_patch=with_gt, ref_offset=OFF, data_num=1000)

    out = {"W": W, "H": H, "patch_len": P, "ref_offset": OFF, "aug_num": AUG, "ref_idx": 1, "gt_u8": np.stack(gt_u8), "sr_u8": np.stack(sr_u8)}
    np.random.seed(7)
    cases = []
    for R, with_gt in ((8, False), (8, True), (3, False), (3, True)):
        torch.manual_seed(5)                       # the same perspectives for every option set
        n_before = len(COEFFS)
        ds = LLFFRefineDataset(options(R, with_gt), "train")
        rows = np.stack([np.array([1.0, 0, 0, 0, 1, 0, 0, 0])] + COEFFS[n_before:])
        assert rows.shape == (AUG, 8) and not rec.take()
        if "coeffs" in out:
            assert np.array_equal(out["coeffs"], rows) and np.array_equal(out["gt_pspc_imgs"], mg.np32(ds.gt_pspc_imgs))
        out["coeffs"], out["bboxs"] = rows, ds.bboxs.numpy().astype(np.int32)
        out["gt_pspc_imgs"], out["sr_pspc_imgs"] = mg.np32(ds.gt_pspc_imgs), mg.np32(ds.sr_pspc_imgs)
        tag = f"train_R{R}_gt{int(with_gt)}"
        cases.append(tag)
        idxs = [1 + 7 * k for k in range(3)] + ([0] if R == 8 else [])      # idx % aug_num covers every row, the identity too
        _store(out, tag, ds, idxs, rec, R, with_gt)
    ds = LLFFRefineDataset(options(8, False), "val")
    # the reference's own 'val' ranges are empty where x or y is 0 (get_start_pos subtracts patch_len a second time) and
    # np.random.randint raises there: such an index is redrawn
    idxs, kept = iter(range(1000)), []
    samples, calls = [], []
    while len(kept) < 4:
        i = next(idxs)
        try:
            s = ds[i]
        except ValueError:
            rec.take()
            continue
        kept.append(i)
        samples.append(s)
        calls.append(rec.take())
    _pack(out, "val_R8_gt0", kept, samples, calls, 8, False, [i % 3 for i in kept])
    cases.append("val_R8_gt0")
    out["cases"] = np.array(cases)
    np.random.randint = rec.orig
    path = os.path.join(HERE, "refine_data.npz")
    np.savez_compressed(path, **out)
    print("bboxs", out["bboxs"].tolist())
    print("->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


def _store(out, tag, ds, idxs, rec, R, with_gt):
    samples, calls = [], []
    for i in idxs:
        samples.append(ds[i])
        calls.append(rec.take())
    _pack(out, tag, idxs, samples, calls, R, with_gt, [i % AUG for i in idxs])


def _pack(out, tag, idxs, samples, calls, R, with_gt, rows):
    n_words = 2 + 2 * R + 1
    starts = np.full((len(idxs), n_words), -1, dtype=np.int32)
    ranges = np.full((len(idxs), n_words, 2), -1, dtype=np.int32)
    for k, c in enumerate(calls):
        assert len(c) == n_words - (0 if with_gt else 1)
        for j, (lo, hi, v) in enumerate(c):
            starts[k, j], ranges[k, j] = v, (lo, hi)
    out[f"{tag}_idx"], out[f"{tag}_aug"] = np.array(idxs, dtype=np.int32), np.array(rows, dtype=np.int32)
    out[f"{tag}_starts"], out[f"{tag}_ranges"] = starts, ranges
    for key in ("sr_patch", "gt_patch", "ref_patches"):
        out[f"{tag}_{key}"] = np.stack([mg.np32(s[key]) for s in samples])
    print(tag, "samples", len(idxs), "ref_patches", out[f"{tag}_ref_patches"].shape)


if __name__ == "__main__":
    main()
