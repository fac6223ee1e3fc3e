"""Training and validation patch batches of the refinement stage, generated on the device (include/nsr_refine_data.h).

The reference's ``LLFFRefineDataset('train')`` (data/llff_refine_dataset.py:113-146, 214-238) warps the ground-truth and the
synthesised image ``aug_num`` times with a random perspective on the host, keeps all ``2 * aug_num`` results as fp32 tensors
(915 MB at 504 x 378, 200 augmentations) and slices 1 + 1 + ``num_ref_patches`` patches per sample with ``np.random.randint``.
A ``RefinePatchSet`` keeps the two 8-bit images, one row of eight perspective coefficients and one bounding box per
augmentation, and produces a batch in ONE launch (``nsr_refine_patch_batch``): sr / gt pixels are warped on the fly with
Pillow's 8-bit PERSPECTIVE + BILINEAR arithmetic, byte for byte what ``TF.perspective`` gives on a PIL image; reference patches
are crops of the 8-bit reference image.  The ``val`` split (:147-159, 240-254) runs through the same kernel.

A batch is ``{"sr_patch": (B, 3, P, P), "gt_patch": (B, 3, P, P), "ref_patches": (B, R, 3, P, P)}`` fp32 in [-1, 1], what
``refine.RefineTrainer.set_input`` takes, plus ``"starts"`` (B, 2 + 2R + 1) int32 -- the positions used -- and ``"aug_idx"``.

Out of scope: the `test` / `test_train` tilers (``refine.tile_refs`` / ``gather_patches``), the commented-out colour jitter.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterator, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ops import _check_device, _p, _stream

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def perspective_coeffs(startpoints, endpoints) -> np.ndarray:
    """The eight coefficients of the map destination -> source that ``TF.perspective(img, startpoints, endpoints)`` hands to
    Pillow: ``(a0 x + a1 y + a2) / (a6 x + a7 y + 1)``, ``(a3 x + a4 y + a5) / (a6 x + a7 y + 1)`` takes every end point to its
    start point.  The 8 x 8 system is solved in double."""
    a = np.zeros((8, 8), dtype=np.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i] = [p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]]
        a[2 * i + 1] = [0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]]
    b = np.asarray(startpoints, dtype=np.float64).reshape(8)
    return np.linalg.solve(a, b)


def perspective_params(width: int, height: int, distortion_scale: float, generator: Optional[torch.Generator] = None):
    """Start and end points by the law of ``RandomPerspective.get_params``: every corner moves inwards by an offset uniform in
    ``[0, int(d * (W // 2))]`` x ``[0, int(d * (H // 2))]``, drawn with ``torch.randint`` on the host in that class's order."""
    hw, hh = int(distortion_scale * (width // 2)), int(distortion_scale * (height // 2))
    r = lambda lo, hi: int(torch.randint(lo, hi, size=(1,), generator=generator).item())
    topleft = [r(0, hw + 1), r(0, hh + 1)]
    topright = [r(width - hw - 1, width), r(0, hh + 1)]
    botright = [r(width - hw - 1, width), r(height - hh - 1, height)]
    botleft = [r(0, hw + 1), r(height - hh - 1, height)]
    return [[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]], [topleft, topright, botright, botleft]


def draw_coeffs(width: int, height: int, aug_num: int, distort_scale: float, generator: Optional[torch.Generator] = None) -> np.ndarray:
    """(aug_num, 8) double: row 0 the identity (the reference's un-warped first entry), then ``aug_num - 1`` random perspectives."""
    rows = [np.asarray(IDENTITY, dtype=np.float64)]
    for _ in range(int(aug_num) - 1):
        rows.append(perspective_coeffs(*perspective_params(width, height, distort_scale, generator)))
    return np.stack(rows)


def _images_u8(x, name: str, device) -> torch.Tensor:
    t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    if t.dtype != torch.uint8 or t.ndim not in (3, 4) or t.shape[-1] != 3:
        raise TypeError(f"{name} must be (H, W, 3) or (n, H, W, 3) uint8 RGB")
    return (t if t.ndim == 4 else t[None]).to(device).contiguous()


class RefinePatchSet:
    """8-bit ground-truth / synthesised images + perspective table on the device; patch batches from them.

    gt_u8, sr_u8     (H, W, 3) or (n, H, W, 3) uint8, numpy or torch.  split 'train': the pair of view ``ref_idx`` is used;
                     split 'val': all n views, the reference image is ``gt_u8[ref_idx]``.  Host images and views are copied to
                     the device as dense tensors; a dense uint8 tensor that is already on the device is KEPT, not copied (the
                     set reads it in place and never writes it: do not change it while the set lives).  Another dtype raises
                     ``TypeError``
    patch_len, num_ref_patches, ref_offset, with_gt_patch, aug_num, distort_scale   the reference's options of the same names
    generator        host ``torch.Generator`` the perspectives are drawn with (``perspective_params``)
    coeffs           (aug_num, 8) coefficients instead of drawn ones (row 0 the identity, by the reference's convention)
    The bounding boxes come from ``nsr_refine_aug_bbox``; a box that is not wider and taller than ``patch_len`` raises
    ``ValueError`` (the reference's ``np.random.randint`` would raise on its empty range at the first such sample).  An identity
    row 0 gets the whole image as its box, as the reference hard-codes.
    """

    def __init__(self, gt_u8, sr_u8, *, patch_len: int = 64, num_ref_patches: int = 8, ref_offset: int = 64, with_gt_patch: bool = False,
                 aug_num: int = 200, distort_scale: float = 0.3, generator: Optional[torch.Generator] = None, coeffs=None,
                 split: str = "train", ref_idx: int = 0, device="cuda"):
        if split not in ("train", "val"):
            raise ValueError(f"split {split!r} is not built here ('train' or 'val'; the test tilers are refine.tile_refs / gather_patches)")
        self.split = split
        self.patch_len, self.num_ref_patches, self.ref_offset = int(patch_len), int(num_ref_patches), int(ref_offset)
        self.with_gt_patch = bool(with_gt_patch)
        if not 1 <= self.num_ref_patches <= _lib.NSR_REFINE_MAX_REF_PATCHES:
            raise ValueError(f"num_ref_patches must be in [1, {_lib.NSR_REFINE_MAX_REF_PATCHES}]")
        if self.patch_len <= 0 or self.ref_offset <= 0:
            raise ValueError("patch_len and ref_offset must be positive")
        if split == "val" and self.with_gt_patch:
            raise ValueError("with_gt_patch belongs to the 'train' split (the reference's 'val' split ignores it)")
        self.device = torch.device(device)
        _check_device(self.device, "device")
        gt, sr = _images_u8(gt_u8, "gt_u8", self.device), _images_u8(sr_u8, "sr_u8", self.device)
        if gt.shape != sr.shape:
            raise ValueError("input size must be equal to synthesized image size")
        ref_idx = int(ref_idx)
        if not 0 <= ref_idx < gt.shape[0]:
            raise IndexError(f"ref_idx {ref_idx} of {gt.shape[0]} views")
        if split == "train":
            gt, sr = gt[ref_idx:ref_idx + 1].contiguous(), sr[ref_idx:ref_idx + 1].contiguous()
        self.gt, self.sr = gt, sr
        self.ref = gt[0] if split == "train" else gt[ref_idx]       # a view: no bytes of its own
        H, W = int(gt.shape[1]), int(gt.shape[2])
        self.img_wh = (W, H)
        P = self.patch_len
        if P >= W or P >= H:
            raise ValueError(f"patch_len {P} leaves no start position in a {W} x {H} image")
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.coeffs = self.bboxs = None
        if split == "train":
            c = draw_coeffs(W, H, aug_num, distort_scale, generator) if coeffs is None else np.asarray(coeffs, dtype=np.float64)
            if c.ndim != 2 or c.shape[1] != 8 or c.shape[0] < 1 or not np.isfinite(c).all():
                raise ValueError("coeffs must be a finite (aug_num, 8) array")
            self.coeffs_host = np.ascontiguousarray(c)
            self.coeffs = torch.from_numpy(self.coeffs_host).to(self.device)
            self.bboxs = torch.zeros(c.shape[0], 4, dtype=torch.int32, device=self.device)
            self._d = self._make_desc()
            _lib.check(_lib.load().nsr_refine_aug_bbox(ctypes.byref(self._d), _p(self.bboxs), _stream()), "nsr_refine_aug_bbox")
            if tuple(self.coeffs_host[0]) == IDENTITY:
                self.bboxs[0] = torch.tensor([0, 0, W, H], dtype=torch.int32, device=self.device)
            self.bboxs_host = self.bboxs.cpu().numpy()
            for a, (x0, y0, x1, y1) in enumerate(self.bboxs_host):
                if x1 - x0 <= P or y1 - y0 <= P:
                    raise ValueError(f"augmentation {a}: its box ({x0}, {y0}, {x1}, {y1}) is not wider and taller than patch_len {P}")
        else:
            self._d = self._make_desc()

    def _make_desc(self) -> _lib.NsrRefinePatchset:
        W, H = self.img_wh
        train = self.split == "train"
        return _lib.NsrRefinePatchset(gt=self.gt.data_ptr(), sr=self.sr.data_ptr(), ref=self.ref.data_ptr(),
                                      coeffs=self.coeffs.data_ptr() if train else 0, bboxs=self.bboxs.data_ptr() if train else 0,
                                      n_img=int(self.gt.shape[0]), n_aug=self.aug_num, H=H, W=W, patch_len=self.patch_len,
                                      num_ref_patches=self.num_ref_patches, ref_offset=self.ref_offset,
                                      with_gt_patch=int(self.with_gt_patch),
                                      mode=_lib.NSR_PATCHES_TRAIN if train else _lib.NSR_PATCHES_VAL)

    # -------------------------------------------------------------------------------------------- sizes
    @property
    def aug_num(self) -> int:
        """Rows ``aug_idx`` counts over: augmentations ('train') or views ('val')."""
        return int(self.coeffs.shape[0]) if self.split == "train" else int(self.gt.shape[0])

    @property
    def n_words(self) -> int:
        return 2 + 2 * self.num_ref_patches + 1

    def resident_bytes(self) -> int:
        """Device bytes the set keeps: the 8-bit images and the two tables (the reference: 2 * aug_num fp32 images)."""
        return sum(t.numel() * t.element_size() for t in (self.gt, self.sr, self.coeffs, self.bboxs) if t is not None)

    # -------------------------------------------------------------------------------------------- the launch
    def _i32(self, t, name: str, shape) -> torch.Tensor:
        t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t), device=self.device)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise TypeError(f"{name} must be integers")
        _check_device(t.device, name)
        if len(shape) == 2 and t.numel() % shape[1]:
            raise ValueError(f"{name} must hold rows of {shape[1]} words, got {tuple(t.shape)}")
        t = t.detach().to(torch.int32).reshape(shape).contiguous()
        return t

    def _launch(self, aug_idx, starts=None, draws=None) -> Dict[str, torch.Tensor]:
        aug_idx = self._i32(aug_idx, "aug_idx", (-1,))
        B, P, R = int(aug_idx.numel()), self.patch_len, self.num_ref_patches
        words = self._i32(starts if draws is None else draws, "starts" if draws is None else "draws", (-1, self.n_words))
        if words.shape[0] != B:
            raise ValueError(f"{B} samples but {words.shape[0]} rows of positions")
        out = {"sr_patch": torch.empty(B, 3, P, P, dtype=torch.float32, device=self.device),
               "gt_patch": torch.empty(B, 3, P, P, dtype=torch.float32, device=self.device),
               "ref_patches": torch.empty(B, R, 3, P, P, dtype=torch.float32, device=self.device),
               "starts": torch.empty(B, self.n_words, dtype=torch.int32, device=self.device), "aug_idx": aug_idx}
        _lib.check(_lib.load().nsr_refine_patch_batch(
            ctypes.byref(self._d), _p(aug_idx), _p(words if draws is None else None), _p(None if draws is None else words), B,
            _p(out["sr_patch"]), _p(out["gt_patch"]), _p(out["ref_patches"]), _p(out["starts"]), _p(self._status), _stream()),
            "nsr_refine_patch_batch")
        return out

    def batch(self, aug_idx, starts) -> Dict[str, torch.Tensor]:
        """The samples at explicit positions: ``starts`` (B, 2 + 2R + 1) = x, y, (ref_x, ref_y) x R, gt_slot, each checked
        against the range the reference would draw it from.  A sample with a value outside yields zero rows and raises the
        INPUT_RANGE flag of ``status()``; it never reaches memory.  gt_slot is read only with ``with_gt_patch``."""
        return self._launch(aug_idx, starts=starts)

    def sample(self, idx, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """``__getitem__`` for the indices ``idx`` (the augmentation / view is ``idx % aug_num``), positions drawn on the device:
        one ``torch.randint`` of raw words (``generator``: a generator of this set's device), mapped to the reference's ranges
        by the kernel.  'val': where the reference's own range is empty (x or y of 0) it raises; here the sample is zeros and
        flagged."""
        idx = self._i32(idx, "idx", (-1,))
        draws = torch.randint(0, 2 ** 31 - 1, (int(idx.numel()), self.n_words), dtype=torch.int32, device=self.device, generator=generator)
        return self._launch(idx % self.aug_num, draws=draws)

    def epoch(self, batch_size: int, n: int, generator: Optional[torch.Generator] = None,
              keep_last: bool = False) -> Iterator[Dict[str, torch.Tensor]]:
        """One shuffled pass over the indices ``0 .. n - 1`` (the reference's ``data_num``) in batches; the remainder is dropped
        unless ``keep_last``."""
        batch_size, n = int(batch_size), int(n)
        if batch_size <= 0 or n < 0:
            raise ValueError("batch_size must be positive and n non-negative")
        perm = torch.randperm(n, device=self.device, generator=generator)
        end = n if keep_last else n - n % batch_size
        for lo in range(0, end, batch_size):
            yield self.sample(perm[lo:min(lo + batch_size, end)], generator)

    def warped_image(self, a: int, source: str = "gt") -> torch.Tensor:
        """(3, H, W) fp32: the whole warped, normalised image of augmentation ``a`` -- the reference's ``gt_pspc_imgs[a]`` /
        ``sr_pspc_imgs[a]``.  For inspection; batches never materialise it."""
        if self.split != "train" or source not in ("gt", "sr"):
            raise ValueError("warped_image: 'train' sets only, source 'gt' or 'sr'")
        W, H = self.img_wh
        out = torch.empty(3, H, W, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().nsr_refine_warp_image(ctypes.byref(self._d), int(a), int(source == "sr"), _p(out), _stream()),
                   "nsr_refine_warp_image")
        return out

    def status(self, clear: bool = False) -> int:
        """Sticky status word of the batches (``NSR_FLAG_INPUT_RANGE``: a sample was outside its ranges).  Waits for the stream."""
        flags = int(self._status.item()) & 0xFFFFFFFF
        if clear:
            self._status.zero_()
        return flags

    # -------------------------------------------------------------------------------------------- images on disk
    @classmethod
    def from_files(cls, gt_path, sr_path, img_wh, **kw) -> "RefinePatchSet":
        """Image files the way the reference reads them (:115-119): the ground truth is converted to RGB and resized to
        ``img_wh`` with LANCZOS (on the device, bit-identical to Pillow), the synthesised image is cropped to ``img_wh`` from
        its top-left corner.  ``gt_path`` / ``sr_path``: one path each, or equally long lists (the views of a 'val' set)."""
        from PIL import Image       # file decoding only
        from . import io as nsr_io
        gts = [gt_path] if isinstance(gt_path, (str, bytes)) or not isinstance(gt_path, Sequence) else list(gt_path)
        srs = [sr_path] if isinstance(sr_path, (str, bytes)) or not isinstance(sr_path, Sequence) else list(sr_path)
        if len(gts) != len(srs):
            raise ValueError(f"{len(gts)} ground-truth files but {len(srs)} synthesised files")
        W, H = int(img_wh[0]), int(img_wh[1])
        dev = kw.get("device", "cuda")
        gt, sr = [], []
        for g, s in zip(gts, srs):
            with Image.open(g) as im:
                gt.append(nsr_io.resize_lanczos_u8(torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev), (W, H)))
            with Image.open(s) as im:
                sr.append(torch.from_numpy(np.asarray(im.convert("RGB").crop((0, 0, W, H)), dtype=np.uint8).copy()))
        return cls(torch.stack(gt), torch.stack(sr), **kw)
