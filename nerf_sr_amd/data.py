"""Training and validation ray batches generated on the device (include/nsr_data.h).

The reference's downX datasets (data/llff_downX_dataset.py, data/blender_downX_dataset.py) materialise three fp32 buffers
over all training views -- ``all_rays`` (N, s*s, 8), ``all_rgbs`` (N, 3), ``all_rgbs_ori`` (N, s*s, 3), N = views x LR
pixels -- and a batch is three gathers.  A ``RaySet`` keeps what the scene is on disk instead: one 3 x 4 pose per view and
the 8-bit HR / LR images (resized on the device, bit-identical to Pillow: ``io.resize_lanczos_u8``), and produces the rows
of a batch in ONE launch (``nsr_rayset_batch``): the ray of a row is generated, its targets are converted from the bytes.
Row numbers are the reference's: ``view * (w*h) + row * w + col`` in LR pixels of the window.

Out of scope, like in the rest of the package: the `gan` split, ``--rand_dir``, ``--sisr_path`` tables, multi-rank
sharding of an epoch.  Image FILES are decoded with Pillow by the two ``from_*`` constructors only.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Iterator, Optional, Tuple

import numpy as np
import torch

from . import _lib, io as nsr_io
from .ops import _check_device, _p, _stream


def crop_window(img_wh: Tuple[int, int], downscale: int, frac: float) -> Tuple[int, int, int, int]:
    """LR-pixel window (x0, y0, w, h) of the Blender ``train_crop`` centre crop (blender_downX_dataset.py:122-136).  The
    reference crops the HR tensors by ``int(H // 2 * frac)`` and the LR image by ``int((H // s) // 2 * frac)`` independently;
    where the two do not cover the same pixels its buffers are misaligned (or the regroup fails): that is an error here."""
    W, H = int(img_wh[0]), int(img_wh[1])
    s = int(downscale)
    w_lr, h_lr = W // s, H // s
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    dh, dw = int(h_lr // 2 * frac), int(w_lr // 2 * frac)
    x0, y0 = w_lr // 2 - dw, h_lr // 2 - dh
    if dw <= 0 or dh <= 0 or (W // 2 - dW, H // 2 - dH, 2 * dW, 2 * dH) != (x0 * s, y0 * s, 2 * dw * s, 2 * dh * s):
        raise ValueError(f"precrop_frac {frac} at img_wh {(W, H)}, downscale {s}: the reference's HR crop ({2 * dW} x {2 * dH} at "
                         f"({W // 2 - dW}, {H // 2 - dH})) and LR crop ({2 * dw} x {2 * dh} at ({x0}, {y0})) do not cover the same pixels")
    return x0, y0, 2 * dw, 2 * dh


class RaySet:
    """Poses + 8-bit images of a scene on the device; batches, epochs, regulariser patches and validation samples from them.

    poses        (n_views, 3, 4) camera-to-world matrices (any float array; kept as fp32, like ``torch.FloatTensor(pose)``)
    images_u8    n_views images (H0, W0, 3 | 4) uint8 -- numpy arrays or tensors of any source size, or one stacked array;
                 each is resized to ``img_wh`` and to ``img_wh / downscale`` with Pillow's 8-bit LANCZOS arithmetic on the
                 device.  4 channels: RGBA, targets blended onto white.  ``None``: poses only (a test path): ``view`` only.
    img_wh       HR size (W, H); downscale: s; focal: HR focal length (keyword, required)
    ndc, near, far   as for ``ops.subpixel_rays``
    ds_method    'lanc' (LR targets from the LANCZOS LR image) | 'avg' (mean of the s*s HR targets, ``F.avg_pool2d``)
    use_pixel_centers / unified_dir   the reference's direction options (models/utils.py:114, llff_downX_dataset.py:270-276)
    window       (x0, y0, w, h) in LR pixels: rows are numbered inside it (``precrop``); default the whole frame
    """

    def __init__(self, poses, images_u8, img_wh, downscale: int, ndc: bool, near: float = 0.0, far: float = 1.0, *, focal: float,
                 ds_method: str = "lanc", use_pixel_centers: bool = True, unified_dir: bool = False, window=None, device="cuda"):
        if ds_method not in ("lanc", "avg"):
            raise ValueError("Downscale option not found: ds_method must be 'lanc' or 'avg'")
        self.device = torch.device(device)
        _check_device(self.device, "device")
        self.img_wh = (int(img_wh[0]), int(img_wh[1]))
        self.downscale = int(downscale)
        W, H = self.img_wh
        s = self.downscale
        if s <= 0 or W <= 0 or H <= 0 or W % s or H % s:
            raise ValueError(f"img_wh {self.img_wh} must be positive multiples of downscale {s}")
        self.focal, self.ndc, self.near, self.far = float(focal), bool(ndc), float(near), float(far)
        self.ds_method = ds_method
        self.options = (0 if use_pixel_centers else _lib.NSR_RAYS_NO_PIXEL_CENTERS) | (_lib.NSR_RAYS_UNIFIED_DIR if unified_dir else 0)
        p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64)[..., :3, :4].astype(np.float32).reshape(-1, 12))
        self.poses_host = p.reshape(-1, 3, 4)
        self.poses = torch.from_numpy(p).to(self.device)
        self.hr = self.lr = None
        if images_u8 is not None:
            if len(images_u8) != len(p):
                raise ValueError(f"{len(p)} poses but {len(images_u8)} images")
            hr, lr = [], []
            for img in images_u8:
                img = torch.as_tensor(np.ascontiguousarray(img) if isinstance(img, np.ndarray) else img).to(self.device)
                if img.dtype != torch.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4):
                    raise TypeError("images must be (H, W, 3) RGB or (H, W, 4) RGBA uint8")
                hr.append(nsr_io.resize_lanczos_u8(img, (W, H)))
                if ds_method == "lanc":
                    lr.append(nsr_io.resize_lanczos_u8(hr[-1], (W // s, H // s)))
            if len({int(t.shape[2]) for t in hr}) != 1:
                raise ValueError("all images must have the same number of channels")
            self.hr = torch.stack(hr).contiguous()
            self.lr = torch.stack(lr).contiguous() if lr else None
        self.window = (0, 0, W // s, H // s) if window is None else tuple(int(v) for v in window)
        x0, y0, w, h = self.window
        if x0 < 0 or y0 < 0 or w <= 0 or h <= 0 or x0 + w > W // s or y0 + h > H // s:
            raise ValueError(f"window {self.window} is outside the LR frame {(W // s, H // s)}")
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._descs: Dict[tuple, _lib.NsrRayset] = {}

    # -------------------------------------------------------------------------------------------- sizes
    @property
    def n_views(self) -> int:
        return int(self.poses.shape[0])

    @property
    def channels(self) -> int:
        return 0 if self.hr is None else int(self.hr.shape[3])

    def __len__(self) -> int:
        return self.n_views * self.window[2] * self.window[3]

    def resident_bytes(self) -> int:
        """Device bytes the set keeps: poses + 8-bit images (the reference: 44 B per HR pixel + 12 B per LR pixel of fp32)."""
        return sum(t.numel() * t.element_size() for t in (self.poses, self.hr, self.lr) if t is not None)

    # -------------------------------------------------------------------------------------------- the launch
    def _desc(self, window=None, lr_mode=None, patch_w=0) -> _lib.NsrRayset:
        if self.hr is None:
            raise ValueError("this RaySet holds poses only (a test path): it has no targets to batch")
        x0, y0, w, h = self.window if window is None else window
        if lr_mode is None:
            lr_mode = _lib.NSR_LR_FROM_IMAGES if self.ds_method == "lanc" else _lib.NSR_LR_MEAN_OF_HR
        key = (x0, y0, w, h, lr_mode, int(patch_w))
        if key not in self._descs:       # a handful of distinct descriptors per set: built once
            self._descs[key] = self._make_desc(*key)
        return self._descs[key]

    def _make_desc(self, x0, y0, w, h, lr_mode, patch_w) -> _lib.NsrRayset:
        W, H = self.img_wh
        return _lib.NsrRayset(poses=self.poses.data_ptr(), n_views=self.n_views, H=H, W=W, s=self.downscale, focal=self.focal,
                              ndc=int(self.ndc), near_=self.near, far_=self.far, options=self.options, x0=x0, y0=y0, w=w, h=h,
                              hr=self.hr.data_ptr(), lr=0 if self.lr is None else self.lr.data_ptr(), C=self.channels,
                              lr_mode=lr_mode, patch_w=int(patch_w))

    def _index(self, idx) -> torch.Tensor:
        idx = torch.as_tensor(idx, device=self.device) if not isinstance(idx, torch.Tensor) else idx
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise TypeError("indices must be integers")
        _check_device(idx.device, "idx")
        return idx.to(torch.int64).reshape(-1).contiguous()

    def _launch(self, idx, layout=0, want=("rays", "rgbs", "rgbs_ori"), **desc_kw) -> Dict[str, torch.Tensor]:
        idx = self._index(idx)
        B, s = int(idx.numel()), self.downscale
        d = self._desc(**desc_kw)
        out = {}
        if layout == 1:
            side_h, side_w = (B // d.patch_w) * s, d.patch_w * s
            shapes = {"rays": (side_h, side_w, 8), "rgbs": (B, 3), "rgbs_ori": (side_h, side_w, 3)}
        else:
            shapes = {"rays": (B, s * s, 8), "rgbs": (B, 3), "rgbs_ori": (B, s * s, 3)}
        for k in want:
            out[k] = torch.empty(shapes[k], dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().nsr_rayset_batch(ctypes.byref(d), _p(idx), B, layout, _p(out.get("rays")), _p(out.get("rgbs")),
                                                _p(out.get("rgbs_ori")), _p(self._status), _stream()), "nsr_rayset_batch")
        return out

    # -------------------------------------------------------------------------------------------- training samples
    def batch(self, idx) -> Dict[str, torch.Tensor]:
        """The reference's training sample for the rows ``idx`` (llff_downX_dataset.py:407-410 after collation): ``rays``
        (B, s*s, 8), ``rgbs`` (B, 3), ``rgbs_ori`` (B, s*s, 3).  ``idx``: integer tensor on the device (or anything
        ``torch.as_tensor`` takes).  An index outside ``[0, len(self))`` yields zero rows and raises the INPUT_RANGE flag
        of ``status()``; it never reaches memory."""
        return self._launch(idx)

    def epoch(self, batch_size: int, generator: Optional[torch.Generator] = None, keep_last: bool = False) -> Iterator[Dict[str, torch.Tensor]]:
        """One shuffled pass (train.py:39, data/__init__.py:108-114: ``shuffle=True``, ``drop_last = not opt.keep_last``):
        a device ``torch.randperm`` cut into batches; the remainder is dropped unless ``keep_last``.  ``generator``: a
        generator of this set's device (``torch.Generator(device=...)``) for reproducible epochs."""
        batch_size = int(batch_size)
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        perm = torch.randperm(len(self), device=self.device, generator=generator)
        end = len(self) if keep_last else len(self) - len(self) % batch_size
        for lo in range(0, end, batch_size):
            yield self.batch(perm[lo:min(lo + batch_size, end)])

    def n_patches(self, length: int) -> int:
        _, _, w, h = self.window
        return max(w - length + 1, 0) * max(h - length + 1, 0) * self.n_views

    def patch(self, view: int, row: int, col: int, length: int) -> Dict[str, torch.Tensor]:
        """The `reg_patch` sample (llff_downX_dataset.py:422-436) of the ``length`` x ``length`` LR pixels whose corner is
        (row, col) of ``view``: ``patch_rays`` as the HR raster (length*s, length*s, 8) -- what ``Trainer.regularize_patch``
        takes -- and ``patch_rgbs`` (length^2, 3)."""
        _, _, w, h = self.window
        view, row, col, length = int(view), int(row), int(col), int(length)
        if length <= 0 or not (0 <= view < self.n_views and 0 <= row <= h - length and 0 <= col <= w - length):
            raise ValueError(f"patch ({view}, {row}, {col}) of length {length} is outside the set ({self.n_views} views of {w} x {h})")
        ar = torch.arange(length, device=self.device)
        idx = view * w * h + (row + ar)[:, None] * w + (col + ar)[None, :]
        out = self._launch(idx, layout=1, want=("rays", "rgbs"), patch_w=length)
        return {"patch_rays": out["rays"], "patch_rgbs": out["rgbs"]}

    def random_patch(self, length: int, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """``patch`` at a location drawn like the reference does (one ``torch.randint(n_patches)`` on the host, decoded
        image-major, then row-major over the valid corners)."""
        _, _, w, h = self.window
        n = self.n_patches(length)
        if n <= 0:
            raise ValueError(f"no {length} x {length} patch fits into a {w} x {h} window")
        i = int(torch.randint(high=n, size=(1,), generator=generator)[0].item())
        per_img, per_row = n // self.n_views, w - length + 1
        return self.patch(i // per_img, (i % per_img) // per_row, (i % per_img) % per_row, length)

    # -------------------------------------------------------------------------------------------- validation sample
    def view_rays(self, i: int) -> torch.Tensor:
        """(H/s * W/s, s*s, 8): the whole frame of view ``i`` with this set's direction options (``nsr_gen_rays_opt``)."""
        W, H = self.img_wh
        s = self.downscale
        n = (H // s) * (W // s)
        rays = torch.empty(n, s * s, 8, dtype=torch.float32, device=self.device)
        c = np.ascontiguousarray(self.poses_host[int(i)].reshape(12))
        _lib.check(_lib.load().nsr_gen_rays_opt(c.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), H, W, self.focal, s, int(self.ndc),
                                                self.near, self.far, self.options, 0, n, _p(rays), _stream()), "nsr_gen_rays_opt")
        return rays

    def view(self, i: int) -> Dict[str, torch.Tensor]:
        """The validation sample of view ``i`` (llff_downX_dataset.py:466-509, blender_downX_dataset.py:180-223), whole frame
        whatever the window: ``rays`` (N_lr, s*s, 8), ``rays_ori`` (H*W, 8) in HR raster order, ``c2w`` (3, 4); with
        images ``rgbs`` (N_lr, 3) and ``rgbs_ori`` (N_lr, s*s, 3).  RGB sets: ``rgbs`` is the pooled HR image whatever
        ``ds_method`` is, as the LLFF dataset does; RGBA sets follow ``ds_method`` like the Blender dataset and add the
        alpha > 0 masks ``valid_mask`` (N_lr,) and ``valid_mask_ori`` (H*W,).  Feeds ``NeRFDownXModel.validate([...])``."""
        from .ops import unflatten_reshape
        i = int(i)
        if not 0 <= i < self.n_views:
            raise IndexError(f"view {i} of {self.n_views}")
        W, H = self.img_wh
        s = self.downscale
        rays = self.view_rays(i)
        out = {"rays": rays, "rays_ori": unflatten_reshape(rays.view(-1, 8), self.img_wh, s).reshape(H * W, 8),
               "c2w": self.poses[i].view(3, 4).clone()}      # the device copy of poses_host[i]: no host staging
        if self.hr is None:
            return out
        n = (H // s) * (W // s)
        rgba = self.channels == 4
        mode = _lib.NSR_LR_MEAN_OF_HR if (not rgba or self.ds_method == "avg") else _lib.NSR_LR_FROM_IMAGES
        t = self._launch(torch.arange(i * n, (i + 1) * n, device=self.device), want=("rgbs", "rgbs_ori"), window=(0, 0, W // s, H // s),
                         lr_mode=mode)
        out.update(t)
        if rgba:
            alpha = self.hr[i, :, :, 3]
            out["valid_mask_ori"] = (alpha > 0).reshape(-1)
            if mode == _lib.NSR_LR_FROM_IMAGES:
                out["valid_mask"] = (self.lr[i, :, :, 3] > 0).reshape(-1)
            else:       # the pooled alpha is positive exactly where one of its s*s bytes is
                out["valid_mask"] = (alpha.view(H // s, s, W // s, s) > 0).any(3).any(1).reshape(-1)
        return out

    # -------------------------------------------------------------------------------------------- windows, status
    def _share(self, window) -> "RaySet":
        other = object.__new__(RaySet)
        other.__dict__.update(self.__dict__)
        other.window = tuple(int(v) for v in window)
        return other

    def precrop(self, frac: float) -> "RaySet":
        """The `train_crop` set (``--precrop_frac``): the same poses and images (shared storage and status word), rows
        numbered inside the centre window of ``crop_window``."""
        return self._share(crop_window(self.img_wh, self.downscale, frac))

    def status(self, clear: bool = False) -> int:
        """Sticky status word of the batches (``NSR_FLAG_INPUT_RANGE``: an index was outside the set).  Waits for the stream."""
        flags = int(self._status.item()) & 0xFFFFFFFF
        if clear:
            self._status.zero_()
        return flags

    # -------------------------------------------------------------------------------------------- scenes on disk
    @staticmethod
    def _decode(path: str, mode: Optional[str]) -> np.ndarray:
        from PIL import Image       # file decoding only (like the reference); every resize runs on the device
        with Image.open(path) as im:
            im = im.convert(mode) if mode else im
            return np.asarray(im, dtype=np.uint8).copy()

    @classmethod
    def from_llff(cls, root: str, img_wh, downscale: int, split: str = "train", include_var: bool = False, spheric_poses: bool = False,
                  n_test_poses: int = 120, **kw) -> "RaySet":
        """An LLFF scene directory (``images/``, ``sparse/0/*.bin``) the way ``LLFFDownXDataset`` reads it.  split: 'train'
        (every view but the validation view, unless ``include_var``), 'val' (the validation view alone: ``view(0)``),
        'test_train' (every view), 'test' (poses only: the spiral / spheric path).  Forward-facing scenes use NDC rays;
        ``spheric_poses`` uses near = ``bounds.min()``, far = ``min(8 * near, bounds.max())``."""
        if split not in ("train", "reg_patch", "val", "test_train", "test"):
            raise ValueError(f"split {split!r} is not built (the `gan` split is out of scope)")
        scene = nsr_io.llff_scene_from_colmap(os.path.join(root, "sparse", "0"), int(img_wh[0]))
        poses, bounds, val = scene["poses"], scene["bounds"], scene["val_idx"]
        near, far = (float(bounds.min()), float(min(8 * bounds.min(), bounds.max()))) if spheric_poses else (0.0, 1.0)
        if split == "test":
            path = nsr_io.spheric_path(1.1 * bounds.min(), n_test_poses) if spheric_poses else \
                nsr_io.spiral_path(np.percentile(np.abs(poses[..., 3]), 90, axis=0), 3.5, n_test_poses)
            return cls(path, None, img_wh, downscale, not spheric_poses, near, far, focal=scene["focal"], **kw)
        if split == "val":
            views = [val]
        elif split == "test_train" or include_var:
            views = list(range(len(poses)))
        else:
            views = [i for i in range(len(poses)) if i != val]
        images = [cls._decode(os.path.join(root, "images", scene["names"][i]), "RGB") for i in views]
        return cls(poses[views], images, img_wh, downscale, not spheric_poses, near, far, focal=scene["focal"], **kw)

    @classmethod
    def from_blender(cls, root: str, img_wh, downscale: int, split: str = "train", precrop_frac: float = 0.5, **kw) -> "RaySet":
        """A Blender scene directory (``transforms_{split}.json`` + RGBA PNGs) the way ``BlenderDownXDataset`` reads it:
        near / far 2 / 6, no NDC, targets blended onto white.  split 'train_crop' is 'train' + ``precrop(precrop_frac)``."""
        if int(img_wh[0]) != int(img_wh[1]):
            raise ValueError("image width must equal image height!")
        name = "train" if split == "train_crop" else split
        meta = nsr_io.load_blender_transforms(os.path.join(root, f"transforms_{name}.json"), int(img_wh[0]))
        images = [cls._decode(os.path.join(root, f"{f}.png"), None) for f in meta["files"]]
        if any(im.ndim != 3 or im.shape[2] != 4 for im in images):
            raise ValueError("Blender scenes hold RGBA images")
        rs = cls(meta["poses"], images, img_wh, downscale, False, meta["near"], meta["far"], focal=meta["focal"], **kw)
        return rs.precrop(precrop_frac) if split == "train_crop" else rs
