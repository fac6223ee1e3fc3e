"""Host mirror of the reference's refinement network over ``include/nsr_refine.h``.

``MaxPoolingModel`` mirrors ``models/networks.py:945-990`` in eval mode: ``forward(x_synth, list_x_candi)`` with
``x_synth`` (B, 3, H, W) and ``list_x_candi`` (B, R, 3, H, W) in [-1, 1] -> refined patch (B, 3, H, W) (tanh).
Weights enter as the reference's ``state_dict`` (``load_state_dict``; the int64 ``num_batches_tracked`` entries are
ignored).  All arithmetic runs in libnsr.so; there is no CPU path.

Training (fp32, with reference patches): ``forward_train`` is the train-mode network as a ``torch.autograd.Function``
over the 72 parameter tensors, ``RefineTrainer`` mirrors ``RefineModel``'s protocol (models/refine_model.py:84-175:
L1 / MSE loss, Adam) on top of it.
"""
from __future__ import annotations

from collections import OrderedDict
import ctypes
from ctypes import c_void_p
from typing import Dict, Optional

import numpy as np
import torch

from torch.autograd.function import once_differentiable

from . import _lib
from .ops import _check_device, _f32, _i32, _p, _stream

# (name, cin, cout, stride, batch-norm name or None) in forward = state_dict order
LAYERS = [
    ("E.conv1", 3, 128, None), ("E.conv2", 128, 128, "E.conv2_bnorm"), ("E.conv3", 128, 256, "E.conv3_bnorm"),
    ("E.conv4", 256, 256, "E.conv4_bnorm"), ("E.conv5", 256, 512, "E.conv5_bnorm"), ("E.conv6", 512, 512, "E.conv6_bnorm"),
    ("E.conv7", 512, 512, "E.conv7_bnorm"),
    ("D.conv1", 1024, 512, "D.conv1_bnorm"), ("D.conv2", 512, 512, "D.conv2_bnorm"), ("D.conv2_up", 512, 512, "D.conv2_up_bnorm"),
    ("D.conv3", 1536, 512, "D.conv3_bnorm"), ("D.conv4", 512, 512, "D.conv4_bnorm"), ("D.conv4_up", 512, 256, "D.conv4_up_bnorm"),
    ("D.conv5", 768, 256, "D.conv5_bnorm"), ("D.conv6", 256, 256, "D.conv6_bnorm"), ("D.conv6_up", 256, 128, "D.conv6_up_bnorm"),
    ("D.conv7", 384, 128, "D.conv7_bnorm"), ("D.conv8", 128, 128, "D.conv8_bnorm"), ("D.conv9", 128, 3, None),
]


# --not_use_ref (Model_VNPCAT_Decoder_NoPooling, networks.py:866-945): the decoder's concatenations carry no F_max_i
# channels, so four convolutions are narrower
NOREF_CIN = {"D.conv1": 512, "D.conv3": 1024, "D.conv5": 512, "D.conv7": 256}


def _refine_spec(not_use_ref: bool = False) -> "OrderedDict[str, tuple]":
    s = OrderedDict()
    for name, cin, cout, bn in LAYERS:
        if not_use_ref:
            cin = NOREF_CIN.get(name, cin)
        s[f"{name}.weight"] = (cout, cin, 3, 3)
        s[f"{name}.bias"] = (cout,)
        if bn:
            for k in ("weight", "bias", "running_mean", "running_var"):
                s[f"{bn}.{k}"] = (cout,)
    return s


#: the 106 float tensors of MaxPoolingModel.state_dict(), in order (and with --not_use_ref)
REFINE_SPEC = _refine_spec()
REFINE_SPEC_NOREF = _refine_spec(True)
assert len(REFINE_SPEC) == 106 and len(REFINE_SPEC_NOREF) == 106
#: the 72 trainable tensors (per layer: conv weight, bias, then the BatchNorm's weight, bias) and the 34 running-statistics
#: tensors (state, not parameters), both in state_dict order
TRAIN_PARAM_KEYS = [k for k in REFINE_SPEC if "running_" not in k]
RUNNING_KEYS = [k for k in REFINE_SPEC if "running_" in k]
assert len(TRAIN_PARAM_KEYS) == 72 and len(RUNNING_KEYS) == 34


def make_refine_state_dict(seed: int, not_use_ref: bool = False) -> Dict[str, np.ndarray]:
    """Deterministic synthetic weights (no checkpoint can be downloaded): xavier-normal convolutions
    (``initialize_weight``, networks.py:776-783), BatchNorm weight ~ N(1, 0.02), and NON-trivial running statistics
    (mean ~ N(0, 0.1), var ~ U(0.5, 1.5)) and biases so that the folded affine map is exercised."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k, shape in (REFINE_SPEC_NOREF if not_use_ref else REFINE_SPEC).items():
        if k.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif k.endswith("running_mean"):
            v = rng.normal(0.0, 0.1, shape)
        elif len(shape) == 4:
            fan_in, fan_out = shape[1] * 9, shape[0] * 9
            v = rng.normal(0.0, np.sqrt(2.0 / (fan_in + fan_out)), shape)
        elif "bnorm.weight" in k:
            v = rng.normal(1.0, 0.02, shape)
        else:
            v = rng.normal(0.0, 0.05, shape)
        sd[k] = v.astype(np.float32)
    return sd


def refine_macs(H: int = 64, W: int = 64, R: int = 8) -> int:
    """True convolution MACs of one forward on a (H, W) patch with R reference patches (networks.py:735-990):
    the encoder runs on 1 + R images, the decoder once; no padding or im2col overhead counted."""
    px = [H * W, H * W // 4, H * W // 16, H * W // 64]
    enc_level = [0, 0, 1, 1, 2, 2, 3]
    dec_level = [3, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0, 0]
    m = 0
    for i, (_, cin, cout, _bn) in enumerate(LAYERS[:7]):
        m += (1 + R) * px[enc_level[i]] * 9 * cin * cout
    for i, (_, cin, cout, _bn) in enumerate(LAYERS[7:]):
        m += px[dec_level[i]] * 9 * cin * cout
    return m


class MaxPoolingModel:
    """Encoder + max over the reference patches + decoder, eval mode (BatchNorm uses its running statistics).
    ``opt.not_use_ref`` (or ``not_use_ref=True``) selects the reference's no-pooling decoder: the encoder runs on the
    synthesised patch only and ``forward`` ignores ``list_x_candi`` (networks.py:958-969)."""

    def __init__(self, opt=None, precision: str = "f16x3", device="cuda", not_use_ref: bool = False):
        self.not_use_ref = bool(not_use_ref or (opt is not None and getattr(opt, "not_use_ref", False)))
        if precision not in ("fp32", "f16x3"):
            raise ValueError("precision must be 'fp32' or 'f16x3'")
        self.precision, self._prec = precision, _lib.PRECISIONS[precision]
        self.device = torch.device(device)
        self.spec = REFINE_SPEC_NOREF if self.not_use_ref else REFINE_SPEC
        lib = _lib.load()
        nbytes = (lib.nsr_refine_packed_bytes_noref if self.not_use_ref else lib.nsr_refine_packed_bytes)(self._prec)
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._loaded = False
        self._ws = None

    def load_state_dict(self, sd):
        missing = [k for k in self.spec if k not in sd]
        if missing:
            raise KeyError(f"state_dict lacks {missing[:3]}{'...' if len(missing) > 3 else ''}")
        dev = []
        for k, shape in self.spec.items():
            v = sd[k]
            v = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach()
            if tuple(v.shape) != tuple(shape):
                raise ValueError(f"{k}: expected shape {shape}, got {tuple(v.shape)}")
            dev.append(v.to(device=self.device, dtype=torch.float32).contiguous())
        ptrs = (c_void_p * len(dev))(*[c_void_p(t.data_ptr()) for t in dev])
        pack = _lib.load().nsr_refine_pack_weights_noref if self.not_use_ref else _lib.load().nsr_refine_pack_weights
        # enqueue only: `dev` may be dropped here -- torch's allocator hands a freed block to later work of this stream alone,
        # which runs behind the pack kernels
        _lib.check(pack(ptrs, _p(self.packed), self._prec, _stream()), "nsr_refine_pack_weights")
        self._loaded = True
        return self

    def eval(self):
        return self

    def forward(self, x_synth: torch.Tensor, list_x_candi: torch.Tensor = None) -> torch.Tensor:
        if not self._loaded:
            raise RuntimeError("MaxPoolingModel.forward called before load_state_dict")
        if self.not_use_ref:
            return self._forward_noref(_f32(x_synth, "x_synth"))
        x, c = _f32(x_synth, "x_synth"), _f32(list_x_candi, "list_x_candi")
        if x.ndim != 4 or x.shape[1] != 3 or c.ndim != 5 or c.shape[0] != x.shape[0] or tuple(c.shape[2:]) != tuple(x.shape[1:]):
            raise ValueError("expected x_synth (B, 3, H, W) and list_x_candi (B, R, 3, H, W)")
        B, _, H, W = x.shape
        R = c.shape[1]
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        lib = _lib.load()
        need = lib.nsr_refine_workspace_bytes_for(self._prec, B, R, H, W)
        if need == 0:
            raise ValueError("H and W must be positive multiples of 8 and R >= 1")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        _lib.check(lib.nsr_refine_forward(_p(self.packed), self._prec, _p(x), _p(c), B, R, H, W, _p(out), _p(self._ws), self._ws.numel(),
                                          _stream()), "nsr_refine_forward")
        return out

    def _forward_noref(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError("expected x_synth (B, 3, H, W)")
        B, _, H, W = x.shape
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        lib = _lib.load()
        need = lib.nsr_refine_workspace_bytes_for(self._prec, B, 1, H, W)
        if need == 0:
            raise ValueError("H and W must be positive multiples of 8")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        _lib.check(lib.nsr_refine_forward_noref(_p(self.packed), self._prec, _p(x), B, H, W, _p(out), _p(self._ws), self._ws.numel(),
                                                _stream()), "nsr_refine_forward_noref")
        return out

    __call__ = forward


# ------------------------------------------------------------------------------------------------ tiler / stitcher
def tile_refs(locs: torch.Tensor, patch_len: int = 64, num_ref_patches: int = 8):
    """locs (H, W, 3) float64 on the GPU (``nerf_sr_amd.warp.depth_warp`` / ``{i}_locs.npz``) -> ``starts`` (n, 2)
    int32 [x, y] of the SR tiles and ``ref_starts`` (n, num_ref_patches, 2) int32 of their reference patches (-1: use
    the SR tile), as ``LLFFRefineDataset.__getitem__`` picks them (data/llff_refine_dataset.py:303-329)."""
    if not locs.is_cuda or locs.dtype != torch.float64 or locs.ndim != 3 or locs.shape[2] != 3:
        raise ValueError("locs must be a (H, W, 3) float64 tensor on the GPU")
    _check_device(locs.device, "locs")
    locs = locs.detach().contiguous()
    H, W = locs.shape[:2]
    n = -(-W // patch_len) * -(-H // patch_len)
    starts = torch.empty(n, 2, dtype=torch.int32, device=locs.device)
    refs = torch.empty(n, num_ref_patches, 2, dtype=torch.int32, device=locs.device)
    _lib.check(_lib.load().nsr_refine_tile(_p(locs), H, W, patch_len, num_ref_patches, _p(starts), _p(refs), _stream()),
               "nsr_refine_tile")
    return starts, refs


def gather_patches(sr_img: torch.Tensor, ref_img: torch.Tensor, starts: torch.Tensor, ref_starts: torch.Tensor, patch_len: int = 64):
    """sr_img, ref_img (3, H, W) fp32 -> sr_patch (n, 3, p, p), ref_patches (n, R, 3, p, p) (the dataset's sample).
    ``starts`` (n, 2) / ``ref_starts`` (n, R, 2): integer tensors on the device, converted to the int32 the kernel reads
    (``tile_refs`` returns int32; ``torch.tensor([[0, 0]])`` is int64); a floating-point index raises ``TypeError``."""
    sr_img, ref_img = _f32(sr_img, "sr_img"), _f32(ref_img, "ref_img")
    starts, ref_starts = _i32(starts, "starts"), _i32(ref_starts, "ref_starts")
    if sr_img.ndim != 3 or sr_img.shape[0] != 3 or tuple(ref_img.shape) != tuple(sr_img.shape):
        raise ValueError(f"sr_img and ref_img must both be (3, H, W), got {tuple(sr_img.shape)} and {tuple(ref_img.shape)}")
    if starts.ndim != 2 or starts.shape[1] != 2 or ref_starts.ndim != 3 or ref_starts.shape[0] != starts.shape[0] \
            or ref_starts.shape[1] < 1 or ref_starts.shape[2] != 2:
        raise ValueError(f"starts must be (n, 2) and ref_starts (n, R >= 1, 2), got {tuple(starts.shape)} and {tuple(ref_starts.shape)}")
    _, H, W = sr_img.shape
    n, R = ref_starts.shape[:2]
    sr = torch.empty(n, 3, patch_len, patch_len, dtype=torch.float32, device=sr_img.device)
    ref = torch.empty(n, R, 3, patch_len, patch_len, dtype=torch.float32, device=sr_img.device)
    _lib.check(_lib.load().nsr_refine_gather(_p(sr_img), _p(ref_img), H, W, patch_len, R, _p(starts),
                                             _p(ref_starts), n, _p(sr), _p(ref), _stream()), "nsr_refine_gather")
    return sr, ref


def stitch_patches(patches: torch.Tensor, starts: torch.Tensor, img_wh) -> torch.Tensor:
    """Paste predictions (n, 3, p, p) fp32 back in tile order, later tiles overwrite earlier ones (models/refine_model.py:211-214).
    ``starts`` (n, 2): an integer tensor on the device, converted to int32 like ``gather_patches``' (``TypeError`` otherwise)."""
    patches, starts = _f32(patches, "patches"), _i32(starts, "starts")
    if patches.ndim != 4 or patches.shape[1] != 3 or patches.shape[2] != patches.shape[3]:
        raise ValueError(f"patches must be (n, 3, p, p), got {tuple(patches.shape)}")
    if tuple(starts.shape) != (patches.shape[0], 2):
        raise ValueError(f"starts must be (n, 2) with n = {patches.shape[0]} patches, got {tuple(starts.shape)}")
    W, H = int(img_wh[0]), int(img_wh[1])
    img = torch.empty(3, H, W, dtype=torch.float32, device=patches.device)
    _lib.check(_lib.load().nsr_refine_stitch(_p(patches), _p(starts), patches.shape[0], patches.shape[-1], H, W,
                                             _p(img), _stream()), "nsr_refine_stitch")
    return img


def refine_image(net: MaxPoolingModel, sr_img: torch.Tensor, ref_img: torch.Tensor, locs: torch.Tensor, patch_len: int = 64,
                 num_ref_patches: int = 8, batch: int = 256) -> torch.Tensor:
    """The refinement pass over one synthesised view (config #5 tail): tile -> network on batches of tiles -> stitch.
    Images are (3, H, W) in [-1, 1] (the dataset's Normalize(0.5, 0.5)); returns the refined (3, H, W) image.
    ``batch``: tiles per network call.  The default takes the 169 tiles of an 800 x 800 frame in ONE call (3.5 GB of
    activations): the 8 x 8-pixel decoder layers of a 32-tile batch fill an eighth of the chip (57 vs 45 ms per frame)."""
    sr_img, ref_img = _f32(sr_img, "sr_img"), _f32(ref_img, "ref_img")
    if sr_img.ndim != 3 or sr_img.shape[0] != 3 or tuple(ref_img.shape) != tuple(sr_img.shape):
        raise ValueError(f"sr_img and ref_img must both be (3, H, W), got {tuple(sr_img.shape)} and {tuple(ref_img.shape)}")
    if not isinstance(locs, torch.Tensor) or tuple(locs.shape) != (sr_img.shape[1], sr_img.shape[2], 3):
        raise ValueError(f"locs must be (H, W, 3) for images of {sr_img.shape[1]} x {sr_img.shape[2]}, got {tuple(getattr(locs, 'shape', ()))}")
    starts, refs = tile_refs(locs, patch_len, num_ref_patches)
    sr, ref = gather_patches(sr_img, ref_img, starts, refs, patch_len)
    pred = torch.cat([net(sr[i:i + batch], ref[i:i + batch]) for i in range(0, sr.shape[0], batch)], 0)
    return stitch_patches(pred, starts, (sr_img.shape[2], sr_img.shape[1]))


def evaluate_image(net: MaxPoolingModel, sr_img: torch.Tensor, ref_img: torch.Tensor, locs: torch.Tensor, gt_img: torch.Tensor,
                   patch_len: int = 64, num_ref_patches: int = 8, batch: int = 256) -> Dict[str, torch.Tensor]:
    """``refine_image``, then the scores of ``RefineModel.test`` / ``validate`` (models/refine_model.py:225-226): the SSIM of
    the SR frame and of the refined frame against ``gt_img`` on the (1, 3, H, W) frames with ``data_range=(-1, 1)``, and a
    PSNR beside each.  Returns ``refined`` (3, H, W) and ``psnr_input``, ``psnr_refine``, ``ssim_input``, ``ssim_refine`` as
    0-d device tensors (no host read here)."""
    from . import metrics
    gt = _f32(gt_img, "gt_img")
    if tuple(gt.shape) != tuple(sr_img.shape):
        raise ValueError(f"gt_img must have the SR image's shape {tuple(sr_img.shape)}, got {tuple(gt.shape)}")
    refined = refine_image(net, sr_img, ref_img, locs, patch_len, num_ref_patches, batch)
    sr = _f32(sr_img, "sr_img")
    ssim, psnr = metrics.SSIM(data_range=(-1, 1)), metrics.PSNR()
    with torch.no_grad():       # scores, not losses: an image that requires grad does not make them differentiable
        return {"refined": refined,
                "psnr_input": psnr(sr, gt), "psnr_refine": psnr(refined, gt),
                "ssim_input": ssim(sr.unsqueeze(0), gt.unsqueeze(0)), "ssim_refine": ssim(refined.unsqueeze(0), gt.unsqueeze(0))}


# ------------------------------------------------------------------------------------------------------- training
_TRAIN_WS: Dict[torch.device, torch.Tensor] = {}     # scratch of the train-mode pair, one per device (grows, never shrinks)


def _train_workspace(need: int, dev) -> torch.Tensor:
    ws = _TRAIN_WS.get(dev)
    if ws is None or ws.numel() < need:
        _TRAIN_WS[dev] = ws = None                   # free the old one first
        _TRAIN_WS[dev] = ws = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def _ptr_array(tensors):
    return (c_void_p * len(tensors))(*[c_void_p(t.data_ptr()) for t in tensors])


# training precisions: name -> the `precision` of nsr_refine_train_forward_p / _backward_p.  "f16x3_mixed": forward and input
# gradients split-fp16; the route of the weight gradients is an option of its own (WEIGHT_GRADS below), so the short name "f16x3"
# is no precision here and keeps raising
TRAIN_PRECISIONS = {"fp32": _lib.NSR_FP32, "f16x3_mixed": _lib.NSR_F16X3}


def _train_precision(precision, who: str) -> int:
    if precision not in TRAIN_PRECISIONS:
        raise ValueError(f"{who}: precision must be 'fp32' or 'f16x3_mixed' (got {precision!r}): the refinement network trains in "
                         "fp32, or with the forward and the input gradients on the split-fp16 MFMA and fp32 weight gradients")
    return TRAIN_PRECISIONS[precision]


# weight-gradient routes: name -> the `weight_grad` of nsr_refine_train_backward_w; independent of `precision`.  "f16x3": every
# weight gradient but E.conv1's as one implicit split-fp16 GEMM per site (three terms per product), no col matrix
WEIGHT_GRADS = {"fp32": _lib.NSR_FP32, "f16x3": _lib.NSR_F16X3}


def _weight_grad(weight_grad, who: str) -> int:
    if not isinstance(weight_grad, str) or weight_grad not in WEIGHT_GRADS:
        raise ValueError(f"{who}: weight_grad must be 'fp32' or 'f16x3' (got {weight_grad!r}): the weight gradients run as im2col + "
                         "fp32 GEMM, or as one implicit split-fp16 GEMM per layer")
    return WEIGHT_GRADS[weight_grad]


class _TrainRun:
    """The arguments of one forward_train call that are not differentiable tensors."""

    def __init__(self, running, momentum, img_chunk, precision=_lib.NSR_FP32, weight_grad=_lib.NSR_FP32):
        self.running, self.momentum, self.img_chunk, self.precision = running, momentum, img_chunk, precision
        self.weight_grad = weight_grad

    def tensors106(self, params):
        by_name = dict(zip(TRAIN_PARAM_KEYS, params))
        by_name.update(zip(RUNNING_KEYS, self.running))
        return _ptr_array([by_name[k] for k in REFINE_SPEC])


class _ForwardTrain(torch.autograd.Function):
    """Output: the refined patches (B, 3, H, W).  Inputs: the run, the two image tensors, the 72 parameter tensors."""

    @staticmethod
    def forward(ctx, run, x, c, *params):
        lib = _lib.load()
        B, _, H, W = x.shape
        R = c.shape[1]
        nbytes = lib.nsr_refine_train_saved_bytes(B, R, H, W)
        if nbytes == 0:
            raise ValueError(f"forward_train: no train-mode network for B={B}, R={R}, {H} x {W}: H and W must be multiples of 8, "
                             "1 <= R <= 255 and B * H * W / 64 >= 2 (a BatchNorm needs two values per channel)")
        ctx.ws_need = lib.nsr_refine_train_workspace_bytes(B, R, H, W, run.img_chunk)
        ws = _train_workspace(ctx.ws_need, x.device)
        saved = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
        _lib.check(lib.nsr_refine_train_forward_p(run.precision, run.tensors106(params), _ptr_array(run.running), run.momentum, _p(x),
                                                  _p(c), B, R, H, W, run.img_chunk, _p(out), _p(ws), ws.numel(), _p(saved),
                                                  saved.numel(), _stream()), "nsr_refine_train_forward_p")
        ctx.save_for_backward(*params)       # an in-place update of a weight before the backward fails autograd's version check
        ctx.run, ctx.state = run, saved
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        params, saved = ctx.saved_tensors, ctx.state
        if saved is None:
            raise RuntimeError("forward_train: the saved state of this forward was released by its first backward")
        grads = [torch.empty_like(p) for p in params]
        ws = _train_workspace(ctx.ws_need, saved.device)
        g_out = g_out.to(torch.float32).contiguous()
        _lib.check(_lib.load().nsr_refine_train_backward_w(ctx.run.precision, ctx.run.weight_grad, ctx.run.tensors106(params), _p(g_out),
                                                           _ptr_array(grads), _p(ws), ws.numel(), _p(saved), saved.numel(), _stream()),
                   "nsr_refine_train_backward_w")
        ctx.state = None
        return (None, None, None) + tuple(grads)


def forward_train(params, running, x_synth: torch.Tensor, list_x_candi: torch.Tensor, momentum: float = 0.1,
                  img_chunk: Optional[int] = None, precision: str = "fp32", *, weight_grad: str = "fp32") -> torch.Tensor:
    """``MaxPoolingModel.forward`` in train mode (networks.py:964-990 under ``.train()``): BatchNorm normalises with the batch
    statistics of each call (the encoder's two calls each with their own), fp32.  ``params``: name -> CUDA fp32 leaf for the 72
    ``TRAIN_PARAM_KEYS``; ``running``: name -> tensor for the 34 ``RUNNING_KEYS``, updated IN PLACE (momentum; the encoder's
    twice).  Returns ``y`` (B, 3, H, W); any loss written in torch over it back-propagates through ``nsr_refine_train_backward``
    into the 72 parameters (once: the backward is not differentiable).  The 17 convolution biases in front of a BatchNorm get
    exact-zero gradients (include/nsr_refine.h).  There is no gradient with respect to the images (None).
    ``img_chunk``: images whose im2col matrix is live at once (None: the library picks).
    ``precision``: ``"fp32"``, or ``"f16x3_mixed"`` -- the forward convolutions and the input gradients on the split-fp16 MFMA
    with implicit gather, BatchNorm and the weight gradients fp32 (include/nsr_refine.h, nsr_refine_train_forward_p).
    ``weight_grad`` (independent of ``precision``): ``"fp32"`` -- im2col + fp32 GEMM --, or ``"f16x3"`` -- the weight gradient of
    every layer but E.conv1 as one implicit split-fp16 GEMM per site, three terms per product, bit-identical from call to call
    and independent of ``img_chunk`` (include/nsr_refine.h, nsr_refine_train_backward_w)."""
    prec = _train_precision(precision, "forward_train")
    wgrad = _weight_grad(weight_grad, "forward_train")
    missing = [k for k in TRAIN_PARAM_KEYS if k not in params] + [k for k in RUNNING_KEYS if k not in running]
    if missing:
        raise KeyError(f"forward_train: missing {missing[:3]}{'...' if len(missing) > 3 else ''}")
    x, c = _f32(x_synth.detach(), "x_synth"), _f32(list_x_candi.detach(), "list_x_candi")
    if x.ndim != 4 or x.shape[1] != 3 or c.ndim != 5 or c.shape[0] != x.shape[0] or tuple(c.shape[2:]) != tuple(x.shape[1:]):
        raise ValueError("expected x_synth (B, 3, H, W) and list_x_candi (B, R, 3, H, W)")
    ps, rs = [params[k] for k in TRAIN_PARAM_KEYS], [running[k] for k in RUNNING_KEYS]
    for k, t in list(zip(TRAIN_PARAM_KEYS, ps)) + list(zip(RUNNING_KEYS, rs)):
        if not isinstance(t, torch.Tensor) or t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous() \
                or tuple(t.shape) != tuple(REFINE_SPEC[k]) or t.data_ptr() % 16:
            # 16-byte aligned: the BatchNorm kernels read the per-channel vectors four floats at a time
            raise ValueError(f"forward_train: {k} must be a contiguous, 16-byte aligned float32 tensor of shape {REFINE_SPEC[k]} on {x.device}")
    run = _TrainRun(rs, float(momentum), 0 if img_chunk is None else int(img_chunk), prec, wgrad)
    return _ForwardTrain.apply(run, x, c, *ps)


class RefineTrainer:
    """``RefineModel``'s training protocol (models/refine_model.py:84-175) for the ``MaxPoolingModel`` with reference patches,
    fp32 (or ``precision="f16x3_mixed"`` and / or ``weight_grad="f16x3"``, see ``forward_train``): ``set_input`` -> ``forward`` -> ``calculate_losses`` -> ``backward`` -> ``optimizer_step`` (``optimize_parameters``
    does the four), Adam(lr, betas=(beta1, 0.999)) over the 72 parameters.  ``sd``: the reference's ``state_dict`` (tensors or
    arrays).  ``refine_with_ssim`` / ``lambda_refine_ssim`` are this build's addition, not the reference's: they add
    ``lambda_refine_ssim * (1 - SSIM(data_range=(-1, 1))(pred, gt_patch))`` -- the score ``evaluate_image`` reports, as a loss --
    to ``loss_tot`` (``metrics.SSIM`` under autograd; patches must be larger than the window's padding, 5 pixels).  Other
    losses are not built in: compose them in torch over ``forward_train``."""

    def __init__(self, sd, lr: float = 5e-4, beta1: float = 0.9, refine_with_l1: bool = True, refine_with_mse: bool = False,
                 lambda_refine_l1: float = 1.0, lambda_refine_mse: float = 10.0, device="cuda", *, refine_with_vgg: bool = False,
                 refine_with_grad: bool = False, refine_as_gan: bool = False, precision: str = "fp32", not_use_ref: bool = False,
                 momentum: float = 0.1, img_chunk: Optional[int] = None, beta2: float = 0.999, eps: float = 1e-8,
                 refine_with_ssim: bool = False, lambda_refine_ssim: float = 1.0, weight_grad: str = "fp32"):
        # every option is checked before a device is touched
        for name, on in (("refine_with_vgg", refine_with_vgg), ("refine_with_grad", refine_with_grad), ("refine_as_gan", refine_as_gan)):
            if on:
                raise NotImplementedError(f"RefineTrainer: {name} is not built in; compose that loss in torch over "
                                          "nerf_sr_amd.refine.forward_train, which back-propagates any torch loss")
        _train_precision(precision, "RefineTrainer")
        _weight_grad(weight_grad, "RefineTrainer")
        if not_use_ref:
            raise NotImplementedError("RefineTrainer: --not_use_ref training is not supported (inference is: MaxPoolingModel(not_use_ref=True))")
        if not (refine_with_l1 or refine_with_mse or refine_with_ssim):
            raise ValueError("RefineTrainer: no loss selected (refine_with_l1 / refine_with_mse / refine_with_ssim)")
        missing = [k for k in REFINE_SPEC if k not in sd]
        if missing:
            raise KeyError(f"state_dict lacks {missing[:3]}{'...' if len(missing) > 3 else ''}")
        self.device = torch.device(device)
        self.lr, self.beta1, self.beta2, self.eps = float(lr), float(beta1), float(beta2), float(eps)
        self.refine_with_l1, self.refine_with_mse = bool(refine_with_l1), bool(refine_with_mse)
        self.lambda_refine_l1, self.lambda_refine_mse = float(lambda_refine_l1), float(lambda_refine_mse)
        self.refine_with_ssim, self.lambda_refine_ssim = bool(refine_with_ssim), float(lambda_refine_ssim)
        self.momentum, self.img_chunk, self.precision, self.weight_grad = float(momentum), img_chunk, precision, weight_grad
        dev = OrderedDict()
        for k, shape in REFINE_SPEC.items():
            v = sd[k]
            v = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach()
            if tuple(v.shape) != tuple(shape):
                raise ValueError(f"{k}: expected shape {shape}, got {tuple(v.shape)}")
            dev[k] = v.to(device=self.device, dtype=torch.float32).contiguous().clone()
        self.params = OrderedDict((k, dev[k].requires_grad_(True)) for k in TRAIN_PARAM_KEYS)
        self.running = OrderedDict((k, dev[k]) for k in RUNNING_KEYS)
        self.exp_avg = OrderedDict((k, torch.zeros_like(v)) for k, v in self.params.items())
        self.exp_avg_sq = OrderedDict((k, torch.zeros_like(v)) for k, v in self.params.items())
        self.step = 0
        self.pred = None
        self._ssim = None

    def set_input(self, input):
        """``sr_patch`` / ``gt_patch`` (B, 3, H, W) and ``ref_patches`` (B, R, 3, H, W), on the host or the device, of any floating
        dtype: copied to the trainer's device as dense fp32 (the reference's ``set_input`` moves its batches the same way); the
        inputs are never written.  Shapes that do not fit each other raise ``ValueError`` here, before anything runs."""
        data = {name: input[name].to(device=self.device, dtype=torch.float32).contiguous() for name in ("sr_patch", "ref_patches", "gt_patch")}
        sr, ref, gt = data["sr_patch"], data["ref_patches"], data["gt_patch"]
        if sr.ndim != 4 or sr.shape[1] != 3 or ref.ndim != 5 or ref.shape[0] != sr.shape[0] or tuple(ref.shape[2:]) != tuple(sr.shape[1:]) \
                or tuple(gt.shape) != tuple(sr.shape):
            raise ValueError(f"expected sr_patch and gt_patch (B, 3, H, W) and ref_patches (B, R, 3, H, W), got {tuple(sr.shape)}, "
                             f"{tuple(gt.shape)} and {tuple(ref.shape)}")
        for name, v in data.items():
            setattr(self, f"data_{name}", v)

    def forward(self):
        self.pred = forward_train(self.params, self.running, self.data_sr_patch, self.data_ref_patches, self.momentum, self.img_chunk,
                                  self.precision, weight_grad=self.weight_grad)
        return self.pred

    def calculate_losses(self):
        """refine_model.py:151-168: lambda-weighted L1 / MSE (reduction 'mean'), their sum, PSNR of the input and the output;
        with ``refine_with_ssim`` also ``loss_ssim = lambda_refine_ssim * (1 - SSIM)`` (this build's addition), added to the sum."""
        zero = torch.zeros((), device=self.device)
        self.loss_l1 = torch.nn.functional.l1_loss(self.pred, self.data_gt_patch) * self.lambda_refine_l1 if self.refine_with_l1 else zero
        self.loss_mse = torch.nn.functional.mse_loss(self.pred, self.data_gt_patch) * self.lambda_refine_mse if self.refine_with_mse else zero
        self.loss_tot = self.loss_mse + self.loss_l1
        self.loss_ssim = zero
        if self.refine_with_ssim:
            from . import metrics
            if self._ssim is None:
                self._ssim = metrics.SSIM(data_range=(-1, 1))
            self.loss_ssim = self.lambda_refine_ssim * (1 - self._ssim(self.pred, self.data_gt_patch))
            self.loss_tot = self.loss_tot + self.loss_ssim
        with torch.no_grad():
            psnr = lambda a, b: -10.0 * torch.log10(torch.mean((a - b) ** 2))
            self.loss_psnr_input = psnr(self.data_sr_patch, self.data_gt_patch)
            self.loss_psnr_refine = psnr(self.pred, self.data_gt_patch)

    def backward(self):
        self.calculate_losses()
        for p in self.params.values():
            p.grad = None
        self.loss_tot.backward()

    def optimizer_step(self):
        """torch.optim.Adam.step over the 72 parameters: nsr_adam_step_n, at most 40 tensors per call."""
        self.step += 1
        keys = [k for k in TRAIN_PARAM_KEYS if self.params[k].grad is not None]
        for i in range(0, len(keys), 40):
            g = keys[i:i + 40]
            numel = (ctypes.c_int64 * len(g))(*[self.params[k].numel() for k in g])
            _lib.check(_lib.load().nsr_adam_step_n(
                len(g), numel, _ptr_array([self.params[k] for k in g]), _ptr_array([self.params[k].grad for k in g]),
                _ptr_array([self.exp_avg[k] for k in g]), _ptr_array([self.exp_avg_sq[k] for k in g]),
                self.step, self.lr, self.beta1, self.beta2, self.eps, _stream()), "nsr_adam_step_n")
        # the weights were written behind autograd's back: the backward of a forward made before this step must fail the
        # version check instead of mixing two sets of weights
        torch.autograd.graph.increment_version(list(self.params.values()))

    def optimize_parameters(self):
        self.forward()
        self.backward()
        self.optimizer_step()
        return self.loss_tot.detach()

    def update_learning_rate(self, epoch: int, lr_policy: str = "exp", **kw) -> float:
        """The reference's per-epoch schedules, the arithmetic of ``train.Trainer.update_learning_rate``."""
        from .train import Trainer
        return Trainer.update_learning_rate(self, epoch, lr_policy, **kw)

    def state_dict(self):
        sd = OrderedDict()
        for k in REFINE_SPEC:
            sd[k] = (self.params[k] if k in self.params else self.running[k]).detach().clone()
        return sd

    def eval_model(self, precision: str = "f16x3") -> MaxPoolingModel:
        """The eval-mode network (BatchNorm folded on the running statistics) of the current state."""
        return MaxPoolingModel(precision=precision, device=self.device).load_state_dict(self.state_dict())
