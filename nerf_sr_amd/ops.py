"""Host-side mirror of the reference's operator interface for the render hot path.

Same names, argument meaning and return shapes as the reference functions they
replace (cited per function), implemented as calls into libnsr.so through the C
ABI.  PyTorch is plumbing only: it owns the device buffers and the stream.
Tensor arguments are fp32 on the current HIP device: another dtype raises ``TypeError``, the host or another GPU
``ValueError`` (``_f32``; nothing is converted silently), a shape that does not fit the other arguments ``ValueError`` --
all before the first allocation and the first library call.  A non-contiguous view is read through a dense copy (the bits
of the dense call), inputs are never written, and results are fresh tensors unless a docstring says otherwise
("Inputs").
"""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_void_p  # noqa: F401
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .weights import (STATE_DICT_SPEC, check_state_dict, pad_no_dir, DIR_W, IN_CH, arch_of, arch_spec, is_default_arch,
                      check_state_dict_arch, normalize_arch, arch_key, embed_of, embed_names, check_embed, EMBED_NO_XYZ)

__all__ = [
    "subpixel_rays", "PositionalEncoding", "sample_along_rays", "resample_along_rays", "cast_rays",
    "VanillaMLP", "VolumetricRenderer", "check_mlp_options", "render_rays", "render_rays_sigma", "render_rays_composited", "forward_rays", "sr_mean", "unflatten_reshape",
]


def _stream() -> c_void_p:
    """torch's current stream on the CURRENT device: libnsr enqueues on the caller's current HIP device
    (include/nsr.h), so every tensor handed to an op must live there (``_check_device``)."""
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_device(dev, name: str) -> None:
    """Kernels run on torch's current device against raw pointers: a tensor on another GPU would fault or be
    reached over the fabric silently.  Fail loudly instead (``torch.cuda.set_device`` / ``with torch.cuda.device``)."""
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise ValueError(f"{name} must live on the GPU (nerf_sr_amd has no CPU path)")
    cur = torch.cuda.current_device()
    if dev.index is not None and dev.index != cur:
        raise ValueError(f"{name} lives on cuda:{dev.index} but the current device is cuda:{cur}; "
                         f"call torch.cuda.set_device({dev.index}) (one process per GPU) before using nerf_sr_amd")


def _p(t: Optional[torch.Tensor]) -> c_void_p:
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (nerf_sr_amd has no CPU path)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    _check_device(t.device, name)
    return t.contiguous()


def _i32(t: torch.Tensor, name: str) -> torch.Tensor:
    """An integer index tensor as the dense int32 the kernels read: any integer dtype is converted (``torch.tensor([[0, 0]])``
    is int64), a floating-point or bool tensor is a ``TypeError``; on the current device, like ``_f32``."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (nerf_sr_amd has no CPU path)")
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"{name} must be an integer tensor, got {t.dtype}")
    _check_device(t.device, name)
    return t.detach().to(torch.int32).contiguous()


def _rays_z(rays: torch.Tensor, z_vals: torch.Tensor):
    """``(rays, z_vals)`` dense fp32 with z_vals (R, N >= 1) for the R rows of rays (R, 8 | 11): the kernels take R and N from
    ``z_vals`` and read R rows of ``rays``."""
    rays, z_vals = _f32(rays, "rays"), _f32(z_vals, "z_vals")
    _ray_stride(rays)
    if z_vals.ndim != 2 or z_vals.shape[0] != rays.shape[0] or z_vals.shape[1] < 1:
        raise ValueError(f"z_vals must be (R, N >= 1) with R = {rays.shape[0]} rays, got {tuple(z_vals.shape)}")
    return rays, z_vals


def _ray_stride(rays: torch.Tensor) -> int:
    """8: nerf_downX rows [o, d, near, far]; 11: vanilla rows with the view direction in columns 8:11."""
    if rays.ndim != 2 or rays.shape[1] not in (8, 11):
        raise ValueError(f"rays must be (R, 8) or (R, 11), got {tuple(rays.shape)}")
    return int(rays.shape[1])


def _pack_rays(ori, dir, near, far) -> torch.Tensor:
    """(R, 8) rows [o, d, near, far] from ``ori`` / ``dir`` (R, 3), already through ``_f32``; a tensor ``near`` / ``far`` goes
    through the same checks and holds one value per ray ((R,) or (R, 1)), a number is broadcast."""
    if ori.ndim != 2 or ori.shape[1] != 3 or tuple(dir.shape) != tuple(ori.shape):
        raise ValueError(f"ori and dir must both be (R, 3), got {tuple(ori.shape)} and {tuple(dir.shape)}")
    R = ori.shape[0]
    bounds = []
    for t, name in ((near, "near"), (far, "far")):
        if isinstance(t, torch.Tensor):
            t = _f32(t, name)
            if tuple(t.shape) not in ((R,), (R, 1)):
                raise ValueError(f"{name} must hold one value per ray, (R,) or (R, 1) with R = {R}, got {tuple(t.shape)}")
            bounds.append(t.reshape(R, 1))
        else:
            bounds.append(torch.full((R, 1), float(t), dtype=torch.float32, device=ori.device))
    return torch.cat([ori, dir] + bounds, 1).contiguous()


def _jitter(u, R: int, num_samples: int):
    if u is None:
        return None
    u = _f32(u, "u")
    if tuple(u.shape) != (R, num_samples):
        raise ValueError(f"u must be (R, num_samples) = ({R}, {num_samples}), got {tuple(u.shape)}")
    return u


def state_dict_to_device(sd, spec, device, own: bool = False) -> Dict[str, torch.Tensor]:
    """The tensors of ``sd`` (numpy arrays or torch tensors, detached) that ``spec`` names, as contiguous fp32 tensors on
    ``device`` in ``spec`` order.  ``own``: cloned, so that the caller may update them in place."""
    out = {}
    for k in spec:
        v = sd[k]
        v = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach()
        v = v.to(device=device, dtype=torch.float32).contiguous()
        out[k] = v.clone() if own else v
    return out


# ----------------------------------------------------------------------------- R1-R4
def subpixel_rays(c2w, img_wh: Tuple[int, int], focal: float, downscale: int, ndc: bool,
                  near: float = 0.0, far: float = 1.0, device="cuda",
                  lr_range: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """(H/s*W/s, s*s, 8) sub-pixel ray tensor of one pose, generated on the device.

    Replaces get_ray_directions + get_rays (+ get_ndc_rays) + the einops regroup
    (models/utils.py:98-196, data/llff_downX_dataset.py:473-490,
    data/blender_downX_dataset.py:207-215).  ``img_wh`` is the HR size (W, H).
    ``lr_range = (lo, hi)`` generates only the LR pixels [lo, hi) (row-major LR index): the ray shard of one
    GPU when the frame is cut into contiguous LR-pixel blocks -> (hi - lo, s*s, 8).
    """
    lib = _lib.load()
    W, H = int(img_wh[0]), int(img_wh[1])
    s = int(downscale)
    c = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(12))
    lo, hi = (0, (H // s) * (W // s)) if lr_range is None else (int(lr_range[0]), int(lr_range[1]))
    _check_device(device, "device")
    rays = torch.empty(max(hi - lo, 0), s * s, 8, dtype=torch.float32, device=device)
    _lib.check(lib.nsr_gen_rays_range(c.ctypes.data_as(ctypes.POINTER(c_float)), H, W, float(focal), s, int(bool(ndc)),
                                      float(near), float(far), lo, hi, _p(rays), _stream()), "nsr_gen_rays_range")
    return rays


# ----------------------------------------------------------------------------- E1
class PositionalEncoding:
    """``x -> [x, sin(f_k x), cos(f_k x)]_k``; mirrors models/embedding.py:14-62 (3 input channels) with its two options read
    from ``opt``: ``no_xyz`` drops the identity columns, ``no_logscale`` replaces the bands ``2^k`` by
    ``linspace(1, 2^(N_freqs-1), N_freqs)`` (nsr_posenc_e, include/nsr.h); ``freq_bands`` is the library's table."""

    def __init__(self, in_channels: int = 3, N_freqs: int = 10, opt=None):
        if in_channels != 3:
            raise ValueError("the built path encodes 3-channel inputs only")
        self.in_channels, self.N_freqs = in_channels, int(N_freqs)
        self.embed = embed_of(opt)

    @property
    def out_channels(self) -> int:
        return self.in_channels * (2 * self.N_freqs + (0 if self.embed & EMBED_NO_XYZ else 1))

    @property
    def freq_bands(self) -> np.ndarray:
        f = (c_float * max(self.N_freqs, 1))()
        _lib.check(_lib.load().nsr_posenc_freqs(self.N_freqs, self.embed, f), "nsr_posenc_freqs")
        return np.array(f[: self.N_freqs], dtype=np.float32)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        x = _f32(x, "x")
        if x.ndim != 2 or x.shape[1] != 3:
            raise ValueError(f"x must be (B, 3), got {tuple(x.shape)}")
        out = torch.empty(x.shape[0], self.out_channels, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().nsr_posenc_e(_p(x), x.shape[0], self.N_freqs, self.embed, _p(out), _stream()), "nsr_posenc_e")
        return out


# ----------------------------------------------------------------------------- S1 / S2
def cast_rays(ori, dir, z_vals):
    """``ori + z*dir`` (models/utils.py:5-14) — kept for API parity; torch elementwise."""
    return ori[..., None, :] + z_vals[..., None] * dir[..., None, :]


def sample_along_rays(ori, dir, near, far, num_samples: int, randomized: bool, lindisp: bool,
                      u: Optional[torch.Tensor] = None):
    """Stratified depths and points; mirrors models/utils.py:17-44.

    ``randomized=True`` draws the per-bin jitter with ``torch.rand`` on the device
    unless ``u`` (R, num_samples) is supplied (used by the parity tests).
    Returns ``(z_vals (R,N), points (R,N,3))``.
    """
    rays = _pack_rays(_f32(ori, "ori"), _f32(dir, "dir"), near, far)
    R = rays.shape[0]
    if randomized and u is None:
        u = torch.rand(R, num_samples, device=rays.device)
    u = _jitter(u, R, num_samples)
    z = torch.empty(R, num_samples, dtype=torch.float32, device=rays.device)
    pts = torch.empty(R, num_samples, 3, dtype=torch.float32, device=rays.device)
    _lib.check(_lib.load().nsr_sample_along_rays(_p(rays), 8, R, num_samples, int(bool(lindisp)), _p(u), _p(z), _p(pts),
                                                 _stream()), "nsr_sample_along_rays")
    return z, pts


def resample_along_rays(ori, dir, z_vals, weights, num_samples: int, randomized: bool,
                        u: Optional[torch.Tensor] = None):
    """Inverse-CDF importance resampling + merge; mirrors models/utils.py:47-95.
    Returns ``(z_vals (R, N+num_samples) sorted, points)``."""
    ori, dir = _f32(ori, "ori"), _f32(dir, "dir")
    z_vals, weights = _f32(z_vals, "z_vals"), _f32(weights, "weights")
    rays = _pack_rays(ori, dir, 0.0, 1.0)
    if z_vals.ndim != 2 or z_vals.shape[0] != rays.shape[0] or tuple(weights.shape) != tuple(z_vals.shape):
        raise ValueError(f"z_vals and weights must both be (R, Nc) with R = {rays.shape[0]} rays, got {tuple(z_vals.shape)} and "
                         f"{tuple(weights.shape)}")
    R, Nc = z_vals.shape
    if randomized and u is None:
        u = torch.rand(R, num_samples, device=z_vals.device)
    u = _jitter(u, R, num_samples)
    z_out = torch.empty(R, Nc + num_samples, dtype=torch.float32, device=z_vals.device)
    pts = torch.empty(R, Nc + num_samples, 3, dtype=torch.float32, device=z_vals.device)
    _lib.check(_lib.load().nsr_resample_along_rays(_p(rays), 8, _p(z_vals), _p(weights), R, Nc, num_samples, _p(u),
                                                   _p(z_out), _p(pts), _stream()), "nsr_resample_along_rays")
    return z_out, pts


# ----------------------------------------------------------------------------- M1
# the one architecture the HIP kernels are built for: the values every script of the reference uses
_MLP_FIXED = {"D": 8, "W": 256, "skips": [4], "deg_pos": 10, "deg_dir": 4, "dim_pos": 3, "dim_dir": 3, "dim_rgb": 3}
_GENERIC_FIXED = {"dim_pos": 3, "dim_dir": 3, "dim_rgb": 3}     # what the ray kernels and the compositor cannot vary either
#                                                                   (GenericMLP on its own takes any dim_rgb)
# built since round 5; stop_grad (a detach: models/networks.py:218-219) changes nothing in a forward pass and is an option of
# train.Trainer
_MLP_CHOICES = {"color_activation": ("sigmoid", "none"), "no_dir": (False, True), "stop_grad": (False, True)}


def check_mlp_options(opt, fused: bool = True) -> None:
    """Reject every VanillaMLP option value the kernels do not implement (models/networks.py:124-128 ``--D --W --skips``;
    models/embedding.py degrees) instead of silently computing the default architecture.  ``no_dir`` and
    ``color_activation`` (:160-180) are options of ``VanillaMLP`` since round 5, ``stop_grad`` of ``train.Trainer``.
    Options that are absent from ``opt`` count as the reference's defaults.  ``fused=False``: the check of ``make_mlp`` /
    ``NeRFDownXModel``, which serve other ``--D --W --skips`` / degrees / ``dim_rgb`` layer by layer (``GenericMLP``)."""
    if opt is None:
        return
    bad = []
    for name, want in (_MLP_FIXED if fused else _GENERIC_FIXED).items():
        if not hasattr(opt, name):
            continue
        got = getattr(opt, name)
        got = list(got) if isinstance(got, (list, tuple)) else got
        if got != want:
            bad.append(f"{name}={got!r} (built: {want!r})")
    for name, choices in _MLP_CHOICES.items():
        if hasattr(opt, name) and getattr(opt, name) not in choices:
            bad.append(f"{name}={getattr(opt, name)!r} (built: {list(choices)!r})")
    if fused and embed_of(opt):
        bad.append(f"{embed_names(embed_of(opt))} (built: the full log-scale encoding; ops.make_mlp / GenericMLP serve the embedding options)")
    if bad:
        raise ValueError("VanillaMLP option(s) outside the built path (the MFMA kernels are laid out for the 8 x 256 network with "
                         "a skip at layer 5, models/networks.py:131-180): "
                         + ", ".join(bad))


class VanillaMLP:
    """The 8x256 NeRF MLP; mirrors models/networks.py:121-226.

    Weights enter as the reference's 24-key ``state_dict`` (``load_state_dict``) and
    are re-laid-out once into the MFMA fragment stream the kernel consumes
    (``nsr_pack_weights``).  ``forward(x, sigma_only=False)``: x (B, 90) embedded rows
    -> (B, 4) = [rgb, sigma] (or (B, 1)).
    """

    def __init__(self, opt=None, precision: str = "fp32", device="cuda"):
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {list(_lib.PRECISIONS)}")
        check_mlp_options(opt)
        self.precision = precision
        self._prec = _lib.PRECISIONS[precision]
        self.device = torch.device(device)
        _check_device(self.device, "VanillaMLP device")
        nbytes = _lib.load().nsr_packed_weights_bytes(self._prec)
        if nbytes == 0:
            raise _lib.NsrError(f"precision {precision!r} is not built into libnsr.so")
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._sd = None
        self._gamma = False
        self._want_gamma = bool(getattr(opt, "gamma_correct", False)) if opt is not None else False
        # --color_activation none (models/networks.py:173-180): the rgb head ends in nn.Identity; --no_dir (:160-169):
        # dir_encoding sees xyz_encoding_final alone (weights.pad_no_dir)
        self.color_activation = getattr(opt, "color_activation", "sigmoid") if opt is not None else "sigmoid"
        self.no_dir = bool(getattr(opt, "no_dir", False)) if opt is not None else False

    def _options_word(self) -> int:
        return (_lib.NSR_OPT_GAMMA if self._want_gamma else 0) | (_lib.NSR_OPT_COLOR_NONE if self.color_activation == "none" else 0)

    def load_state_dict(self, sd: Dict[str, "np.ndarray | torch.Tensor"]):
        check_state_dict(sd, self.no_dir)
        dev = state_dict_to_device(sd, STATE_DICT_SPEC, self.device)
        packed_from = dict(dev)
        if self.no_dir:
            packed_from[DIR_W] = pad_no_dir(dev[DIR_W]).contiguous()
        ptrs = (c_void_p * len(dev))(*[c_void_p(t.data_ptr()) for t in packed_from.values()])
        rc = _lib.load().nsr_pack_weights(ptrs, _p(self.packed), self._prec, _stream())
        if rc == _lib.NSR_ERR_RANGE:
            # the blob HAS been overwritten with the out-of-range network (include/nsr.h): this object no longer holds a
            # usable one -- forward() / state_dict() must not go on serving the previous tensors against the new blob
            self._sd = None
            self._gamma = False
            raise _lib.NsrNumericsError(
                f"state_dict cannot be carried at precision {self.precision!r}: a weight or bias is non-finite"
                + (" or |w| >= 1023.75 (the split-fp16 stream holds 2^6 w in fp16; so does dir_encoding[:, :256] @ xyz_encoding_final, "
                   "which the pack folds into one matrix)" if self.precision == "f16x3" else
                   " or |w| >= 65520 (fp16 operands)" if self.precision == "f16" else "")
                + "; load it with precision='fp32'", 1)
        _lib.check(rc, "nsr_pack_weights")
        self._sd = dev     # keep the fp32 originals alive (state_dict() round trip)
        self._gamma = False
        if self._options_word():   # packing clears the blob's option word: the requested colour-head options are re-applied
            self._write_options()
        return self

    def _write_options(self):
        _lib.check(_lib.load().nsr_weights_set_options(_p(self.packed), self._prec, self._options_word(), _stream()),
                   "nsr_weights_set_options")
        self._gamma = self._want_gamma

    def set_gamma_correct(self, enable: bool = True):
        """``--gamma_correct`` (models/nerf_downX_model.py:271-276): the colour head returns ``rgb ** (1 / 2.2)``.
        An option of the PACKED network: call it after ``load_state_dict`` (re-packing clears it)."""
        if self._sd is None:
            raise RuntimeError("VanillaMLP.set_gamma_correct called before load_state_dict")
        self._want_gamma = bool(enable)       # remembered: every later load_state_dict re-applies it
        self._write_options()
        return self

    def status(self, clear: bool = False) -> int:
        """The network's sticky numerics status word (``NSR_FLAG_*`` bits, include/nsr.h): 0 = every launch through this
        network so far saw finite inputs, in-range activations and finite outputs.  Waits for the current stream."""
        if self._sd is None:
            raise RuntimeError("VanillaMLP.status called before load_state_dict (the blob, and its status word, are not initialised)")
        flags = ctypes.c_uint(0)
        _lib.check(_lib.load().nsr_weights_status(_p(self.packed), self._prec, int(bool(clear)), ctypes.byref(flags), _stream()),
                   "nsr_weights_status")
        return int(flags.value)

    def check(self, what: str = "network"):
        """Raise ``NsrNumericsError`` if the status word is set (and clear it): the reference drops into pdb on NaN
        colours (models/nerf_downX_model.py:273-274); this is the error a replacement reports instead."""
        flags = self.status(clear=True)
        if flags:
            names = _lib.flag_names(flags)
            hint = " -- values left the split-fp16 operand range: re-run with precision='fp32'" \
                if (flags & 4 or (flags & 2 and self.precision in ("f16x3", "f16"))) else ""
            raise _lib.NsrNumericsError(f"{what} ({self.precision}): numerics status {flags:#x} = {' | '.join(names)}{hint}", flags)
        return self

    def state_dict(self):
        if self._sd is None:
            raise RuntimeError("no weights loaded")
        return {k: v.clone() for k, v in self._sd.items()}

    def forward(self, x: torch.Tensor, sigma_only: bool = False) -> torch.Tensor:
        if self._sd is None:
            raise RuntimeError("VanillaMLP.forward called before load_state_dict")
        x = _f32(x, "x")
        if x.ndim != 2 or x.shape[1] != IN_CH:
            raise ValueError(f"x must be (B, {IN_CH}), got {tuple(x.shape)}")
        out = torch.empty(x.shape[0], 1 if sigma_only else 4, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().nsr_mlp_forward(_p(self.packed), self._prec, _p(x), x.shape[0], int(bool(sigma_only)),
                                               _p(out), _stream()), "nsr_mlp_forward")
        return out

    __call__ = forward


class GenericMLP:
    """``VanillaMLP`` (models/networks.py:121-226) for the architecture flags the fused kernels are not laid out for:
    ``--D --W --skips`` (:124-126), ``--deg_pos --deg_dir --dim_rgb`` (models/nerf_model.py:53-57), with ``--no_dir`` and
    ``--color_activation none`` as there.  Every ``nn.Linear`` (+ activation) is one launch of the training step's fp32-MFMA
    GEMM (``nsr_linear``, include/nsr_train.h) over zero-padded operands -- K and N rounded up to multiples of 32 with
    zero weight columns / rows, whose products are exact zeros -- writing straight into the next layer's input buffer, so
    ``cat([input_xyz, h])`` of a skip layer and ``cat([final, dir])`` are column ranges of one buffer, never copies of
    activations.  Same interface as ``VanillaMLP`` (``forward(x, sigma_only)``, ``state_dict``, ``check``).  Training such a
    network is ``train.Trainer(..., arch=)`` / ``train.forward_rays_train(..., arch=)``: the same layout, layer by layer, with the
    backward products (``nsr_train_arch_forward`` / ``nsr_train_arch_backward``); its ``state_dicts()`` load here."""

    POINT_CHUNK = 262144          # rows per pass (the reference's point_chunk, options/base_options.py:70): bounds the buffers

    def __init__(self, opt=None, device="cuda", precision: str = "fp32", fused: bool = False, embed: Optional[int] = None, **arch):
        self.arch = normalize_arch(opt, **arch)             # validates
        # the embedding's option word (--no_xyz / --no_logscale; default: read from opt): narrower layers under no_xyz, and the
        # word every descriptor entry point of the fused route takes (the `_e` forms, include/nsr_train.h)
        self.embed = check_embed(embed_of(opt) if embed is None else embed, self.arch)
        self.no_xyz = bool(self.embed & EMBED_NO_XYZ)
        self.spec = arch_spec(no_xyz=self.no_xyz, **self.arch)
        # fused=True (opt-in, precision 'f16x3'): the whole network in ONE launch per POINT_CHUNK, activations never leave the
        # chip (nsr_arch_fused_forward, include/nsr_train.h) -- the arithmetic of the layer-by-layer route in another summation
        # order.  Refused, before a device is touched, for a precision or an architecture the kernel does not cover.
        self.fused = bool(fused)
        if self.fused:
            check_arch_fused(self.arch, precision)
        self.color_activation = getattr(opt, "color_activation", "sigmoid") if opt is not None else "sigmoid"
        if self.color_activation not in ("sigmoid", "none"):
            raise ValueError(f"color_activation={self.color_activation!r}: 'sigmoid' or 'none' (models/networks.py:173-180)")
        # --gamma_correct is not a property of the network in the reference either: render_rays raises the colours to 1 / 2.2
        # after the network call (models/nerf_downX_model.py:271-276).  The fused kernels carry it as an option of their
        # colour head; on this route NeRFDownXModel.render_rays applies it to what forward() returns.
        self.gamma_correct = bool(getattr(opt, "gamma_correct", False)) if opt is not None else False
        self.device = torch.device(device)
        _check_device(self.device, "GenericMLP device")
        first = 0 if self.no_xyz else 3
        self.in_xyz, self.in_dir = first + 6 * self.arch["deg_pos"], first + 6 * self.arch["deg_dir"]
        # "fp32": every nn.Linear on the fp32 MFMA (nsr_linear); "f16x3" (round 6): on the split-fp16 MFMA, three terms per
        # product, products exact to ~2^-21 (nsr_linear_f16x3: the weights are split once at load time) -- the arithmetic of
        # the fused kernels' default precision, layer by layer.  The single-operand fast precisions have no layer-by-layer form.
        if precision not in ("fp32", "f16x3"):
            raise ValueError(f"GenericMLP precision {precision!r}: 'fp32' or 'f16x3' (the layer-by-layer route has no single-operand fast path)")
        self.precision = precision
        self._sd = None
        color_none = self.color_activation == "none"
        self._route = _FusedRoute(self.arch, self.device, color_none, self.embed) if self.fused else \
            _LayerRoute(self.arch, self.device, precision, color_none, self.embed)

    @property
    def _split(self):
        """The linears that carry split-fp16 halves: all of them under 'f16x3' layer by layer, none otherwise."""
        return [rec for rec in getattr(self._route, "linears", ()) if rec[2] is not None]

    def load_state_dict(self, sd):
        check_state_dict_arch(sd, no_xyz=self.no_xyz, **self.arch)
        dev = state_dict_to_device(sd, self.spec, self.device)
        self._sd = None                 # a load that raises leaves nothing usable behind
        self._route.load(dev)
        self._sd = dev
        return self

    def state_dict(self):
        if self._sd is None:
            raise RuntimeError("no weights loaded")
        return {k: v.clone() for k, v in self._sd.items()}

    # -- numerics status: the reference drops into pdb on NaN colours (models/nerf_downX_model.py:273-274) ---------------------------
    def status(self, clear: bool = False) -> int:
        return self._route.status(clear)

    def check(self, what: str = "network"):
        flags = self.status(clear=True)
        if flags:
            raise _lib.NsrNumericsError(f"{what} {self._route.describe(flags)}", flags)
        return self

    def forward(self, x: torch.Tensor, sigma_only: bool = False) -> torch.Tensor:
        if self._sd is None:
            raise RuntimeError("GenericMLP.forward called before load_state_dict")
        x = _f32(x, "x")
        n_in = self.in_xyz + (0 if sigma_only else self.in_dir)
        if x.ndim != 2 or x.shape[1] < n_in:
            raise ValueError(f"x must be (B, {n_in}), got {tuple(x.shape)}")
        out = torch.empty(x.shape[0], 1 if sigma_only else self.arch["dim_rgb"] + 1, dtype=torch.float32, device=x.device)
        for r0 in range(0, x.shape[0], self.POINT_CHUNK):
            self._route.forward(x[r0:r0 + self.POINT_CHUNK], out[r0:r0 + self.POINT_CHUNK], sigma_only)
        return out

    __call__ = forward


class _LayerRoute:
    """``GenericMLP`` layer by layer: the zero-padded operands of every ``nn.Linear`` as one record ``(w, b, hi, lo)`` -- ``hi``
    / ``lo`` the fp16 halves of 64 w under 'f16x3', None under 'fp32' -- and the sticky non-finite-output flag."""

    def __init__(self, arch: dict, device, precision: str, color_none: bool, embed: int = 0):
        self.arch, self.device, self.precision, self.color_none = arch, device, precision, color_none
        first = 0 if embed & EMBED_NO_XYZ else 3      # the route sees the option word only as the width of the encoded rows
        self.in_xyz, self.in_dir = first + 6 * arch["deg_pos"], first + 6 * arch["deg_dir"]
        r32 = lambda n: (n + 31) // 32 * 32
        self.Kx, self.Wp, self.Hp, self.Dp, self.Rp = r32(self.in_xyz), r32(arch["W"]), r32(arch["W"] // 2), r32(self.in_dir), r32(arch["dim_rgb"])
        self.linears = []
        self._bad = None

    def _padded(self, w, rows, col_map, cols):
        """(rows, cols) zero matrix with w's column ranges placed by col_map = [(src0, n, dst0), ...]."""
        out = torch.zeros(rows, cols, dtype=torch.float32, device=self.device)
        for s0, n, d0 in col_map:
            out[: w.shape[0], d0:d0 + n] = w[:, s0:s0 + n]
        return out

    def _padded_bias(self, b, n):
        out = torch.zeros(n, dtype=torch.float32, device=self.device)
        out[: b.shape[0]] = b
        return out

    def _linear(self, w, b):
        hi = lo = None
        if self.precision == "f16x3":       # (hi, lo) fp16 halves of 64 w, made once
            hi, lo = torch.empty(2, w.numel(), dtype=torch.int16, device=self.device)
            _lib.check(_lib.load().nsr_split_weights(_p(w), w.numel(), _p(hi), _p(lo), _stream()), "nsr_split_weights")
        self.linears.append((w, b, hi, lo))
        return self.linears[-1]

    def load(self, dev):
        a, W, ix, Kx, Wp = self.arch, self.arch["W"], self.in_xyz, self.Kx, self.Wp
        self.linears = []
        self._trunk = []                        # (linear, first input column, K): inputs = slots [pe | h]
        for i in range(a["D"]):
            w, b = dev[f"xyz_encoding_{i + 1}.0.weight"], self._padded_bias(dev[f"xyz_encoding_{i + 1}.0.bias"], Wp)
            if i == 0:
                self._trunk.append((self._linear(self._padded(w, Wp, [(0, ix, 0)], Kx), b), 0, Kx))
            elif i in a["skips"]:               # cat([input_xyz, h]): pe at columns 0.., h at columns Kx..
                self._trunk.append((self._linear(self._padded(w, Wp, [(0, ix, 0), (ix, W, Kx)], Kx + Wp), b), 0, Kx + Wp))
            else:
                self._trunk.append((self._linear(self._padded(w, Wp, [(0, W, 0)], Wp), b), Kx, Wp))
        self._sigma = self._linear(self._padded(dev["sigma.weight"], 32, [(0, W, 0)], Wp), self._padded_bias(dev["sigma.bias"], 32))
        self._final = self._linear(self._padded(dev["xyz_encoding_final.weight"], Wp, [(0, W, 0)], Wp),
                                   self._padded_bias(dev["xyz_encoding_final.bias"], Wp))
        dmap = [(0, W, 0)] + ([] if a["no_dir"] else [(W, self.in_dir, Wp)])
        self._dir = self._linear(self._padded(dev["dir_encoding.0.weight"], self.Hp, dmap, Wp + (0 if a["no_dir"] else self.Dp)),
                                 self._padded_bias(dev["dir_encoding.0.bias"], self.Hp))
        self._rgb = self._linear(self._padded(dev["rgb.0.weight"], self.Rp, [(0, W // 2, 0)], self.Hp), self._padded_bias(dev["rgb.0.bias"], self.Rp))
        self._bad = torch.zeros((), dtype=torch.bool, device=self.device)

    def status(self, clear: bool) -> int:
        flags = _lib.NSR_FLAG_OUTPUT_NONFINITE if (self._bad is not None and bool(self._bad)) else 0
        if clear and self._bad is not None:
            self._bad.zero_()
        return flags

    def describe(self, flags: int) -> str:
        return "(layer-by-layer fp32): non-finite network output"

    def _gemm(self, x, col0, ldx, K, linear, act, y, ycol0, ldy, P):
        lib, esz = _lib.load(), 4
        w, b, hi, lo = linear
        if hi is not None:
            _lib.check(lib.nsr_linear_f16x3(c_void_p(x.data_ptr() + col0 * esz), ldx, _p(hi), _p(lo),
                                            w.shape[1], _p(b), act, c_void_p(y.data_ptr() + ycol0 * esz), ldy, P, K, w.shape[0], _stream()),
                       "nsr_linear_f16x3")
            return
        _lib.check(lib.nsr_linear(c_void_p(x.data_ptr() + col0 * esz), ldx, _p(w), w.shape[1], _p(b), act,
                                  c_void_p(y.data_ptr() + ycol0 * esz), ldy, c_void_p(0), 0, P, K, w.shape[0], _stream()), "nsr_linear")

    def forward(self, x: torch.Tensor, out: torch.Tensor, sigma_only: bool) -> None:
        a, P = self.arch, x.shape[0]
        Kx, Wp, Ls = self.Kx, self.Wp, self.Kx + self.Wp
        slots = [torch.zeros(P, Ls, dtype=torch.float32, device=x.device) for _ in range(2)]     # [pe | pad | h | pad] twice
        for s in slots:
            s[:, : self.in_xyz] = x[:, : self.in_xyz]
        for i, (lin, c0, K) in enumerate(self._trunk):           # layer i reads slot (i - 1) % 2, writes h of slot i % 2
            self._gemm(slots[(i - 1) % 2], c0, Ls, K, lin, 1, slots[i % 2], Kx, Ls, P)
        h = slots[(a["D"] - 1) % 2]
        small = torch.empty(P, 32, dtype=torch.float32, device=x.device)
        self._gemm(h, Kx, Ls, Wp, self._sigma, 0, small, 0, 32, P)
        if sigma_only:
            out[:, 0] = small[:, 0]
        else:
            Ld = Wp + (0 if a["no_dir"] else self.Dp)
            dbuf = torch.zeros(P, Ld, dtype=torch.float32, device=x.device)                             # [final | pad | dir pe | pad]
            self._gemm(h, Kx, Ls, Wp, self._final, 0, dbuf, 0, Ld, P)
            if not a["no_dir"]:
                dbuf[:, Wp:Wp + self.in_dir] = x[:, self.in_xyz:self.in_xyz + self.in_dir]
            c = torch.empty(P, self.Hp, dtype=torch.float32, device=x.device)
            self._gemm(dbuf, 0, Ld, Ld, self._dir, 1, c, 0, self.Hp, P)
            rgb = torch.empty(P, self.Rp, dtype=torch.float32, device=x.device)
            self._gemm(c, 0, self.Hp, self.Hp, self._rgb, 0 if self.color_none else 2, rgb, 0, self.Rp, P)
            out[:, : a["dim_rgb"]] = rgb[:, : a["dim_rgb"]]
            out[:, a["dim_rgb"]] = small[:, 0]
        self._bad |= ~torch.isfinite(out).all()


class _FusedRoute:
    """``GenericMLP(fused=True)``: the weights split and re-laid once into the kernel's stream (nsr_arch_fused_pack), the
    kernel's sticky ``NSR_FLAG_*`` word, and the descriptor every ``nsr_arch_fused_*`` call takes."""

    def __init__(self, arch: dict, device, color_none: bool, embed: int = 0):
        self.arch, self.device, self.color_none, self.embed = arch, device, color_none, int(embed)
        self._c_arch = _lib.NsrArch.from_arch(arch)
        self._packed = self._status = None

    def _flags(self, sigma_only: bool) -> int:
        return (_lib.NSR_ARCH_FUSED_SIGMA_ONLY if sigma_only else 0) | (_lib.NSR_ARCH_FUSED_COLOR_NONE if self.color_none else 0)

    def load(self, dev):
        lib, arch = _lib.load(), ctypes.byref(self._c_arch)
        self._packed = None
        nbytes = lib.nsr_arch_fused_packed_bytes_e(arch, self.embed)
        if nbytes == 0:
            raise _lib.NsrError(f"nsr_arch_fused_packed_bytes_e refuses {self.arch} with embedding option word {self.embed:#x}")
        packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        ptrs = (c_void_p * len(dev))(*[_p(t) for t in dev.values()])
        _lib.check(lib.nsr_arch_fused_pack_e(arch, self.embed, ptrs, _p(packed), _p(self._status), _stream()), "nsr_arch_fused_pack_e")
        if int(self._status.item()) & 1:    # the stream holds the out-of-range network: nothing usable is loaded
            self._status.zero_()
            raise _lib.NsrNumericsError(
                "state_dict cannot be carried at precision 'f16x3': a weight or bias is non-finite or |w| >= 1023.75 (the "
                "split-fp16 stream holds 2^6 w in fp16); load it with precision='fp32'", 1)
        self._packed = packed

    def status(self, clear: bool) -> int:
        if self._packed is None:
            raise RuntimeError("GenericMLP.status called before load_state_dict")
        flags = int(self._status.item()) & 0xF          # waits for the device
        if clear:
            self._status.zero_()
        return flags

    def describe(self, flags: int) -> str:
        hint = " -- values left the split-fp16 operand range: re-run with precision='fp32'" if flags & 6 else ""
        return f"(fused f16x3): numerics status {flags:#x} = {' | '.join(_lib.flag_names(flags))}{hint}"

    def forward(self, x: torch.Tensor, out: torch.Tensor, sigma_only: bool) -> None:
        """One launch, no intermediate buffers."""
        _lib.check(_lib.load().nsr_arch_fused_forward_e(ctypes.byref(self._c_arch), self.embed, _p(self._packed), _p(x), x.shape[1],
                                                        x.shape[0], self._flags(sigma_only), _p(out), out.shape[1], _p(self._status),
                                                        _stream()), "nsr_arch_fused_forward_e")

    def render_rays(self, rays: torch.Tensor, z_vals: torch.Tensor, raw: torch.Tensor, sigma_only: bool) -> None:
        R, N = z_vals.shape
        _lib.check(_lib.load().nsr_arch_fused_render_rays_e(ctypes.byref(self._c_arch), self.embed, _p(self._packed), _p(rays),
                                                            rays.shape[1], _p(z_vals), R, N, self._flags(sigma_only), _p(raw),
                                                            raw.shape[2], _p(self._status), _stream()), "nsr_arch_fused_render_rays_e")


def check_arch_fused(arch: dict, precision: str) -> None:
    """``ValueError`` unless the fused split-fp16 kernel for non-default architectures (nsr_arch_fused_forward,
    include/nsr_train.h) covers ``arch`` at ``precision``; the message names the limit that is exceeded.  Host only."""
    if precision != "f16x3":
        raise ValueError(f"the fused route for non-default architectures is built for precision 'f16x3' only, not {precision!r} "
                         "(leave fused / arch_fused off to run layer by layer)")
    arch_spec(**arch)                   # malformed descriptors: D < 1, odd W, a skip outside 1 .. D - 1
    bad = []
    for name, lim in (("D", _lib.NSR_ARCH_FUSED_MAX_D), ("W", _lib.NSR_ARCH_FUSED_MAX_W),
                      ("deg_pos", _lib.NSR_ARCH_FUSED_MAX_DEG_POS), ("deg_dir", _lib.NSR_ARCH_FUSED_MAX_DEG_DIR)):
        if int(arch[name]) > lim:
            bad.append(f"{name}={arch[name]} (limit: {name} <= {lim})")
    if int(arch.get("dim_rgb", 3)) != 3:
        bad.append(f"dim_rgb={arch['dim_rgb']} (limit: dim_rgb == 3)")
    if bad:
        raise ValueError("architecture outside the fused split-fp16 kernel's set: " + ", ".join(bad)
                         + " (leave fused / arch_fused off to run layer by layer)")


def make_mlp(opt=None, precision: str = "fp32", device="cuda", arch_fused: Optional[bool] = None):
    """The network class for an options object: the fused-kernel ``VanillaMLP`` for the architecture every script of the
    reference uses, ``GenericMLP`` for other ``--D --W --skips`` / degrees / ``dim_rgb`` -- layer by layer, or, with
    ``arch_fused`` (default: ``opt.arch_fused``, off) under precision 'f16x3', in one fused launch (``GenericMLP(fused=True)``)."""
    if arch_fused is None:
        arch_fused = bool(getattr(opt, "arch_fused", False)) if opt is not None else False
    embed = embed_of(opt)
    if is_default_arch(arch_of(opt)) and not embed:
        return VanillaMLP(opt, precision=precision, device=device)
    if embed and precision not in ("fp32", "f16x3"):     # an option is never served by another precision than the one asked for
        raise ValueError(f"{embed_names(embed)} with precision={precision!r}: the embedding options run on the descriptor routes "
                         "(ops.GenericMLP), which have 'fp32' and 'f16x3' only; the single-operand fast paths are the 8 x 256 kernels'")
    if arch_fused:
        return GenericMLP(opt, device=device, precision=precision, fused=True)
    warn_generic_mlp(arch_of(opt), precision, embed)
    return GenericMLP(opt, device=device, precision="f16x3" if precision == "f16x3" else "fp32")


_GENERIC_WARNED = set()


def warn_generic_mlp(arch: dict, precision: str = "fp32", embed: int = 0) -> None:
    """One warning per architecture and process: a non-default ``--D --W --skips`` / encoding degree leaves the fused MFMA
    kernels (whose register, LDS and weight-stream layouts ARE the 8 x 256 network with a skip at layer 5) for the
    layer-by-layer fp32 GEMM route -- correct (tests/golden/arch.npz, made by the reference's own forward), but every
    activation matrix travels through HBM: `bench.py --arch D,W,skips` times it (README: ~an order of magnitude slower per
    sample point than the fused f16x3 kernel at the default size) -- on the fp32 MFMA, or under precision 'f16x3' on the split-fp16 MFMA (three terms per product, nsr_linear_f16x3)."""
    import warnings
    key = arch_key(arch) + ((embed_names(embed),) if embed else ())     # an embedding option makes any network, the default
    if key in _GENERIC_WARNED:                                           # one included, "a non-default architecture"
        return
    _GENERIC_WARNED.add(key)
    with_embed = f" with {embed_names(embed)} (models/embedding.py:17-18)" if embed else ""
    note = "" if precision in ("fp32", "f16x3") else f"; precision={precision!r} has no layer-by-layer form: running fp32"
    how = "split-fp16 (three-term)" if precision == "f16x3" else "fp32"
    warnings.warn(f"NeRF-SR network D={key[0]} W={key[1]} skips={list(key[2])} deg_pos={key[3]} deg_dir={key[4]}{with_embed} is not the "
                  f"architecture of the fused kernels (8 x 256, skip at 4, degrees 10 / 4, full log-scale encodings): running the layer-by-layer {how} GEMM "
                  f"path (ops.GenericMLP), several times slower per sample point{note}", RuntimeWarning, stacklevel=3)


# ----------------------------------------------------------------------------- V1
def renderer_flags(white_bkgd: bool, sigma_activation: str = "relu") -> int:
    """The renderer option word of the compositing entry points (include/nsr.h): white background | softplus density."""
    if sigma_activation not in ("relu", "softplus"):
        raise ValueError(f"sigma_activation={sigma_activation!r}: 'relu' or 'softplus' (models/rendering.py:69-73)")
    return (_lib.NSR_WHITE_BKGD if white_bkgd else 0) | (_lib.NSR_SIGMA_SOFTPLUS if sigma_activation == "softplus" else 0)


class VolumetricRenderer:
    """Alpha compositing; mirrors models/rendering.py:66-111 (``opt.sigma_activation``: 'relu' or 'softplus' =
    ``log(1 + exp(sigma - 1))``, :69-73)."""

    def __init__(self, opt=None):
        self.sigma_activation = getattr(opt, "sigma_activation", "relu") if opt is not None else "relu"
        renderer_flags(False, self.sigma_activation)     # validates

    def forward(self, rgb, sigma, z_vals, white_bkgd: bool):
        rgb, sigma, z_vals = _f32(rgb, "rgb"), _f32(sigma, "sigma"), _f32(z_vals, "z_vals")
        R, N = z_vals.shape
        if rgb.shape != (R, N, 3) or sigma.shape != (R, N):
            raise ValueError("rgb must be (R,N,3) and sigma (R,N) matching z_vals (R,N)")
        dev = z_vals.device
        comp = torch.empty(R, 3, dtype=torch.float32, device=dev)
        depth = torch.empty(R, dtype=torch.float32, device=dev)
        opac = torch.empty(R, dtype=torch.float32, device=dev)
        w = torch.empty(R, N, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().nsr_composite(_p(rgb), 3, _p(sigma), 1, _p(z_vals), R, N, renderer_flags(white_bkgd, self.sigma_activation),
                                             _p(comp), _p(depth), _p(opac), _p(w), _stream()), "nsr_composite")
        return comp, depth, opac, w

    __call__ = forward


# ----------------------------------------------------------------------------- D2 / D3
def _arch_render_rays(model: "GenericMLP", rays: torch.Tensor, z_vals: torch.Tensor, sigma_only: bool) -> torch.Tensor:
    """One ``nsr_arch_fused_render_rays`` launch over all R * N sample points (not chunked: there are no encoded rows whose
    size a chunk would bound) -> the (R, N, 4) buffer, or (R, N, 1) under ``sigma_only``."""
    if not isinstance(model, GenericMLP):
        raise TypeError(f"render_rays takes a VanillaMLP or a GenericMLP built with fused=True, not {type(model).__name__}")
    if not model.fused:
        raise ValueError("render_rays needs the fused kernels: this GenericMLP runs layer by layer (built without fused=True) -- "
                         "use the explicit route, model(cat([PositionalEncoding(points), PositionalEncoding(dirs) repeated]))")
    if model._sd is None:
        raise RuntimeError("render_rays called before load_state_dict")
    rays, z_vals = _rays_z(rays, z_vals)
    R, N = z_vals.shape
    raw = torch.empty(R, N, 1 if sigma_only else 4, dtype=torch.float32, device=rays.device)
    model._route.render_rays(rays, z_vals, raw, sigma_only)
    return raw


def render_rays(model, rays: torch.Tensor, z_vals: torch.Tensor):
    """Fused render_rays (models/nerf_downX_model.py:260-278): MLP at every sample of
    every ray, positional encodings computed in-kernel.  rays (R,8), z (R,N) ->
    ``(rgbs (R,N,3), sigmas (R,N))`` as views of one (R,N,4) buffer.

    ``model``: a ``VanillaMLP``, or a ``GenericMLP`` built with ``fused=True`` (nsr_arch_fused_render_rays: one launch for
    all R * N points, bit-identical to the network on the explicitly encoded rows, ``color_activation none`` and the
    network's status word as there; ``gamma_correct`` stays the caller's, as on the explicit route).  A layer-by-layer
    ``GenericMLP`` has no ray-level kernel: ``ValueError``."""
    if isinstance(model, GenericMLP):
        raw = _arch_render_rays(model, rays, z_vals, False)
        return raw[..., :3], raw[..., 3]
    rays, z_vals = _rays_z(rays, z_vals)
    R, N = z_vals.shape
    stride = _ray_stride(rays)
    raw = torch.empty(R, N, 4, dtype=torch.float32, device=rays.device)
    _lib.check(_lib.load().nsr_render_rays(_p(model.packed), model._prec, _p(rays), stride, _p(z_vals), R, N, _p(raw),
                                           _stream()), "nsr_render_rays")
    return raw[..., :3], raw[..., 3]


def render_rays_sigma(model: "GenericMLP", rays: torch.Tensor, z_vals: torch.Tensor) -> torch.Tensor:
    """The density-only form of ``render_rays`` for a fused ``GenericMLP`` (the reference's ``sigma_only``,
    models/networks.py:182-226): trunk and density head, no colour branch, no direction encoding -> sigmas (R, N), the
    bits of ``render_rays(...)[1]``."""
    return _arch_render_rays(model, rays, z_vals, True)[..., 0]


def check_early_stop(early_stop: float, net, n_last: int, sigma_activation: str = "relu") -> float:
    """Validates the early-ray-termination threshold of ``render_rays_composited`` / ``forward_rays`` against everything the
    bound of include/nsr.h needs (``n_last``: the sample count of the pass that would be cut) and returns it as a float; a
    ``ValueError`` names the condition that fails -- the option is never ignored silently.  0 is "off" and always passes."""
    eps = float(early_stop)
    if not (0.0 <= eps < 1.0):          # NaN included
        raise ValueError(f"early_stop={early_stop!r}: a transmittance threshold in [0, 1) (0 = off)")
    if eps == 0.0:
        return eps
    if getattr(net, "embed", 0):
        raise ValueError(f"early_stop needs the 8 x 256 render kernel, which has no embedding options: the network was built with "
                         f"{embed_names(net.embed)}")
    if not isinstance(net, VanillaMLP) or net.precision != "f16x3":
        raise ValueError(f"early_stop needs precision 'f16x3' (the split-fp16 render kernel), not {getattr(net, 'precision', None)!r}")
    if sigma_activation != "relu":
        raise ValueError("early_stop needs the relu density: under sigma_activation='softplus' a raw density of 0 still has weight")
    if net.color_activation == "none":
        raise ValueError("early_stop needs colours in [0, 1]: the network was built with color_activation='none'")
    if int(n_last) not in (64, 128):
        raise ValueError(f"early_stop needs 64 or 128 samples in the pass that is cut, not {int(n_last)}")
    return eps


def render_rays_composited(model: VanillaMLP, rays: torch.Tensor, z_vals: torch.Tensor, white_bkgd: bool,
                           want_raw: bool = False, sigma_activation: str = "relu", early_stop: float = 0.0,
                           want_cut_count: bool = False):
    """``render_rays`` + ``VolumetricRenderer.forward`` in one launch (models/nerf_downX_model.py:289-291): 64 or 128
    samples per ray, fp32 / f16x3; f16x3 also 192 or 256.  Returns ``(comp_rgb (R,3), depth (R), opacity (R), weights (R,N))`` and, if
    ``want_raw``, the (R, N, 4) network output as a fifth element.  Bit-identical to the two-call route.

    ``early_stop`` = eps > 0 (f16x3 only): early ray termination -- a group of four consecutive rays stops after a 32-sample
    window once every one of its rays has optical depth >= -ln(eps); outputs move by at most eps + 2e-6 (include/nsr.h).
    Not bit-identical to anything, not combinable with ``want_raw``.  ``want_cut_count`` appends the number of windows not
    run as a 1-element int32 device tensor (0 with the option off)."""
    rays, z_vals = _rays_z(rays, z_vals)
    R, N = z_vals.shape
    dev = rays.device
    eps = check_early_stop(early_stop, model, N, sigma_activation)
    if eps > 0.0 and want_raw:
        raise ValueError("early_stop and want_raw exclude each other: the windows that are cut have no network output")
    comp = torch.empty(R, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(R, dtype=torch.float32, device=dev)
    opac = torch.empty(R, dtype=torch.float32, device=dev)
    w = torch.empty(R, N, dtype=torch.float32, device=dev)
    raw = torch.empty(R, N, 4, dtype=torch.float32, device=dev) if want_raw else None
    cut = torch.zeros(1, dtype=torch.int32, device=dev) if want_cut_count else None
    if eps > 0.0:
        _lib.check(_lib.load().nsr_render_rays_composited_ert(_p(model.packed), model._prec, _p(rays), _ray_stride(rays), _p(z_vals), R, N,
                                                              renderer_flags(white_bkgd, sigma_activation), eps, _p(comp), _p(depth),
                                                              _p(opac), _p(w), _p(cut), _stream()), "nsr_render_rays_composited_ert")
        return (comp, depth, opac, w, cut) if want_cut_count else (comp, depth, opac, w)
    _lib.check(_lib.load().nsr_render_rays_composited(_p(model.packed), model._prec, _p(rays), _ray_stride(rays), _p(z_vals), R, N,
                                                      renderer_flags(white_bkgd, sigma_activation), _p(raw), _p(comp), _p(depth), _p(opac), _p(w),
                                                      _stream()), "nsr_render_rays_composited")
    res = (comp, depth, opac, w, raw) if want_raw else (comp, depth, opac, w)
    return res + (cut,) if want_cut_count else res


FUSED_SAMPLES_F16X3 = (64, 128, 192, 256)     # sample counts of the split-fp16 render + composite launch (include/nsr.h)


def check_density_coarse(net, n_coarse: int, n_importance: Optional[int] = None) -> None:
    """Validates the test-time mode (``coarse_rgb=False`` / ``render_rays_density``): a ``ValueError`` names the condition
    that fails -- the option is never ignored silently.  ``n_importance`` None: a direct density launch (no fine pass)."""
    if getattr(net, "embed", 0):
        raise ValueError(f"coarse_rgb=False (the density-only pass) needs the 8 x 256 render kernel, which has no embedding options: "
                         f"the network was built with {embed_names(net.embed)}")
    if not isinstance(net, VanillaMLP) or net.precision != "f16x3":
        raise ValueError(f"coarse_rgb=False (the density-only pass) needs precision 'f16x3' (the split-fp16 render kernel), "
                         f"not {getattr(net, 'precision', None)!r}")
    if int(n_coarse) not in FUSED_SAMPLES_F16X3:
        raise ValueError(f"coarse_rgb=False (the density-only pass) needs 64, 128, 192 or 256 samples per ray, not {int(n_coarse)}")
    if n_importance is not None and int(n_importance) <= 0:
        raise ValueError("coarse_rgb=False needs a fine pass (N_importance > 0): without one the coarse colour is the image")


def render_rays_density(model: VanillaMLP, rays: torch.Tensor, z_vals: torch.Tensor, sigma_activation: str = "relu"):
    """The density-only pass of ``render_rays_composited`` (f16x3; 64, 128, 192 or 256 samples per ray): trunk and density
    head at every sample, no colour branch, then compositing.  Returns ``(depth (R), opacity (R), weights (R, N))``,
    bit-identical to the same three outputs of ``render_rays_composited`` under either density: what a coarse pass that only
    feeds the resampler needs (the reference's ``sigma_only``, models/networks.py:182-226)."""
    rays, z_vals = _rays_z(rays, z_vals)
    R, N = z_vals.shape
    dev = rays.device
    check_density_coarse(model, N)
    flags = renderer_flags(False, sigma_activation)
    depth = torch.empty(R, dtype=torch.float32, device=dev)
    opac = torch.empty(R, dtype=torch.float32, device=dev)
    w = torch.empty(R, N, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().nsr_render_rays_density(_p(model.packed), model._prec, _p(rays), _ray_stride(rays), _p(z_vals), R, N, flags,
                                                   _p(depth), _p(opac), _p(w), _stream()), "nsr_render_rays_density")
    return depth, opac, w


OUT_KEYS = ("coarse_comp_rgbs", "coarse_depth", "coarse_opacity", "coarse_weights",
            "fine_comp_rgbs", "fine_depth", "fine_opacity", "fine_weights")


def forward_rays(coarse: VanillaMLP, fine: Optional[VanillaMLP], rays: torch.Tensor, N_coarse: int = 64,
                 N_importance: int = 64, white_bkgd: bool = False, lindisp: bool = False,
                 workspace: Optional[torch.Tensor] = None, outs: Optional[Dict[str, torch.Tensor]] = None,
                 want_weights: bool = True, events=None, check: bool = False,
                 sigma_activation: str = "relu", early_stop: float = 0.0,
                 cut_count: Optional[torch.Tensor] = None, coarse_rgb: bool = True) -> Dict[str, torch.Tensor]:
    """Eval-mode forward_rays for the WHOLE batch in one enqueue sequence
    (models/nerf_downX_model.py:280-324; with 11-wide rays: the vanilla model's models/nerf_model.py:207-242):
    returns the reference's 8-entry dict.
    ``workspace`` / ``outs`` let a caller reuse buffers across frames; ``events`` (4 raw
    hipEvent_t handles from ``HipEvents``) brackets the coarse / fine MLP launches.
    ``check=True`` reads both networks' numerics status words after the enqueue (one stream wait) and raises
    ``NsrNumericsError`` on non-finite inputs / outputs or out-of-range activations -- the reference's NaN trap
    (models/nerf_downX_model.py:273-274) as an exception; ``False`` leaves the sticky flags for a later
    ``net.check()`` / ``net.status()`` (nothing is synchronised).
    ``early_stop`` = eps > 0 (f16x3 only): early ray termination in the LAST network pass (the fine one, or the coarse one when
    ``N_importance == 0``; the coarse pass that feeds the resampler is never cut), see ``render_rays_composited`` and
    include/nsr.h; ``cut_count``: a 1-element int32 device tensor the launch ADDS the number of windows not run to.
    ``coarse_rgb=False`` (f16x3, ``N_importance > 0``, ``N_coarse`` 64 / 128 / 192 / 256): test-time mode -- the coarse pass
    runs the density-only launch (``render_rays_density``); the returned dict has no ``coarse_comp_rgbs`` (a caller's
    ``outs["coarse_comp_rgbs"]`` is neither read nor written) and the seven other outputs are bit-identical."""
    if not coarse_rgb:
        check_density_coarse(coarse, N_coarse, N_importance)
    lib = _lib.load()
    rays = _f32(rays, "rays")
    rays = rays.reshape(-1, rays.shape[-1])
    stride = _ray_stride(rays)
    R = rays.shape[0]
    if N_importance > 0 and fine is None:
        raise ValueError("N_importance > 0 needs the fine network")
    if fine is not None and fine._prec != coarse._prec:
        raise ValueError("coarse and fine networks must use the same precision")
    eps = check_early_stop(early_stop, fine if N_importance > 0 else coarse, N_coarse + N_importance, sigma_activation)
    if cut_count is not None and (cut_count.dtype != torch.int32 or cut_count.numel() != 1 or cut_count.device != rays.device):
        raise ValueError("cut_count must be a 1-element int32 tensor on the rays' device")
    dev = rays.device
    need = lib.nsr_forward_rays_workspace_bytes_for(coarse._prec, R, N_coarse, N_importance)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    Nf = N_coarse + N_importance
    shapes = {"coarse_comp_rgbs": (R, 3), "coarse_depth": (R,), "coarse_opacity": (R,), "coarse_weights": (R, N_coarse),
              "fine_comp_rgbs": (R, 3), "fine_depth": (R,), "fine_opacity": (R,), "fine_weights": (R, Nf)}
    if outs is None:
        outs = {}
    keys = OUT_KEYS if N_importance > 0 else OUT_KEYS[:4]
    for k in keys:
        if (k.endswith("weights") and not want_weights) or (k == "coarse_comp_rgbs" and not coarse_rgb):
            continue
        if k not in outs or tuple(outs[k].shape) != shapes[k]:
            outs[k] = torch.empty(shapes[k], dtype=torch.float32, device=dev)
    ptrs = (c_void_p * 8)(*[_p(outs.get(k)) if (coarse_rgb or k != "coarse_comp_rgbs") else c_void_p(0) for k in OUT_KEYS])
    ev = (c_void_p * 4)(*events) if events is not None else None
    args = (_p(coarse.packed), _p(fine.packed) if fine is not None else c_void_p(0), coarse._prec, _p(rays), stride, R, N_coarse,
            N_importance, renderer_flags(white_bkgd, sigma_activation), int(bool(lindisp)), ptrs, _p(workspace), workspace.numel(),
            _stream(), ev)
    if not coarse_rgb:
        _lib.check(lib.nsr_forward_rays_density_coarse(*args, eps, _p(cut_count) if eps > 0.0 else c_void_p(0)),
                   "nsr_forward_rays_density_coarse")
    elif eps > 0.0:
        _lib.check(lib.nsr_forward_rays_ert(*args, eps, _p(cut_count)), "nsr_forward_rays_ert")
    else:
        _lib.check(lib.nsr_forward_rays_profiled(*args), "nsr_forward_rays")
    if check:
        coarse.check("coarse network")
        if fine is not None and N_importance > 0:
            fine.check("fine network")
    if not coarse_rgb:     # the reference's dict minus the entry that was not computed (a caller's buffer stays the caller's)
        return {k: v for k, v in outs.items() if k != "coarse_comp_rgbs"}
    return outs


class HipEvents:
    """n raw hipEvent_t handles (created through libnsr so they belong to its HIP runtime)."""

    def __init__(self, n: int):
        lib = _lib.load()
        self.handles = []
        for _ in range(n):
            h = c_void_p()
            _lib.check(lib.nsr_event_create(ctypes.byref(h)), "nsr_event_create")
            self.handles.append(h)

    def elapsed_ms(self, i: int, j: int) -> float:
        ms = c_float()
        _lib.check(_lib.load().nsr_event_elapsed_ms(self.handles[i], self.handles[j], ctypes.byref(ms)),
                   "nsr_event_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        try:
            lib = _lib.load()
            for h in self.handles:
                lib.nsr_event_destroy(h)
        except Exception:
            pass


# ----------------------------------------------------------------------------- A1 / A2
def sr_mean(hr: torch.Tensor, n_lr: int, s2: int) -> torch.Tensor:
    """``reshape(N_lr, s^2, c).mean(1)`` (models/nerf_downX_model.py:337-348)."""
    hr = _f32(hr, "hr")
    n_lr, s2 = int(n_lr), int(s2)
    if hr.ndim not in (1, 2) or n_lr < 0 or s2 < 1 or hr.shape[0] != n_lr * s2:
        raise ValueError(f"hr must be (n_lr * s2, c) or (n_lr * s2,) with n_lr * s2 = {n_lr * s2}, got {tuple(hr.shape)}")
    c = int(hr.shape[1]) if hr.ndim == 2 else 1
    lr = torch.empty(n_lr, c, dtype=torch.float32, device=hr.device)
    _lib.check(_lib.load().nsr_sr_mean(_p(hr), n_lr, s2, c, _p(lr), _stream()), "nsr_sr_mean")
    return lr


def unflatten_reshape(x: torch.Tensor, img_wh: Tuple[int, int], downscale: int) -> torch.Tensor:
    """(N_lr*s^2, c) -> HR image (H, W, c) (models/nerf_downX_model.py:410-416)."""
    x = _f32(x, "x")
    W, H = int(img_wh[0]), int(img_wh[1])
    if x.ndim not in (1, 2) or x.shape[0] != H * W:
        raise ValueError(f"x must be (H * W, c) or (H * W,) with H * W = {H * W}, got {tuple(x.shape)}")
    c = int(x.shape[1]) if x.ndim == 2 else 1
    out = torch.empty(H, W, c, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().nsr_unflatten(_p(x), H, W, int(downscale), c, _p(out), _stream()), "nsr_unflatten")
    return out
