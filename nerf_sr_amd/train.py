"""Host mirror of the reference's training iteration over ``include/nsr_train.h``.

``Trainer`` holds what ``NeRFDownXModel`` holds in train mode (``models/nerf_downX_model.py:133-205``): the two
networks' 24-tensor state dicts as fp32 device tensors, their gradients, and the Adam moments; its methods follow
the reference's call protocol:

    set_input(rays, rgbs)  ->  optimize_parameters()            (:235-248, :398-408)
        = forward (train mode) + comp_low_res_output + calculate_losses + backward + optimizer.step

All arithmetic runs in libnsr.so (``nsr_train_loss_and_grads``, ``nsr_adam_step_n``); torch supplies device memory,
the stream and the random draws (``torch.rand`` / ``torch.randn`` on the device, exactly the four tensors the
reference draws).  There is no CPU path.

For losses the fused step does not compute (``regularize_patch``'s TV loss, ``--sisr_path``, ``--with_ref``, gradient
clipping, anything written in torch), ``forward_rays_train`` is train-mode ``forward_rays`` as a ``torch.autograd.Function``
over ``nsr_train_forward`` / ``nsr_train_backward`` -- the same kernels, split at the loss -- and ``Trainer.forward`` /
``Trainer.backward`` / ``Trainer.regularize_patch`` / ``Trainer.clip_grads`` drive it with the trainer's own tensors:

    out = t.forward(); loss = my_loss(out); t.backward(loss); t.clip_grads(); t.optimizer_step()
"""
from __future__ import annotations

import ctypes
from ctypes import c_void_p
from typing import Dict, Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .ops import OUT_KEYS, _f32, _p, _ray_stride, _stream, renderer_flags, state_dict_to_device
from .weights import STATE_DICT_SPEC, check_state_dict_arch, pad_no_dir, DIR_W, arch_key, arch_spec
from .weights import normalize_arch as _normalize_arch
from .weights import check_embed, embed_names, EMBED_NO_XYZ


def _ptr_array(tensors):
    return (c_void_p * len(tensors))(*[c_void_p(t.data_ptr()) for t in tensors])


def _flat_like(params: Dict[str, torch.Tensor]):
    """One flat fp32 buffer + per-tensor views with the state_dict's shapes (so a whole network's gradients or
    Adam moments are ONE contiguous range: a single all-reduce / memset covers them).  Views start 16-byte aligned."""
    sizes = [(k, v.numel(), tuple(v.shape)) for k, v in params.items()]
    offs, total = [], 0
    for _, n, _ in sizes:
        offs.append(total)
        total += (n + 3) // 4 * 4
    flat = torch.zeros(total, dtype=torch.float32, device=next(iter(params.values())).device)
    views = {k: flat[o:o + n].view(shape) for (k, n, shape), o in zip(sizes, offs)}
    return flat, views


def linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, act: int = 0, transposed: bool = False):
    """One ``nn.Linear`` (+ activation) on the training GEMM (``nsr_linear``): y = act(x w^T + b).
    K must be a multiple of 32; returns y (P, N) and, if asked, also y^T (N, P)."""
    x, w = _f32(x, "x"), _f32(w, "w")
    if x.ndim != 2 or w.ndim != 2 or w.shape[1] != x.shape[1] or x.shape[1] % 32:
        raise ValueError(f"x must be (P, K) and w (N, K) with K a multiple of 32, got {tuple(x.shape)} and {tuple(w.shape)}")
    P, K = x.shape
    N = w.shape[0]
    if transposed and P % 4:
        raise ValueError(f"transposed=True needs a multiple of 4 rows (the leading dimension of y^T), got P = {P}")
    if b is not None:
        b = _f32(b, "b")
        if tuple(b.shape) != (N,):
            raise ValueError(f"b must be (N,) = ({N},), got {tuple(b.shape)}")
    y = torch.empty(P, N, dtype=torch.float32, device=x.device)
    yt = torch.empty(N, P, dtype=torch.float32, device=x.device) if transposed else None
    _lib.check(_lib.load().nsr_linear(_p(x), K, _p(w), K, _p(b), act, _p(y), N,
                                      _p(yt), P, P, K, N, _stream()), "nsr_linear")
    return (y, yt) if transposed else y


# ---------------------------------------------------------------------------------------------------------------------
# train-mode forward_rays as a torch.autograd.Function (nsr_train_forward / nsr_train_backward)
# ---------------------------------------------------------------------------------------------------------------------
class TrainWorkspace:
    """The training workspace: scratch of one pass + the sticky numerics status block at its start (include/nsr_train.h).
    Any number of pending forwards share it (each keeps its own saved state); it grows on demand and keeps its flags."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, need: int, device) -> torch.Tensor:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:      # "cuda" (Trainer's default) is the current device
            device = torch.device("cuda", torch.cuda.current_device())
        if self.buf is None or self.buf.numel() < need or self.buf.device != device:
            carried = self.status() if self.buf is not None else 0     # a regrown workspace keeps the sticky flags
            self.buf = torch.empty(need, dtype=torch.uint8, device=device)
            _lib.check(_lib.load().nsr_train_status_reset(_p(self.buf), _stream()), "nsr_train_status_reset")
            if carried:
                self.buf[:4].copy_(torch.tensor([carried], dtype=torch.int32).view(torch.uint8))
        return self.buf

    def status(self, clear: bool = False) -> int:
        if self.buf is None:
            return 0
        flags = ctypes.c_uint(0)
        _lib.check(_lib.load().nsr_train_status(_p(self.buf), int(bool(clear)), ctypes.byref(flags), _stream()), "nsr_train_status")
        return int(flags.value)


_DEFAULT_WS: Dict[torch.device, TrainWorkspace] = {}


def _weights(params, name: str, arch: Optional[dict] = None, no_xyz: bool = False):
    """A network's tensors in state_dict order for ``arch`` (None: the default network's 24): an nn.Module such as the
    reference's own ``netCoarse`` built with those flags (``parameters()`` has the state_dict's order), a dict keyed like
    ``weights.arch_spec``, or a sequence.  Count and shapes are checked before anything else about the tensors."""
    spec = STATE_DICT_SPEC if arch is None else arch_spec(no_xyz=no_xyz, **arch)
    if isinstance(params, torch.nn.Module):
        ts = list(params.parameters())
    elif isinstance(params, dict):
        missing = [k for k in spec if k not in params]
        if missing:
            raise ValueError(f"{name}: missing keys {missing}")
        ts = [params[k] for k in spec]
    else:
        ts = list(params)
    if len(ts) != len(spec):
        raise ValueError(f"{name}: expected {len(spec)} tensors, got {len(ts)}")
    for i, (t, (k, shape)) in enumerate(zip(ts, spec.items())):
        if arch is None and k == DIR_W and tuple(t.shape) == (shape[0], shape[1] - 27):
            # --no_dir (models/networks.py:160-169): the narrow layer with 27 zero columns (weights.pad_no_dir, as Trainer
            # holds it); the padding is a constant, so autograd hands the narrow weight the gradient of its 256 columns
            ts[i] = t = pad_no_dir(t)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: {k} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    for t, k in zip(ts, spec):
        _f32(t, f"{name}.{k}")
    return [t if t.is_contiguous() else t.contiguous() for t in ts]


# ---------------------------------------------------------------------------------------------------------------------
# non-default architectures (--D --W --skips --deg_pos --deg_dir --no_dir): struct nsr_arch of include/nsr_train.h
# ---------------------------------------------------------------------------------------------------------------------
# what the layer-by-layer training pair runs; 'f16x3' maps to 'f16x3_gemm'.  'f16x3_gemm_bwd' (opt-in) is 'f16x3_gemm' with every
# gradient product on the split-fp16 MFMA as well (three terms, fp32 accumulation; include/nsr_train.h NSR_F16X3_GEMM_BWD)
ARCH_PRECISIONS = ("fp32", "f16x3_gemm", "f16x3_gemm_bwd")
_ARCH_WARNED = set()


def normalize_arch(arch) -> dict:
    """``weights.normalize_arch`` (a dict with any of D, W, skips, deg_pos, deg_dir, no_dir, or an options object carrying the
    reference's flags; validates, ValueError) for the training pair, whose compositor renders three colours."""
    a = _normalize_arch(arch)
    if a["dim_rgb"] != 3:
        raise ValueError("arch: dim_rgb must be 3 (the compositor renders three colours)")
    return a


def arch_precision(arch: dict, precision: str) -> str:
    """The precision the layer-by-layer pair runs for ``precision``: 'fp32', 'f16x3_gemm' and 'f16x3_gemm_bwd' as they are; 'f16x3' (the
    chain kernels, laid out for the default network) maps to 'f16x3_gemm' -- the same split-fp16 forward products, gradients
    on the fp32 MFMA -- with one RuntimeWarning per architecture and process; the other chain names raise ValueError."""
    if precision in ARCH_PRECISIONS:
        return precision
    if precision != "f16x3":
        raise ValueError(f"precision={precision!r} with arch=...: a non-default architecture trains layer by layer under "
                         f"{list(ARCH_PRECISIONS)} ('f16x3' maps to 'f16x3_gemm'); the chain kernels are the default network's")
    key = arch_key(arch, no_dir=True)
    if key not in _ARCH_WARNED:
        _ARCH_WARNED.add(key)
        import warnings
        warnings.warn(f"training architecture D={arch['D']} W={arch['W']} skips={list(arch['skips'])} degrees "
                      f"{arch['deg_pos']}/{arch['deg_dir']}: precision 'f16x3' names the chain kernels of the default 8 x 256 "
                      "network; running 'f16x3_gemm' (layer by layer, forward products split-fp16, gradients fp32)",
                      RuntimeWarning, stacklevel=3)
    return "f16x3_gemm"


def embed_precision(embed: int, precision: str) -> str:
    """``arch_precision`` for a network with an embedding option: the layer-by-layer precisions as they are; every chain name
    raises ``ValueError`` naming the option (the chain kernels compute the full log-scale encodings)."""
    if precision in ARCH_PRECISIONS:
        return precision
    raise ValueError(f"precision={precision!r} with {embed_names(embed)}: the embedding options train layer by layer under "
                     f"{list(ARCH_PRECISIONS)}; the chain kernels are the default network's, with its encodings")


def train_flags(white_bkgd: bool = False, gamma_correct: bool = False, sigma_activation: str = "relu",
                color_activation: str = "sigmoid", stop_grad: bool = False) -> int:
    """The option word of the training entry points (include/nsr_train.h): the renderer's word (``ops.renderer_flags``) plus
    --gamma_correct (render_rays applies rgb ** (1 / 2.2) per sample in training too, models/nerf_downX_model.py:271-276),
    --color_activation none (models/networks.py:173-180) and --stop_grad (:127, 218-219).  Validates (ValueError)."""
    if sigma_activation not in ("relu", "softplus") or color_activation not in ("sigmoid", "none"):
        raise ValueError("sigma_activation: 'relu' or 'softplus'; color_activation: 'sigmoid' or 'none'")
    if gamma_correct and color_activation == "none":
        raise ValueError("gamma_correct with color_activation='none': pow(rgb, 1 / 2.2) of an unbounded head is NaN for every negative value")
    return renderer_flags(white_bkgd, sigma_activation) | (_lib.NSR_TRAIN_GAMMA_CORRECT if gamma_correct else 0) \
        | (_lib.NSR_TRAIN_COLOR_NONE if color_activation == "none" else 0) | (_lib.NSR_TRAIN_STOP_GRAD if stop_grad else 0)


DRAW_KEYS = ("u_coarse", "u_fine", "noise_coarse", "noise_fine")


def _draws(draws, R: int, nc: int, ni: int, device) -> Dict[str, Optional[torch.Tensor]]:
    """The four random tensors of one train-mode forward as dense fp32 device tensors of the shapes the kernels read --
    ``u_coarse`` / ``noise_coarse`` (R, Nc), ``u_fine`` (R, Ni), ``noise_fine`` (R, Nc + Ni) -- or None; ValueError otherwise."""
    shapes = {"u_coarse": (R, nc), "u_fine": (R, ni), "noise_coarse": (R, nc), "noise_fine": (R, nc + ni)}
    out = {}
    for k in DRAW_KEYS:
        v = (draws or {}).get(k)
        if v is not None:
            v = _f32(torch.as_tensor(v, device=device), k)
            if tuple(v.shape) != shapes[k]:
                raise ValueError(f"draws[{k!r}] must be {shapes[k]} for {R} rays and {nc} + {ni} samples, got {tuple(v.shape)}")
        out[k] = v
    return out


def _rays_per_pass(ray_chunk: int, R: int) -> int:
    """The effective ray chunk of a batch of R rays (``ray_chunk`` 0 = all)."""
    return ray_chunk if 0 < ray_chunk < R else R


def _alloc_outs(R: int, nc: int, ni: int, device):
    """The eight output tensors of one train-mode forward, in ``OUT_KEYS`` order."""
    stage = lambda n: [torch.empty(R, 3, device=device), torch.empty(R, device=device), torch.empty(R, device=device),
                       torch.empty(R, n, device=device)]
    return stage(nc) + stage(nc + ni)


class _TrainRun:
    """The arguments of one forward_rays_train call that are not tensors, and the pair of entry points it runs: the default
    network's, or with ``arch`` (struct nsr_arch) the layer-by-layer pair, which differs by that leading argument only."""

    def __init__(self, nc, ni, flags, lindisp, noise_std, prec, chunk, workspace, arch=None, embed: int = 0, ray_grad: bool = False,
                 chain_ray_grad: bool = False):
        self.nc, self.ni, self.flags, self.lindisp = nc, ni, flags, lindisp
        self.noise_std, self.prec, self.chunk, self.workspace = noise_std, prec, chunk, workspace
        self.arch = arch
        self.lead = () if arch is None else (ctypes.byref(arch),)
        self.embed = int(embed)
        self.names = {"saved_bytes": "nsr_train_saved_bytes", "workspace_bytes": "nsr_train_workspace_bytes_for",
                      "forward": "nsr_train_forward", "backward": "nsr_train_backward"} if arch is None else \
            {"saved_bytes": "nsr_train_arch_saved_bytes", "workspace_bytes": "nsr_train_arch_workspace_bytes",
             "forward": "nsr_train_arch_forward", "backward": "nsr_train_arch_backward"}
        self.ray_grad = bool(ray_grad)      # rays that require grad: the `_r` backward and its workspace (always behind a descriptor)
        if self.embed or self.ray_grad:      # the embedding's option word behind the descriptor: the `_e` forms of the same four (include/nsr_train.h)
            self.lead += (self.embed,)
            self.names = {k: v + "_e" for k, v in self.names.items()}
        if self.ray_grad:
            self.names.update(workspace_bytes="nsr_train_arch_workspace_bytes_r", backward="nsr_train_arch_backward_r")
        # rays that require grad on the chain pair (the default network under a chain precision, opt-in): the forward is
        # nsr_train_forward as it is, the backward nsr_train_backward_r, which also takes the rays and an option word
        self.chain_ray_grad = bool(chain_ray_grad)
        if self.chain_ray_grad:
            assert arch is None and not self.embed and not self.ray_grad
            self.names.update(workspace_bytes="nsr_train_workspace_bytes_r", backward="nsr_train_backward_r")

    def call(self, what: str, *args):
        """``(name, result)`` of this run's entry point ``what`` on ``args`` behind the leading descriptor."""
        name = self.names[what]
        return name, getattr(_lib.load(), name)(*self.lead, *args)


class _ForwardRaysTrain(torch.autograd.Function):
    """Outputs: the eight OUT_KEYS tensors.  Inputs: the run, rays, the four draws, then both networks' weight tensors (48;
    2 (2 D + 8) with an architecture)."""

    @staticmethod
    def forward(ctx, run, rays, u_c, u_f, n_c, n_f, *weights):
        R, nc, ni = rays.shape[0], run.nc, run.ni
        dev = rays.device
        outs = _alloc_outs(R, nc, ni, dev)
        what, nbytes = run.call("saved_bytes", run.prec, R, nc, ni, run.chunk)
        if nbytes == 0:
            raise _lib.NsrError(f"{what}: no saved state for R={R}, samples {nc} + {ni}, ray_chunk {run.chunk} "
                                "(every ray chunk must hold a multiple of 32 sample points in both networks)")
        saved = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ctx.ws_need = run.call("workspace_bytes", run.prec, _rays_per_pass(run.chunk, R), nc, ni)[1]
        ws = run.workspace.get(ctx.ws_need, dev)
        nt = len(weights) // 2
        what, rc = run.call(
            "forward", _ptr_array(weights[:nt]), _ptr_array(weights[nt:]), _p(rays), _ray_stride(rays), R, nc, ni, run.flags, run.lindisp,
            _p(u_c), _p(u_f), _p(n_c), _p(n_f), run.noise_std, run.prec, run.chunk, _ptr_array(outs),
            _p(ws), ws.numel(), _p(saved), saved.numel(), _stream())
        _lib.check(rc, what)
        # an in-place update of a weight before the backward fails autograd's version check; the chain pair's ray gradient
        # recomputes the encodings from the rays, which are therefore kept the same way
        ctx.save_for_backward(*weights, *((rays,) if run.chain_ray_grad else ()))
        ctx.run, ctx.state, ctx.rays_shape = run, saved, tuple(rays.shape)
        ctx.set_materialize_grads(False)     # an output the loss does not use arrives as None: a NULL upstream gradient
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *g_outs):
        weights = ctx.saved_tensors
        saved = ctx.state
        if saved is None:
            raise RuntimeError("forward_rays_train: the saved state of this forward was released by its first backward")
        g_outs = [None if g is None else g.to(torch.float32).contiguous() for g in g_outs]
        if ctx.run.chain_ray_grad:
            return _ForwardRaysTrain._backward_chain_rays(ctx, weights[:-1], weights[-1], g_outs)
        grads = [torch.empty_like(w) for w in weights]
        ws = ctx.run.workspace.get(ctx.ws_need, saved.device)
        nt = len(weights) // 2
        g_rays = torch.empty(ctx.rays_shape, dtype=torch.float32, device=saved.device) if ctx.run.ray_grad else None
        to_rays = (_p(g_rays), ctx.rays_shape[1]) if ctx.run.ray_grad else ()      # the `_r` backward: g_rays, g_ray_stride
        what, rc = ctx.run.call(
            "backward", _ptr_array(weights[:nt]), _ptr_array(weights[nt:]), (c_void_p * 8)(*[_p(g) for g in g_outs]),
            _ptr_array(grads[:nt]), _ptr_array(grads[nt:]), *to_rays, _p(ws), ws.numel(), _p(saved), saved.numel(), _stream())
        _lib.check(rc, what)
        ctx.state = None
        return (None, g_rays) + (None,) * 4 + tuple(grads)

    @staticmethod
    def _backward_chain_rays(ctx, weights, rays, g_outs):
        """``nsr_train_backward_r``: d(loss)/d(rays) from the backward chain's panels; a frozen field (no weight leaf needs a
        gradient) skips the weight-gradient launches."""
        saved = ctx.state
        nt = len(weights) // 2
        frozen = not any(ctx.needs_input_grad[6:])
        grads = [] if frozen else [torch.empty_like(w) for w in weights]
        ws = ctx.run.workspace.get(ctx.ws_need, saved.device)
        g_rays = torch.empty(ctx.rays_shape, dtype=torch.float32, device=saved.device)
        what, rc = ctx.run.call(
            "backward", _ptr_array(weights[:nt]), _ptr_array(weights[nt:]), _p(rays), ctx.rays_shape[1],
            (c_void_p * 8)(*[_p(g) for g in g_outs]), None if frozen else _ptr_array(grads[:nt]),
            None if frozen else _ptr_array(grads[nt:]), _p(g_rays), ctx.rays_shape[1],
            _lib.NSR_BACKWARD_NO_WEIGHT_GRADS if frozen else 0, _p(ws), ws.numel(), _p(saved), saved.numel(), _stream())
        _lib.check(rc, what)
        ctx.state = None
        return (None, g_rays) + (None,) * 4 + (tuple(grads) if not frozen else (None,) * len(weights))


def forward_rays_train(params_c, params_f, rays: torch.Tensor, draws: Optional[Dict[str, Optional[torch.Tensor]]] = None, *,
                       N_coarse: int = 64, N_importance: int = 64, white_bkgd: bool = False, lindisp: bool = False,
                       noise_std: float = 0.0, gamma_correct: bool = False, sigma_activation: str = "relu",
                       color_activation: str = "sigmoid", stop_grad: bool = False, precision: str = "f16x3",
                       ray_chunk: int = 0, workspace: Optional[TrainWorkspace] = None, arch=None, embed: int = 0,
                       chain_ray_grad: bool = False) -> Dict[str, torch.Tensor]:
    """Train-mode ``forward_rays`` (``models/nerf_downX_model.py:280-313``) that autograd differentiates with respect to the
    24 + 24 weight tensors of ``params_c`` / ``params_f`` (the reference's ``netCoarse`` / ``netFine`` modules, their
    parameter lists, or state-dict-like dicts such as ``Trainer.params``).  Returns the eight ``OUT_KEYS`` outputs; any loss
    written in torch over them back-propagates through ``nsr_train_backward`` (once: the backward is not differentiable).

    ``draws``: ``u_coarse`` (R, Nc), ``u_fine`` (R, Ni), ``noise_coarse`` (R, Nc), ``noise_fine`` (R, Nc + Ni) fp32 on the device
    (a host tensor or array is copied there; another shape is a ``ValueError``), or None for the deterministic branch of that stage (``Trainer.draw`` makes them in the reference's order).  ``ray_chunk``:
    rays per pass (0 = all).  Every call keeps its own saved state (5.4 KB per sample point under 'f16x3', include/nsr_train.h)
    until its backward; ``workspace`` (shared scratch + the sticky status block) defaults to one per device.

    ``arch``: the architecture flags of both networks (a dict with any of D, W, skips, deg_pos, deg_dir, no_dir, or an options
    object carrying ``--D --W --skips --deg_pos --deg_dir --no_dir``): the layer-by-layer pair ``nsr_train_arch_forward`` /
    ``nsr_train_arch_backward`` over the 2 D + 8 tensors of each network, e.g. the reference's own ``netCoarse`` /
    ``netFine`` built with those flags.  ``precision``: 'fp32', 'f16x3_gemm' or 'f16x3_gemm_bwd' ('f16x3' maps to 'f16x3_gemm' with
    one RuntimeWarning per architecture; the chain names raise ValueError).  None = the default network, as before.
    'f16x3_gemm_bwd' (opt-in) has 'f16x3_gemm''s forward, bit for bit, and runs every product of the backward -- input gradients,
    weight gradients, the ray gradient's products -- on the split-fp16 MFMA too: hi / lo fp16 halves, three MFMAs per product
    (lo hi + hi lo + hi hi), fp32 accumulation, gradients scaled by exact powers of two per sample point (input gradients) or
    per matrix (weight gradients).

    ``rays`` that require grad get ``d(loss)/d(rays)`` (``nsr_train_arch_backward_r``) when the run is the layer-by-layer pair's:
    ``arch=`` or ``embed=`` given, or ``precision`` 'fp32' / 'f16x3_gemm' on the default network (which then runs as the default
    descriptor, the same bits); the chain precisions raise ``ValueError``.  A sample point is ``o + z d`` with ``z`` independent
    of ``o`` and ``d`` (the fine depths come from the detached coarse weights and near / far only, as in the reference); columns
    6:8 (near, far) get exact zeros -- the gradient with respect to near / far needs the resampler's backward and is not computed.
    At 11 columns the direction encoding's part goes to columns 8:11, at 8 it joins columns 3:6; none under ``stop_grad``.

    ``chain_ray_grad=True`` (opt-in) lifts that refusal: rays that require grad under a chain precision on the default network
    run the chain pair, and the backward is ``nsr_train_backward_r`` -- three small products of the backward chain's gradient
    panels with the weight columns of the encoded position / direction on the fp16 MFMA, the encodings' backward on sin / cos
    recomputed from the rays (which are saved like the weights: an in-place change before the backward is an error).  The
    outputs and the weight gradients have the bits of the same call with rays that do not require grad.  When no weight needs
    a gradient (a frozen field) the weight-gradient launches are skipped.  With ``arch=`` / ``embed=`` or 'fp32' / 'f16x3_gemm'
    the keyword has no effect: those run the layer-by-layer pair as above.

    ``embed``: the embedding's option word (``weights.embed_of(opt)``: ``--no_xyz`` / ``--no_logscale``).  A non-zero word runs the
    layer-by-layer pair (``nsr_train_arch_forward_e`` / ``_backward_e``) -- on the default descriptor when ``arch`` is None -- over
    networks whose layer 0, skip layers and ``dir_encoding`` have the option's widths (``weights.arch_spec(no_xyz=...)``)."""
    ray_grad = bool(rays.requires_grad)
    if ray_grad:      # the tensor the extra gradient is for is looked at first
        _ray_stride(_f32(rays, "rays"))
    chain_rays = ray_grad and bool(chain_ray_grad) and arch is None and not int(embed) and precision not in ARCH_PRECISIONS
    if chain_rays:
        ray_grad = False      # the chain pair itself: no descriptor, nsr_train_backward_r behind nsr_train_forward
    if ray_grad and arch is None and not int(embed) and precision not in ARCH_PRECISIONS:
        raise ValueError(f"forward_rays_train: rays require grad under precision={precision!r}: the gradient with respect to rays "
                         f"is the layer-by-layer pair's, precision {list(ARCH_PRECISIONS)} (or arch= / embed=); the chain kernels "
                         "do not differentiate through the encodings")
    flags = train_flags(white_bkgd, gamma_correct, sigma_activation, color_activation, stop_grad)
    embed = int(embed)
    if (embed or ray_grad) and arch is None:     # the chain kernels have no embedding options and no ray gradient: the default
        arch = {}                                # network as a descriptor
    if arch is not None:      # everything about the architecture is checked before a device is touched
        arch = normalize_arch(arch)
        check_embed(embed, arch)
        precision = embed_precision(embed, precision) if embed else arch_precision(arch, precision)
        no_xyz = bool(embed & EMBED_NO_XYZ)
        wc, wf = _weights(params_c, "params_c", arch, no_xyz), _weights(params_f, "params_f", arch, no_xyz)
    rays = _f32(rays, "rays")
    _ray_stride(rays)
    if precision not in _lib.TRAIN_PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_lib.TRAIN_PRECISIONS)}")
    if arch is None:          # the default network's order of checks: the rays come first
        wc, wf = _weights(params_c, "params_c"), _weights(params_f, "params_f")
    for t in wc + wf:
        if t.device != rays.device:
            raise ValueError("the weights must live on the rays' device")
    d = list(_draws(draws, rays.shape[0], int(N_coarse), int(N_importance), rays.device).values())
    if workspace is None:
        workspace = _DEFAULT_WS.setdefault(rays.device, TrainWorkspace())
    run = _TrainRun(int(N_coarse), int(N_importance), flags, int(bool(lindisp)), float(noise_std),
                    _lib.TRAIN_PRECISIONS[precision], int(ray_chunk), workspace,
                    None if arch is None else _lib.NsrArch.from_arch(arch), embed, ray_grad, chain_rays)
    outs = _ForwardRaysTrain.apply(run, rays, *d, *wc, *wf)
    return dict(zip(OUT_KEYS, outs))


def tv_loss(x: torch.Tensor) -> torch.Tensor:
    """Total-variation loss of an (H, W, C) image as the reference's TVLoss defines it (models/criterions.py:56-69): the mean
    squared difference of vertically adjacent pixels plus that of horizontally adjacent ones."""
    dh = x[1:, :, :] - x[:-1, :, :]
    dw = x[:, 1:, :] - x[:, :-1, :]
    return dh.pow(2).sum() / dh.numel() + dw.pow(2).sum() / dw.numel()


class Trainer:
    """Coarse + fine networks, gradients, Adam state and one-call training iterations."""

    def __init__(self, sd_coarse, sd_fine, N_coarse: int = 64, N_importance: int = 64, white_bkgd: bool = False,
                 lindisp: bool = False, downscale: int = 2, randomized: bool = True, noise_std: float = 0.0,
                 lr: float = 5e-4, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                 lambda_coarse_mse: float = 1.0, lambda_fine_mse: float = 1.0, ray_chunk: int = 4096,
                 precision: str = "f16x3", device="cuda", gamma_correct: bool = False,
                 use_var_loss: bool = False, lambda_coarse_var: float = 0.01, lambda_fine_var: float = 0.01,
                 use_depth_var_loss: bool = False, lambda_coarse_depth_var: float = 0.01, lambda_fine_depth_var: float = 0.01,
                 no_dir: bool = False, sigma_activation: str = "relu", color_activation: str = "sigmoid", stop_grad: bool = False,
                 grad_clip_val: float = 0.0, grad_clip_type: str = "norm", arch=None, embed: int = 0, chain_ray_grad: bool = False):
        # chain_ray_grad: forward() / backward() on rays that require grad run the chain pair under a chain precision
        # (forward_rays_train); the fused step does not differentiate with respect to rays either way
        self.chain_ray_grad = bool(chain_ray_grad)
        # embed: the embedding's option word (weights.embed_of(opt): --no_xyz / --no_logscale).  Non-zero: the architecture route
        # below (on the default descriptor when arch is None) with the `_e` pair; precision 'fp32' or 'f16x3_gemm'
        self.embed = int(embed)
        if self.embed and arch is None:
            arch = {}
        # arch: the architecture flags of both networks (see forward_rays_train); None = the default network and the fused step.
        # With an architecture the iteration is forward -> losses in torch -> backward -> Adam over the 2 D + 8 tensors
        # (nsr_train_arch_forward / _backward, nsr_adam_step_n), --no_dir runs natively as the narrow dir_encoding
        self.arch = None if arch is None else normalize_arch(arch)
        if self.arch is not None:
            check_embed(self.embed, self.arch)
            precision = embed_precision(self.embed, precision) if self.embed else arch_precision(self.arch, precision)
            if bool(no_dir) and not self.arch["no_dir"]:
                self.arch["no_dir"] = True
        # --grad_clip_val / --grad_clip_type (models/nerf_downX_model.py:403-407): both networks' gradients together, between
        # the backward and the optimiser step; 0 = off
        if grad_clip_type not in ("norm", "value"):
            raise ValueError("grad_clip_type: 'norm' or 'value'")
        self.grad_clip_val, self.grad_clip_type = float(grad_clip_val), grad_clip_type
        # the options of the step's option word (train_flags; --sigma_activation softplus: models/rendering.py:69-73)
        train_flags(white_bkgd, gamma_correct, sigma_activation, color_activation, stop_grad)      # validates
        self.gamma_correct, self.stop_grad = bool(gamma_correct), bool(stop_grad)
        self.sigma_activation, self.color_activation = sigma_activation, color_activation
        if precision not in _lib.TRAIN_PRECISIONS:
            raise ValueError("precision must be 'fp32' (every product on the fp32 MFMA, layer by layer), 'f16x3' (the chain "
                             "kernels: forward on the split-fp16 MFMA, weight gradients on one fp16 MFMA per product, input "
                             "gradients on the default number of MFMA terms), 'f16x3_bwd3' / 'f16x3_bwd2' / 'f16x3_bwd1' / 'f16x3_bwdm' (the "
                             "chain kernels with three / two / one / mixed two-one MFMAs per product of the input gradients, include/nsr_train.h) "
                             "'f16x3_gemm' (layer by layer, forward products split-fp16, gradients fp32) or 'f16x3_gemm_bwd' "
                             "(the same forward; every gradient product split-fp16 as well: three fp16 MFMAs per product, fp32 "
                             "accumulation, power-of-two scaling per sample point / per matrix)")
        self.precision, self._prec = precision, _lib.TRAIN_PRECISIONS[precision]
        self.device = torch.device(device)
        # --no_dir (models/networks.py:160-169): the networks are trained as the full layout with 27 zero columns in
        # dir_encoding's weight (weights.pad_no_dir) whose gradients are dropped every step, so Adam never moves them
        # (m = v = 0 -> update 0): the function, its gradients and the trajectory are the narrow network's
        self.no_dir = bool(no_dir) if self.arch is None else bool(self.arch["no_dir"])
        self._padded = self.no_dir and self.arch is None      # an architecture keeps the narrow layer natively
        desc = self.arch if self.arch is not None else _normalize_arch(no_dir=self.no_dir)
        self.params = []
        for sd in (sd_coarse, sd_fine):
            check_state_dict_arch(sd, no_xyz=bool(self.embed & EMBED_NO_XYZ), **desc)
            p = state_dict_to_device(sd, arch_spec(no_xyz=bool(self.embed & EMBED_NO_XYZ), **desc), self.device, own=True)
            if self._padded:
                p[DIR_W] = pad_no_dir(p[DIR_W])
            self.params.append(p)
        flat = [_flat_like(p) for p in self.params]
        self.flat_grads, self.grads = [f for f, _ in flat], [v for _, v in flat]
        self.exp_avg = [_flat_like(p)[1] for p in self.params]
        self.exp_avg_sq = [_flat_like(p)[1] for p in self.params]
        # nsr_adam_step_n's arguments per network, built once: the tensors are only ever updated in place
        self._numel = [(ctypes.c_int64 * len(p))(*[v.numel() for v in p.values()]) for p in self.params]
        self._ptrs = {name: [_ptr_array(list(d.values())) for d in getattr(self, name)]
                      for name in ("params", "grads", "exp_avg", "exp_avg_sq")}
        # data parallelism: every rank scales its loss by 1 / world so that the all-reduce SUM is the gradient of the
        # global-batch MEAN loss, like DistributedDataParallel's averaging (models/networks.py:84).  None = derive it
        # from the default process group at each step; a number pins it (e.g. a custom group).
        self.grad_scale: Optional[float] = None
        self.group = None          # process group of the data-parallel replicas (None = the default group); the 1 / world
        #                            loss scale, the gradient all-reduce and the finite-loss vote all use THIS group
        self.check_finite = False  # debug: raise when the loss is not finite (see optimize_parameters)
        self.N_coarse, self.N_importance = int(N_coarse), int(N_importance)
        self.white_bkgd, self.lindisp = bool(white_bkgd), bool(lindisp)
        self.s2 = int(downscale) ** 2
        self.randomized, self.noise_std = bool(randomized), float(noise_std)
        self.lr, self.beta1, self.beta2, self.eps = float(lr), float(beta1), float(beta2), float(eps)
        self.lambda_coarse, self.lambda_fine = float(lambda_coarse_mse), float(lambda_fine_mse)
        # the optional variance losses of comp_low_res_output (models/nerf_downX_model.py:107-112, 332-336, 349-353, 374-378);
        # 0 = off, like the reference's flags.  [coarse rgb, fine rgb, coarse depth, fine depth]
        self.lambda_var = [float(lambda_coarse_var) if use_var_loss else 0.0, float(lambda_fine_var) if use_var_loss else 0.0,
                           float(lambda_coarse_depth_var) if use_depth_var_loss else 0.0,
                           float(lambda_fine_depth_var) if use_depth_var_loss else 0.0]
        self.var_losses = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.ray_chunk = int(ray_chunk) - int(ray_chunk) % self.s2
        self.step = 0
        self._workspace = TrainWorkspace()     # shared by loss_and_grads and the autograd pair (forward / backward)
        self._leaves = None
        self.losses = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.out: Dict[str, torch.Tensor] = {}

    @property
    def _ws(self) -> Optional[torch.Tensor]:
        return self._workspace.buf

    def _grad_scale(self) -> float:
        """What every loss is scaled by so that the all-reduce SUM is the global-batch MEAN's gradient (see ``grad_scale``)."""
        from .dist import _world
        return float(self.grad_scale) if self.grad_scale is not None else 1.0 / _world(self.group)[1]

    def _chunk(self, R: int) -> int:
        return _rays_per_pass(self.ray_chunk, R)

    def _zero_padding_grads(self):
        """--no_dir on the default network: the gradients of the 27 zero columns are dropped, so Adam never moves them."""
        if self._padded:
            for g in self.grads:
                g[DIR_W][:, 256:].zero_()

    # -- reference protocol ------------------------------------------------------------------------------
    def set_input(self, rays: torch.Tensor, rgbs: torch.Tensor):
        """rays (N_lr, s2, 8 | 11) or (N_lr * s2, 8 | 11); rgbs (N_lr, 3) LR targets (set_input, :235-248)."""
        rays = _f32(rays.reshape(-1, rays.shape[-1]), "rays")
        if rgbs.ndim < 1 or rgbs.shape[-1] != 3:
            raise ValueError(f"rgbs must be (N_lr, 3), got {tuple(rgbs.shape)}")
        self.data_rays, self.data_rgbs = rays, _f32(rgbs.reshape(-1, 3), "rgbs")
        if rays.shape[0] != self.data_rgbs.shape[0] * self.s2:
            raise ValueError("rays must hold s^2 sub-rays per LR target pixel")

    def draw(self, R: int) -> Dict[str, Optional[torch.Tensor]]:
        """The random tensors of one train-mode forward, in the reference's order (models/utils.py:40, 210, 73)."""
        d = {"u_coarse": None, "noise_coarse": None, "u_fine": None, "noise_fine": None}
        if self.randomized:
            nc, nf = self.N_coarse, self.N_coarse + self.N_importance
            d["u_coarse"] = torch.rand(R, nc, device=self.device)
            if self.noise_std > 0:
                d["noise_coarse"] = torch.randn(R, nc, device=self.device)
            d["u_fine"] = torch.rand(R, self.N_importance, device=self.device)
            if self.noise_std > 0:
                d["noise_fine"] = torch.randn(R, nf, device=self.device)
        return d

    def loss_and_grads(self, draws: Optional[Dict[str, Optional[torch.Tensor]]] = None):
        """forward + comp_low_res_output + calculate_losses + backward (:316-396): fills ``self.out``,
        ``self.losses`` (device float[2], UNscaled: this rank's lambda-weighted MSEs) and ``self.grads`` (already
        scaled by 1 / world for the data-parallel SUM, see ``grad_scale``)."""
        if self.arch is not None:
            return self._loss_and_grads_arch(draws)
        gs = self._grad_scale()
        rays = self.data_rays
        R, stride = rays.shape[0], _ray_stride(rays)
        if draws is None:
            draws = self.draw(R)
        draws = _draws(draws, R, self.N_coarse, self.N_importance, self.device)
        nc, chunk = self.N_coarse, self._chunk(R)
        lib = _lib.load()
        need = lib.nsr_train_workspace_bytes_for(self._prec, chunk, nc, self.N_importance)   # the buffers of the path this precision takes
        if need == 0:
            raise _lib.NsrError("sample counts outside the built path")
        self._workspace.get(need, self.device)
        dev = self.device
        o = dict(zip(OUT_KEYS, _alloc_outs(R, nc, self.N_importance, dev)))
        lr_c = torch.empty(R // self.s2, 3, device=dev)
        lr_f = torch.empty(R // self.s2, 3, device=dev)
        outs = _ptr_array(list(o.values()))
        (wc, wf), (gc, gf) = self._ptrs["params"], self._ptrs["grads"]
        # int(self.white_bkgd) as it stands: the C entry point is the one that refuses a word with unknown or exclusive bits
        flags = int(self.white_bkgd) | train_flags(False, self.gamma_correct, self.sigma_activation, self.color_activation, self.stop_grad)
        common = (wc, wf, gc, gf, _p(rays), stride, R, self.s2, _p(self.data_rgbs), nc, self.N_importance, flags, int(self.lindisp),
                  _p(draws.get("u_coarse")), _p(draws.get("u_fine")),
                  _p(draws.get("noise_coarse")), _p(draws.get("noise_fine")), self.noise_std,
                  self.lambda_coarse * gs, self.lambda_fine * gs, self._prec, chunk, outs, _p(lr_c), _p(lr_f), _p(self.losses),
                  _p(self._ws), self._ws.numel(), _stream())
        if any(self.lambda_var):
            # self.far of the reference (nerf_downX_model.py:284): forward_rays overwrites it per ray_chunk, so what
            # calculate_losses divides by is the far bound of the FIRST ray of the LAST chunk.  Only the depth-variance
            # terms use it: read (one host sync) only when one of them is on; the colour-variance terms never need it.
            far = 1.0
            if any(self.lambda_var[2:]):
                far = float(rays[((R - 1) // chunk) * chunk, 7].item())
            var = (ctypes.c_float * 5)(*[l * gs for l in self.lambda_var], far)       # struct nsr_train_var_losses
            _lib.check(lib.nsr_train_loss_and_grads_var(*common, ctypes.cast(var, c_void_p), _p(self.var_losses)),
                       "nsr_train_loss_and_grads_var")
        else:
            _lib.check(lib.nsr_train_loss_and_grads(*common), "nsr_train_loss_and_grads")
        self._zero_padding_grads()
        if gs != 1.0:
            self.losses.mul_(1.0 / gs)          # report this rank's own losses, not the 1 / world share
            self.var_losses.mul_(1.0 / gs)
        o["lr_coarse"], o["lr_fine"] = lr_c, lr_f
        self.out = o
        return self.losses, self.grads

    def _loss_and_grads_arch(self, draws=None):
        """``loss_and_grads`` of a non-default architecture: the autograd pair with the reference's losses written in torch
        (comp_low_res_output + calculate_losses, models/nerf_downX_model.py:326-378): s^2 means, the two lambda-weighted
        MSEs, the variance terms when they are on."""
        rays = self.data_rays
        R = rays.shape[0]
        out = self.forward(draws)
        n_lr = R // self.s2
        lr_c = out["coarse_comp_rgbs"].view(n_lr, self.s2, 3).mean(1)
        lr_f = out["fine_comp_rgbs"].view(n_lr, self.s2, 3).mean(1)
        mse = torch.nn.functional.mse_loss
        loss_c, loss_f = mse(lr_c, self.data_rgbs) * self.lambda_coarse, mse(lr_f, self.data_rgbs) * self.lambda_fine
        total = loss_c + loss_f
        self.var_losses = torch.zeros(4, dtype=torch.float32, device=self.device)
        if any(self.lambda_var):
            var_of = lambda t: torch.sum(torch.var(t.reshape(n_lr, self.s2, -1), dim=1))
            terms = [None] * 4
            if any(self.lambda_var[:2]):
                terms[0], terms[1] = var_of(out["coarse_comp_rgbs"]), var_of(out["fine_comp_rgbs"])
            if any(self.lambda_var[2:]):
                # self.far of the reference (:284): the far bound of the first ray of the last ray chunk
                chunk = self._chunk(R)
                far = rays[((R - 1) // chunk) * chunk, 7]
                terms[2], terms[3] = var_of(out["coarse_depth"] / far), var_of(out["fine_depth"] / far)
            for i, (lam, t) in enumerate(zip(self.lambda_var, terms)):
                if lam and t is not None:
                    total = total + lam * t
                    self.var_losses[i] = (lam * t).detach()
        self.losses = torch.stack([loss_c.detach(), loss_f.detach()])
        self.backward(total)
        o = {k: v.detach() for k, v in out.items()}
        o["lr_coarse"], o["lr_fine"] = lr_c.detach(), lr_f.detach()
        self.out = o
        return self.losses, self.grads

    # -- autograd protocol: forward() -> any loss in torch -> backward(loss) -> [clip_grads()] -> optimizer_step() ---------
    def _weight_leaves(self):
        """Per network 24 tensors that alias ``self.params`` and require grad (autograd leaves; they share the storage and the
        version counter, so an in-place update of a weight between a forward and its backward is caught: a torch in-place op
        bumps the counter itself, ``optimizer_step`` -- which writes through raw pointers -- bumps it explicitly)."""
        if self._leaves is None:
            self._leaves = [[p.detach().requires_grad_(True) for p in self.params[n].values()] for n in range(2)]
        return self._leaves

    def forward(self, draws: Optional[Dict[str, Optional[torch.Tensor]]] = None, rays: Optional[torch.Tensor] = None):
        """Train-mode ``forward_rays`` of the current batch (or of ``rays``: a patch, a ``--with_ref`` batch) through the
        autograd pair: the eight outputs, differentiable with respect to both networks' weights.  Losses of several forwards
        may be summed before ONE ``backward``."""
        rays = self.data_rays if rays is None else _f32(rays.reshape(-1, rays.shape[-1]), "rays")
        if draws is None:
            draws = self.draw(rays.shape[0])
        draws = {k: v for k, v in draws.items() if k != "noise_std"}
        lc, lf = self._weight_leaves()
        self._ray_grad_pending = getattr(self, "_ray_grad_pending", False) or bool(rays.requires_grad)
        return forward_rays_train(lc, lf, rays, draws, N_coarse=self.N_coarse, N_importance=self.N_importance,
                                  white_bkgd=self.white_bkgd, lindisp=self.lindisp, noise_std=self.noise_std,
                                  gamma_correct=self.gamma_correct, sigma_activation=self.sigma_activation,
                                  color_activation=self.color_activation, stop_grad=self.stop_grad, precision=self.precision,
                                  ray_chunk=self.ray_chunk, workspace=self._workspace, arch=self.arch, embed=self.embed,
                                  chain_ray_grad=self.chain_ray_grad)

    def backward(self, loss: torch.Tensor):
        """d(loss)/d(weights) of the forwards behind ``loss`` into ``self.grads`` / ``self.flat_grads`` (OVERWRITTEN; scaled by
        1 / world like ``loss_and_grads``, see ``grad_scale``), where ``all_reduce_grads`` and ``optimizer_step`` find them.
        A weight the loss does not reach gets a zero gradient.  Where a forward behind ``loss`` took rays that require grad
        (``precision`` 'fp32' / 'f16x3_gemm', or a chain precision with ``chain_ray_grad=True``), the gradient also flows on through them: ``rays.grad`` -- or the ``.grad`` of
        whatever leaf produced the rays, a pose under ``cameras.rays_from_pose`` -- is accumulated as ``loss.backward()`` does."""
        gs = self._grad_scale()
        leaves = self._weight_leaves()
        flat = leaves[0] + leaves[1]
        g_out = None if gs == 1.0 else torch.full_like(loss, gs)
        if getattr(self, "_ray_grad_pending", False):
            self._ray_grad_pending = False
            for l in flat:
                l.grad = None
            torch.autograd.backward(loss, g_out)
            grads = [l.grad for l in flat]
            for l in flat:
                l.grad = None
        else:
            grads = torch.autograd.grad(loss, flat, grad_outputs=g_out, allow_unused=True)
        dst = list(self.grads[0].values()) + list(self.grads[1].values())
        torch._foreach_copy_([d for d, g in zip(dst, grads) if g is not None], [g for g in grads if g is not None])
        for d, g in zip(dst, grads):
            if g is None:
                d.zero_()
        self._zero_padding_grads()
        return self.grads

    def clip_grads(self) -> Optional[torch.Tensor]:
        """``nn.utils.clip_grad_norm_`` / ``clip_grad_value_`` over both networks together (:403-407), in place on
        ``self.grads``.  Returns the total 2-norm before clipping ('norm'), None otherwise or when ``grad_clip_val`` is 0."""
        if self.grad_clip_val <= 0:
            return None
        grads = list(self.grads[0].values()) + list(self.grads[1].values())
        if self.grad_clip_type == "value":
            torch._foreach_clamp_min_(grads, -self.grad_clip_val)
            torch._foreach_clamp_max_(grads, self.grad_clip_val)
            return None
        # torch.nn.utils.clip_grad_norm_ (norm_type 2): the norm of the per-tensor norms, coefficient clamped to 1
        total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2.0) for g in grads]), 2.0)
        coef = torch.clamp(self.grad_clip_val / (total + 1e-6), max=1.0)
        torch._foreach_mul_(grads, coef)
        return total

    def regularize_patch(self, patch_rays: torch.Tensor, patch_len: int, reg_lambda_tv: float = 1.0, draws=None,
                         fused_tv: bool = False):
        """The reference's patch regulariser iteration (``regularize_patch``, models/nerf_downX_model.py:596-618, called from
        train.py when --reg_patch is on): render a (patch_len * downscale)^2 HR patch (rays in raster order), total-variation
        loss of its coarse and fine colours (``tv_loss``) times ``reg_lambda_tv``, backward, its own Adam step.  Returns the
        device tensor [tv_coarse, tv_fine] (before the lambda).  ``fused_tv``: the two losses and their gradients through
        ``losses.TVLoss`` (two launches forward, one backward, double arithmetic) instead of the chain of torch ops."""
        side = int(patch_len) * int(round(self.s2 ** 0.5))
        if not isinstance(patch_rays, torch.Tensor) or patch_rays.ndim < 2 or patch_rays.numel() != side * side * patch_rays.shape[-1]:
            raise ValueError(f"patch_rays must hold the {side} x {side} rays of the HR patch in raster order, got "
                             f"{tuple(getattr(patch_rays, 'shape', ()))}")
        out = self.forward(draws, rays=patch_rays)
        tv = tv_loss
        if fused_tv:
            from .losses import TVLoss
            tv = TVLoss()
        loss_c = tv(out["coarse_comp_rgbs"].view(side, side, -1))
        loss_f = tv(out["fine_comp_rgbs"].view(side, side, -1))
        self.backward((loss_c + loss_f) * reg_lambda_tv)
        self.all_reduce_grads()
        self.optimizer_step()
        self.out_patch = out
        return torch.stack([loss_c.detach(), loss_f.detach()])

    def all_reduce_grads(self, group=None):
        """Data-parallel training (replaces DistributedDataParallel's bucketed gradient all-reduce,
        models/networks.py:84): every rank renders its own ray batch with ``grad_scale = 1 / world`` and ONE
        all-reduce (SUM) per network of the flat 2.4 MB gradient buffer (RCCL over xGMI; gloo in the CPU tests of
        ``dist.py``) leaves the global-mean gradient on every rank; the Adam step then runs replicated."""
        from .dist import all_reduce_sum_
        all_reduce_sum_(self.flat_grads, self.group if group is None else group)

    def optimizer_step(self):
        """torch.optim.Adam.step over both networks (:201-204, :408)."""
        self.step += 1
        for n, numel in enumerate(self._numel):
            _lib.check(_lib.load().nsr_adam_step_n(
                len(numel), numel, *(self._ptrs[k][n] for k in ("params", "grads", "exp_avg", "exp_avg_sq")),
                self.step, self.lr, self.beta1, self.beta2, self.eps, _stream()), "nsr_adam_step_n")
        if self._leaves is not None:
            # nsr_adam_step_n wrote the weights behind autograd's back: mark them modified, so that the backward of a forward
            # made before this step fails the version check instead of mixing two sets of weights
            torch.autograd.graph.increment_version(self._leaves[0] + self._leaves[1])

    def status(self, clear: bool = False) -> int:
        """Sticky numerics status word of the training step (``NSR_FLAG_*``, include/nsr_train.h): 0 = every iteration so
        far packed in-range weights and saw in-range inputs / activations and finite outputs.  Waits for the stream."""
        return self._workspace.status(clear)

    def optimize_parameters(self, draws=None):
        """One training iteration (:398-408); returns the device tensor [coarse_mse, fine_mse] (lambda-weighted).

        ``precision='f16x3'`` carries the forward activations as fp16 (hi, lo) pairs: values beyond 65,504 saturate.
        None of the reference's configurations come near (|h| ~ 1e2), but a diverging run would turn into inf / NaN
        weights silently; ``self.check_finite = True`` adds a host check of the loss (one sync per step) that raises
        and points at ``precision='fp32'`` (the reference itself drops into pdb on NaN, nerf_downX_model.py:273)."""
        self.loss_and_grads(draws)
        if self.check_finite:
            # every rank votes and every rank raises: a rank that raised alone would leave the others waiting in the
            # gradient all-reduce
            from .dist import all_ranks_agree
            flags = self.status(clear=True)
            if not all_ranks_agree(flags == 0, self.device, self.group):
                raise _lib.NsrNumericsError(
                    f"training step {self.step + 1}: numerics status {flags:#x} = {' | '.join(_lib.flag_names(flags)) or 'raised on another rank'}"
                    " -- weights or activations left the split-fp16 operand range; retry with precision='fp32'", flags)
            if not all_ranks_agree(bool(torch.isfinite(self.losses).all()), self.device, self.group):
                raise FloatingPointError(
                    f"non-finite training loss at step {self.step + 1} (this rank: {self.losses.tolist()}): the run diverged"
                    + (" or left the fp16 range of the split-fp16 forward; retry with precision='fp32'"
                       if self.precision != "fp32" else ""))
        self.all_reduce_grads()
        if self.grad_clip_val > 0:
            self.clip_grads()
        self.optimizer_step()
        return self.losses

    def update_learning_rate(self, epoch: int, lr_policy: str = "exp", n_epochs: int = 20, n_epochs_decay: int = 10,
                             lr_final: float = 5e-6, lr_decay_epochs: int = 10, lr_decay_gamma: float = 0.1,
                             lr_initial: Optional[float] = None) -> float:
        """The reference's per-epoch schedules (models/networks.py:89-118 `get_scheduler`, called from
        base_model.update_learning_rate): 'linear' / 'exp' interpolate (in lr / in log lr) from ``lr`` to ``lr_final``
        over the last ``n_epochs_decay`` of ``n_epochs`` epochs, 'step' multiplies by gamma every ``lr_decay_epochs``.
        ``epoch`` is the number of finished epochs (the scheduler's ``last_epoch``); returns and installs the new lr."""
        import math
        lr0 = self._lr_initial = lr_initial if lr_initial is not None else getattr(self, "_lr_initial", self.lr)
        if lr_policy in ("linear", "exp"):
            t = max(0, epoch + 1 - n_epochs + n_epochs_decay) / float(n_epochs_decay + 1)
            self.lr = (lr0 * (1 - t) + lr_final * t) if lr_policy == "linear" else \
                math.exp(math.log(lr0) * (1 - t) + math.log(lr_final) * t)
        elif lr_policy == "step":
            self.lr = lr0 * lr_decay_gamma ** (epoch // lr_decay_epochs)
        else:
            raise NotImplementedError(f"learning rate policy [{lr_policy}] is not implemented")
        return self.lr

    def state_dicts(self):
        return [{k: (v[:, :256] if (self._padded and k == DIR_W) else v).clone() for k, v in p.items()} for p in self.params]
