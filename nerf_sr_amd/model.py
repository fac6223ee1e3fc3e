"""Host-side mirror of ``NeRFDownXModel`` for the render path and its scoring.

Reproduces the call protocol the reference's loops use
(``set_input -> forward -> out_* -> comp_low_res_output``; train.py:79-80,
test.py:52, models/nerf_downX_model.py:235-353,410-416,621-669) on top of the HIP
path, and the eval-side ``calculate_losses`` / ``validate`` (:355-388, :469-516) over
``nerf_sr_amd.metrics``.  Training losses and optimisers live in ``nerf_sr_amd.train``;
checkpoints, visualisers and the GAN branches are out of scope.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import ops
from .ops import VanillaMLP, GenericMLP, VolumetricRenderer, PositionalEncoding


def default_options(**kw) -> SimpleNamespace:
    """The option values that define the path (SURVEY §5 'Config / flags')."""
    opt = SimpleNamespace(
        N_coarse=64, N_importance=64, lindisp=False, white_bkgd=False, randomized=True, noise_std=0.0,
        deg_pos=10, deg_dir=4, dim_pos=3, dim_dir=3, dim_rgb=3, downscale=2, img_wh=(504, 378),
        D=8, W=256, skips=[4],                      # models/networks.py:124-128; other values run layer by layer (ops.GenericMLP)
        no_xyz=False, no_logscale=False,            # models/embedding.py:17-18: True runs the descriptor routes (ops.GenericMLP)
        no_dir=False, color_activation="sigmoid",   # :128, :160-180 ('none'; True): options of VanillaMLP
        sigma_activation="relu", gamma_correct=False,   # models/rendering.py:69-73 ('softplus'); nerf_downX_model.py:271-276
        ray_chunk=4096, point_chunk=262144, precision="fp32",
        check_numerics=True,    # forward() raises on NaN / out-of-range values (the reference: pdb, nerf_downX_model.py:273-274)
        early_stop=0.0,         # eval mode, precision 'f16x3': early ray termination at this transmittance (0 = off; include/nsr.h)
        coarse_rgb=True,        # False: test-time mode, eval + 'f16x3' -- the coarse pass computes densities only (include/nsr.h)
        arch_fused=False,       # True: a non-default D / W / skips / degrees runs in ONE fused launch under 'f16x3' (ops.GenericMLP(fused=True))
        arch_fused_rays=True,   # with arch_fused: that launch takes (rays, z) and encodes in the kernel (ops.render_rays); False: the
                                # encoded-rows route (posenc + cat in HBM, then the same kernel) -- the same bits, kept for A/B runs
    )
    for k, v in kw.items():
        setattr(opt, k, v)
    if opt.arch_fused and not (ops.is_default_arch(ops.arch_of(opt)) and not ops.embed_of(opt)):      # refused here, on the host, not at the first launch
        ops.check_arch_fused(ops.arch_of(opt), opt.precision)
    return opt


class NeRFDownXModel:
    """``model.set_input(data); model.forward(); model.comp_low_res_output()`` as in the
    reference; the ``out_*`` attributes carry the same tensors (same shapes, fp32)."""

    def __init__(self, opt: Optional[SimpleNamespace] = None, device="cuda"):
        self.opt = opt or default_options()
        ops.check_mlp_options(self.opt, fused=False)
        if int(self.opt.N_coarse) < 2 or int(self.opt.N_importance) < 0:
            raise ValueError("N_coarse must be >= 2 and N_importance >= 0")
        self.renderer = VolumetricRenderer(self.opt)      # validates sigma_activation before any device is touched
        self._check_early_stop()                          # ... and the early-termination option with its restrictions
        self._check_coarse_rgb()                          # ... and the test-time mode with its own
        self.device = torch.device(device)
        # the fused kernels for the architecture every script of the reference uses, nn.Linear by nn.Linear for any other
        self.netCoarse = ops.make_mlp(self.opt, precision=self.opt.precision, device=self.device)
        self.netFine = ops.make_mlp(self.opt, precision=self.opt.precision, device=self.device)
        self.fused = isinstance(self.netCoarse, VanillaMLP)
        # a GenericMLP pair on the fused descriptor kernel: its network passes can take (rays, z) too (opt.arch_fused_rays)
        self.arch_fused = isinstance(self.netCoarse, GenericMLP) and self.netCoarse.fused and self.netFine.fused
        self.models = {"coarse": self.netCoarse, "fine": self.netFine}
        self.embeddings = {"pos": PositionalEncoding(3, self.opt.deg_pos, self.opt), "dir": PositionalEncoding(3, self.opt.deg_dir, self.opt)}
        self.randomized = False
        self._ws = None
        self._outs: Dict[str, torch.Tensor] = {}

    # -- weights ---------------------------------------------------------------
    def load_networks(self, sd_coarse, sd_fine):
        """Takes the two 24-key state_dicts the reference stores as
        ``{epoch}_net_Coarse.pth`` / ``{epoch}_net_Fine.pth`` (models/base_model.py:181-219)."""
        self.netCoarse.load_state_dict(sd_coarse)
        self.netFine.load_state_dict(sd_fine)
        return self        # (the colour-head options of `opt` -- gamma_correct, color_activation -- are applied by VanillaMLP)

    def _check_early_stop(self) -> float:
        """``opt.early_stop`` checked against the options it depends on, before any device is touched (ops.check_early_stop
        repeats the check on the networks themselves at every call).  Like every other option it is read from ``opt`` at
        call time: the constructor checks it early, every eval-mode forward checks it again, so a later
        ``model.opt.early_stop = eps`` takes effect or raises, never passes unnoticed."""
        opt = self.opt
        eps = float(getattr(opt, "early_stop", 0.0))
        if not (0.0 <= eps < 1.0):
            raise ValueError(f"early_stop={getattr(opt, 'early_stop', None)!r}: a transmittance threshold in [0, 1) (0 = off)")
        if eps == 0.0:
            return eps
        if opt.precision != "f16x3":
            raise ValueError(f"early_stop needs precision 'f16x3' (the split-fp16 render kernel), not {opt.precision!r}")
        if self.renderer.sigma_activation != "relu":
            raise ValueError("early_stop needs the relu density: under sigma_activation='softplus' a raw density of 0 still has weight")
        if getattr(opt, "color_activation", "sigmoid") == "none":
            raise ValueError("early_stop needs colours in [0, 1]: color_activation='none' leaves them unbounded")
        if int(opt.N_coarse) + int(opt.N_importance) not in (64, 128):
            raise ValueError(f"early_stop needs 64 or 128 samples in the pass that is cut, not {int(opt.N_coarse) + int(opt.N_importance)}")
        if ops.embed_of(opt):
            raise ValueError(f"early_stop needs the 8 x 256 render kernel, which has no embedding options ({ops.embed_names(ops.embed_of(opt))})")
        if not ops.is_default_arch(ops.arch_of(opt)):
            raise ValueError("early_stop needs the architecture of the fused kernels (8 x 256, skip at 4, degrees 10 / 4)")
        return eps

    def _check_coarse_rgb(self, coarse_rgb: Optional[bool] = None) -> bool:
        """``opt.coarse_rgb`` (or the per-call override) checked against the options the density-only coarse pass depends on,
        before any device is touched; ``ops.check_density_coarse`` repeats the check on the networks at every call.  Read
        from ``opt`` at call time, like ``early_stop``: a later ``model.opt.coarse_rgb = False`` takes effect or raises."""
        opt = self.opt
        on = bool(getattr(opt, "coarse_rgb", True)) if coarse_rgb is None else bool(coarse_rgb)
        if on:
            return True
        if opt.precision != "f16x3":
            raise ValueError(f"coarse_rgb=False needs precision 'f16x3' (the split-fp16 render kernel), not {opt.precision!r}")
        if int(opt.N_importance) <= 0:
            raise ValueError("coarse_rgb=False needs a fine pass (N_importance > 0): without one the coarse colour is the image")
        if int(opt.N_coarse) not in ops.FUSED_SAMPLES_F16X3:
            raise ValueError(f"coarse_rgb=False needs N_coarse of 64, 128, 192 or 256, not {int(opt.N_coarse)}")
        if ops.embed_of(opt):
            raise ValueError(f"coarse_rgb=False needs the 8 x 256 render kernel, which has no embedding options ({ops.embed_names(ops.embed_of(opt))})")
        if not ops.is_default_arch(ops.arch_of(opt)):
            raise ValueError("coarse_rgb=False needs the architecture of the fused kernels (8 x 256, skip at 4, degrees 10 / 4)")
        return False

    # -- mode toggles (nerf_downX_model.py:250-258) ------------------------------
    def train(self):
        self.randomized = bool(self.opt.randomized)
        return self

    def eval(self):
        self.randomized = False
        return self

    # -- D1 ------------------------------------------------------------------------
    def set_input(self, input: Dict[str, torch.Tensor]):
        for name, v in input.items():
            v = v.squeeze(0) if (v.ndim > 0 and v.shape[0] == 1) else v
            v = v.reshape(-1, v.shape[-1]) if v.ndim in (3, 4) else v
            setattr(self, f"data_{name}", v.to(self.device))

    # -- D2 ------------------------------------------------------------------------
    def render_rays(self, model: VanillaMLP, xyz: torch.Tensor, dir_embedded: torch.Tensor, **kwargs):
        """Reference signature (xyz (R,N,3), dir_embedded (R,27)) -> (rgbs, sigmas): the
        unfused route through explicit positional encoding and ``VanillaMLP.forward``."""
        R, N = xyz.shape[:2]
        x = torch.cat([self.embeddings["pos"](xyz.reshape(-1, 3)), dir_embedded.repeat_interleave(N, dim=0)], -1)
        out = model(x, **kwargs).view(R, N, -1)
        rgb = out[..., :3]
        if isinstance(model, GenericMLP) and model.gamma_correct and not kwargs.get("sigma_only", False):
            # models/nerf_downX_model.py:271-276: pow(rgb, 1 / 2.2) after the network (VanillaMLP's fused colour head has
            # done it already: nsr_weights_set_gamma); the NaN trap that follows it there is the network's status word here
            rgb = torch.pow(rgb, 1.0 / 2.2)
        return rgb, out[..., 3]

    def _render_by_rays(self, model, rays: torch.Tensor, z: torch.Tensor):
        """``ops.render_rays`` -- no encoded row exists on this route -- plus, for a ``GenericMLP``, the ``pow(rgb, 1 / 2.2)``
        of ``gamma_correct`` that ``render_rays`` above applies (its fused kernel has no colour-head option for it)."""
        rgb, sig = ops.render_rays(model, rays, z)
        if isinstance(model, GenericMLP) and model.gamma_correct:
            rgb = torch.pow(rgb, 1.0 / 2.2)
        return rgb, sig

    # -- D3 ------------------------------------------------------------------------
    def forward_rays(self, rays: torch.Tensor, coarse_rgb: Optional[bool] = None) -> Dict[str, torch.Tensor]:
        """``opt.early_stop`` applies to the eval-mode forward only (the fine pass, include/nsr.h); ``train()`` mode ignores it.
        ``coarse_rgb`` (default: ``opt.coarse_rgb``) False is the test-time mode: eval only, no ``coarse_comp_rgbs`` in the
        result; the randomized forward needs the coarse colour for its loss and raises."""
        opt = self.opt
        with_rgb = self._check_coarse_rgb(coarse_rgb)
        if not with_rgb and self.randomized:
            raise ValueError("coarse_rgb=False is a test-time mode: the randomized (train()) forward feeds the coarse colour to its loss")
        if not self.randomized and self.fused:
            self._outs = ops.forward_rays(self.netCoarse, self.netFine if opt.N_importance > 0 else None, rays,
                                          opt.N_coarse, opt.N_importance, opt.white_bkgd, opt.lindisp,
                                          check=bool(getattr(opt, "check_numerics", True)),
                                          sigma_activation=self.renderer.sigma_activation, early_stop=self._check_early_stop(),
                                          coarse_rgb=with_rgb)
            return self._outs
        # randomized (training-mode) forward, and every forward of a GenericMLP pair: same kernels, stage by stage, jitter
        # drawn with torch.rand
        o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
        rnd = self.randomized
        z, xyz = ops.sample_along_rays(o, d, near, far, opt.N_coarse, rnd, opt.lindisp)
        # the ray-level launch (encodings in the kernel): the default pair, and a fused GenericMLP pair unless the option
        # asks for the encoded-rows route; read at call time, so both routes can be timed in one process
        by_rays = self.fused or (self.arch_fused and bool(getattr(opt, "arch_fused_rays", True)))
        if not by_rays:
            dir_emb = self.embeddings["dir"]((rays[:, 8:11] if rays.shape[1] == 11 else d).contiguous())
        rgb, sig = self._render_by_rays(self.netCoarse, rays, z) if by_rays else self.render_rays(self.netCoarse, xyz, dir_emb)
        rgb, sig = rgb.contiguous(), sig.contiguous()
        if rnd and opt.noise_std > 0:          # add_gaussian_noise (models/utils.py:199-212): only when randomized
            sig = sig + torch.randn_like(sig) * opt.noise_std
        c = self.renderer(rgb, sig, z, opt.white_bkgd)
        out = dict(zip(ops.OUT_KEYS[:4], c))
        if opt.N_importance > 0:
            z2, xyz2 = ops.resample_along_rays(o, d, z, c[3], opt.N_importance, rnd)
            rgb2, sig2 = self._render_by_rays(self.netFine, rays, z2) if by_rays else self.render_rays(self.netFine, xyz2, dir_emb)
            rgb2, sig2 = rgb2.contiguous(), sig2.contiguous()
            if rnd and opt.noise_std > 0:
                sig2 = sig2 + torch.randn_like(sig2) * opt.noise_std
            out.update(zip(ops.OUT_KEYS[4:], self.renderer(rgb2, sig2, z2, opt.white_bkgd)))
        if getattr(opt, "check_numerics", True):
            self.netCoarse.check("coarse network")
            if opt.N_importance > 0:
                self.netFine.check("fine network")
        return out

    def forward(self, coarse_rgb: Optional[bool] = None):
        """With ``coarse_rgb`` False (default: ``opt.coarse_rgb``) ``out_coarse_comp_rgbs`` is not set -- and one left by an
        earlier forward is removed: the reference's loops test the ``out_*`` attributes with ``hasattr``."""
        out = self.forward_rays(self.data_rays, coarse_rgb)
        for name in ("out_coarse_comp_rgbs", "out_coarse_comp_rgbs_ori"):
            if "coarse_comp_rgbs" not in out and hasattr(self, name):
                delattr(self, name)
        for name, v in out.items():
            setattr(self, f"out_{name}", v)

    # -- A1 / A2 ---------------------------------------------------------------------
    def comp_low_res_output(self):
        s2 = self.opt.downscale ** 2
        any_out = self.out_coarse_comp_rgbs if hasattr(self, "out_coarse_comp_rgbs") else self.out_fine_comp_rgbs
        n_lr = self.data_rgbs.shape[0] if hasattr(self, "data_rgbs") else any_out.shape[0] // s2
        for name in ("coarse_comp_rgbs", "coarse_depth", "fine_comp_rgbs", "fine_depth"):
            if hasattr(self, f"out_{name}"):
                hr = getattr(self, f"out_{name}")
                setattr(self, f"out_{name}_ori", hr)
                setattr(self, f"out_{name}", ops.sr_mean(hr, n_lr, s2))

    def unflatten_reshape(self, input: torch.Tensor) -> torch.Tensor:
        return ops.unflatten_reshape(input, self.opt.img_wh, self.opt.downscale)

    # -- scoring (nerf_downX_model.py:355-388, the eval-side half; :469-516) ---------------
    @torch.no_grad()
    def calculate_losses(self):
        """``comp_low_res_output()``, then the MSE losses and the PSNRs of the LR means against ``data_rgbs`` and, when
        ``data_rgbs_ori`` is set, of the rendered rays against it -- each a 0-d fp32 device tensor out of ``nsr_psnr`` (sums in
        double, no host read).  Like the reference's, it reduces the ``out_*`` of ONE ``forward()``: call it once per forward."""
        from . import metrics
        if not hasattr(self, "out_coarse_comp_rgbs"):
            raise ValueError("calculate_losses scores the coarse colour, which the last forward() did not compute: "
                             "coarse_rgb=False (opt.coarse_rgb) is a test-time mode -- score with coarse_rgb=True")
        self.comp_low_res_output()
        fine = hasattr(self, "out_fine_comp_rgbs")
        mse_c, psnr_c = metrics.mse_psnr(self.out_coarse_comp_rgbs, self.data_rgbs)
        self.loss_coarse_mse = (mse_c * float(getattr(self.opt, "lambda_coarse_mse", 1))).float()
        self.loss_coarse_psnr = psnr_c.float()
        if fine:
            mse_f, psnr_f = metrics.mse_psnr(self.out_fine_comp_rgbs, self.data_rgbs)
            self.loss_fine_mse = (mse_f * float(getattr(self.opt, "lambda_fine_mse", 1))).float()
            self.loss_fine_psnr = psnr_f.float()
        else:
            self.loss_fine_mse, self.loss_fine_psnr = 0, 0
        self.loss_tot = self.loss_coarse_mse + self.loss_fine_mse
        if hasattr(self, "data_rgbs_ori"):
            self.loss_coarse_psnr_ori = metrics.mse_psnr(self.out_coarse_comp_rgbs_ori, self.data_rgbs_ori)[1].float()
            if fine:
                self.loss_fine_psnr_ori = metrics.mse_psnr(self.out_fine_comp_rgbs_ori, self.data_rgbs_ori)[1].float()

    @torch.no_grad()
    def calculate_ssim(self):
        """This build's addition (the reference lists SSIM as a to-do, nerf_downX_model.py:103): ``loss_fine_ssim`` of the LR
        image against ``data_rgbs`` and ``loss_fine_ssim_ori`` of the HR image against ``data_rgbs_ori``, (H, W, 3) frames
        read in place (layout BHWC), data_range (0, 1).  Needs ``opt.img_wh`` to be the frame the rays cover; returns False
        (and sets nothing) when it is not, or when there is no fine pass."""
        from . import metrics
        W, H = int(self.opt.img_wh[0]), int(self.opt.img_wh[1])
        s = int(self.opt.downscale)
        H1, W1 = H // s, W // s
        if not hasattr(self, "out_fine_comp_rgbs_ori") or not hasattr(self, "data_rgbs") or self.data_rgbs.shape[0] != H1 * W1 \
                or self.out_fine_comp_rgbs_ori.shape[0] != H1 * W1 * s * s:
            return False
        if not hasattr(self, "_ssim"):
            self._ssim = metrics.SSIM(data_range=(0, 1))
        self.loss_fine_ssim = self._ssim(self.out_fine_comp_rgbs.reshape(1, H1, W1, 3), self.data_rgbs.reshape(1, H1, W1, 3), layout="BHWC")
        if hasattr(self, "data_rgbs_ori"):
            self.loss_fine_ssim_ori = self._ssim(self.unflatten_reshape(self.out_fine_comp_rgbs_ori).unsqueeze(0),
                                                 self.unflatten_reshape(self.data_rgbs_ori).unsqueeze(0), layout="BHWC")
        return True

    @torch.no_grad()
    def validate(self, dataset) -> Dict[str, float]:
        """The reference's validation loop without its savers: for every dict of ``dataset`` ``set_input`` -> ``forward`` ->
        ``calculate_losses`` (-> ``calculate_ssim``) in eval mode, the scores averaged over the dataset.  They are accumulated on the
        device and read ONCE at the end (the reference: four ``.item()`` per image); the ``loss_*`` attributes end up as
        Python floats, as there, and are returned by name."""
        names = ["loss_coarse_psnr", "loss_fine_psnr", "loss_coarse_psnr_ori", "loss_fine_psnr_ori", "loss_fine_ssim",
                 "loss_fine_ssim_ori"]
        for k in names[2:]:
            if hasattr(self, k):
                delattr(self, k)
        if not bool(getattr(self.opt, "coarse_rgb", True)):
            raise ValueError("validate scores the coarse colour: opt.coarse_rgb=False is a test-time mode -- validate with coarse_rgb=True")
        was, self.randomized = self.randomized, False
        sums, n = {}, 0
        try:
            for data in dataset:
                self.set_input(data)
                self.forward()
                self.calculate_losses()
                self.calculate_ssim()
                for k in names:
                    v = getattr(self, k, None)
                    if isinstance(v, torch.Tensor):
                        sums[k] = v.double() if k not in sums else sums[k] + v.double()
                n += 1
        finally:
            self.randomized = was
        if n == 0:
            raise ValueError("validate: the dataset is empty")
        keys = list(sums)
        means = (torch.stack([sums[k] for k in keys]) / n).tolist() if keys else []       # the one host read
        res = dict(zip(keys, means))
        for k, v in res.items():
            setattr(self, k, v)
        return res

    # -- full image (test loop body, nerf_downX_model.py:621-669 without the savers) -----
    @torch.no_grad()
    def render_image(self, c2w, focal: float, ndc: bool, near: float = 0.0, far: float = 1.0, coarse_rgb: Optional[bool] = None):
        """Rays generated on the device -> forward -> LR means + HR image of one pose.  ``coarse_rgb`` (default:
        ``opt.coarse_rgb``) False: the coarse pass computes densities only; the frame is bit-identical."""
        rays = ops.subpixel_rays(c2w, self.opt.img_wh, focal, self.opt.downscale, ndc, near, far, self.device)
        self.set_input({"rays": rays})
        self.forward(coarse_rgb)
        hr = self.unflatten_reshape(self.out_fine_comp_rgbs)
        self.comp_low_res_output()
        return {"hr_rgb": hr, "lr_rgb": self.out_fine_comp_rgbs, "lr_depth": self.out_fine_depth}

    @torch.no_grad()
    def render_image_sharded(self, c2w, focal: float, ndc: bool, near: float = 0.0, far: float = 1.0, group=None,
                             lr_range=None, workspace=None, outs=None, gather: str = "lr", want_weights: bool = False,
                             coarse_rgb: Optional[bool] = None):
        """One frame rendered by all ranks of ``group`` together (BASELINE config #4): the LR-pixel range
        is cut into contiguous blocks (``dist.shard_bounds``; an LR pixel's s*s sub-rays stay on one GPU), every rank
        GENERATES its own ray block on its device (nothing is scattered), runs the eval-mode ``forward_rays`` on it, and
        ONE all-gather assembles the frame on every rank.  Replaces the per-MLP-call scatter / gather of
        nn.DataParallel (models/networks.py:54-69).  No reduction crosses a block boundary, so the result is
        bit-identical to ``render_image`` on one GPU.  That holds with ``opt.early_stop`` too, at the same threshold: the kernel
        decides per group of four consecutive rays, shards start at multiples of s*s >= 4 rays, so the groups of a sharded
        render are the groups of the whole frame.  The exception is ``downscale`` s = 1, whose shards start at any ray: the
        groups then differ between the two renders and the frames agree within the option's bound only.

        ``gather``: what the collective carries.
          * ``"lr"`` (default): the s*s means, [r, g, b, depth] per LR pixel (16 B / LR pixel) -> ``lr_rgb``, ``lr_depth``.
          * ``"hr"``: the rendered pixels themselves -- ``fine_comp_rgbs``, 12 B per ray (9.1 MB for config
            #4) -- the reference's test-time deliverable (``unflatten_reshape`` of ``out_fine_comp_rgbs_ori``,
            models/nerf_downX_model.py:410-416, feeding calculate_vis :430-450 and test :621-669).  Blocks are
            LR-pixel-major, so the gathered buffer IS the (n_lr * s*s, 3) ray-major tensor ``unflatten_reshape`` takes:
            every rank returns ``hr_rgb`` (H, W, 3), and ``lr_rgb`` as the s*s means of the gathered rays (the same
            arithmetic on the same values as the per-block means).  ``lr_depth`` is not part of this exchange.
        ``want_weights`` (default False): a frame render does not use the per-sample ``weights`` arrays of the reference's
        8-entry dict; leaving them out saves 195 of the 261 MB the fine-pass launch moves through HBM on config #2
        (``forward_rays`` itself, the drop-in for the reference's method, still returns all eight).
        ``coarse_rgb`` (default: ``opt.coarse_rgb``) False: the density-only coarse pass (same frame, bit for bit); it needs a
        fine pass and the fused f16x3 networks.
        ``lr_range`` overrides this rank's block and skips the collective (single-process tests).  Returns the assembled
        arrays plus this rank's own outputs (``local``) and ``bytes_per_rank`` (payload of the collective)."""
        from . import dist as nsr_dist
        if gather not in ("lr", "hr"):
            raise ValueError("gather must be 'lr' or 'hr'")
        opt = self.opt
        with_rgb = self._check_coarse_rgb(coarse_rgb)
        s, s2 = int(opt.downscale), int(opt.downscale) ** 2
        n_lr = (opt.img_wh[1] // s) * (opt.img_wh[0] // s)
        rank, world = nsr_dist._world(group)
        lo, hi = lr_range if lr_range is not None else nsr_dist.shard_bounds(n_lr, world)[rank]
        rays = ops.subpixel_rays(c2w, opt.img_wh, focal, s, ndc, near, far, self.device, lr_range=(lo, hi)).view(-1, 8)
        fine = opt.N_importance > 0
        if self.fused:
            out = ops.forward_rays(self.netCoarse, self.netFine if fine else None, rays, opt.N_coarse, opt.N_importance,
                                   opt.white_bkgd, opt.lindisp, workspace=workspace, outs=outs, want_weights=want_weights,
                                   sigma_activation=self.renderer.sigma_activation, early_stop=self._check_early_stop(),
                                   coarse_rgb=with_rgb)
        else:               # a GenericMLP pair: the eval-mode staged route
            was, self.randomized = self.randomized, False
            try:
                out = self.forward_rays(rays, with_rgb)
            finally:
                self.randomized = was
        tag = "fine" if fine else "coarse"
        cap = (lo, hi) if lr_range is not None else nsr_dist.shard_bounds(n_lr, world)[0]   # the block the payload is sized by
        if gather == "hr":
            # one row per LR pixel holding its s*s rendered rays: the block structure all_gather_pixels assumes
            local = out[f"{tag}_comp_rgbs"].reshape(hi - lo, s2 * 3)
            full = local if lr_range is not None else nsr_dist.all_gather_pixels(local, n_lr, group)
            res = {"lr_range": (lo, hi), "local": out, "bytes_per_rank": (cap[1] - cap[0]) * s2 * 12}
            if lr_range is None:
                hr_rays = full.reshape(n_lr * s2, 3)
                res["hr_rgb"] = self.unflatten_reshape(hr_rays)
                res["lr_rgb"] = ops.sr_mean(hr_rays, n_lr, s2)
            else:
                res["hr_rays"] = full.reshape((hi - lo) * s2, 3)
            return res
        local = torch.empty(hi - lo, 4, dtype=torch.float32, device=self.device)
        if hi > lo:
            local[:, :3] = ops.sr_mean(out[f"{tag}_comp_rgbs"], hi - lo, s2)
            local[:, 3:] = ops.sr_mean(out[f"{tag}_depth"], hi - lo, s2)
        full = local if lr_range is not None else nsr_dist.all_gather_pixels(local, n_lr, group)
        return {"lr_rgb": full[:, :3], "lr_depth": full[:, 3], "lr_range": (lo, hi), "local": out,
                "bytes_per_rank": (cap[1] - cap[0]) * 16}
