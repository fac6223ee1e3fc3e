"""Every caller-owned workspace is pure scratch, and its stated size suffices.

The headers call the `workspace` of every entry point scratch ("the workspace is scratch and may be shared by any number of
them", include/nsr_train.h; "device scratch of nsr_forward_rays_workspace_bytes_for(...) bytes", include/nsr.h), and the Python
layer relies on it: its workspaces are grow-only buffers reused across shapes and paths.  For every entry point that takes one,
at the smallest shapes where the carve, an exact-extent memset or a ragged last pass could go wrong, this file asserts four
properties, all bitwise (tests/scratch_state.py: guarded views, the fills, the reporter):

  1. baseline        two calls after the same fill (ZERO) give the same bits in every output;
  2. fill            the outputs after ONES (0xFF: NaN / -1) and LEFTOVER (the bytes a call of another shape or path left in
                     its workspace) equal those after ZERO; outputs are pre-filled with 0xFF and come back fully overwritten;
                     for the train-mode pairs `saved` is pre-filled too, the workspace is filled again between the forward and
                     the backward (it may be shared, include/nsr_train.h), and the backward's gradients are compared;
  3. sizes           workspace, `saved` and every output are views of exactly the stated number of bytes in front of a 1 MiB
                     guard of 0xA5 bytes; after the call and a synchronize every guard is intact;
  4. reuse           through the Python object that owns the grow-only buffer: a call at a larger shape or on another path,
                     then the small call, which must give the bits it gives on a fresh owner.

State that is NOT scratch, excluded exactly:
  * the first 64 bytes of a training workspace, the sticky status block -- include/nsr_train.h: "The FIRST 64 BYTES of the
    workspace are a sticky status block ... nsr_train_status_reset zeroes the block (call it once when the workspace is
    allocated: the step never clears it)".  Every run here calls nsr_train_status_reset after filling and asserts that the
    flags read 0 after the healthy call;
  * `saved` between a forward and its backward -- include/nsr_train.h: "What the backward needs stays in the caller's `saved`
    buffer ... `saved` is not modified"; include/nsr_refine.h says the same of the refinement pair.  It is filled BEFORE the
    forward only;
  * packed weight blobs and their status tails (include/nsr.h, nsr_pack_weights; include/nsr_refine.h) are not workspaces: the
    tests pack once per module and never touch them.

Integer regions of the workspaces and saved buffers, and where a call writes each before any kernel reads it (read from the
carve functions: work_floats / carve_kept in csrc/nsr_train.hip, carve_pack in csrc/nsr_train_gemm.hip, work_floats in
csrc/nsr_refine.hip, carve_saved / carve_work in csrc/nsr_refine_train.hip).  None of them is ever read as an index, a count
or an offset, so no fill can send a kernel out of bounds; what a stale value could do is change arithmetic:
  * training workspace, word 0 of the status block (NSR_FLAG_* bits): only ORed into by kernels, read by nsr_train_status on
    the host.  Word 1 (chain path: the colour-head option word the TRAIN forward kernel reads): written on every call by
    nsr_chain_bwd_pack2 from prepare_call, in front of the first forward launch (csrc/nsr_train.hip, prepare_call);
  * Kept.sgn (chain path: sign bits of the forward activations, one bit per value): written by nsr_f16x3_train_forward for
    every point of the pass in front of nsr_chain_bwd, which reads them as bit masks;
  * Work.gmax (chain path: ten words, float bits of the largest gradient magnitude per panel): cleared by block 0 of
    composite_bwd_kernel, the launch in front of the chain kernel that atomicMax'es into them (csrc/nsr_train.hip,
    composite_bwd_kernel; nsr_chain_bwd is told gmax_is_zero = 1), read by chain_weight_grads as float bits;
  * Work.carry (eight doubles, loss sums across chunks): chain path: cleared by nsr_chain_bwd_pack2; GEMM path: hipMemsetAsync
    in prepare_call; the pair's entry points do not use it;
  * Work.g_comp (float): hipMemsetAsync in train_backward only `if (!go[0])`, otherwise the caller's upstream gradient is read;
  * saved header of the training pair (magic, floats, R, chunk, sample counts, flags, precision, descriptor, embed word):
    written by saved_header_kernel first thing in train_forward; train_backward reads it to the HOST and validates every field
    against the buffer size before anything loops over it;
  * refinement-training saved header (magic, floats, B, R, H, W, img_chunk, precision): header_kernel first thing in
    nsr_refine_train_forward_p; validated on the host by the backward;
  * refinement-training Saved.win (one byte per max-pooled feature: which reference won): written by max_idx_kernel for every
    element in the forward; route_kernel COMPARES it with r (`win == r`), it never indexes with it;
  * refinement-training range word (float bits, behind the re-laid weight in Work.wr): hipMemsetAsync per site in front of the
    kernel that atomicMax'es into it (site_backward), only on the split-fp16 routes;
  * 16-bit operand planes (Work.wr under f16x3, the refinement inference activations, the chain panels) are float data.
Metrics, losses and the render driver keep only floats / doubles (depths, weights, per-tile partial sums).

A failure names the case, the fill and the tensor.  Nothing here is meant to fault: the guard is ordinary allocated memory."""
import ctypes
import os
import time
from collections import OrderedDict
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from nerf_sr_amd.weights import make_state_dict, make_state_dict_arch, arch_spec, normalize_arch, STATE_DICT_SPEC
from tests import scratch_state as ss
from tests.scratch_state import ZERO, ONES, LEFTOVER

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    t0 = time.time()
    yield _lib.load()
    print(f"\ntests/test_gpu_scratch_state.py: {time.time() - t0:.1f} s wall")


def _p(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _ptrs(ts):
    return (c_void_p * len(ts))(*[_p(t) for t in ts])


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _snap(g: ss.Guarded) -> torch.Tensor:
    """The bytes a call left in a guarded buffer's body: the LEFTOVER of a later run."""
    return g.base[:g.nbytes].clone()


def _four_runs(case: str, run, donor):
    """``run(fill, leftover) -> (name -> tensor, problems)``: properties 1-3 of the module docstring.  ``donor()``: the bytes a
    call of another shape or path left behind."""
    bad = []
    zero, p = run(ZERO, None)
    bad += [f"{case} [ZERO]: {x}" for x in p]
    again, p = run(ZERO, None)
    bad += [f"{case} [ZERO, second call]: {x}" for x in p]
    bad += ss.diff_all(f"{case} [baseline: ZERO twice]", again, zero)
    for fill, left in ((ONES, None), (LEFTOVER, donor())):
        got, p = run(fill, left)
        bad += [f"{case} [{fill}]: {x}" for x in p]
        bad += ss.diff_all(f"{case} [{fill} against ZERO]", got, zero)
    assert not bad, "\n".join(bad)
    return zero


def _assert_live(case: str, res: dict):
    """The case is not degenerate (a guard on the test's own inputs): both passes render something without saturating every
    ray, and of a training case's gradient tensors at least nine in ten hold a non-zero element."""
    for k in ("coarse_opacity", "fine_opacity"):
        assert 0.0 < float(res[k].max()) and float(res[k].min()) < 1.0, (case, k, res[k])
    grads = [v for k, v in res.items() if k.startswith("grad ")]
    live = sum(int(bool(v.any())) for v in grads)
    assert live >= 0.9 * len(grads), (case, live, len(grads))


def _collect(guards, outputs):
    """After a synchronize: damage lines of the guards, the elements the call left unwritten, and CPU copies of the outputs."""
    torch.cuda.synchronize()
    problems = ss.check_guards(guards)
    res = OrderedDict()
    for name, t in outputs.items():
        line = ss.unwritten(name, t)
        if line:
            problems.append(line)
        res[name] = t.detach().cpu().clone()
    return res, problems


# =========================================================================================================== A. render
@pytest.fixture(scope="module")
def render():
    from nerf_sr_amd import cameras, ops
    lo = 252 * 95 + 100
    rays = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, 0.0, 1.0, device=DEV,
                             lr_range=(lo, lo + 65)).view(-1, 8)[:259].contiguous()
    nets = {}

    def net(prec):
        if prec not in nets:
            nets[prec] = tuple(ops.VanillaMLP(None, precision=prec).load_state_dict(make_state_dict(seed, "smooth"))
                               for seed in ss.RENDER_SEEDS)
        return nets[prec]
    return ops, rays, net


def _render_run(render, prec, R, nc, ni, opts, fill, leftover):
    ops, rays, net = render
    coarse, fine = net(prec)
    need = _lib.load().nsr_forward_rays_workspace_bytes_for(coarse._prec, R, nc, ni)
    ws = ss.guarded(need, fill, DEV, leftover=leftover)
    shapes = {"coarse_comp_rgbs": (R, 3), "coarse_depth": (R,), "coarse_opacity": (R,), "coarse_weights": (R, nc),
              "fine_comp_rgbs": (R, 3), "fine_depth": (R,), "fine_opacity": (R,), "fine_weights": (R, nc + ni)}
    if opts.get("coarse_rgb") is False:
        del shapes["coarse_comp_rgbs"]                       # neither read nor written in test-time mode (include/nsr.h)
    outs = {k: ss.guarded_like(s, torch.float32, DEV, name=k) for k, s in shapes.items()}
    given = {k: g.view for k, g in outs.items()}
    got = ops.forward_rays(coarse, fine, rays[:R], nc, ni, False, workspace=ws.view, outs=dict(given), **opts)
    assert all(got[k].data_ptr() == given[k].data_ptr() for k in given), "forward_rays replaced a caller's buffer"
    res, problems = _collect([ws] + list(outs.values()), given)
    for n in (coarse, fine):
        if n.status() != 0:
            problems.append(f"status {n.status(clear=True):#x}")
    return res, problems, ws


_RENDER_IDS = [f"{p}-R{R}-{nc}+{ni}" + "".join(f"-{k}" for k in o) for p, R, nc, ni, o in ss.RENDER_CASES]


@pytest.mark.parametrize("prec,R,nc,ni,opts", ss.RENDER_CASES, ids=_RENDER_IDS)
def test_render_workspace_is_scratch(render, prec, R, nc, ni, opts):
    """ops.forward_rays(workspace=, outs=): eight (seven in test-time mode) guarded outputs, a guarded workspace of exactly
    nsr_forward_rays_workspace_bytes_for bytes.  LEFTOVER: what the same precision left at another ray count and the other
    importance count (192 samples take the unfused route under fp32 and the 16-bit precisions: another carve)."""
    def donor():
        return _snap(_render_run(render, prec, 264 - R, nc, 192 - ni, {}, ZERO, None)[2])
    case = f"render {prec} R={R} {nc}+{ni} {opts}"
    _assert_live(case, _four_runs(case, lambda f, l: _render_run(render, prec, R, nc, ni, opts, f, l)[:2], donor))


def test_render_reuse_across_shapes(render):
    """R = 259 with 128 importance samples, then R = 5 with 64 in the same buffer and the same output dict's storage."""
    ops, rays, net = render
    (prec, Rb, ncb, nib), (_, Rs, ncs, nis) = ss.RENDER_REUSE
    coarse, fine = net(prec)
    fresh = ops.forward_rays(coarse, fine, rays[:Rs], ncs, nis, False)
    fresh = {k: v.cpu().clone() for k, v in fresh.items()}
    ws = torch.empty(_lib.load().nsr_forward_rays_workspace_bytes_for(coarse._prec, Rb, ncb, nib), dtype=torch.uint8, device=DEV)
    ops.forward_rays(coarse, fine, rays[:Rb], ncb, nib, False, workspace=ws)
    got = ops.forward_rays(coarse, fine, rays[:Rs], ncs, nis, False, workspace=ws)
    torch.cuda.synchronize()
    bad = ss.diff_all("render reuse: R=5 after R=259", {k: v.cpu() for k, v in got.items()}, fresh)
    assert not bad, "\n".join(bad)


# ================================================================================ B, C. training: fused step and the pair
def _load_train(golden_dir):
    g = np.load(os.path.join(golden_dir, "train_llff_rand.npz"))
    assert g["rays"].shape == (ss.TRAIN_R, 8) and int(g["s2"]) == ss.TRAIN_S2
    return g


@pytest.fixture(scope="module")
def batch(golden_dir):
    g = _load_train(golden_dir)
    dev = lambda k: torch.from_numpy(np.ascontiguousarray(g[k])).to(DEV)
    draws = {k: dev(k) for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine")}
    gen = torch.Generator().manual_seed(41)
    R, nc, nf = ss.TRAIN_R, ss.TRAIN_NC, ss.TRAIN_NC + ss.TRAIN_NI
    # upstream gradients of all eight outputs of the pair (any loss written in torch), fixed
    shapes = [(R, 3), (R,), (R,), (R, nc), (R, 3), (R,), (R,), (R, nf)]
    g_outs = [(torch.randn(*s, generator=gen) * 0.1).to(DEV) for s in shapes]
    return {"rays": dev("rays"), "target": dev("target_lr"), "draws": draws, "noise_std": float(g["noise_std"]), "g_outs": g_outs,
            "w": [[torch.from_numpy(v).to(DEV) for v in make_state_dict(int(g[s])).values()] for s in ("seed_coarse", "seed_fine")]}


def _rays_per_pass(chunk, R):
    return chunk if 0 < chunk < R else R


def _status(ws_view, what, problems):
    flags = ctypes.c_uint(0)
    _lib.check(_lib.load().nsr_train_status(_p(ws_view), 0, ctypes.byref(flags), _stream()), "nsr_train_status")
    if flags.value != 0:
        problems.append(f"status block reads {flags.value:#x} after {what}")


def _train_ws(need, fill, leftover):
    ws = ss.guarded(need, fill, DEV, leftover=leftover)
    _lib.check(_lib.load().nsr_train_status_reset(_p(ws.view), _stream()), "nsr_train_status_reset")   # the block is not scratch
    return ws


def _refill(ws, fill, leftover):
    ss.fill_bytes(ws.view, fill, leftover)
    _lib.check(_lib.load().nsr_train_status_reset(_p(ws.view), _stream()), "nsr_train_status_reset")


def _out_guards(R, nc, nf):
    from nerf_sr_amd.ops import OUT_KEYS
    shapes = [(R, 3), (R,), (R,), (R, nc), (R, 3), (R,), (R,), (R, nf)]
    return OrderedDict((k, ss.guarded_like(s, torch.float32, DEV, name=k)) for k, s in zip(OUT_KEYS, shapes))


def _grad_guards(weights):
    return [[ss.guarded_like(tuple(t.shape), torch.float32, DEV, name=f"grad[{n}][{i}]") for i, t in enumerate(ws)]
            for n, ws in enumerate(weights)]


def _fused_run(batch, prec, chunk, fill, leftover):
    """nsr_train_loss_and_grads through ctypes (what Trainer.loss_and_grads calls) with guarded workspace, outputs, s2 means,
    losses and gradients."""
    lib = _lib.load()
    R, nc, ni, s2 = ss.TRAIN_R, ss.TRAIN_NC, ss.TRAIN_NI, ss.TRAIN_S2
    p = _lib.TRAIN_PRECISIONS[prec]
    ws = _train_ws(lib.nsr_train_workspace_bytes_for(p, _rays_per_pass(chunk, R), nc, ni), fill, leftover)
    outs = _out_guards(R, nc, nc + ni)
    lr = [ss.guarded_like((R // s2, 3), torch.float32, DEV, name=f"lr_{n}") for n in ("coarse", "fine")]
    losses = ss.guarded_like((2,), torch.float32, DEV, name="losses")
    grads = _grad_guards(batch["w"])
    d = batch["draws"]
    rc = lib.nsr_train_loss_and_grads(
        _ptrs(batch["w"][0]), _ptrs(batch["w"][1]), _ptrs([g.view for g in grads[0]]), _ptrs([g.view for g in grads[1]]),
        _p(batch["rays"]), 8, R, s2, _p(batch["target"]), nc, ni, 0, 0, _p(d["u_coarse"]), _p(d["u_fine"]), _p(d["noise_coarse"]),
        _p(d["noise_fine"]), batch["noise_std"], 1.0, 1.0, p, chunk, _ptrs([g.view for g in outs.values()]), _p(lr[0].view),
        _p(lr[1].view), _p(losses.view), _p(ws.view), ws.nbytes, _stream())
    _lib.check(rc, "nsr_train_loss_and_grads")
    named = OrderedDict((k, g.view) for k, g in outs.items())
    named.update({"lr_coarse": lr[0].view, "lr_fine": lr[1].view, "losses": losses.view})
    for n in range(2):
        for k, g in zip(STATE_DICT_SPEC, grads[n]):
            named[f"grad {'coarse' if n == 0 else 'fine'} {k}"] = g.view
    res, problems = _collect([ws, losses] + lr + list(outs.values()) + grads[0] + grads[1], named)
    _status(ws.view, "nsr_train_loss_and_grads", problems)
    return res, problems, ws


def _pair_run(run, names, weights, rays, draws, g_outs, fill, leftover, leftover_saved=None):
    """The forward / backward pair behind train.forward_rays_train (``run``: its _TrainRun, which picks nsr_train_forward /
    nsr_train_arch_forward[_e] and their size functions) through ctypes: guarded workspace, `saved`, outputs and gradients.
    `saved` is filled before the forward; the workspace is filled again between the two calls."""
    R, nc, ni = rays.shape[0], run.nc, run.ni
    what, need = run.call("workspace_bytes", run.prec, _rays_per_pass(run.chunk, R), nc, ni)
    what_s, nsaved = run.call("saved_bytes", run.prec, R, nc, ni, run.chunk)
    assert need > 0 and nsaved > 0, (what, need, what_s, nsaved)
    ws = _train_ws(need, fill, leftover)
    saved = ss.guarded(nsaved, fill, DEV, leftover=leftover_saved if leftover_saved is not None else leftover, name="saved")
    outs = _out_guards(R, nc, nc + ni)
    grads = _grad_guards(weights)
    d = [draws.get(k) for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine")]
    what, rc = run.call("forward", _ptrs(weights[0]), _ptrs(weights[1]), _p(rays), 8, R, nc, ni, run.flags, run.lindisp,
                        *[_p(t) for t in d], run.noise_std, run.prec, run.chunk, _ptrs([g.view for g in outs.values()]),
                        _p(ws.view), ws.nbytes, _p(saved.view), saved.nbytes, _stream())
    _lib.check(rc, what)
    problems = []
    _status(ws.view, what, problems)
    after_forward = _snap(ws)
    _refill(ws, fill, leftover)              # the workspace may serve other calls between a forward and its backward
    what, rc = run.call("backward", _ptrs(weights[0]), _ptrs(weights[1]), _ptrs(g_outs), _ptrs([g.view for g in grads[0]]),
                        _ptrs([g.view for g in grads[1]]), _p(ws.view), ws.nbytes, _p(saved.view), saved.nbytes, _stream())
    _lib.check(rc, what)
    named = OrderedDict((k, g.view) for k, g in outs.items())
    for n in range(2):
        for k, g in zip(names, grads[n]):
            named[f"grad {'coarse' if n == 0 else 'fine'} {k}"] = g.view
    res, p2 = _collect([ws, saved] + list(outs.values()) + grads[0] + grads[1], named)
    _status(ws.view, what, p2)
    return res, problems + p2, ws, after_forward, saved


def _default_pair(batch, prec, chunk, fill, leftover, R=None):
    from nerf_sr_amd.train import _TrainRun
    R = ss.TRAIN_R if R is None else R
    run = _TrainRun(ss.TRAIN_NC, ss.TRAIN_NI, 0, 0, batch["noise_std"], _lib.TRAIN_PRECISIONS[prec], chunk, None)
    draws = {k: v[:R].contiguous() for k, v in batch["draws"].items()}
    return _pair_run(run, list(STATE_DICT_SPEC), batch["w"], batch["rays"][:R].contiguous(), draws,
                     [g[:R].contiguous() for g in batch["g_outs"]], fill, leftover)


_TRAIN_IDS = [f"{e}-{p}-chunk{c}" for e, p, c in ss.TRAIN_CASES]


@pytest.mark.parametrize("entry,prec,chunk", ss.TRAIN_CASES, ids=_TRAIN_IDS)
def test_default_training_workspace_is_scratch(batch, entry, prec, chunk):
    """nsr_train_loss_and_grads and the nsr_train_forward / nsr_train_backward pair on the batch and draws of
    tests/golden/train_llff_rand.npz, unchunked and in 40-ray chunks with a ragged 16-ray last pass (passes after the first see
    the previous pass's bytes in a differently sized carve).  LEFTOVER: what the pair left at 32 rays under the other kind of
    path (the GEMM path for the chain precision and the reverse): other buffers at other offsets."""
    def donor():
        other = "fp32" if prec == "f16x3" else "f16x3"
        _, _, ws, after_forward, _ = _default_pair(batch, other, 0, ZERO, None, R=32)
        return torch.cat([after_forward, _snap(ws)])
    if entry == "fused":
        run = lambda f, l: _fused_run(batch, prec, chunk, f, l)[:2]
    else:
        run = lambda f, l: _default_pair(batch, prec, chunk, f, l)[:2]
    case = f"train {entry} {prec} ray_chunk={chunk}"
    _assert_live(case, _four_runs(case, run, donor))


def _patch_and_draws():
    """The 8 x 8 HR raster of 64 rays and the seeded draws of tests/test_gpu_losses.py::_patch_and_draws."""
    from nerf_sr_amd import ops, cameras
    patch = ops.subpixel_rays(cameras.spiral_pose(0.5), (64, 48), cameras.llff_focal(64), 2, True)
    patch = patch.reshape(24, 32, 2, 2, 8)[4:8, 4:8].permute(0, 2, 1, 3, 4).reshape(-1, 8).contiguous()
    gen = torch.Generator().manual_seed(2)
    draws = {"u_coarse": torch.rand(64, 64, generator=gen), "noise_coarse": torch.randn(64, 64, generator=gen),
             "u_fine": torch.rand(64, 64, generator=gen), "noise_fine": torch.randn(64, 128, generator=gen)}
    return patch, {k: v.to(DEV) for k, v in draws.items()}


def _grads_of(t):
    return {f"grad {n} {k}": v.detach().cpu().clone() for n in range(2) for k, v in t.grads[n].items()}


@pytest.mark.parametrize("prec", ss.TRAIN_PRECISIONS)
def test_trainer_reuses_one_workspace_across_paths(golden_dir, prec):
    """One Trainer: a full fused step, regularize_patch on the 8 x 8 patch (the autograd pair at 64 rays, in the buffer the
    96-ray step grew), the full step again.  lr = 0 keeps the weights, so the second full step must give the bits of the first,
    and the patch step the bits it gives on a fresh Trainer."""
    from nerf_sr_amd import train
    g = _load_train(golden_dir)
    draws = {k: torch.from_numpy(g[k]).to(DEV) for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine")}
    patch, pdraws = _patch_and_draws()

    def make():
        t = train.Trainer(make_state_dict(int(g["seed_coarse"])), make_state_dict(int(g["seed_fine"])), downscale=2, randomized=True,
                          noise_std=float(g["noise_std"]), precision=prec, lr=0.0, ray_chunk=0)
        t.set_input(torch.from_numpy(g["rays"]).to(DEV), torch.from_numpy(g["target_lr"]).to(DEV))
        return t

    def step(t):
        t.loss_and_grads(draws)
        torch.cuda.synchronize()
        res = {k: v.detach().cpu().clone() for k, v in t.out.items()}
        res["losses"] = t.losses.cpu().clone()
        res.update(_grads_of(t))
        return res

    def patch_step(t):
        tv = t.regularize_patch(patch, 4, 0.7, draws=pdraws)
        torch.cuda.synchronize()
        res = {k: v.detach().cpu().clone() for k, v in t.out_patch.items()}
        res["tv"] = tv.cpu().clone()
        res.update(_grads_of(t))
        return res

    fresh_patch = patch_step(make())
    t = make()
    first = step(t)
    buf = t._ws
    got_patch = patch_step(t)
    again = step(t)
    assert t._ws is buf, "the workspace was reallocated: the reuse was not exercised"
    bad = ss.diff_all(f"trainer {prec}: patch step after a full step, against a fresh Trainer", got_patch, fresh_patch)
    bad += ss.diff_all(f"trainer {prec}: full step after the patch step, against the first", again, first)
    if t.status() != 0:
        bad.append(f"trainer {prec}: status {t.status():#x}")
    assert not bad, "\n".join(bad)


@pytest.fixture(scope="module")
def arch_batch(batch):
    R = ss.ARCH_R
    gen = torch.Generator().manual_seed(43)
    draws = {"u_coarse": torch.rand(R, 64, generator=gen).to(DEV), "u_fine": torch.rand(R, 64, generator=gen).to(DEV),
             "noise_coarse": torch.randn(R, 64, generator=gen).to(DEV), "noise_fine": torch.randn(R, 128, generator=gen).to(DEV)}
    arch = normalize_arch(dict(ss.ARCH))
    w = {}
    for embed in (0, 1):
        w[embed] = [[torch.from_numpy(v).to(DEV) for v in make_state_dict_arch(seed, no_xyz=bool(embed), **ss.ARCH).values()]
                    for seed in ss.ARCH_SEEDS]
    return {"rays": batch["rays"][:R].contiguous(), "draws": draws, "g_outs": [g[:R].contiguous() for g in batch["g_outs"]],
            "arch": arch, "w": w}


def _arch_pair(ab, prec, embed, chunk, fill, leftover, R=None):
    from nerf_sr_amd.train import _TrainRun
    R = ss.ARCH_R if R is None else R
    run = _TrainRun(64, 64, 0, 0, 1.0, _lib.TRAIN_PRECISIONS[prec], chunk, None, _lib.NsrArch.from_arch(ab["arch"]), embed)
    names = list(arch_spec(no_xyz=bool(embed), **ss.ARCH))
    return _pair_run(run, names, ab["w"][embed], ab["rays"][:R].contiguous(), {k: v[:R].contiguous() for k, v in ab["draws"].items()},
                     [g[:R].contiguous() for g in ab["g_outs"]], fill, leftover)


@pytest.mark.parametrize("prec,embed,chunk", ss.ARCH_CASES, ids=[f"{p}-embed{e}-chunk{c}" for p, e, c in ss.ARCH_CASES])
def test_arch_training_workspace_is_scratch(arch_batch, prec, embed, chunk):
    """nsr_train_arch_forward / _backward (embed 1: the `_e` pair under --no_xyz) for D = 3, W = 48 (Wp = 64), a skip at layer
    1: 7 rays = 448 coarse points, 3.5 tiles of 128 (P / 128 + 1 = 4 rows of tile sums); in chunks of 3 the passes hold
    192 / 384 / 192 / 384 / 64 / 128 points.  LEFTOVER: the same pair at 4 rays with the other embedding word (other widths)."""
    def donor():
        _, _, ws, after_forward, _ = _arch_pair(arch_batch, prec, 1 - embed, 0, ZERO, None, R=4)
        return torch.cat([after_forward, _snap(ws)])
    case = f"arch train {prec} embed={embed} ray_chunk={chunk}"
    _assert_live(case, _four_runs(case, lambda f, l: _arch_pair(arch_batch, prec, embed, chunk, f, l)[:2], donor))


# ================================================================================================ D. refinement inference
@pytest.fixture(scope="module")
def refine_nets():
    from nerf_sr_amd import refine as rf
    made = {}

    def get(prec, with_ref):
        key = (prec, with_ref)
        if key not in made:
            made[key] = rf.MaxPoolingModel(precision=prec, device=DEV, not_use_ref=not with_ref).load_state_dict(
                rf.make_refine_state_dict(5, not_use_ref=not with_ref))
        return made[key]
    return get


def _refine_inputs(B, R, H, W):
    gen = torch.Generator().manual_seed(100 * B + R)
    return (torch.rand(B, 3, H, W, generator=gen) * 2 - 1).to(DEV), (torch.rand(B, R, 3, H, W, generator=gen) * 2 - 1).to(DEV)


def _refine_run(net, with_ref, shape, fill, leftover):
    lib = _lib.load()
    B, R, H, W = shape
    x, c = _refine_inputs(B, R, H, W)
    need = lib.nsr_refine_workspace_bytes_for(net._prec, B, R if with_ref else 1, H, W)
    ws = ss.guarded(need, fill, DEV, leftover=leftover)
    out = ss.guarded_like((B, 3, H, W), torch.float32, DEV, name="refined")
    if with_ref:
        rc = lib.nsr_refine_forward(_p(net.packed), net._prec, _p(x), _p(c), B, R, H, W, _p(out.view), _p(ws.view), ws.nbytes, _stream())
    else:
        rc = lib.nsr_refine_forward_noref(_p(net.packed), net._prec, _p(x), B, H, W, _p(out.view), _p(ws.view), ws.nbytes, _stream())
    _lib.check(rc, "nsr_refine_forward")
    res, problems = _collect([ws, out], {"refined": out.view})
    return res, problems, ws


@pytest.mark.parametrize("prec,with_ref,shape", ss.REFINE_CASES,
                         ids=[f"{p}-{'ref' if r else 'noref'}-{'x'.join(map(str, s))}" for p, r, s in ss.REFINE_CASES])
def test_refine_workspace_is_scratch(refine_nets, prec, with_ref, shape):
    """nsr_refine_forward / nsr_refine_forward_noref at B = 3, R = 2, 16 x 24 (an incomplete eight-image block: the clamped
    gather of tests/test_gpu_refine.py) and B = 9, R = 1, 16 x 16.  LEFTOVER: the other of the two shapes."""
    net = refine_nets(prec, with_ref)
    other = [s for s in ss.REFINE_SHAPES if s != shape][0]
    donor = lambda: _snap(_refine_run(net, with_ref, other, ZERO, None)[2])
    _four_runs(f"refine {prec} {'with' if with_ref else 'without'} references {shape}", lambda f, l: _refine_run(net, with_ref, shape, f, l)[:2], donor)


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("with_ref", [True, False], ids=["ref", "noref"])
def test_refine_model_reuses_its_workspace(prec, with_ref):
    """MaxPoolingModel._ws: B = 9 first, then B = 3 in the same buffer, against a freshly constructed model."""
    from nerf_sr_amd import refine as rf
    small, big = ss.REFINE_SHAPES
    sd = rf.make_refine_state_dict(5, not_use_ref=not with_ref)
    make = lambda: rf.MaxPoolingModel(precision=prec, device=DEV, not_use_ref=not with_ref).load_state_dict(sd)
    xs, cs = _refine_inputs(*small)
    xb, cb = _refine_inputs(*big)
    fresh = make()(xs, cs).cpu().clone()
    m = make()
    m(xb, cb)
    buf = m._ws
    got = m(xs, cs).cpu().clone()
    assert m._ws is buf and buf.numel() > _lib.load().nsr_refine_workspace_bytes_for(m._prec, small[0], small[1] if with_ref else 1, *small[2:])
    line = ss.diff(f"refine {prec} {'ref' if with_ref else 'noref'}: B=3 after B=9 in one _ws", got, fresh)
    assert line is None, line


# ================================================================================================= E. refinement training
@pytest.fixture(scope="module")
def refine_train(golden_dir):
    from nerf_sr_amd import refine as rf
    fx = np.load(os.path.join(golden_dir, "refine_train.npz"))
    sd = rf.make_refine_state_dict(int(fx["weights_seed"]))
    return rf, fx, OrderedDict((k, torch.from_numpy(sd[k]).to(DEV)) for k in rf.REFINE_SPEC)


def _refine_train_run(refine_train, combo, tag, img_chunk, fill, leftover):
    rf, fx, sd0 = refine_train
    lib = _lib.load()
    prec, wgrad = rf.TRAIN_PRECISIONS[combo[0]], rf.WEIGHT_GRADS[combo[1]]
    x, c = (torch.from_numpy(fx[f"{tag}_{k}"]).to(DEV) for k in ("x", "c"))
    B, R, H, W = c.shape[0], c.shape[1], c.shape[3], c.shape[4]
    assert (B, R, H, W) == ss.REFINE_TRAIN_SHAPES[tag]
    sd = OrderedDict((k, v.clone()) for k, v in sd0.items())      # the running statistics are updated in place: same start
    running = [ss.guarded_like(tuple(sd[k].shape), torch.float32, DEV, name=k) for k in rf.RUNNING_KEYS]
    for g, k in zip(running, rf.RUNNING_KEYS):
        g.view.copy_(sd[k])
        sd[k] = g.view
    ws = ss.guarded(lib.nsr_refine_train_workspace_bytes(B, R, H, W, img_chunk), fill, DEV, leftover=leftover)
    saved = ss.guarded(lib.nsr_refine_train_saved_bytes(B, R, H, W), fill, DEV, leftover=leftover, name="saved")
    y = ss.guarded_like((B, 3, H, W), torch.float32, DEV, name="y")
    t106 = _ptrs(list(sd.values()))
    rc = lib.nsr_refine_train_forward_p(prec, t106, _ptrs([g.view for g in running]), 0.1, _p(x), _p(c), B, R, H, W, img_chunk,
                                        _p(y.view), _p(ws.view), ws.nbytes, _p(saved.view), saved.nbytes, _stream())
    _lib.check(rc, "nsr_refine_train_forward_p")
    torch.cuda.synchronize()
    after_forward = _snap(ws)
    ss.fill_bytes(ws.view, fill, leftover)
    gen = torch.Generator().manual_seed(9)
    g_out = (torch.randn(B, 3, H, W, generator=gen) / (B * 3 * H * W)).to(DEV)
    grads = [ss.guarded_like(tuple(sd[k].shape), torch.float32, DEV, name=f"grad {k}") for k in rf.TRAIN_PARAM_KEYS]
    rc = lib.nsr_refine_train_backward_w(prec, wgrad, t106, _p(g_out), _ptrs([g.view for g in grads]), _p(ws.view), ws.nbytes,
                                         _p(saved.view), saved.nbytes, _stream())
    _lib.check(rc, "nsr_refine_train_backward_w")
    named = OrderedDict([("y", y.view)])
    named.update((g.name, g.view) for g in running)
    named.update((g.name, g.view) for g in grads)
    res, problems = _collect([ws, saved, y] + running + grads, named)
    return res, problems, ws, after_forward


@pytest.mark.parametrize("combo,tag,img_chunk", ss.REFINE_TRAIN_CASES,
                         ids=[f"{c[0]}-wgrad_{c[1]}-{t}-chunk{i}" for c, t, i in ss.REFINE_TRAIN_CASES])
def test_refine_training_workspace_is_scratch(refine_train, combo, tag, img_chunk):
    """nsr_refine_train_forward_p / nsr_refine_train_backward_w at the shapes of fixture cases A (2, 2, 16, 24) and B
    (3, 1, 16, 16), img_chunk 0 and 1: at the deepest sites M = nc * rows_img is 4 .. 24 and one level up 16 .. 48 (the sites
    are named in tests/test_scratch_state_cpu.py), so the `Kp > M` rows of the col matrix and the 32 zeroed rows behind dZ are
    read.  Outputs: y, the 34 running statistics (updated in place from the same copies), the 72 gradients.  LEFTOVER: the other
    case's shape with the other img_chunk."""
    def donor():
        other = "B" if tag == "A" else "A"
        _, _, ws, after_forward = _refine_train_run(refine_train, combo, other, 1 - img_chunk, ZERO, None)
        return torch.cat([after_forward, _snap(ws)])
    _four_runs(f"refine train {combo} case {tag} img_chunk={img_chunk}",
               lambda f, l: _refine_train_run(refine_train, combo, tag, img_chunk, f, l)[:2], donor)


@pytest.mark.parametrize("combo", ss.REFINE_TRAIN_COMBOS, ids=[f"{c[0]}-wgrad_{c[1]}" for c in ss.REFINE_TRAIN_COMBOS])
def test_refine_forward_train_reuses_train_ws(refine_train, combo):
    """refine.forward_train and the module's _TRAIN_WS: fixture case C's shape (2, 8, 16, 16) first, then case B's, against
    case B on an empty _TRAIN_WS."""
    rf, fx, sd0 = refine_train

    def run(tag):
        params = OrderedDict((k, sd0[k].clone().requires_grad_(True)) for k in rf.TRAIN_PARAM_KEYS)
        running = OrderedDict((k, sd0[k].clone()) for k in rf.RUNNING_KEYS)
        x, c, gt = (torch.from_numpy(fx[f"{tag}_{k}"]).to(DEV) for k in ("x", "c", "gt"))
        y = rf.forward_train(params, running, x, c, precision=combo[0], weight_grad=combo[1])
        torch.nn.functional.l1_loss(y, gt).backward()
        torch.cuda.synchronize()
        res = {"y": y.detach().cpu().clone()}
        res.update((k, v.cpu().clone()) for k, v in running.items())
        res.update((f"grad {k}", v.grad.cpu().clone()) for k, v in params.items())
        return res

    rf._TRAIN_WS.clear()
    fresh = run("B")
    rf._TRAIN_WS.clear()
    run("C")
    (buf,) = rf._TRAIN_WS.values()
    got = run("B")
    assert next(iter(rf._TRAIN_WS.values())) is buf
    bad = ss.diff_all(f"refine forward_train {combo}: case B after case C in _TRAIN_WS", got, fresh)
    assert not bad, "\n".join(bad)


# =========================================================================================================== F. metrics
@pytest.fixture(scope="module")
def metric_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


def _ssim_run(fx, tag, fill, leftover):
    from nerf_sr_amd import metrics
    lib = _lib.load()
    x, y = torch.from_numpy(fx[f"x_{tag}"]).to(DEV), torch.from_numpy(fx[f"y_{tag}"]).to(DEV)
    B, C, H, W = x.shape
    s = metrics.SSIM(data_range=tuple(fx[f"range_{tag}"].tolist()), kernel_size=tuple(int(k) for k in fx[f"kernel_size_{tag}"]),
                     sigma=tuple(fx[f"sigma_{tag}"].tolist()), gaussian=bool(fx[f"gaussian_{tag}"]))
    ws = ss.guarded(lib.nsr_ssim_workspace_bytes(B, C, H, W), fill, DEV, leftover=leftover)
    vals = ss.guarded_like((B,), torch.float64, DEV, name="ssim")
    smap = ss.guarded_like((B, C, H, W), torch.float32, DEV, name="ssim_map")
    rc = lib.nsr_ssim(_p(x), _p(y), B, C, H, W, metrics.LAYOUTS["BCHW"], _p(s._window(x.device)), s.kernel_size[0], s.kernel_size[1],
                      s.c1, s.c2, _p(vals.view), _p(smap.view), _p(ws.view), ws.nbytes, _stream())
    _lib.check(rc, "nsr_ssim")
    res, problems = _collect([ws, vals, smap], {"ssim": vals.view, "ssim_map": smap.view})
    return res, problems, ws


def _psnr_run(fx, tag, fill, leftover):
    lib = _lib.load()
    x, y = torch.from_numpy(fx[f"x_{tag}"]).to(DEV), torch.from_numpy(fx[f"y_{tag}"]).to(DEV)
    B, n = x.shape[0], x[0].numel()
    mask = (torch.rand(B, n, generator=torch.Generator().manual_seed(3)) < 0.7).to(torch.uint8).to(DEV)       # an element mask
    ws = ss.guarded(lib.nsr_psnr_workspace_bytes(B, n), fill, DEV, leftover=leftover)
    mse = ss.guarded_like((B,), torch.float64, DEV, name="mse")
    psnr = ss.guarded_like((B,), torch.float64, DEV, name="psnr")
    rc = lib.nsr_psnr(_p(x), _p(y), B, n, _p(mask), 1, _p(mse.view), _p(psnr.view), _p(ws.view), ws.nbytes, _stream())
    _lib.check(rc, "nsr_psnr")
    res, problems = _collect([ws, mse, psnr], {"mse": mse.view, "psnr": psnr.view})
    return res, problems, ws


@pytest.mark.parametrize("tag", ss.METRIC_TAGS)
@pytest.mark.parametrize("metric", ["ssim", "psnr"])
def test_metric_workspace_is_scratch(metric_fx, metric, tag):
    """nsr_ssim (values and map) and nsr_psnr (per image, with an element mask) on the `ragged` (45 x 70: ragged 32 x 32 tiles)
    and `tiny` (6 x 7) fixtures.  LEFTOVER: what the same metric left on the other fixture."""
    fn = _ssim_run if metric == "ssim" else _psnr_run
    other = [t for t in ss.METRIC_TAGS if t != tag][0]
    _four_runs(f"{metric} {tag}", lambda f, l: fn(metric_fx, tag, f, l)[:2], lambda: _snap(fn(metric_fx, other, ZERO, None)[2]))


def _loss_inputs(kind):
    gen = torch.Generator().manual_seed(13)
    if kind == "tv":
        return (torch.rand(45, 70, 3, generator=gen).to(DEV),)
    if kind == "gradient":
        return torch.rand(2, 3, 45, 70, generator=gen).to(DEV), torch.rand(2, 3, 45, 70, generator=gen).to(DEV)
    return torch.rand(2, 45, 70, generator=gen).to(DEV), torch.rand(2, 45, 70, 3, generator=gen).to(DEV)


@pytest.mark.parametrize("kind", ["tv", "gradient", "laplacian"])
def test_loss_forward_workspace_guard_and_ones(kind):
    """The forward workspaces of the three patch losses (tests/test_gpu_losses.py already has
    test_reproducible_and_fully_overwritten): a guard behind exactly nsr_loss_workspace_bytes bytes, and ONES against ZERO."""
    lib = _lib.load()
    t = _loss_inputs(kind)
    res, bad = {}, []
    for fill in (ZERO, ONES):
        loss = ss.guarded_like((1,), torch.float64, DEV, name="loss")
        if kind == "tv":
            H, W, C = t[0].shape
            ws = ss.guarded(lib.nsr_loss_workspace_bytes(_lib.NSR_LOSS_TV, 1, C, H, W), fill, DEV)
            rc = lib.nsr_tv_loss(_p(t[0]), H, W, C, _p(loss.view), _p(ws.view), ws.nbytes, _stream())
        elif kind == "gradient":
            B, C, H, W = t[0].shape
            ws = ss.guarded(lib.nsr_loss_workspace_bytes(_lib.NSR_LOSS_GRADIENT, B, C, H, W), fill, DEV)
            rc = lib.nsr_gradient_loss(_p(t[0]), _p(t[1]), B, C, H, W, _p(loss.view), _p(ws.view), ws.nbytes, _stream())
        else:
            N, H, W = t[0].shape
            ws = ss.guarded(lib.nsr_loss_workspace_bytes(_lib.NSR_LOSS_LAPLACIAN, N, 3, H, W), fill, DEV)
            rc = lib.nsr_laplacian_loss(_p(t[0]), _p(t[1]), N, H, W, 3, 0.1, _p(loss.view), _p(ws.view), ws.nbytes, _stream())
        _lib.check(rc, f"{kind} loss")
        res[fill], p = _collect([ws, loss], {"loss": loss.view})
        bad += [f"{kind} loss [{fill}]: {x}" for x in p]
    bad += ss.diff_all(f"{kind} loss [ONES against ZERO]", res[ONES], res[ZERO])
    assert not bad, "\n".join(bad)


def test_metrics_reuse_one_workspace(metric_fx):
    """metrics._WS, shared by SSIM, PSNR and the patch losses: a bilateral Laplacian loss at 70 x 45 first, then SSIM at the
    `tiny` shape, against SSIM on an empty _WS."""
    from nerf_sr_amd import losses, metrics
    fx = metric_fx
    x, y = torch.from_numpy(fx["x_tiny"]).to(DEV), torch.from_numpy(fx["y_tiny"]).to(DEV)
    s = metrics.SSIM(data_range=tuple(fx["range_tiny"].tolist()))
    run = lambda: {k: v.cpu().clone() for k, v in zip(("ssim", "ssim_map"), s(x, y, reduction="none", return_map=True))}
    metrics._WS.clear()
    fresh = run()
    metrics._WS.clear()
    d, guide = _loss_inputs("laplacian")
    losses.BilateralLaplacianLoss(gamma=0.1)(d, guide)
    losses.GradientLoss()(*_loss_inputs("gradient"))
    (buf,) = metrics._WS.values()
    got = run()
    assert next(iter(metrics._WS.values())) is buf
    bad = ss.diff_all("SSIM tiny after a 70 x 45 loss in metrics._WS", got, fresh)
    assert not bad, "\n".join(bad)
