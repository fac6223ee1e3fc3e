"""d(loss)/d(rays) of the CHAIN training pair (nsr_train_forward / nsr_train_backward_r, include/nsr_train.h) behind
``train.forward_rays_train(..., chain_ray_grad=True)`` on the default network, and d(loss)/d(c2w) through
``cameras.rays_from_pose``.

Reference: the fp64 restatement of the reference's iteration (tests/arch_util.forward_train with ``rays.requires_grad_()``), as in
tests/test_gpu_ray_grads.py, whose cases, oracle cache and helpers are shared.  Bound: the project's per-tensor gradient bound,
2e-3 of the norm, on each of the g_o (columns 0:3) and g_d (3:6) blocks of the gated cases (on which the restatement's own fp32
run stays within 2.7e-4 of fp64); ``llff_rand`` / ``blender_rand`` are computed and recorded, not gated, for the reason given
there.  With NSR_RECORD_PROFILES set, the figures go to profiles/chain_ray_grads_parity.json (a directory as the variable's value
receives the file instead), next to the layer-by-layer 'f16x3_gemm' ray gradient's distance from the same oracle."""
import json
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from oracle import nerf_oracle as oc
from tests import arch_util as au
from tests import scratch_state as ss
from tests.test_gpu_ray_grads import (BOUND, DEFAULT_GATED, DEFAULT_RECORDED, _ORACLE, _aux_loss, _blocks, _case, _oracle, _oracle_of,
                                      _oracle_rays, _p, _ptrs, _rays11, _reference_loss, _stream, _sum_loss, _upstream)
from tests.test_gpu_ray_grads import _hip as _hip_layers

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ("f16x3", "f16x3_bwd3")
_PARITY = {}


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import train as _tr
    yield _tr
    dst = os.environ.get("NSR_RECORD_PROFILES")
    if dst and _PARITY:
        path = os.path.join(dst if os.path.isdir(dst) else os.path.join(REPO, "profiles"), "chain_ray_grads_parity.json")
        with open(path, "w") as f:
            json.dump({"reference": "fp64 restatement of the reference's iteration with rays.requires_grad_(); figures are "
                                    "|delta| / |g| over the g_o, g_d blocks; f16x3_gemm = the layer-by-layer pair's ray gradient "
                                    "against the same oracle (not gated here)",
                       "bound": BOUND, "cases": _PARITY}, f, indent=1, sort_keys=True)
            f.write("\n")


def _hip(tr, c, prec, loss=None, rays=None, chunk=0, wrt_rays=True, wrt_weights=True):
    """(rays.grad, weight gradients, outputs) of forward_rays_train on the chain pair."""
    p = [{k: torch.from_numpy(np.asarray(v)).cuda().requires_grad_(wrt_weights) for k, v in s.items()} for s in c["sds"]]
    r = torch.as_tensor(c["rays"] if rays is None else rays).cuda().clone().requires_grad_(wrt_rays)
    draws = {k: torch.as_tensor(v).cuda() for k, v in c["draws"].items()}
    out = tr.forward_rays_train(p[0], p[1], r, draws, N_coarse=c["nc"], N_importance=c["ni"], white_bkgd=c["white_bkgd"],
                                noise_std=c["noise_std"], precision=prec, ray_chunk=chunk, chain_ray_grad=True, **c["flags"])
    total = (loss or _reference_loss(c, torch.float32, "cuda"))(out)
    leaves = [p[n][k] for n in range(2) for k in p[n]] if wrt_weights else []
    grads = torch.autograd.grad(total, leaves + ([r] if wrt_rays else []), allow_unused=True)
    return (grads[-1] if wrt_rays else None), grads[:len(leaves)], out


def _trim(golden_dir, R, nc=64, ni=64, name="llff_gamma", s2=1):
    """the first R rays of a default-network case at nc + ni samples"""
    c = _case(golden_dir, name)
    d = c["draws"]
    c.update(rays=c["rays"][:R].copy(), nc=nc, ni=ni, target=c["target"][:R // s2], s2=s2,
             draws={k: np.asarray(v)[:R, :{"u_coarse": nc, "u_fine": ni, "noise_coarse": nc, "noise_fine": nc + ni}[k]].copy()
                    for k, v in d.items()})
    return c


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(DEFAULT_GATED) + list(DEFAULT_RECORDED))
def test_ray_gradient_vs_fp64_oracle(golden_dir, tr, name, prec):
    c, want = _oracle_of(golden_dir, name)
    assert c["arch"] == dict(au.DEFAULT_ARCH)
    got = _hip(tr, c, prec)[0].cpu().numpy()
    fig = _blocks(got, want)
    entry = _PARITY.setdefault(name, {})
    entry[prec] = fig
    if os.environ.get("NSR_RECORD_PROFILES") and "f16x3_gemm" not in entry:
        entry["f16x3_gemm"] = _blocks(_hip_layers(tr, c, "f16x3_gemm")[0].cpu().numpy(), want)
    print(f"chain ray gradient {name}-{prec}: g_o {fig['g_o']:.2e} g_d {fig['g_d']:.2e} (|g_o| {np.linalg.norm(want[:, :3]):.3e}, "
          f"|g_d| {np.linalg.norm(want[:, 3:6]):.3e}) {entry.get('f16x3_gemm', '')}")
    assert got.shape == c["rays"].shape and np.isfinite(got).all()
    assert (got[:, 6:8] == 0.0).all(), "near / far get exact zeros"
    assert np.linalg.norm(want[:, :6]) > 0.0
    if name in DEFAULT_GATED:
        assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND, (name, prec, fig)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_eleven_wide_rays(golden_dir, tr, prec):
    c = _trim(golden_dir, 8, s2=4)
    rays = _rays11(c["rays"])
    if "chain_eleven" not in _ORACLE:
        _ORACLE["chain_eleven"] = (_oracle(c, rays=rays)[0], _oracle(c)[0])
    want, want8 = _ORACLE["chain_eleven"]
    got = _hip(tr, c, prec, rays=rays)[0].cpu().numpy()
    fig = _blocks(got, want)
    print(f"chain ray gradient at 11 columns, {prec}: {fig}")
    assert got.shape == (8, 11) and (got[:, 6:8] == 0.0).all()
    assert np.linalg.norm(want[:, 8:11]) > 0.0 and np.linalg.norm(want[:, 3:6] - want8[:, 3:6]) > 0.0
    assert max(fig.values()) <= BOUND, fig


@pytest.mark.parametrize("prec", PRECISIONS)
def test_loss_over_all_eight_outputs(golden_dir, tr, prec):
    c = _trim(golden_dir, 8, s2=4)
    f = _aux_loss(8, 64, 128)
    if "chain_aux" not in _ORACLE:
        _ORACLE["chain_aux"] = _oracle(c, loss=f)[0]
    fig = _blocks(_hip(tr, c, prec, loss=f)[0].cpu().numpy(), _ORACLE["chain_aux"])
    print(f"chain ray gradient, loss over all eight outputs, {prec}: {fig}")
    assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND, fig


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("R,nc,ni", ((4, 8, 8), (2, 16, 32)))      # several rays in a 32-point group; a ray that starts mid-group
def test_small_shapes(golden_dir, tr, prec, R, nc, ni):
    c = _trim(golden_dir, R, nc, ni, s2=R)
    key = ("chain_small", R, nc, ni)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(c)[0]
    fig = _blocks(_hip(tr, c, prec)[0].cpu().numpy(), _ORACLE[key])
    print(f"chain ray gradient, {R} rays of {nc} + {ni} samples, {prec}: {fig}")
    assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND, fig


@pytest.mark.parametrize("prec", PRECISIONS)
def test_pose_gradient(golden_dir, tr, prec):
    """d(loss)/d(c2w) through cameras.rays_from_pose + the chain pair on an 8 x 6 <- 4 x 3 frame, against the fp64 chain."""
    from nerf_sr_amd import cameras
    rg = np.load(os.path.join(golden_dir, "raygrid.npz"))
    W, H, s = 8, 6, 2
    c2w, focal = rg["blender_c2w"].astype(np.float64)[:3, :4], float(rg["blender_focal"]) * W / int(rg["W"])
    ndc, near, far = False, 2.0, 6.0
    R = H * W
    c = _trim(golden_dir, R, name="blender_softplus", s2=4)
    c.update(target=np.random.default_rng(11).random((R // 4, 3)).astype(np.float32))
    if "chain_pose" not in _ORACLE:
        p64 = torch.from_numpy(c2w).clone().requires_grad_(True)
        sd = [oc.to_torch_sd(sd_, torch.float64) for sd_ in c["sds"]]
        out = au.forward_train(sd[0], sd[1], _oracle_rays(p64, H, W, focal, s, ndc, near, far), c["arch"], 64, 64, c["white_bkgd"],
                               noise_std=c["noise_std"], **{k: torch.as_tensor(v).double() for k, v in c["draws"].items()}, **c["flags"])
        _reference_loss(c, torch.float64, "cpu")(out).backward()
        _ORACLE["chain_pose"] = p64.grad.numpy().copy()
    want = _ORACLE["chain_pose"]
    pose = torch.from_numpy(c2w.astype(np.float32)).cuda().requires_grad_(True)
    rays = cameras.rays_from_pose(pose, H, W, focal, s, ndc, near, far)
    p = [{k: torch.from_numpy(v).cuda() for k, v in s_.items()} for s_ in c["sds"]]
    out = tr.forward_rays_train(p[0], p[1], rays, {k: torch.as_tensor(v).cuda() for k, v in c["draws"].items()},
                                white_bkgd=c["white_bkgd"], noise_std=c["noise_std"], precision=prec, chain_ray_grad=True, **c["flags"])
    _reference_loss(c, torch.float32, "cuda")(out).backward()
    got = pose.grad.cpu().double().numpy()
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"chain pose gradient {prec}: {rel:.2e} of |g| = {np.linalg.norm(want):.3e}")
    assert np.linalg.norm(want) > 0.0 and rel <= BOUND, (prec, rel)


def test_trainer_fills_rays_grad(golden_dir, tr):
    c, want = _oracle_of(golden_dir, "llff_gamma")
    t = tr.Trainer(*c["sds"], white_bkgd=c["white_bkgd"], downscale=2, noise_std=c["noise_std"], precision="f16x3", chain_ray_grad=True,
                   **c["flags"])
    rays = torch.from_numpy(c["rays"]).cuda().requires_grad_(True)
    out = t.forward({k: torch.as_tensor(v).cuda() for k, v in c["draws"].items()}, rays=rays)
    t.backward(_reference_loss(c, torch.float32, "cuda")(out))
    assert rays.grad is not None
    fig = _blocks(rays.grad.cpu().numpy(), want)
    assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND and float(t.grads[0]["sigma.weight"].abs().max()) > 0.0
    # without the keyword the trainer refuses as before
    t0 = tr.Trainer(*c["sds"], precision="f16x3")
    with pytest.raises(ValueError, match="fp32"):
        t0.forward(None, rays=rays)


# ---- bit identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_bit_identities(golden_dir, tr, prec):
    """R = 5 rays of 64 + 64 samples: the rows do not depend on ray_chunk (2 and 3 leave a ragged last chunk), follow a
    permutation of the batch, repeat bit for bit; outputs and weight gradients are those of the call without the ray gradient;
    a frozen field (no weight leaf requires grad: NSR_BACKWARD_NO_WEIGHT_GRADS) gives the same rows."""
    c = _trim(golden_dir, 5)
    base, wg, out = _hip(tr, c, prec, loss=_sum_loss)
    assert float(base[:, :6].abs().max()) > 0.0 and bool((base[:, 6:8] == 0).all())
    again, wg2, _ = _hip(tr, c, prec, loss=_sum_loss)
    assert torch.equal(base, again) and all(torch.equal(a, b) for a, b in zip(wg, wg2))
    for chunk in (2, 3):
        assert torch.equal(_hip(tr, c, prec, loss=_sum_loss, chunk=chunk)[0], base), chunk
    perm = np.array([3, 0, 4, 2, 1])
    cp = dict(c, rays=c["rays"][perm].copy(), draws={k: v[perm].copy() for k, v in c["draws"].items()})
    assert torch.equal(_hip(tr, cp, prec, loss=_sum_loss)[0], base[torch.from_numpy(perm).cuda()])
    _, wg0, out0 = _hip(tr, c, prec, loss=_sum_loss, wrt_rays=False)      # nsr_train_backward
    assert all(torch.equal(a, b) for a, b in zip(wg, wg0)) and all(torch.equal(out[k], out0[k]) for k in out)
    frozen, none, _ = _hip(tr, c, prec, loss=_sum_loss, wrt_weights=False)
    assert torch.equal(frozen, base) and len(none) == 0


@pytest.mark.parametrize("prec", PRECISIONS)
def test_exact_zeros(golden_dir, tr, prec):
    c = _trim(golden_dir, 4, 8, 8, s2=4)
    colour = lambda o: o["fine_comp_rgbs"].square().sum() + o["coarse_comp_rgbs"].square().sum()
    rays = _rays11(c["rays"])
    g, _, _ = _hip(tr, dict(c, flags=dict(c["flags"], stop_grad=True)), prec, loss=colour, rays=rays)
    assert bool((g[:, 8:11] == 0.0).all()) and bool((g[:, 6:8] == 0.0).all()) and float(g[:, :6].abs().max()) > 0.0
    g, _, _ = _hip(tr, c, prec, loss=colour, rays=rays)
    assert float(g[:, 8:11].abs().max()) > 0.0 and bool((g[:, 6:8] == 0.0).all())


# ---- the C entry point itself ---------------------------------------------------------------------------------------------------
class _ChainPair:
    """One nsr_train_forward on case ``c`` through ctypes; ``backward`` calls a backward entry on its saved state."""

    def __init__(self, c, prec, flags=0):
        self.lib = _lib.load()
        self.prec = _lib.TRAIN_PRECISIONS[prec]
        self.w = [[torch.from_numpy(np.asarray(v)).cuda() for v in s.values()] for s in c["sds"]]
        self.rays = torch.as_tensor(c["rays"]).cuda().contiguous()
        self.R, self.nc, self.ni = self.rays.shape[0], c["nc"], c["ni"]
        d = [None if c["draws"].get(k) is None else torch.as_tensor(c["draws"][k]).cuda().contiguous()
             for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine")]
        self.need_for = self.lib.nsr_train_workspace_bytes_for(self.prec, self.R, self.nc, self.ni)
        self.need_r = self.lib.nsr_train_workspace_bytes_r(self.prec, self.R, self.nc, self.ni)
        nsaved = self.lib.nsr_train_saved_bytes(self.prec, self.R, self.nc, self.ni, 0)
        assert 0 < self.need_for <= self.need_r and nsaved > 0
        self.saved = torch.empty(nsaved, dtype=torch.uint8, device="cuda")
        self.ws = torch.zeros(self.need_r, dtype=torch.uint8, device="cuda")
        shapes = [(self.R, 3), (self.R,), (self.R,), (self.R, self.nc), (self.R, 3), (self.R,), (self.R,), (self.R, self.nc + self.ni)]
        self.outs = [torch.empty(s, device="cuda") for s in shapes]
        _lib.check(self.lib.nsr_train_forward(
            _ptrs(self.w[0]), _ptrs(self.w[1]), _p(self.rays), self.rays.shape[1], self.R, self.nc, self.ni, flags, 0,
            *[_p(t) for t in d], c["noise_std"], self.prec, 0, _ptrs(self.outs), _p(self.ws), self.need_for, _p(self.saved), nsaved,
            _stream()), "nsr_train_forward")

    def backward(self, entry, g_outs, g_rays=None, flags=0, stride=None, g_stride=None, ws=None, ws_bytes=None, no_grads=False):
        """entry 'plain' / 'r'; returns (status, weight gradients prefilled with 7.0)."""
        grads = [[torch.full_like(t, 7.0) for t in n] for n in self.w]
        ws = self.ws if ws is None else ws
        s = self.rays.shape[1]
        tail = (_p(ws), ws.numel() if ws_bytes is None else ws_bytes, _p(self.saved), self.saved.numel(), _stream())
        gc, gf = (None, None) if no_grads else (_ptrs(grads[0]), _ptrs(grads[1]))
        if entry == "plain":
            rc = self.lib.nsr_train_backward(_ptrs(self.w[0]), _ptrs(self.w[1]), _ptrs(g_outs), gc, gf, *tail)
        else:
            rc = self.lib.nsr_train_backward_r(_ptrs(self.w[0]), _ptrs(self.w[1]), _p(self.rays), s if stride is None else stride,
                                               _ptrs(g_outs), gc, gf, _p(g_rays), s if g_stride is None else g_stride, flags, *tail)
        torch.cuda.synchronize()
        return rc, grads


@pytest.mark.parametrize("prec", PRECISIONS)
def test_entry_point_identities(golden_dir, prec):
    """g_rays NULL and flags 0 IS nsr_train_backward (in its workspace size); with g_rays the weight gradients keep their bits;
    under NSR_BACKWARD_NO_WEIGHT_GRADS the rows keep theirs and gradient buffers prefilled with 7.0 stay 7.0 (or may be NULL)."""
    c = _trim(golden_dir, 5)
    pair = _ChainPair(c, prec)
    g_outs = _upstream(5, 64, 128)
    rc_p, gp = pair.backward("plain", g_outs, ws_bytes=pair.need_for)
    rc_0, g0 = pair.backward("r", g_outs, None, ws_bytes=pair.need_for)
    g_rays = torch.full((5, 8), float("nan"), device="cuda")
    rc_r, gr = pair.backward("r", g_outs, g_rays)
    assert (rc_p, rc_0, rc_r) == (0, 0, 0)
    for a, b, d in zip(gp[0] + gp[1], g0[0] + g0[1], gr[0] + gr[1]):
        assert torch.equal(a, b) and torch.equal(a, d) and not bool((a == 7.0).all())
    assert bool(torch.isfinite(g_rays).all()) and float(g_rays[:, :6].abs().max()) > 0.0 and bool((g_rays[:, 6:8] == 0).all())
    g_frozen = torch.full((5, 8), float("nan"), device="cuda")
    rc_f, gfz = pair.backward("r", g_outs, g_frozen, flags=_lib.NSR_BACKWARD_NO_WEIGHT_GRADS)
    assert rc_f == 0 and torch.equal(g_frozen, g_rays) and all(bool((t == 7.0).all()) for n in gfz for t in n)
    g_null = torch.full((5, 8), float("nan"), device="cuda")
    assert pair.backward("r", g_outs, g_null, flags=_lib.NSR_BACKWARD_NO_WEIGHT_GRADS, no_grads=True)[0] == 0
    assert torch.equal(g_null, g_rays)
    g_zero = torch.full((5, 8), float("nan"), device="cuda")
    assert pair.backward("r", [None] * 8, g_zero)[0] == 0 and bool((g_zero == 0.0).all()), "all upstream gradients NULL"


def test_misuse_leaves_everything_untouched(golden_dir):
    c = _trim(golden_dir, 5)
    pair = _ChainPair(c, "f16x3")
    g_outs = _upstream(5, 64, 128)
    g_rays = torch.full((5, 11), 7.0, device="cuda")
    for what, kw, want in (("another stride than the forward's", {"stride": 11, "g_stride": 11}, -1),
                           ("two strides", {"g_stride": 11}, -1), ("a stride that is none", {"stride": 9, "g_stride": 9}, -1),
                           ("a workspace one granule short", {"ws_bytes": pair.need_r - 256}, -4),
                           ("an unknown flag", {"flags": 2}, -1)):
        rc, grads = pair.backward("r", g_outs, g_rays, **kw)
        assert rc == want, (what, rc)
        assert bool((g_rays == 7.0).all()) and all(bool((t == 7.0).all()) for n in grads for t in n), what
    rc, grads = pair.backward("r", g_outs, None, flags=_lib.NSR_BACKWARD_NO_WEIGHT_GRADS)
    assert rc == -1 and all(bool((t == 7.0).all()) for n in grads for t in n), "the flag without g_rays"
    assert pair.need_r > pair.need_for
    # a saved state of a layer-by-layer precision has nsr_train_arch_backward_r: unsupported here, with g_rays or with a flag
    fp = _ChainPair(c, "fp32")
    g8 = torch.full((5, 8), 7.0, device="cuda")
    for kw in ({"g_rays": g8}, {"g_rays": g8, "flags": _lib.NSR_BACKWARD_NO_WEIGHT_GRADS}):
        rc, grads = fp.backward("r", g_outs, **kw)
        assert rc == -2 and bool((g8 == 7.0).all()) and all(bool((t == 7.0).all()) for n in grads for t in n), kw
    rc, grads = fp.backward("r", g_outs, None)      # ... and without either it is nsr_train_backward
    rc_p, gp = fp.backward("plain", g_outs)
    assert rc == 0 and rc_p == 0 and all(torch.equal(a, b) for a, b in zip(grads[0] + grads[1], gp[0] + gp[1]))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_r_workspace_is_scratch(golden_dir, prec):
    """nsr_train_backward_r in a guarded workspace of exactly nsr_train_workspace_bytes_r, filled with zeros, with ones and with
    what another call left: the same bits everywhere, no byte outside written (tests/scratch_state.py)."""
    c = _trim(golden_dir, 5)
    pair = _ChainPair(c, prec)
    g_outs = _upstream(5, 64, 128)
    res, bad = {}, []
    for fill, left in ((ss.ZERO, None), (ss.ONES, None), (ss.LEFTOVER, pair.ws.clone())):
        ws = ss.guarded(pair.need_r, fill, "cuda", leftover=left)
        _lib.check(pair.lib.nsr_train_status_reset(_p(ws.view), _stream()), "nsr_train_status_reset")
        g_rays = ss.guarded_like((5, 8), torch.float32, "cuda", name="g_rays")
        rc, grads = pair.backward("r", g_outs, g_rays.view, ws=ws.view, ws_bytes=ws.nbytes)
        assert rc == 0
        bad += [f"[{fill}] {x}" for x in ss.check_guards([ws, g_rays])]
        line = ss.unwritten("g_rays", g_rays.view)
        if line:
            bad.append(f"[{fill}] {line}")
        res[fill] = {"g_rays": g_rays.view.cpu().clone(), **{f"grad {i}": t.cpu() for i, t in enumerate(grads[0] + grads[1])}}
    for fill in (ss.ONES, ss.LEFTOVER):
        bad += ss.diff_all(f"nsr_train_backward_r {prec} [{fill} against ZERO]", res[fill], res[ss.ZERO])
    assert not bad, "\n".join(bad)
    assert float(res[ss.ZERO]["g_rays"][:, :6].abs().max()) > 0.0
