"""d(loss)/d(rays) of the layer-by-layer training pair (nsr_train_arch_backward_r, include/nsr_train.h) behind
``train.forward_rays_train`` with rays that require grad, and d(loss)/d(c2w) through ``cameras.rays_from_pose``.

Reference: the fp64 restatement of the reference's iteration (tests/arch_util.py over oracle/nerf_oracle.py) with
``rays.requires_grad_()``, and the reference's own ``data_rays.grad`` (tests/golden/ray_grads.npz).  Bound: the project's
per-tensor gradient bound, 2e-3 of the norm, on each of the g_o (columns 0:3) and g_d (3:6) blocks.  The oracle's own fp32 run
differs from its fp64 run by 2e-6 .. 2.7e-4 on the gated cases and by 1.1e-3 .. 3.9e-3 on ``train_llff_rand`` /
``train_blender_rand``, which are therefore computed and recorded, not gated.  With NSR_RECORD_PROFILES set, the figures of
every case go to profiles/ray_grads_parity.json (a directory as the variable's value receives the file instead)."""
import ctypes
import json
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from nerf_sr_amd import _lib
from nerf_sr_amd.weights import arch_spec, make_state_dict
from oracle import nerf_oracle as oc
from tests import arch_util as au
from tests import scratch_state as ss
from tests.util import train_draws

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ("fp32", "f16x3_gemm")
BOUND = 2e-3
DEFAULT_GATED = {"llff_gamma": {"gamma_correct": True}, "blender_stopgrad": {"stop_grad": True},
                 "blender_softplus": {"sigma_activation": "softplus"}}
DEFAULT_RECORDED = {"llff_rand": {}, "blender_rand": {}}
_PARITY = {}


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import train as _tr
    yield _tr
    dst = os.environ.get("NSR_RECORD_PROFILES")
    if dst and _PARITY:
        path = os.path.join(dst if os.path.isdir(dst) else os.path.join(REPO, "profiles"), "ray_grads_parity.json")
        with open(path, "w") as f:
            json.dump({"reference": "fp64 restatement of the reference's iteration with rays.requires_grad_(); figures are "
                                    "|delta| / |g| over the g_o, g_d blocks; oracle_fp32 = the restatement's own fp32 run",
                       "bound": BOUND, "cases": _PARITY}, f, indent=1, sort_keys=True)
            f.write("\n")


# ---- the cases: (state dicts, rays, draws, arch, flags, loss) ---------------------------------------------------------------
def _case(golden_dir, name):
    if name in au.CASES:
        g = au.load_case(golden_dir, name)
        sds, arch, flags = au.state_dicts(g), g["arch"], {}
        draws = au.draws_of(g)
    else:
        g = np.load(os.path.join(golden_dir, f"train_{name}.npz"))
        sds, arch = (make_state_dict(int(g["seed_coarse"])), make_state_dict(int(g["seed_fine"]))), dict(au.DEFAULT_ARCH)
        flags = dict({**DEFAULT_GATED, **DEFAULT_RECORDED}[name])
        draws = {k: v for k, v in train_draws(g).items() if k != "noise_std" and v is not None}
    return {"sds": sds, "arch": arch, "flags": flags, "rays": np.asarray(g["rays"], np.float32), "draws": draws,
            "white_bkgd": bool(g["white_bkgd"]), "noise_std": float(g["noise_std"]), "target": np.asarray(g["target_lr"]),
            "s2": int(g["s2"]), "lam": (float(g["lambda_coarse"]), float(g["lambda_fine"])), "nc": 64, "ni": 64}


def _reference_loss(c, dtype, device):
    f = au.mse_loss_of(torch.as_tensor(c["target"]).to(device=device, dtype=dtype), c["s2"], *c["lam"])
    return lambda out: f(out)[0]


def _oracle(c, dtype=torch.float64, loss=None, rays=None, wrt_rays=True):
    """(d loss / d rays, weight gradients) of the restatement; ``loss``: out -> scalar (default: the reference's loss_tot)."""
    sd = [{k: v.clone().requires_grad_(True) for k, v in oc.to_torch_sd(s, dtype).items()} for s in c["sds"]]
    rays = torch.as_tensor(c["rays"] if rays is None else rays).to(dtype).clone().requires_grad_(True)
    draws = {k: torch.as_tensor(v).to(dtype) for k, v in c["draws"].items()}
    out = au.forward_train(sd[0], sd[1], rays, c["arch"], c["nc"], c["ni"], c["white_bkgd"], noise_std=c["noise_std"], **draws,
                           **c["flags"])
    total = (loss or _reference_loss(c, dtype, "cpu"))(out)
    total.backward()
    zero = lambda v: v.grad.detach() if v.grad is not None else torch.zeros_like(v)
    return rays.grad.detach().double().numpy(), [{k: zero(v) for k, v in s.items()} for s in sd]


def _hip(tr, c, prec, loss=None, rays=None, chunk=0, wrt_rays=True):
    """(rays.grad, weight gradients, outputs) of forward_rays_train on the device."""
    p = [{k: torch.from_numpy(np.asarray(v)).cuda().requires_grad_(True) for k, v in s.items()} for s in c["sds"]]
    r = torch.as_tensor(c["rays"] if rays is None else rays).cuda().clone().requires_grad_(wrt_rays)
    draws = {k: torch.as_tensor(v).cuda() for k, v in c["draws"].items()}
    out = tr.forward_rays_train(p[0], p[1], r, draws, N_coarse=c["nc"], N_importance=c["ni"], white_bkgd=c["white_bkgd"],
                                noise_std=c["noise_std"], precision=prec, ray_chunk=chunk, arch=c["arch"], **c["flags"])
    total = (loss or _reference_loss(c, torch.float32, "cuda"))(out)
    leaves = [p[n][k] for n in range(2) for k in p[n]]
    grads = torch.autograd.grad(total, leaves + ([r] if wrt_rays else []), allow_unused=True)
    g_rays = grads[-1] if wrt_rays else None
    return g_rays, grads[:len(leaves)], out


def _blocks(got, want):
    """|delta| / |g| of the g_o and g_d blocks (and of columns 8:11 at 11 columns)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rel = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    res = {"g_o": rel(got[:, 0:3], want[:, 0:3]), "g_d": rel(got[:, 3:6], want[:, 3:6])}
    if got.shape[1] == 11:
        res["g_v"] = rel(got[:, 8:11], want[:, 8:11])
    return res


_ORACLE = {}


def _oracle_of(golden_dir, name):
    if name not in _ORACLE:
        c = _case(golden_dir, name)
        _ORACLE[name] = (c, _oracle(c)[0])
    return _ORACLE[name]


ALL_CASES = list(au.CASES) + list(DEFAULT_GATED) + list(DEFAULT_RECORDED)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ALL_CASES)
def test_ray_gradient_vs_fp64_oracle(golden_dir, tr, name, prec):
    c, want = _oracle_of(golden_dir, name)
    g_rays, _, _ = _hip(tr, c, prec)
    got = g_rays.cpu().numpy()
    fig = _blocks(got, want)
    entry = _PARITY.setdefault(name, {})
    entry[prec] = fig
    if os.environ.get("NSR_RECORD_PROFILES") and "oracle_fp32" not in entry:
        entry["oracle_fp32"] = _blocks(_oracle(c, torch.float32)[0], want)
    print(f"ray gradient {name}-{prec}: g_o {fig['g_o']:.2e} g_d {fig['g_d']:.2e} (|g_o| {np.linalg.norm(want[:, :3]):.3e}, "
          f"|g_d| {np.linalg.norm(want[:, 3:6]):.3e}) {entry.get('oracle_fp32', '')}")
    assert got.shape == c["rays"].shape and np.isfinite(got).all()
    assert (got[:, 6:8] == 0.0).all(), "near / far get exact zeros"
    assert np.linalg.norm(want[:, :6]) > 0.0
    if name not in DEFAULT_RECORDED:
        assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND, (name, prec, fig)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ("small", "odd_dense"))
def test_ray_gradient_vs_the_reference_itself(golden_dir, tr, name, prec):
    """tests/golden/ray_grads.npz: data_rays.grad[:, :6] of the reference's own optimize_parameters (fp32) on the stored rays and
    draws of train_arch.npz."""
    ref = np.load(os.path.join(golden_dir, "ray_grads.npz"))[name].astype(np.float64)
    c = _case(golden_dir, name)
    got = _hip(tr, c, prec)[0].cpu().numpy()
    fig = _blocks(got, np.concatenate([ref, np.zeros((ref.shape[0], 2))], 1))
    print(f"ray gradient vs the reference {name}-{prec}: {fig}")
    assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND, (name, prec, fig)


def _aux_loss(R, nc, nf):
    """A loss over every output: depth, opacity and weights of both passes and the colours, with fixed coefficients."""
    gen = torch.Generator().manual_seed(17)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    co = {"coarse_depth": rnd(R), "coarse_opacity": rnd(R), "coarse_weights": rnd(R, nc), "fine_depth": rnd(R), "fine_opacity": rnd(R),
          "fine_weights": rnd(R, nf), "coarse_comp_rgbs": rnd(R, 3), "fine_comp_rgbs": rnd(R, 3)}

    def f(out):
        ref = out["fine_depth"]
        return sum((out[k] * v.to(device=ref.device, dtype=ref.dtype)).sum() for k, v in co.items()) / R
    return f


@pytest.mark.parametrize("prec", PRECISIONS)
def test_loss_over_depth_opacity_weights(golden_dir, tr, prec):
    c = _case(golden_dir, "odd")
    f = _aux_loss(c["rays"].shape[0], 64, 128)
    if "aux" not in _ORACLE:
        _ORACLE["aux"] = _oracle(c, loss=f)[0]
    fig = _blocks(_hip(tr, c, prec, loss=f)[0].cpu().numpy(), _ORACLE["aux"])
    print(f"ray gradient, loss over all eight outputs, odd-{prec}: {fig}")
    assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND, fig


def _rays11(rays8, seed=5):
    v = np.random.default_rng(seed).standard_normal((rays8.shape[0], 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([rays8, v], 1).astype(np.float32)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_eleven_wide_rays(golden_dir, tr, prec):
    """Columns 3:6 carry the point part only, columns 8:11 the direction encoding's part."""
    c = _case(golden_dir, "small")
    rays = _rays11(c["rays"])
    if "eleven" not in _ORACLE:
        _ORACLE["eleven"] = (_oracle(c, rays=rays)[0], _oracle(c)[0])
    want, want8 = _ORACLE["eleven"]
    got = _hip(tr, c, prec, rays=rays)[0].cpu().numpy()
    fig = _blocks(got, want)
    print(f"ray gradient at 11 columns, small-{prec}: {fig}")
    assert got.shape == (rays.shape[0], 11) and (got[:, 6:8] == 0.0).all()
    assert np.linalg.norm(want[:, 8:11]) > 0.0 and np.linalg.norm(want[:, 3:6] - want8[:, 3:6]) > 0.0
    assert max(fig.values()) <= BOUND, fig


def _small5(golden_dir, R=5, nc=32, ni=32):
    c = _case(golden_dir, "small")
    c.update(rays=c["rays"][:R].copy(), nc=nc, ni=ni, target=c["target"][:1], s2=1,
             draws={"u_coarse": c["draws"]["u_coarse"][:R, :nc].copy(), "u_fine": c["draws"]["u_fine"][:R, :ni].copy(),
                    "noise_coarse": c["draws"]["noise_coarse"][:R, :nc].copy(), "noise_fine": c["draws"]["noise_fine"][:R, :nc + ni].copy()})
    return c


def _sum_loss(out):
    return out["fine_comp_rgbs"].square().sum() + out["coarse_comp_rgbs"].square().sum() + out["fine_depth"].sum() \
        + out["coarse_weights"].sum() * 0.5


@pytest.mark.parametrize("prec", PRECISIONS)
def test_bit_identities(golden_dir, tr, prec):
    """R = 5 rays of 32 + 32 samples: the rows do not depend on ray_chunk (2 and 3 leave a ragged last chunk), follow a
    permutation of the batch, repeat bit for bit, and leave the weight gradients what they are without the ray gradient."""
    c = _small5(golden_dir)
    base, wg, _ = _hip(tr, c, prec, loss=_sum_loss)
    assert float(base[:, :6].abs().max()) > 0.0
    again, wg2, _ = _hip(tr, c, prec, loss=_sum_loss)
    assert torch.equal(base, again) and all(torch.equal(a, b) for a, b in zip(wg, wg2))
    for chunk in (2, 3):
        assert torch.equal(_hip(tr, c, prec, loss=_sum_loss, chunk=chunk)[0], base), chunk
    perm = np.array([3, 0, 4, 2, 1])
    cp = dict(c, rays=c["rays"][perm].copy(), draws={k: v[perm].copy() for k, v in c["draws"].items()})
    assert torch.equal(_hip(tr, cp, prec, loss=_sum_loss)[0], base[torch.from_numpy(perm).cuda()])
    _, wg0, _ = _hip(tr, c, prec, loss=_sum_loss, wrt_rays=False)      # nsr_train_arch_backward_e
    assert all(torch.equal(a, b) for a, b in zip(wg, wg0))


# ---- the C entry point itself ------------------------------------------------------------------------------------------------
def _p(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _ptrs(ts):
    return (c_void_p * len(ts))(*[_p(t) for t in ts])


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class _Pair:
    """One forward of the `_e` entry point on case ``c`` through ctypes; ``backward`` calls a backward entry on its saved state."""

    def __init__(self, tr, c, prec, rays=None, flags=0):
        self.lib = _lib.load()
        self.arch = _lib.NsrArch.from_arch(tr.normalize_arch(c["arch"]))
        self.prec = _lib.TRAIN_PRECISIONS[prec]
        self.w = [[torch.from_numpy(np.asarray(v)).cuda() for v in s.values()] for s in c["sds"]]
        self.rays = torch.as_tensor(c["rays"] if rays is None else rays).cuda().contiguous()
        self.R, self.nc, self.ni = self.rays.shape[0], c["nc"], c["ni"]
        d = [torch.as_tensor(c["draws"][k]).cuda().contiguous() for k in ("u_coarse", "u_fine", "noise_coarse", "noise_fine")]
        lead = (ctypes.byref(self.arch), 0)
        self.need_e = self.lib.nsr_train_arch_workspace_bytes_e(*lead, self.prec, self.R, self.nc, self.ni)
        self.need_r = self.lib.nsr_train_arch_workspace_bytes_r(*lead, self.prec, self.R, self.nc, self.ni)
        nsaved = self.lib.nsr_train_arch_saved_bytes_e(*lead, self.prec, self.R, self.nc, self.ni, 0)
        assert 0 < self.need_e <= self.need_r and nsaved > 0
        self.saved = torch.empty(nsaved, dtype=torch.uint8, device="cuda")
        self.ws = torch.zeros(self.need_r, dtype=torch.uint8, device="cuda")
        shapes = [(self.R, 3), (self.R,), (self.R,), (self.R, self.nc), (self.R, 3), (self.R,), (self.R,), (self.R, self.nc + self.ni)]
        self.outs = [torch.empty(s, device="cuda") for s in shapes]
        _lib.check(self.lib.nsr_train_arch_forward_e(
            *lead, _ptrs(self.w[0]), _ptrs(self.w[1]), _p(self.rays), self.rays.shape[1], self.R, self.nc, self.ni, flags, 0,
            *[_p(t) for t in d], c["noise_std"], self.prec, 0, _ptrs(self.outs), _p(self.ws), self.need_e, _p(self.saved), nsaved,
            _stream()), "nsr_train_arch_forward_e")

    def backward(self, entry, g_outs, g_rays=None, stride=None, ws=None, ws_bytes=None):
        """entry 'e' / 'r'; returns (status, weight gradients)."""
        grads = [[torch.full_like(t, 7.0) for t in n] for n in self.w]
        ws = self.ws if ws is None else ws
        head = (ctypes.byref(self.arch), 0, _ptrs(self.w[0]), _ptrs(self.w[1]), _ptrs(g_outs), _ptrs(grads[0]), _ptrs(grads[1]))
        tail = (_p(ws), ws.numel() if ws_bytes is None else ws_bytes, _p(self.saved), self.saved.numel(), _stream())
        if entry == "e":
            rc = self.lib.nsr_train_arch_backward_e(*head, *tail)
        else:
            rc = self.lib.nsr_train_arch_backward_r(*head, _p(g_rays), self.rays.shape[1] if stride is None else stride, *tail)
        torch.cuda.synchronize()
        return rc, grads


def _upstream(R, nc, nf, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen).cuda() for s in ((R, 3), (R,), (R,), (R, nc), (R, 3), (R,), (R,), (R, nf))]


@pytest.mark.parametrize("prec", PRECISIONS)
def test_null_g_rays_is_backward_e(golden_dir, tr, prec):
    """With g_rays NULL the `_r` entry is the `_e` entry (in the `_e` workspace size); with g_rays the weight gradients keep
    their bits; all-NULL upstream gradients give exact zeros."""
    c = _small5(golden_dir, R=8)
    pair = _Pair(tr, c, prec)
    g_outs = _upstream(8, 32, 64)
    rc_e, ge = pair.backward("e", g_outs)
    rc_0, g0 = pair.backward("r", g_outs, None, ws_bytes=pair.need_e)
    g_rays = torch.full((8, 8), float("nan"), device="cuda")
    rc_r, gr = pair.backward("r", g_outs, g_rays)
    assert (rc_e, rc_0, rc_r) == (0, 0, 0)
    for a, b, d in zip(ge[0] + ge[1], g0[0] + g0[1], gr[0] + gr[1]):
        assert torch.equal(a, b) and torch.equal(a, d) and not bool((a == 7.0).all())
    assert bool(torch.isfinite(g_rays).all()) and float(g_rays[:, :6].abs().max()) > 0.0 and bool((g_rays[:, 6:8] == 0).all())
    g_rays2 = torch.full((8, 8), float("nan"), device="cuda")
    assert pair.backward("r", [None] * 8, g_rays2)[0] == 0
    assert bool((g_rays2 == 0.0).all()), "all upstream gradients NULL"


def test_misuse_leaves_g_rays_untouched(golden_dir, tr):
    c = _small5(golden_dir, R=8)
    pair = _Pair(tr, c, "fp32")
    g_outs = _upstream(8, 32, 64)
    g_rays = torch.full((8, 11), 7.0, device="cuda")
    for what, kw, want in (("another stride than the forward's", {"stride": 11}, -1), ("a stride that is none", {"stride": 9}, -1),
                           ("a workspace one granule short", {"ws_bytes": pair.need_r - 256}, -4)):
        rc, grads = pair.backward("r", g_outs, g_rays, **kw)
        assert rc == want, (what, rc)
        assert bool((g_rays == 7.0).all()) and all(bool((t == 7.0).all()) for n in grads for t in n), what
    assert pair.need_r > pair.need_e
    # the chain precisions have no ray gradient: forward_rays_train refuses before anything runs, naming the precisions that do
    cd = _case(golden_dir, "llff_gamma")
    p = [{k: torch.from_numpy(v).cuda() for k, v in s.items()} for s in cd["sds"]]
    rays = torch.from_numpy(cd["rays"]).cuda().requires_grad_(True)
    for prec in ("f16x3", "f16x3_bwd2"):
        with pytest.raises(ValueError, match="fp32"):
            tr.forward_rays_train(p[0], p[1], rays, None, precision=prec)
    # ... and their saved state is refused by the entry point (default descriptor, chain precision in the header)
    out = tr.forward_rays_train(*[{k: v.clone().requires_grad_(True) for k, v in n.items()} for n in p], rays.detach(), None,
                                precision="f16x3")
    saved = out["fine_comp_rgbs"].grad_fn.state
    dflt = _lib.NsrArch.from_arch(tr.normalize_arch(au.DEFAULT_ARCH))
    w = [list(n.values()) for n in p]
    grads = [[torch.full_like(t, 7.0) for t in n] for n in w]
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")      # never looked at: the header is refused first
    g8 = torch.full((96, 8), 7.0, device="cuda")
    rc = _lib.load().nsr_train_arch_backward_r(ctypes.byref(dflt), 0, _ptrs(w[0]), _ptrs(w[1]), _ptrs([None] * 8), _ptrs(grads[0]),
                                               _ptrs(grads[1]), _p(g8), 8, _p(big), big.numel(), _p(saved), saved.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((g8 == 7.0).all())


@pytest.mark.parametrize("prec", PRECISIONS)
def test_exact_zeros(golden_dir, tr, prec):
    c = _small5(golden_dir, R=8)
    # an empty field: sigma.bias = -1e3 in both networks -> no weight anywhere, no gradient anywhere
    empty = dict(c, sds=[dict(s, **{"sigma.bias": np.full_like(s["sigma.bias"], -1e3)}) for s in c["sds"]])
    g, _, out = _hip(tr, empty, prec, loss=_sum_loss)
    assert float(out["fine_opacity"].abs().max()) == 0.0 and bool((g == 0.0).all())
    # --stop_grad with a loss on the colours only: dir_encoding's input is detached, so nothing reaches columns 8:11
    colour = lambda o: o["fine_comp_rgbs"].square().sum() + o["coarse_comp_rgbs"].square().sum()
    rays = _rays11(c["rays"])
    g, _, _ = _hip(tr, dict(c, flags={"stop_grad": True}), prec, loss=colour, rays=rays)
    assert bool((g[:, 8:11] == 0.0).all()) and bool((g[:, 6:8] == 0.0).all()) and float(g[:, :6].abs().max()) > 0.0
    g, _, _ = _hip(tr, c, prec, loss=colour, rays=rays)
    assert float(g[:, 8:11].abs().max()) > 0.0


@pytest.mark.parametrize("prec", PRECISIONS)
def test_smallest_legal_run(golden_dir, tr, prec):
    """R = 4 rays of 8 + 8 samples: 32 and 64 points per pass."""
    c = _small5(golden_dir, R=4, nc=8, ni=8)
    c.update(target=_case(golden_dir, "small")["target"][:1], s2=4)
    if "smallest" not in _ORACLE:
        _ORACLE["smallest"] = _oracle(c)[0]
    fig = _blocks(_hip(tr, c, prec)[0].cpu().numpy(), _ORACLE["smallest"])
    print(f"ray gradient, 4 rays of 8 + 8 samples, {prec}: {fig}")
    assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND, fig


# ---- the pose gradient ---------------------------------------------------------------------------------------------------
def _oracle_rays(c2w, H, W, focal, s, ndc, near, far):
    """oc.subpixel_ray_grid in c2w's dtype (its pixel grid is fp32): the same stage functions, differentiable in fp64."""
    o, d = oc.rays_from_pose(oc.ray_directions(H, W, focal).to(c2w.dtype), c2w)
    if ndc:
        o, d = oc.ndc_rays(H, W, focal, 1.0, o, d)
        near, far = 0.0, 1.0
    one = torch.ones_like(o[:, :1])
    rays = torch.cat([o, d, near * one, far * one], 1).view(H, W, 8)
    return rays.view(H // s, s, W // s, s, 8).permute(0, 2, 1, 3, 4).reshape(-1, 8)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("scene", ("llff", "blender"))
def test_pose_gradient(golden_dir, tr, scene, prec):
    """d(loss)/d(c2w) through cameras.rays_from_pose + the pair on an 8 x 6 <- 4 x 3 frame with the `small` networks, against
    the oracle's fp64 chain."""
    from nerf_sr_amd import cameras
    rg = np.load(os.path.join(golden_dir, "raygrid.npz"))
    W, H, s = 8, 6, 2
    c2w, focal = rg[f"{scene}_c2w"].astype(np.float64)[:3, :4], float(rg[f"{scene}_focal"]) * W / int(rg["W"])
    ndc, near, far = scene == "llff", 2.0, 6.0
    c = _case(golden_dir, "small")
    R = H * W
    gen = np.random.default_rng(11)
    c.update(target=gen.random((R // 4, 3)).astype(np.float32), s2=4, white_bkgd=not ndc,
             draws={k: v[:R].copy() for k, v in c["draws"].items()})
    key = ("pose", scene)
    if key not in _ORACLE:
        p64 = torch.from_numpy(c2w).clone().requires_grad_(True)
        sd = [oc.to_torch_sd(sd_, torch.float64) for sd_ in c["sds"]]
        out = au.forward_train(sd[0], sd[1], _oracle_rays(p64, H, W, focal, s, ndc, near, far), c["arch"], 64, 64, c["white_bkgd"],
                               noise_std=c["noise_std"], **{k: torch.as_tensor(v).double() for k, v in c["draws"].items()})
        _reference_loss(c, torch.float64, "cpu")(out).backward()
        _ORACLE[key] = p64.grad.numpy().copy()
    want = _ORACLE[key]
    pose = torch.from_numpy(c2w.astype(np.float32)).cuda().requires_grad_(True)
    rays = cameras.rays_from_pose(pose, H, W, focal, s, ndc, near, far)
    p = [{k: torch.from_numpy(v).cuda() for k, v in s_.items()} for s_ in c["sds"]]
    out = tr.forward_rays_train(p[0], p[1], rays, {k: torch.as_tensor(v).cuda() for k, v in c["draws"].items()},
                                white_bkgd=c["white_bkgd"], noise_std=c["noise_std"], precision=prec, arch=c["arch"])
    _reference_loss(c, torch.float32, "cuda")(out).backward()
    got = pose.grad.cpu().double().numpy()
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"pose gradient {scene}-{prec}: {rel:.2e} of |g| = {np.linalg.norm(want):.3e}")
    assert np.linalg.norm(want) > 0.0 and rel <= BOUND, (scene, prec, rel)


@pytest.mark.parametrize("scene", ("llff", "blender"))
def test_rays_from_pose_rows_are_gen_rays_rows(golden_dir, tr, scene):
    """On the device, in fp32: every row of cameras.rays_from_pose within 2.4e-7 of nsr_gen_rays' row."""
    from nerf_sr_amd import cameras, ops
    rg = np.load(os.path.join(golden_dir, "raygrid.npz"))
    W, H, s = 8, 6, 2
    c2w, focal = rg[f"{scene}_c2w"].astype(np.float32)[:3, :4], float(rg[f"{scene}_focal"]) * W / int(rg["W"])
    ndc = scene == "llff"
    rows = cameras.rays_from_pose(torch.from_numpy(c2w).cuda(), H, W, focal, s, ndc, 2.0, 6.0)
    dev_rows = ops.subpixel_rays(c2w, (W, H), focal, s, ndc, 2.0, 6.0, device="cuda").view(-1, 8)
    diff = float((rows - dev_rows).abs().max())
    print(f"rays_from_pose against nsr_gen_rays, {scene}: max |delta| {diff:.3e}")
    assert rows.shape == dev_rows.shape == (48, 8) and diff <= 2.4e-7, (scene, diff)


def test_trainer_fills_rays_grad(golden_dir, tr):
    """Trainer.forward(draws, rays=) / Trainer.backward need no new argument: rays.grad fills under a layer-by-layer precision."""
    c = _case(golden_dir, "small")
    t = tr.Trainer(*c["sds"], white_bkgd=c["white_bkgd"], downscale=2, noise_std=c["noise_std"], arch=c["arch"], precision="fp32")
    rays = torch.from_numpy(c["rays"]).cuda().requires_grad_(True)
    out = t.forward({k: torch.as_tensor(v).cuda() for k, v in c["draws"].items()}, rays=rays)
    loss = _reference_loss(c, torch.float32, "cuda")(out)
    t.backward(loss)
    want = _oracle_of(golden_dir, "small")[1]
    assert rays.grad is not None
    fig = _blocks(rays.grad.cpu().numpy(), want)
    assert fig["g_o"] <= BOUND and fig["g_d"] <= BOUND and float(t.grads[0]["sigma.weight"].abs().max()) > 0.0


# ---- the `_r` workspace is scratch, and its stated size suffices ------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_r_workspace_is_scratch(golden_dir, tr, prec):
    """The `_r` backward in a guarded workspace of exactly nsr_train_arch_workspace_bytes_r, filled with zeros, with ones and
    with what another call left: the same bits everywhere, no byte outside written (tests/scratch_state.py)."""
    c = _small5(golden_dir, R=8)
    pair = _Pair(tr, c, prec)
    g_outs = _upstream(8, 32, 64)
    res, bad = {}, []
    for fill, left in ((ss.ZERO, None), (ss.ONES, None), (ss.LEFTOVER, pair.ws.clone())):
        ws = ss.guarded(pair.need_r, fill, "cuda", leftover=left)
        _lib.check(pair.lib.nsr_train_status_reset(_p(ws.view), _stream()), "nsr_train_status_reset")
        g_rays = ss.guarded_like((8, 8), torch.float32, "cuda", name="g_rays")
        rc, grads = pair.backward("r", g_outs, g_rays.view, ws=ws.view, ws_bytes=ws.nbytes)
        assert rc == 0
        bad += [f"[{fill}] {x}" for x in ss.check_guards([ws, g_rays])]
        line = ss.unwritten("g_rays", g_rays.view)
        if line:
            bad.append(f"[{fill}] {line}")
        res[fill] = {"g_rays": g_rays.view.cpu().clone(), **{f"grad {i}": t.cpu() for i, t in enumerate(grads[0] + grads[1])}}
    for fill in (ss.ONES, ss.LEFTOVER):
        bad += ss.diff_all(f"`_r` backward {prec} [{fill} against ZERO]", res[fill], res[ss.ZERO])
    assert not bad, "\n".join(bad)
    assert float(res[ss.ZERO]["g_rays"][:, :6].abs().max()) > 0.0
