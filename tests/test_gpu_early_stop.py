"""Early ray termination in the split-fp16 render kernel (include/nsr.h "early ray termination"; csrc/nsr_mlp_f16.hip, "ERT"):
a group of 4 consecutive rays stops after a 32-sample window once every ray present has optical depth >= -ln(eps).

1. constructed rays with exact expectations: constant density 64, depths chosen per ray so that tau after each window is
   32 / 8e-3 / 5-10-15, five groups (one mixed, one ragged): the counter, the weights in front of and behind each cut, the
   groups that must not cut, the bounds, the analytic opacity;
2. fields: dense (every window but the first is cut), empty (nothing cut, everything still skipped by the empty-window
   rule, bit-identical), the benchmark's smooth field and a thick one on which the outputs do move (the counter equals
   tests/early_stop_ref.py fed with the two-call route's raw densities);
3. ``forward_rays``: only the fine pass is cut; 4. the model class, sharded render, train() mode; 5. refusals.

Bounds (derived in include/nsr.h, not measured): |d comp_rgb|, |d opacity| <= eps + 2e-6, |d depth| <= (eps + 2e-6) max z."""
from ctypes import c_float, c_int, c_int64, c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import make_state_dict
from tests import early_stop_ref as ref
from tests import hooks

pytestmark = pytest.mark.gpu

NAMES = ("comp_rgb", "depth", "opacity", "weights")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


def _rays(n):
    """n consecutive rays from the middle of the benchmark's frame (BASELINE config #2), as tests/test_gpu_empty_skip.py"""
    from nerf_sr_amd import cameras, ops
    lo = 252 * 95 + 100
    r = ops.subpixel_rays(cameras.spiral_pose(0.4), (504, 378), cameras.llff_focal(504), 2, True, 0.0, 1.0, device="cuda",
                          lr_range=(lo, lo + (n + 3) // 4)).view(-1, 8)
    return r[:n].contiguous()


def _z(ops, rays, N):
    z, _ = ops.sample_along_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8], N, False, False)
    return z.contiguous()


def _field(name, seed=99):
    if name == "smooth":
        return make_state_dict(seed, name)
    sd = make_state_dict(seed, "smooth")
    # dense: transmittance exactly 0 after one window; thick: tau grows by ~11 per 32 of 64 samples, ~5.5 per 32 of 128, so at
    # eps = 1e-4 the 128-sample launch stops after its SECOND window with a residual transmittance of ~5e-5: the case in which
    # the outputs do move (on the CPU oracle no tau of these rays is within 5e-4 of the threshold)
    sd["sigma.bias"] = np.full((1,), {"empty": -1e3, "dense": 1e3, "thick": 19.0}[name], dtype=np.float32)
    return sd


def _assert_bounds(got, want, z, eps, what=""):
    """the three bounds of include/nsr.h between a cut launch `got` and the uncut launch `want` (comp, depth, opacity, ...)"""
    b = eps + 2e-6
    zmax = z.abs().max(dim=1)[0].double()
    d_rgb = float((got[0] - want[0]).abs().max())
    d_op = float((got[2] - want[2]).abs().max())
    d_depth = (got[1].double() - want[1].double()).abs()
    print(f"{what}: |dRGB| {d_rgb:.3e} |dopacity| {d_op:.3e} max |ddepth| / (max z) {float((d_depth / zmax).max()):.3e}   bound {b:.3e}")
    assert d_rgb <= b and d_op <= b and bool((d_depth <= b * zmax).all()), what
    return d_rgb


# ------------------------------------------------------------------------------------------------ 1. constructed rays
GROUPS = ("early",) * 4 + ("thin",) * 4 + ("mid",) * 4 + ("early",) * 3 + ("thin",) + ("early",) * 2      # R = 18: A B C D E
STEP = {"early": 1 / 64, "thin": 2.0 ** -20, "mid": 5 / 2048}                                              # z_k = k * step
# windows cut per group (A, C, E; B and D never cut) -> total
EXPECT = {(128, 1e-5): ((3, 1, 3), 7), (128, 1e-3): ((3, 2, 3), 8), (64, 1e-5): ((1, 0, 1), 2), (64, 1e-3): ((1, 0, 1), 2)}


@pytest.fixture(scope="module")
def constant_net(ops):
    """all weights zero, sigma.bias = 64, three distinct colour biases: density 64 everywhere, colour constant"""
    sd = {k: np.zeros_like(v) for k, v in make_state_dict(99).items()}
    sd["sigma.bias"] = np.full((1,), 64, dtype=np.float32)
    sd["rgb.0.bias"] = np.array([-1.0, 0.25, 2.0], dtype=np.float32)
    return ops.VanillaMLP(precision="f16x3").load_state_dict(sd)


@pytest.mark.parametrize("N,eps", sorted(EXPECT))
def test_constructed_rays_cut_exactly_where_expected(ops, constant_net, N, eps):
    R = len(GROUPS)
    rays = torch.zeros(R, 8, device="cuda")
    rays[:, 5], rays[:, 7] = -1.0, 1.0
    k = torch.arange(N, dtype=torch.float32)
    z = torch.stack([k * np.float32(STEP[g]) for g in GROUPS]).cuda().contiguous()      # exact products (powers of two, 5 k)
    (cut_a, cut_c, cut_e), total = EXPECT[(N, eps)]
    thr = float(ref.threshold(eps))
    for g in GROUPS:                                    # no case is marginal: no tau within 13 % of the threshold
        for w in range(N // 32 - 1):
            assert abs(64 * STEP[g] * 32 * (w + 1) / thr - 1) > 0.13
    colour = torch.sigmoid(torch.tensor([-1.0, 0.25, 2.0], dtype=torch.float64))
    for white in (False, True):
        want = ops.render_rays_composited(constant_net, rays, z, white)
        same = ops.render_rays_composited(constant_net, rays, z, white, early_stop=0.0, want_cut_count=True)
        assert int(same[4].item()) == 0 and all(torch.equal(a, b) for a, b in zip(same[:4], want))
        got = ops.render_rays_composited(constant_net, rays, z, white, early_stop=eps, want_cut_count=True)
        assert int(got[4].item()) == total, (int(got[4].item()), total)
        # weights: in front of each group's cut bit-identical, behind it exactly 0
        for rows, cut in ((slice(0, 4), cut_a), (slice(8, 12), cut_c), (slice(16, 18), cut_e)):
            first_cut = N - 32 * cut
            assert torch.equal(got[3][rows, :first_cut], want[3][rows, :first_cut])
            assert not bool(got[3][rows, first_cut:].any())
        if cut_c == 0:
            assert all(torch.equal(a[8:12], b[8:12]) for a, b in zip(got[:4], want))
        # the groups that do not cut: thin, and three spent rays held back by a thin one
        for rows in (slice(4, 8), slice(12, 16)):
            for name, a, b in zip(NAMES, got[:4], want):
                assert torch.equal(a[rows], b[rows]), name
        _assert_bounds(got, want, z, eps, f"N {N} eps {eps:g} white {white}")
        # opacity against the analytic 1 - exp(-tau) of what was evaluated (an uncut ray ends in delta = 1e10: opacity 1),
        # within the compositor's own tolerance (tests/test_gpu_parity.py: 3e-6)
        tau = torch.full((R,), float("inf"), dtype=torch.float64)
        for rows, cut, g in ((slice(0, 4), cut_a, "early"), (slice(8, 12), cut_c, "mid"), (slice(16, 18), cut_e, "early")):
            if cut:
                tau[rows] = 64 * STEP[g] * (N - 32 * cut)
        opacity = 1 - torch.exp(-tau)
        assert float((got[2].cpu().double() - opacity).abs().max()) <= 3e-6
        rgb = colour[None, :] * opacity[:, None] + ((1 - opacity)[:, None] if white else 0)
        assert float((got[0].cpu().double() - rgb).abs().max()) <= 3e-6


# ------------------------------------------------------------------------------------------------ 2. fields
@pytest.fixture(scope="module")
def counted():
    """the launch through the test-hook library, with BOTH counters: -> (comp, depth, opacity, weights, skipped, cut)"""
    fn = hooks.load().nsr_test_f16x3_render_composite_ert
    fn.restype = c_int
    fn.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_float] + [c_void_p] * 7

    def run(net, rays, z, white, eps):
        R, N = z.shape
        outs = [torch.full(s, float("nan"), device="cuda") for s in ((R, 3), (R,), (R,), (R, N))]
        skipped, cut = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
        rc = fn(hooks.ptr(net.packed), hooks.ptr(rays), rays.shape[1], hooks.ptr(z), R, N, int(white), float(ref.threshold(eps)),
                *[hooks.ptr(o) for o in outs], hooks.ptr(skipped), hooks.ptr(cut), hooks.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return (*outs, int(skipped.item()), int(cut.item()))
    return run


@pytest.mark.parametrize("R", [1, 5, 4099])
@pytest.mark.parametrize("field", ["dense", "empty", "smooth", "thick"])
def test_fields(ops, counted, field, R):
    eps = 1e-4
    net = ops.VanillaMLP(precision="f16x3").load_state_dict(_field(field))
    rays = _rays(R)
    n_groups = (R + 3) // 4
    for N in (64, 128):
        z = _z(ops, rays, N)
        for white in (False, True):
            want = ops.render_rays_composited(net, rays, z, white)
            got = ops.render_rays_composited(net, rays, z, white, early_stop=eps, want_cut_count=True)
            count = int(got[4].item())
            hooked = counted(net, rays, z, white, eps)
            assert all(torch.equal(a, b) for a, b in zip(hooked[:4], got[:4])) and hooked[5] == count
            _assert_bounds(got, want, z, eps, f"{field} R {R} N {N} white {white}: {count} cut, {hooked[4]} skipped")
            if field == "dense":       # every window but the first of every group
                assert count == n_groups * (N // 32 - 1) and hooked[4] == 0
            elif field == "empty":     # nothing is cut, everything is still skipped, nothing moves
                assert count == 0 and hooked[4] == n_groups * (N // 32)
                assert all(torch.equal(a, b) for a, b in zip(got[:4], want))
            else:
                rgb, sig = ops.render_rays(net, rays, z)          # the two-call route's raw network output
                t = ref.truncate(rgb.cpu().numpy(), sig.cpu().numpy(), z.cpu().numpy(), eps)
                print(f"{field} R {R} N {N}: kernel {count}, emulation {t.n_cut} [{t.n_cut_lo}, {t.n_cut_hi}], {len(t.marginal)} marginal")
                # a condition on the inputs, not a tolerance: with more marginal windows the rays are badly chosen
                assert len(t.marginal) <= 4, sorted(t.marginal)
                assert t.n_cut_lo <= count <= t.n_cut_hi
                if not t.marginal:
                    assert count == t.n_cut
                # in front of each group's cut the weights are the uncut launch's, behind it exactly zero
                if not t.marginal:
                    first_cut = torch.from_numpy(32 * (t.last_window + 1)).repeat_interleave(4)[:R].cuda()
                    behind = torch.arange(N, device="cuda")[None, :] >= first_cut[:, None]
                    assert torch.equal(got[3][~behind], want[3][~behind]) and not bool(got[3][behind].any())


def test_gamma_correct_with_the_option(ops):
    """--gamma_correct: colours pow(rgb, 1 / 2.2) of a sigmoid output stay in [0, 1], the bound holds"""
    net = ops.VanillaMLP(precision="f16x3").load_state_dict(_field("smooth"))
    net.set_gamma_correct(True)
    rays = _rays(4099)
    z = _z(ops, rays, 128)
    want = ops.render_rays_composited(net, rays, z, True)
    got = ops.render_rays_composited(net, rays, z, True, early_stop=1e-4, want_cut_count=True)
    _assert_bounds(got, want, z, 1e-4, f"gamma_correct: {int(got[4].item())} cut")
    plain = ops.VanillaMLP(precision="f16x3").load_state_dict(_field("smooth"))
    assert int(got[4].item()) == int(ops.render_rays_composited(plain, rays, z, True, early_stop=1e-4, want_cut_count=True)[4].item())


# ------------------------------------------------------------------------------------------------ 3. forward_rays
@pytest.mark.parametrize("field", ["dense", "smooth"])
def test_forward_rays_cuts_the_fine_pass_only(ops, field):
    eps = 1e-4
    coarse = ops.VanillaMLP(precision="f16x3").load_state_dict(_field(field, 99))
    fine = ops.VanillaMLP(precision="f16x3").load_state_dict(_field(field, 100))
    rays = _rays(260)
    want = ops.forward_rays(coarse, fine, rays, 64, 64, True)
    flags = (coarse.status(clear=True), fine.status(clear=True))
    off = ops.forward_rays(coarse, fine, rays, 64, 64, True, early_stop=0.0)
    assert all(torch.equal(off[k], want[k]) for k in ops.OUT_KEYS)
    coarse.status(clear=True), fine.status(clear=True)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.forward_rays(coarse, fine, rays, 64, 64, True, early_stop=eps, cut_count=count)
    for k in ops.OUT_KEYS[:4]:
        assert torch.equal(got[k], want[k]), k           # the coarse pass that feeds the resampler is never cut
    # the fine depths are the resampler's, the same in both calls; their maximum is below far = 1 (NDC)
    z_bound = torch.ones(260, 1, device="cuda")
    _assert_bounds([got[k] for k in ops.OUT_KEYS[4:7]], [want[k] for k in ops.OUT_KEYS[4:7]], z_bound, eps,
                   f"forward_rays {field}: {int(count.item())} cut")
    assert bool((got["fine_weights"][want["fine_weights"] == 0] == 0).all())
    if field == "dense":
        assert int(count.item()) == 65 * 3
    now = (coarse.status(clear=True), fine.status(clear=True))
    assert now[0] & ~flags[0] == 0 and now[1] & ~flags[1] == 0
    # the coarse pass is the last one without importance samples
    count.zero_()
    alone = ops.forward_rays(coarse, None, rays, 64, 0, True, early_stop=eps, cut_count=count)
    ref_alone = ops.forward_rays(coarse, None, rays, 64, 0, True)
    _assert_bounds([alone[k] for k in ops.OUT_KEYS[:3]], [ref_alone[k] for k in ops.OUT_KEYS[:3]], z_bound, eps, "coarse alone")
    if field == "dense":
        assert int(count.item()) == 65


# ------------------------------------------------------------------------------------------------ 4. the model class
def test_model_frame_sharded_and_train_mode(ops, monkeypatch):
    from nerf_sr_amd import cameras, dist as nsr_dist
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    eps = 1e-4
    wh, s = (16, 12), 2
    c2w, f = cameras.spiral_pose(0.4), cameras.llff_focal(wh[0])
    sds = _field("dense", 99), _field("dense", 100)
    kw = dict(img_wh=wh, downscale=s, white_bkgd=False, precision="f16x3")
    plain = NeRFDownXModel(default_options(**kw)).load_networks(*sds).eval()
    model = NeRFDownXModel(default_options(early_stop=eps, **kw)).load_networks(*sds).eval()
    seen, real = [], ops.forward_rays
    monkeypatch.setattr(ops, "forward_rays", lambda *a, **k: (seen.append(k.get("early_stop")), real(*a, **k))[1])
    want = {k: v.clone() for k, v in plain.render_image(c2w, f, True).items()}
    got = {k: v.clone() for k, v in model.render_image(c2w, f, True).items()}
    hr_rays = model.out_fine_comp_rgbs_ori.clone()
    assert got["hr_rgb"].shape == (12, 16, 3) and got["lr_rgb"].shape == (48, 3)
    b = eps + 2e-6
    assert float((got["hr_rgb"] - want["hr_rgb"]).abs().max()) <= b and float((got["lr_rgb"] - want["lr_rgb"]).abs().max()) <= b
    assert float((got["lr_depth"] - want["lr_depth"]).abs().max()) <= b          # NDC depths: max z <= 1
    assert seen == [0.0, eps]                                                       # the option did reach the launch
    # two contiguous LR-pixel blocks on one device: the groups of four rays are the whole frame's, so are the bits
    parts = [model.render_image_sharded(c2w, f, True, lr_range=blk) for blk in nsr_dist.shard_bounds(48, 2)]
    assert torch.equal(torch.cat([p["lr_rgb"] for p in parts], 0), got["lr_rgb"])
    assert torch.equal(torch.cat([p["lr_depth"] for p in parts], 0), got["lr_depth"].reshape(-1))
    assert torch.equal(torch.cat([p["local"]["fine_comp_rgbs"] for p in parts], 0), hr_rays)
    assert seen == [0.0, eps, eps, eps]
    # train() mode ignores the option
    rays = _rays(64)
    outs = []
    for m in (plain, model):
        m.train()
        torch.manual_seed(7)
        outs.append({k: v.clone() for k, v in m.forward_rays(rays).items()})
        m.eval()
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in ops.OUT_KEYS)
    assert len(seen) == 4                       # the randomized forward is the staged route: no fused launch, no option
    # the option is read from `opt` at call time, like every other one: set later it takes effect or raises, never passes unnoticed
    plain.opt.early_stop = eps
    assert torch.equal(plain.render_image(c2w, f, True)["hr_rgb"], got["hr_rgb"]) and seen[-1] == eps
    plain.opt.early_stop = 1.5
    with pytest.raises(ValueError, match="0, 1"):
        plain.render_image(c2w, f, True)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_on_the_device(ops):
    rays = _rays(8)
    z128, z96 = _z(ops, rays, 128), _z(ops, rays, 96)
    sd = _field("smooth")
    f16x3 = ops.VanillaMLP(precision="f16x3").load_state_dict(sd)
    fp32 = ops.VanillaMLP(precision="fp32").load_state_dict(sd)
    none = ops.VanillaMLP(SimpleNamespace(color_activation="none"), precision="f16x3").load_state_dict(sd)
    for net, z, kw, word in ((fp32, z128, {}, "f16x3"), (f16x3, z128, {"sigma_activation": "softplus"}, "softplus"),
                             (none, z128, {}, "color_activation"), (f16x3, z96, {}, "64 or 128"),
                             (f16x3, z128, {"want_raw": True}, "want_raw")):
        with pytest.raises(ValueError, match=word):
            ops.render_rays_composited(net, rays, z, False, early_stop=1e-4, **kw)
    for nets, kw, word in (((fp32, fp32), {}, "f16x3"), ((f16x3, f16x3), {"sigma_activation": "softplus"}, "softplus"),
                           ((f16x3, none), {}, "color_activation"), ((f16x3, f16x3), {"N_importance": 32}, "64 or 128"),
                           ((f16x3, f16x3), {"early_stop": 1.0}, "0, 1")):
        with pytest.raises(ValueError, match=word):
            ops.forward_rays(*nets, rays, **{"N_coarse": 64, "N_importance": 64, "early_stop": 1e-4, **kw})
    # nothing of this left a mark, and the accepted call still runs
    out = ops.forward_rays(f16x3, f16x3, rays, 64, 64, early_stop=1e-4)
    assert bool(torch.isfinite(out["fine_comp_rgbs"]).all())
