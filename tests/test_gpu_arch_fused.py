"""The fused split-fp16 forward for non-default architectures (csrc/nsr_mlp_arch_f16.hip; ops.GenericMLP(fused=True),
default_options(arch_fused=True)): against the reference's own forward (tests/golden/arch.npz), against exact integer
arithmetic (a wrong fragment map or k permutation changes every output; a random-data tolerance could let one pass), against
the fp64 oracle with the layer-by-layer f16x3 route as the yardstick, and the bit-for-bit properties the kernel promises --
a row's output depends on that row and the weights only."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import arch_spec, make_state_dict_arch
from oracle import nerf_oracle as oc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH_CASES = {"small": ({"D": 4, "W": 128, "skips": (2,), "deg_pos": 6, "deg_dir": 2}, "llff", False),
              "odd": ({"D": 6, "W": 192, "skips": (1, 3), "deg_pos": 10, "deg_dir": 4}, "blender", True)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


def _fused_model(arch, sd_c, sd_f, **kw):
    from nerf_sr_amd.model import NeRFDownXModel, default_options
    opt = default_options(precision="f16x3", arch_fused=True, **{**arch, "skips": list(arch["skips"])}, **kw)
    return NeRFDownXModel(opt).load_networks(sd_c, sd_f)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's own forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ARCH_CASES))
def test_fixture_parity_through_the_model(ops, golden_dir, case):
    """Both cases of tests/golden/arch.npz through NeRFDownXModel with arch_fused on: the assertions and bounds of
    test_architecture_flags_run_layer_by_layer, on the fused route, without the layer-by-layer RuntimeWarning."""
    g = np.load(os.path.join(golden_dir, "arch.npz"))
    arch, tag, white = ARCH_CASES[case]
    p = np.load(os.path.join(golden_dir, f"path_{tag}.npz"))
    sd_c, sd_f = make_state_dict_arch(int(g["seed_coarse"]), **arch), make_state_dict_arch(int(g["seed_fine"]), **arch)
    ops._GENERIC_WARNED.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        m = _fused_model(arch, sd_c, sd_f, white_bkgd=white).eval()
    assert isinstance(m.netCoarse, ops.GenericMLP) and m.netCoarse.fused and m.netFine.fused and m.netCoarse.precision == "f16x3"
    assert not m.fused and len(m.netCoarse._split) == 0            # no layer-by-layer operands were made
    x = torch.from_numpy(g[f"{case}_mlp_in_256"]).cuda()
    assert float((m.netCoarse(x).cpu() - torch.from_numpy(g[f"{case}_mlp_out_256"])).abs().max()) <= 2e-5
    assert float((m.netCoarse(x[:64], sigma_only=True).cpu() - torch.from_numpy(g[f"{case}_mlp_sigma_only_64"])).abs().max()) <= 2e-5
    r = torch.from_numpy(p["rays"])[:int(g["n_rays"])].cuda()
    m.set_input({"rays": r[None]})
    m.forward()
    for k in ("coarse_comp_rgbs", "fine_comp_rgbs", "coarse_opacity", "fine_opacity"):
        assert float((getattr(m, f"out_{k}").cpu() - torch.from_numpy(g[f"{case}_{k}"])).abs().max()) <= 1e-4, k
    assert float((m.out_coarse_weights.cpu() - torch.from_numpy(g[f"{case}_coarse_weights"])).abs().max()) <= 1e-5
    assert all(torch.equal(v.cpu(), torch.from_numpy(sd_c[k])) for k, v in m.netCoarse.state_dict().items())
    assert m.netCoarse.status() == 0 and m.netFine.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact inputs
# ---------------------------------------------------------------------------------------------------------------------
def _int_state_dict(arch, seed):
    """Small-integer weights, independent draws per element (asymmetric in both indices); biases too."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for k, shape in arch_spec(**arch).items():
        lo, hi = (-2, 3) if (k.startswith("xyz_encoding_1.") or k.endswith("bias")) else (-1, 2)
        sd[k] = rng.integers(lo, hi, size=shape).astype(np.int64)
    return sd


def _int_forward(sd, x, arch):
    """The network in int64 (color_activation none).  Also returns the largest |value| any layer reads and the largest
    sum of |w| |a| of any output: the magnitudes that decide whether the split-fp16 arithmetic is exact."""
    ix, idr = 3 + 6 * arch["deg_pos"], 3 + 6 * arch["deg_dir"]
    pe, de = x[:, :ix], x[:, ix:ix + idr]
    peak = {"in": 0, "sum": 0}

    def lin(k, a):
        w = sd[k + ".weight"]
        peak["in"] = max(peak["in"], int(np.abs(a).max()))
        peak["sum"] = max(peak["sum"], int((np.abs(a) @ np.abs(w.T)).max()) + int(np.abs(sd[k + ".bias"]).max()))
        return a @ w.T + sd[k + ".bias"]
    h = pe
    for i in range(arch["D"]):
        h = np.maximum(lin(f"xyz_encoding_{i + 1}.0", np.concatenate([pe, h], 1) if (i > 0 and i in arch["skips"]) else h), 0)
    sigma, f = lin("sigma", h), lin("xyz_encoding_final", h)
    c = np.maximum(lin("dir_encoding.0", f if arch["no_dir"] else np.concatenate([f, de], 1)), 0)
    return np.concatenate([lin("rgb.0", c), sigma], 1), peak


EXACT = {"skip": ({"D": 2, "W": 64, "skips": (1,), "deg_pos": 2, "deg_dir": 1, "no_dir": False}, 3),
         "no_dir": ({"D": 3, "W": 96, "skips": (), "deg_pos": 2, "deg_dir": 1, "no_dir": True}, 1)}


@pytest.mark.parametrize("case", list(EXACT))
def test_exact_integer_inputs_bit_for_bit(ops, case):
    """Integer weights and inputs whose every partial sum is an exactly representable integer: every activation stays below
    2^15 (so its (hi, lo) fp16 split is exact), every sum of |w| |a| below 2^24 (so fp32 accumulation is exact in any order) --
    the output must then equal the int64 result in every bit, for all 65 rows (two wave tiles and a one-row tail)."""
    from types import SimpleNamespace
    arch, amp = EXACT[case]
    sd = _int_state_dict(arch, 7)
    rng = np.random.Generator(np.random.PCG64(11))
    x = rng.integers(-amp, amp + 1, size=(65, 15 + 9)).astype(np.int64)
    want, peak = _int_forward(sd, x, arch)
    assert peak["in"] < 2 ** 15 and peak["sum"] < 2 ** 24, peak          # the precondition of exactness
    assert np.abs(want).max() > 100                                        # ... and the case is not degenerate
    net = ops.GenericMLP(SimpleNamespace(color_activation="none"), precision="f16x3", fused=True, **arch)
    net.load_state_dict({k: v.astype(np.float32) for k, v in sd.items()})
    got = net(torch.from_numpy(x.astype(np.float32)).cuda()).cpu().numpy()
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))
    sig = net(torch.from_numpy(x[:, :15].astype(np.float32)).cuda(), sigma_only=True).cpu().numpy()
    assert np.array_equal(sig[:, 0], want[:, 3].astype(np.float32))
    assert net.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. sweep against fp64, the layer-by-layer f16x3 route as the yardstick
# ---------------------------------------------------------------------------------------------------------------------
SWEEP = [
    {"D": 1, "W": 32, "skips": (), "deg_pos": 0, "deg_dir": 0},
    {"D": 2, "W": 64, "skips": (1,), "deg_pos": 1, "deg_dir": 0},
    {"D": 3, "W": 100, "skips": (1, 2), "deg_pos": 4, "deg_dir": 1},
    {"D": 5, "W": 160, "skips": (2,), "deg_pos": 10, "deg_dir": 4, "no_dir": True},
    {"D": 8, "W": 256, "skips": (4,), "deg_pos": 10, "deg_dir": 4},
    {"D": 8, "W": 256, "skips": (1, 2, 3, 4, 5, 6, 7), "deg_pos": 10, "deg_dir": 4, "color_activation": "none"},
]
SWEEP_P = (1, 31, 33, 257)
_PARITY = {}


def _sweep_id(a):
    return f"D{a['D']}_W{a['W']}_s{'-'.join(map(str, a['skips'])) or 'none'}_deg{a['deg_pos']}-{a['deg_dir']}" + \
        ("_nodir" if a.get("no_dir") else "") + ("_colornone" if a.get("color_activation") == "none" else "")


@pytest.fixture(scope="module")
def parity_record():
    """profiles/arch_fused_parity.json: both routes' errors per case, written when NSR_RECORD_PROFILES is set."""
    yield _PARITY
    if os.environ.get("NSR_RECORD_PROFILES") and _PARITY:
        with open(os.path.join(REPO, "profiles", "arch_fused_parity.json"), "w") as f:
            json.dump({"reference": "oracle.nerf_oracle.mlp_forward in float64", "bound": "max(2e-5 * scale, 2 * layered error)",
                       "cases": _PARITY}, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.mark.parametrize("spec", SWEEP, ids=_sweep_id)
def test_sweep_against_fp64(ops, parity_record, spec):
    """Six architectures x P in {1, 31, 33, 257}: rows = posenc of uniform points in [-1, 1]^3.  With scale = max(1, max|oracle|)
    the fused error must be <= max(2e-5 scale, 2 x the layer-by-layer f16x3 route's error on the same inputs): the layered
    route is the yardstick, 2 covers another fp32 summation order of equally exact products, 2e-5 is the project's MLP bound."""
    from types import SimpleNamespace
    spec = dict(spec)
    colour = spec.pop("color_activation", "sigmoid")
    arch = {"no_dir": False, **spec}
    sd = make_state_dict_arch(1234 + arch["D"] * 1000 + arch["W"], **arch)
    opt = SimpleNamespace(color_activation=colour)
    fused = ops.GenericMLP(opt, precision="f16x3", fused=True, **arch).load_state_dict(sd)
    layered = ops.GenericMLP(opt, precision="f16x3", **arch).load_state_dict(sd)
    assert fused.fused and not layered.fused
    sd64 = oc.to_torch_sd(sd, torch.float64)
    rng = np.random.Generator(np.random.PCG64(5))
    pts = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(max(SWEEP_P), 3)).astype(np.float32))
    dirs = torch.from_numpy(rng.standard_normal((max(SWEEP_P), 3)).astype(np.float32))
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    rows = torch.cat([oc.posenc(pts, arch["deg_pos"]), oc.posenc(dirs, arch["deg_dir"])], 1).float().contiguous()
    want_all = oc.mlp_forward(sd64, rows.double(), color_activation=colour)
    for P in SWEEP_P:
        x = rows[:P].contiguous().cuda()
        want = want_all[:P]
        scale = max(1.0, float(want.abs().max()))
        e_fused = float((fused(x).cpu().double() - want).abs().max())
        e_layer = float((layered(x).cpu().double() - want).abs().max())
        parity_record[f"{_sweep_id({**arch, 'color_activation': colour})}_P{P}"] = {"fused": e_fused, "layered": e_layer, "scale": scale}
        print(f"{_sweep_id(arch)} P={P}: fused {e_fused:.3e} layered {e_layer:.3e} scale {scale:.3f}")
        assert e_fused <= max(2e-5 * scale, 2.0 * e_layer), (P, e_fused, e_layer, scale)
    assert fused.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4 / 5. a row's bits depend on that row and the weights only
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net_rows(ops):
    arch = {"D": 3, "W": 100, "skips": (1, 2), "deg_pos": 4, "deg_dir": 1, "no_dir": False}
    sd = make_state_dict_arch(77, **arch)
    net = ops.GenericMLP(precision="f16x3", fused=True, **arch).load_state_dict(sd)
    rng = np.random.Generator(np.random.PCG64(9))
    pts = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(257, 3)).astype(np.float32))
    rows = torch.cat([oc.posenc(pts, 4), oc.posenc(pts.flip(1), 1)], 1).float().contiguous().cuda()
    return net, rows, net(rows).clone()


def test_rows_are_independent_bit_for_bit(net_rows):
    net, rows, full = net_rows
    for i in (0, 130, 256):                                      # first, middle, last (the one-row tail tile)
        assert torch.equal(net(rows[i:i + 1].contiguous()), full[i:i + 1]), i
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).permutation(257)).cuda()
    assert torch.equal(net(rows[perm].contiguous()), full[perm])
    big = rows.repeat(5, 1)                                       # 1,285 rows in passes of 512, 512, 261
    try:
        net.POINT_CHUNK = 512
        assert torch.equal(net(big), full.repeat(5, 1))
    finally:
        del net.POINT_CHUNK
    assert net.POINT_CHUNK == 262144


def test_sigma_only_is_column_3_of_the_full_forward(net_rows):
    net, rows, full = net_rows
    for n in (257, 64, 1):
        sig = net(rows[:n].contiguous(), sigma_only=True)
        assert sig.shape == (n, 1) and torch.equal(sig[:, 0], full[:n, 3])
    narrow = rows[:, :27].contiguous()                            # the encoded position alone is enough
    assert torch.equal(net(narrow, sigma_only=True)[:, 0], full[:, 3])


# ---------------------------------------------------------------------------------------------------------------------
# 6. status
# ---------------------------------------------------------------------------------------------------------------------
def test_status_word(ops, net_rows):
    from nerf_sr_amd import _lib
    net, rows, _ = net_rows
    net(rows)
    net(rows[:33].contiguous(), sigma_only=True)
    assert net.status() == 0
    net.check()                                                  # healthy rows: nothing to raise
    bad = rows.clone()
    bad[200, 5] = float("nan")
    out = net(bad)
    assert torch.isfinite(out[:200]).all() and torch.isfinite(out[201:]).all() and not torch.isfinite(out[200]).all()
    assert net.status() == 2 | 8                                 # INPUT_RANGE | OUTPUT_NONFINITE, sticky
    with pytest.raises(_lib.NsrNumericsError) as e:
        net.check()
    assert e.value.flags == 10 and net.status() == 0             # check() cleared it
    # a weight the fp16 split cannot carry is reported at load, as VanillaMLP does under f16x3
    sd = {k: v.cpu().numpy().copy() for k, v in net.state_dict().items()}
    sd["xyz_encoding_2.0.weight"][3, 7] = 2048.0
    other = ops.GenericMLP(precision="f16x3", fused=True, **net.arch)
    with pytest.raises(_lib.NsrNumericsError) as e:
        other.load_state_dict(sd)
    assert e.value.flags == 1
    with pytest.raises(RuntimeError):
        other(rows)                                              # nothing usable is loaded
    sd["xyz_encoding_2.0.weight"][3, 7] = 1023.0
    other.load_state_dict(sd)                                    # the largest magnitudes the stream carries load fine
    assert other.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. model modes
# ---------------------------------------------------------------------------------------------------------------------
def test_model_runs_in_eval_and_train_mode(ops, golden_dir):
    arch, tag, white = ARCH_CASES["small"]
    p = np.load(os.path.join(golden_dir, f"path_{tag}.npz"))
    sd_c, sd_f = make_state_dict_arch(21, **arch), make_state_dict_arch(22, **arch)
    m = _fused_model(arch, sd_c, sd_f, white_bkgd=white)
    r = torch.from_numpy(p["rays"])[:64].cuda()
    m.eval().set_input({"rays": r[None]})
    m.forward()
    ref = oc.forward_rays(oc.to_torch_sd(sd_c, torch.float64), oc.to_torch_sd(sd_f, torch.float64), r.cpu().double(), 64, 64, white,
                          deg_pos=arch["deg_pos"], deg_dir=arch["deg_dir"])
    for k in ("coarse_comp_rgbs", "fine_comp_rgbs"):
        assert float((getattr(m, f"out_{k}").cpu().double() - ref[k]).abs().max()) <= 1e-4, k
    m.train()
    assert m.randomized
    torch.manual_seed(0)
    m.forward()
    assert m.out_fine_comp_rgbs.shape == (64, 3) and bool(torch.isfinite(m.out_fine_comp_rgbs).all())
    assert not torch.equal(m.out_fine_comp_rgbs.cpu().double(), ref["fine_comp_rgbs"])      # the sample positions were jittered
    assert m.netCoarse.status() == 0 and m.netFine.status() == 0
