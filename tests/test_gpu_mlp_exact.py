"""The default 8 x 256 network's inference kernels (mlp_fp32_kernel in csrc/nsr_mlp.hip, the split-fp16 kernel and its
instantiations in csrc/nsr_mlp_f16.hip, the single-16-bit kernel in csrc/nsr_mlp_h1.hip) on inputs whose arithmetic is
exact: every operand and every partial sum is representable in the precision under test (tests/mlp_exact_ref.py; the cases
are checked on the CPU in tests/test_mlp_exact_cpu.py), so the kernel must return the int64 / dyadic result in every bit.  A
weight column in the wrong k slot, a wrong bias row, a skip column off by one, a block without its a_hi * w_lo term or a
ragged tile that reads its neighbour changes that result; the tolerance tests of tests/test_gpu_parity.py cannot tell those
from rounding.

Ray-level entry points: the in-kernel encoding is exact only on the three un-encoded coordinates of each block (and, at the
origin, on all of them: sin 0 = 0, cos 0 = 1 exactly), so the ray cases carry zero weights on every sin / cos column; those
columns are tested bit for bit in tests/test_gpu_encoding.py, against a numpy restatement of nsr_sincos."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mlp_exact_ref as er

pytestmark = pytest.mark.gpu

P_EDGE = (1, 129)                # a lone point; one full 128-point tile and a one-row tail
COLOUR_BOUND = 2e-6              # the project's colour bound for the fp32 kernel (tests/test_gpu_parity.py); the
#                                  pre-activation is exact here at every precision, so it holds for all four


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from nerf_sr_amd import ops as _ops
    return _ops


def _net(ops, case, precision, colour="none"):
    net = ops.VanillaMLP(SimpleNamespace(color_activation=colour, no_dir=case.no_dir), precision=precision)
    return net.load_state_dict(case.state_dict())


def _diff(name, got, want):
    """None if got (float32) equals the exact result in every bit, else a line that says where it does not."""
    got = np.asarray(got)
    if got.shape == want.shape and got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32)) \
            and np.array_equal(got.astype(np.float64), want):
        return None
    if got.shape != want.shape:
        return f"{name}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got.astype(np.float64) != want)
    i = tuple(bad[0])
    return (f"{name}: {len(bad)} of {want.size} elements differ, max |d| {np.nanmax(np.abs(got.astype(np.float64) - want)):.6g}, "
            f"first at {i}: got {got[i]!r}, exact {want[i]!r}; rows {sorted(set(bad[:, 0].tolist()))[:8]} columns {sorted(set(bad[:, -1].tolist()))}")


def _dense_config(precision):
    return [cfg for cfg, d in er.FAMILY_A.items() if precision in d["precisions"]][-1]


ROW_GROUPS = [(p, f) for p in er.PRECISIONS for f in "ABC" if not (f == "C" and p in ("f16", "bf16"))]


@pytest.mark.parametrize("precision,family", ROW_GROUPS, ids=[f"{p}-{f}" for p, f in ROW_GROUPS])
def test_rows_bit_for_bit(ops, precision, family):
    """VanillaMLP on 333 rows (two 128-point tiles and a 77-row tail; one 256-point tile and a tail for the 16-bit kernel) of
    every case valid at the precision -- Family A with its no_dir networks, B per tensor, C per tensor (fp32, f16x3) --: the
    full forward and the sigma_only forward equal the exact result in every bit, the status word stays 0."""
    cases = [c for c in er.row_cases(precision) if c.family == family]
    assert cases and (family != "A" or any(c.no_dir for c in cases))
    bad = []
    for c in cases:
        want = c.forward()[0]
        net = _net(ops, c, precision)
        x = torch.from_numpy(c.rows()).cuda()
        bad.append(_diff(c.name, net(x).cpu().numpy(), want))
        bad.append(_diff(c.name + " sigma_only", net(x, sigma_only=True).cpu().numpy(), c.forward(sigma_only=True)[0]))
        if net.status() != 0:
            bad.append(f"{c.name}: status {net.status():#x}")
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("precision", er.PRECISIONS)
def test_ragged_row_counts_bit_for_bit(ops, precision):
    """The densest Family A case of the precision at P = 1 and P = 129."""
    cfg = _dense_config(precision)
    c = er.family_a(cfg, er.FAMILY_A[cfg]["seeds"][0])
    net = _net(ops, c, precision)
    rows, want = torch.from_numpy(c.rows()), c.forward()[0]
    bad = []
    for P in P_EDGE:
        x = rows[:P].contiguous().cuda()
        bad.append(_diff(f"{c.name} P={P}", net(x).cpu().numpy(), want[:P]))
        bad.append(_diff(f"{c.name} P={P} sigma_only", net(x, sigma_only=True).cpu().numpy(), want[:P, 3:4]))
    bad = [b for b in bad if b]
    assert not bad and net.status() == 0, "\n".join(bad)


@pytest.mark.parametrize("precision", er.PRECISIONS)
def test_rays_bit_for_bit(ops, precision):
    """5 rays x 64 samples (f16x3: one group of four rays plus a one-ray tail, two 32-sample windows; also 2 rays x 128
    samples): ops.render_rays at every precision, and ops.render_rays_composited(want_raw=True) -- the benchmark's kernel,
    which with raw requested evaluates every window's colour branch -- at fp32 (64 samples) and f16x3: the raw (R, N, 4)
    network output equals the exact result in every bit.  Exact columns only: see the module docstring."""
    bad = []
    for c in er.ray_cases(precision):
        want = c.forward()[0]
        R, N = c.z.shape
        net = _net(ops, c, precision)
        rays, z = torch.from_numpy(c.rays).cuda(), torch.from_numpy(c.z).cuda()
        rgbs, sigmas = ops.render_rays(net, rays, z)
        got = torch.cat([rgbs, sigmas[..., None]], -1).reshape(R * N, 4).cpu().numpy()
        bad.append(_diff(c.name + " render_rays", got, want))
        if precision == "f16x3" or (precision == "fp32" and N == 64):
            raw = ops.render_rays_composited(net, rays, z, False, want_raw=True)[4]
            bad.append(_diff(c.name + " render_rays_composited", raw.reshape(R * N, 4).cpu().numpy(), want))
        if net.status() != 0:
            bad.append(f"{c.name}: status {net.status():#x}")
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("precision", er.PRECISIONS)
def test_sigmoid_of_an_exact_pre_activation(ops, precision):
    """Family A, first seed, default colour activation -- the m = 3 configuration (pre-activations within +-110, many of
    them small) and the precision's densest one -- against the float64 sigmoid of the exact pre-activation: 2e-6, the
    project's colour bound for the fp32 kernel, at all four precisions; the density column stays exact."""
    for cfg in dict.fromkeys(("m3", _dense_config(precision))):
        c = er.family_a(cfg, er.FAMILY_A[cfg]["seeds"][0])
        want = c.forward()[0]
        with np.errstate(over="ignore"):
            colour = 1.0 / (1.0 + np.exp(-want[:, :3]))
        net = _net(ops, c, precision, colour="sigmoid")
        got = net(torch.from_numpy(c.rows()).cuda()).cpu().numpy()
        err = float(np.abs(got[:, :3].astype(np.float64) - colour).max())
        print(f"{precision} {c.name}: max |sigmoid - float64| {err:.3e}, {int((np.abs(want[:, :3]) < 10).sum())} pre-activations within +-10")
        assert err <= COLOUR_BOUND, (precision, c.name, err)
        assert _diff(c.name + " density", got[:, 3:4], want[:, 3:4]) is None and net.status() == 0


@pytest.mark.parametrize("precision", er.PRECISIONS)
def test_the_comparison_bites(ops, precision):
    """Teeth: the same Family B case packed with two adjacent columns of its dense tensor swapped, and with that tensor's
    bias shifted by one row, is still an exact case -- the device returns the exact result of the network it was given, and
    that result is not the unswapped network's: a kernel that routed those columns, or that bias row, wrongly would fail
    test_rows_bit_for_bit."""
    for tensor in ("xyz_encoding_3.0", er.SKIP, "dir_encoding.0"):
        c = er.family_b("narrow", tensor, 0)
        sd, wrong = c.state_dict(), dict(c.sd)
        w = wrong[tensor + ".weight"].copy()
        w[:, [100, 101]] = w[:, [101, 100]]
        wrong[tensor + ".weight"], wrong[tensor + ".bias"] = w, np.roll(wrong[tensor + ".bias"], 1)
        want_wrong = er.forward(wrong, c.exp, c.x, c.x_exp)[0]
        sd[tensor + ".weight"], sd[tensor + ".bias"] = w.astype(np.float32), wrong[tensor + ".bias"].astype(np.float32)
        net = ops.VanillaMLP(SimpleNamespace(color_activation="none"), precision=precision).load_state_dict(sd)
        got = net(torch.from_numpy(c.rows()).cuda()).cpu().numpy()
        assert _diff(c.name + " swapped", got, want_wrong) is None
        assert _diff(c.name, got, c.forward()[0]) is not None
