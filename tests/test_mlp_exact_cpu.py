"""The exact-input cases of tests/mlp_exact_ref.py are what they claim (CPU only; the kernels run them in
tests/test_gpu_mlp_exact.py): the dyadic reference agrees with the float64 oracle to the last bit, every case meets the
precondition of every precision it is run at, Family B observes the tensor it is about, no case is degenerate, and -- shown
with numpy emulations of the arithmetic, not with the kernels -- the cases can see the faults they are for."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as oc
from tests import mlp_exact_ref as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RECORD = {"preconditions": {}, "observability": {}, "family_a": {}}


@pytest.fixture(scope="module", autouse=True)
def case_record():
    """profiles/mlp_exact_cases.json: precondition peaks per precision and case, Family B observability, Family A
    non-degeneracy figures; written when NSR_RECORD_PROFILES is set."""
    yield _RECORD
    if os.environ.get("NSR_RECORD_PROFILES") and all(_RECORD.values()):
        with open(os.path.join(REPO, "profiles", "mlp_exact_cases.json"), "w") as f:
            json.dump({"source": "tests/test_mlp_exact_cpu.py", "rows": er.P_ROWS, **_RECORD}, f, indent=1, sort_keys=True)
            f.write("\n")


def _oracle(case, sigma_only=False):
    sd = oc.to_torch_sd(case.state_dict(np.float64), torch.float64)
    x = torch.from_numpy(case.rows(np.float64))
    return oc.mlp_forward(sd, x, sigma_only=sigma_only, color_activation="none").numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["A", "B", "C", "rays"])
def test_reference_equals_the_float64_oracle(family):
    """Difference exactly zero on every case, sigma_only and the no_dir networks included: two implementations that share
    no code (int64 with exponents here, torch.nn.functional.linear in float64 there)."""
    cases = [c for c in er.all_row_cases() if c.family == family] if family != "rays" else \
        list({c.name: c for p in er.PRECISIONS for c in er.ray_cases(p)}.values())
    assert cases
    assert family != "A" or any(c.no_dir for c in cases)
    for c in cases:
        want = _oracle(c)
        got = c.forward()[0]
        assert got.dtype == np.float64 and np.array_equal(got, want), c.name
        assert np.array_equal(c.forward(sigma_only=True)[0], _oracle(c, sigma_only=True)), c.name
        assert np.array_equal(c.forward(sigma_only=True)[0][:, 0], got[:, 3]), c.name
        # the float32 images the kernels get are the same numbers
        assert all(np.array_equal(v.astype(np.float64), c.state_dict(np.float64)[k]) for k, v in c.state_dict().items()), c.name
        assert np.array_equal(c.rows().astype(np.float64), c.rows(np.float64)) and np.array_equal(got.astype(np.float32).astype(np.float64), got)


def test_ray_case_rows_are_the_exact_encoding_inputs():
    """Ray cases: the rows the reference gets are o + z d and d in columns 0..2 of each block; every weight on a sin / cos
    column is zero -- except in the at-origin case, whose rows are the exact encoding of 0 (sin 0, cos 1)."""
    for p in er.PRECISIONS:
        for c in er.ray_cases(p):
            R, N = c.z.shape
            o, d = c.rays[:, None, 0:3].astype(np.float64), c.rays[:, None, 3:6].astype(np.float64)
            xyz = (o + c.z[:, :, None].astype(np.float64) * d).reshape(-1, 3)
            rows = c.rows(np.float64)
            assert np.array_equal(rows[:, 0:3], xyz) and np.array_equal(rows[:, 63:66], np.repeat(c.rays[:, 3:6], N, 0))
            f32 = c.rays[:, None, 0:3] + c.z[:, :, None] * c.rays[:, None, 3:6]      # the kernel's fp32 multiply and add
            assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64).reshape(-1, 3), xyz)
            assert np.all(np.diff(c.z, axis=1) >= 0)
            if c.name.endswith("origin"):
                x = torch.zeros(1, 3, dtype=torch.float64)
                enc = torch.cat([oc.posenc(x, 10), oc.posenc(x, 4)], 1).numpy()
                assert np.array_equal(rows, np.repeat(enc, R * N, 0))
                assert np.abs(c.sd["xyz_encoding_1.0.weight"][:, 3:]).sum() > 0
            else:
                assert not c.sd["xyz_encoding_1.0.weight"][:, 3:].any() and not c.sd["xyz_encoding_5.0.weight"][:, 3:63].any()
                assert not c.sd["dir_encoding.0.weight"][:, 259:].any() and not rows[:, 3:63].any() and not rows[:, 66:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. preconditions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", er.PRECISIONS)
def test_every_case_meets_its_preconditions(precision):
    cases = er.row_cases(precision) + list(er.ray_cases(precision))
    assert {c.family for c in cases} >= ({"A", "B", "C"} if precision in ("fp32", "f16x3") else {"A", "B"})
    rec = _RECORD["preconditions"].setdefault(precision, {})
    for c in cases:
        rep = er.precondition(c, precision)
        rec[c.name] = {k: (bool(v) if isinstance(v, (bool, np.bool_)) else v) for k, v in rep.items()}
        print(precision, c.name, rep)
        assert "failed" not in rep, (precision, c.name, rep)


def test_family_a_is_as_dense_as_the_precision_allows():
    """m: with one more nonzero per row (fp32: eight more) the precision that binds the configuration refuses the case on
    at least one of eight seeds."""
    for cfg, d in list(er.FAMILY_A.items()):
        if cfg == "m6d":
            continue                                     # the dyadic twin of m6
        name = f"probe-{cfg}"
        er.FAMILY_A[name] = dict(d, m=d["m"] + (8 if cfg == "m24" else 1))
        try:
            reps = [er.precondition(er.family_a(name, s), d["binds"]) for s in range(8)]
        finally:
            del er.FAMILY_A[name]
        print(cfg, d["binds"], [r.get("failed") for r in reps])
        assert any("failed" in r for r in reps), cfg


# ---------------------------------------------------------------------------------------------------------------------
# 3. Family B observes its tensor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(er.FAMILY_B))
def test_family_b_observability(config):
    """Over the union of the seeds of a tensor (at most four): >= 99 % of T's elements observed, every row and every column
    of T has an observed element, every bias element observed."""
    assert len(er.B_SEEDS) <= 4
    for t in er.LAYERS:
        w = b = None
        for s in er.B_SEEDS:
            ow, ob = er.observability(er.family_b(config, t, s))
            w, b = (ow, ob) if w is None else (w | ow, b | ob)
        frac = float(w.mean())
        _RECORD["observability"][f"{config}/{t}"] = {"weights": frac, "bias": float(b.mean()), "seeds": len(er.B_SEEDS)}
        print(config, t, "observed", frac, "bias", float(b.mean()))
        assert w.shape == er.family_b(config, t, 0).sd[t + ".weight"].shape
        assert frac >= 0.99 and w.any(1).all() and w.any(0).all() and b.all(), (config, t, frac)


# ---------------------------------------------------------------------------------------------------------------------
# 4. no case is degenerate
# ---------------------------------------------------------------------------------------------------------------------
def test_no_case_is_degenerate():
    for c in er.all_row_cases():
        out, tr = c.forward()
        assert all(len(np.unique(out[:, j])) > 1 for j in range(4)), c.name
        if c.family == "A":
            live = [float((tr[k]["z"] > 0).mean()) for k in er.TRUNK]
            _RECORD["family_a"][c.name] = {"max_abs_out": float(np.abs(out).max()), "live_min": min(live), "live_max": max(live)}
            assert np.abs(out).max() > 100, c.name
            assert 0.2 <= min(live) and max(live) <= 0.8, (c.name, live)
        if c.family == "C":                              # the wide tensor really needs the lo half: more than 11 bits
            assert er.sigbits(c.sd[c.tensor + ".weight"]) > 11 and er.sigbits(c.sd[c.tensor + ".bias"]) > 11
    for p in er.PRECISIONS:
        for c in er.ray_cases(p):
            out = c.forward()[0]
            assert c.name.endswith("origin") or all(len(np.unique(out[:, j])) > 1 for j in range(4)), c.name


# ---------------------------------------------------------------------------------------------------------------------
# 5. the cases see what they are for
# ---------------------------------------------------------------------------------------------------------------------
def _busiest_columns(case, key):
    """Two columns of the tensor to swap: of the elements the outputs observe (a sparse network reads only part of a
    tensor), the column with the most nonzeros, and the next one that differs from it in an observed row."""
    w = case.sd[key + ".weight"] * er.observability(case, key)[0]
    order = np.argsort(-(w != 0).sum(0), kind="stable")
    i = int(order[0])
    j = next(int(k) for k in order[1:] if not np.array_equal(w[:, k], w[:, i]))
    return i, j


def _perturbed(case, key, what):
    sd = dict(case.sd)
    if what == "swap":
        w = sd[key + ".weight"].copy()
        i, j = _busiest_columns(case, key)
        w[:, [i, j]] = w[:, [j, i]]
        sd[key + ".weight"] = w
    else:
        sd[key + ".bias"] = np.roll(sd[key + ".bias"], 1)
    return er.forward(sd, case.exp, case.x, case.x_exp)[0]


def test_a_swapped_column_or_a_shifted_bias_changes_the_expectation():
    """Family A (first seed of every configuration: every tensor), Family B (the dense tensor of every case): swapping two
    columns of one tensor, or shifting its bias by one row, changes the expected output on the first 128 rows.  (sigma.bias has one row, and a bias
    whose rows are all equal has nothing to shift.)"""
    todo = [(er.family_a(cfg, d["seeds"][0]), er.LAYERS) for cfg, d in er.FAMILY_A.items()]
    todo += [(er.family_b(cfg, t, 0), (t,)) for cfg in er.FAMILY_B for t in er.LAYERS]
    for full, keys in todo:
        case = er.Case(full.name, full.family, full.sd, full.exp, full.x[:128], full.x_exp, full.precisions, tensor=full.tensor)
        base = case.forward()[0]
        for key in keys:
            assert not np.array_equal(_perturbed(case, key, "swap"), base), (case.name, key, "swap")
            if not np.array_equal(np.roll(case.sd[key + ".bias"], 1), case.sd[key + ".bias"]):
                assert not np.array_equal(_perturbed(case, key, "bias"), base), (case.name, key, "bias")


def test_f16x3_emulation_is_exact_under_the_precondition():
    """hi*hi + hi*lo + lo*hi on 11-bit halves, folded dir_encoding, in float64: equal to the exact result on every f16x3
    case -- the precondition and the documented arithmetic agree before any kernel is asked."""
    for c in er.row_cases("f16x3"):
        assert np.array_equal(er.emulate_f16x3(c), c.forward()[0]), c.name


def test_family_c_sees_a_lost_hi_lo_term():
    """a_hi * w_lo dropped for tensor T: differs from the exact result in T's Family C case, for every T (the colour head is
    an fp32 dot product in the kernel: there the dropped term is the low half of an fp32 weight)."""
    for t in er.LAYERS:
        c = er.family_c(t)
        assert not np.array_equal(er.emulate_f16x3(c, (t, "w_lo")), c.forward()[0]), t


def test_family_a_sees_a_lost_lo_hi_term():
    """a_lo * w_hi dropped for one layer: differs in the dyadic Family A cases, for every layer of the matrix pipe -- the
    integer cases cannot see it (an integer activation below 2048 has an empty lo half)."""
    c = er.family_a("m6d", er.FAMILY_A["m6d"]["seeds"][0])
    want = c.forward()[0]
    for t in er.LAYERS[:-1]:
        assert not np.array_equal(er.emulate_f16x3(c, (t, "a_lo")), want), t
    ci = er.family_a("m6", er.FAMILY_A["m6"]["seeds"][0])
    assert np.array_equal(er.emulate_f16x3(ci, ("xyz_encoding_3.0", "a_lo")), ci.forward()[0])
