"""Unit layer between the matrix products and the gradient tensors, part 3: ``nsr::chain_weight_grads`` as a whole
(csrc/nsr_train_wgrad.hip) -- the host plan that wires twelve fp16 panel products (one launch), two head streams
(panel_wsums_kernel) and 26 second passes (one launch of finish_jobs_kernel) into the 24 gradient tensors of the default
network.  The hook takes the pointers of the ``Work`` fields the function reads; the test lays both panel sets out as the
product carves them (tests/train_reduce_gpu.py run_chain_weight_grads) and packs them with ``nsr_test_pack_panel``.

Inputs (tests/train_reduce_ref.py chain_case): twelve forward and ten gradient panels of integers in -4 .. 4, per-point scales
2^-3 .. 2^3 with ``gmax`` = each gradient panel's largest true magnitude (as run_wgrad of tests/test_gpu_gemm_units.py),
integer ``d4`` and ``bias_part``.  The exact regime is asserted (assert_chain_exact): all 24 tensors, every element, must equal
the product table's fp64 result bit for bit -- whatever the plan's split of the point groups over the workgroups.

Shapes (P, rays): (128, 2) one workgroup, one slot per product, four head slices; (160, 5) a pass that is no multiple of 128
points: three zero point groups of padding behind five; (4,128, 129) nine split-K slots' worth: 80 workgroups that start and end
inside products, 129 head slices, the heads' finish jobs on the wavefront path (more than 64 slices), 129 per-ray bias rows = two
sweeps of a wavefront plus one.  Each shape runs twice: acc = 0 over tensors filled with other integers, which it must
overwrite, then acc = 1 on other inputs over the first call's results.
"""
import numpy as np
import pytest

from tests import train_reduce_gpu as dv
from tests import train_reduce_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    return dv.load()


def check(c, got, want):
    for t in range(24):
        dv.assert_bits(got[t], want[t], f"{c.name} tensor {t} {rr.TENSOR_SHAPES[t]}")
    # the two tensors assembled from two products each, half by half
    w5, want5 = got[8].reshape(256, 319), want[8].reshape(256, 319)
    dv.assert_bits(w5[:, :63], want5[:, :63], c.name + ": layer 5, the encoded position's columns 0..62")
    dv.assert_bits(w5[:, 63:], want5[:, 63:], c.name + ": layer 5, the trunk's columns 63..318")
    wd, wantd = got[18].reshape(128, 283), want[18].reshape(128, 283)
    dv.assert_bits(wd[:, :256], wantd[:, :256], c.name + ": dir_encoding, columns 0..255")
    dv.assert_bits(wd[:, 256:], wantd[:, 256:], c.name + ": dir_encoding, the encoded direction's columns 256..282")


@pytest.mark.parametrize("P,n_rays", rr.CHAIN_SHAPES)
def test_chain_weight_grads_exact(hk, P, n_rays):
    first = rr.chain_case(P, n_rays, 0)
    rr.assert_chain_exact(first)
    want = rr.chain_weight_grads(first)
    got = dv.run_chain_weight_grads(hk, first)
    check(first, got, want)
    assert all(not np.array_equal(w, g0) for w, g0 in zip(want, first.g0))
    second = rr.chain_case(P, n_rays, 1, g0=got, seed=1)
    rr.assert_chain_exact(second)
    check(second, dv.run_chain_weight_grads(hk, second), rr.chain_weight_grads(second))


def test_wrong_references_are_told_apart(hk):
    dv.check_teeth(hk, ("chain_weight_grads",))
