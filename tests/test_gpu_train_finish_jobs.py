"""Unit layer between the matrix products and the gradient tensors, part 2: finish_jobs_kernel of the chain path
(csrc/nsr_train_wgrad.hip) -- all second passes of a network's gradients in ONE launch -- through the product's launcher
``nsr::finish_jobs`` and a ctypes mirror of ``FinishJob`` (tests/hooks.py, checked against the header when the library loads).
Reference and jobs: tests/train_reduce_ref.py (finish_job, finish_case), pinned by tests/test_train_reduce_cpu.py; device side:
tests/train_reduce_gpu.py.  Integer inputs: every comparison is bit for bit, on the job's WHOLE dst buffer.

Which job reaches which branch:
  kind 0   enc_rows 0 / 1 / 2 with 256 / 63 / 27 columns (identity, the encoded position's and direction's column maps; the
           panel's other columns are NaN); splits 1, 7 (tail only), 8 (no tail), 9, 21 (both); 256 x 256 = 65,536 elements: the last
           thread of the job's grid row owns the last element; 256 x 257 is refused
  kind 1   splits <= 64: the generic path, rows 1, 128, 256; splits 65 and 1,024: one wavefront per element, rows 1, 384 (fewer
           waves than the grid has) and 1,025 (the loop over 4 x gridDim.x waves takes a second turn), scale 2^-3
  kind 2   rows 1..4 at stride 4 (rows = 1 from column 3, the density head's bias), splits 1, 63, 64 (one sweep of the lanes), 65,
           5,000; rows = 5 is refused
  launch   32 mixed jobs at once, each on its own buffers; 33 and 0 jobs are refused; a refused launch writes nothing, whichever
           job is at fault
"""
import copy

import pytest

from tests import hooks
from tests import train_reduce_gpu as dv
from tests import train_reduce_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    return dv.load()


def check(hk, qs):
    for q, got in zip(qs, dv.run_finish_jobs(hk, qs)):
        dv.assert_bits(got, rr.finish_ref(q), q.name)


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_finish_jobs_each_kind_exact(hk, kind):
    qs = [q for q in rr.finish_cases() if q.kind == kind]
    assert qs
    for i in range(0, len(qs), rr.MAX_FINISH_JOBS):
        check(hk, qs[i:i + rr.MAX_FINISH_JOBS])
    for q in qs[:3] + qs[-3:]:                       # and alone: a launch of one job
        check(hk, [q])


def test_finish_jobs_thirty_two_mixed_jobs_one_launch(hk):
    """every job's output is right and, its buffer being its own with a guard behind it, no job touched another's"""
    qs = rr.mixed_jobs()
    assert len(qs) == hooks.MAX_FINISH_JOBS == rr.MAX_FINISH_JOBS
    check(hk, qs)
    check(hk, qs[::-1])


def test_finish_jobs_refuses_what_its_grid_cannot_hold(hk):
    good = rr.mixed_jobs(3)
    wide = rr.finish_case(0, 256, 256, 1, 0)
    wide.cols = 257                                  # 65,792 elements for 65,536 threads
    tall = rr.finish_case(1, 256, 1, 9, 1)
    tall.cols = 257                                  # the generic path of kind 1 counts rows x cols too
    five = rr.finish_case(2, 4, 1, 63, 0)
    five.rows = 5
    odd = copy.copy(good[0])
    odd.kind = 3
    for bad, rc in ((wide, hooks.NSR_ERR_UNSUPPORTED), (tall, hooks.NSR_ERR_UNSUPPORTED), (five, hooks.NSR_ERR_UNSUPPORTED),
                    (odd, hooks.NSR_ERR_INVALID_ARG)):
        dv.run_finish_jobs(hk, [bad], expect=rc)
        dv.run_finish_jobs(hk, good + [bad], expect=rc)          # the jobs in front of it are not run either
    dv.run_finish_jobs(hk, rr.mixed_jobs(33), expect=hooks.NSR_ERR_INVALID_ARG)
    dv.run_finish_jobs(hk, good, expect=hooks.NSR_ERR_INVALID_ARG, n=0)
    dv.run_finish_jobs(hk, good, expect=hooks.NSR_ERR_INVALID_ARG, n=-1)
    check(hk, good)                                  # the same jobs are accepted on their own


def test_wrong_references_are_told_apart(hk):
    dv.check_teeth(hk, ("finish_jobs",))
