"""CPU-side checks of the test-hook library (tests/hooks.py, tests/csrc/nsr_test_hooks.hip): it compiles for gfx950, links
against the product's objects and binds; the ctypes mirrors match the C++ structs; `gemm` rejects bad arguments with the
documented statuses before it touches a device; and the work-list planner of the one-launch weight-gradient kernel
(`wgrad_jobs_plan`, host code) hands every workgroup and every partial slot out exactly as `wgrad_jobs_kernel` consumes them.
"""
import ctypes
import itertools
import subprocess

import pytest

from nerf_sr_amd import _lib, build as nsr_build
from tests import hooks

INV, UNSUP = hooks.NSR_ERR_INVALID_ARG, hooks.NSR_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    return hooks.load()          # builds with hipcc if missing / stale; raises otherwise (no skip)


def test_hook_library_builds_links_and_binds(lib):
    for name in hooks.SIGNATURES:
        assert hasattr(lib, name)
    # a second link of the product's objects: the product library's own exports are all there as well, and libnsr.so itself
    # exports none of the hooks
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    product = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in product if s.startswith("nsr_test_")]
    out = subprocess.run(["nm", "-D", "--defined-only", nsr_build.TEST_HOOKS_LIB], capture_output=True, text=True, check=True).stdout
    hooked = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(_lib.SIGNATURES) <= hooked and set(hooks.SIGNATURES) <= hooked


def test_struct_mirrors_match_the_headers(lib):
    for which, cls in hooks.MIRRORS.items():
        want = hooks.layout_of(lib, which)
        got = hooks.mirror_layout(cls)
        assert want[0] == got[0], f"sizeof({cls.__name__}): C++ {want[0]}, ctypes {got[0]}"
        assert want[1:len(got)] == got[1:], f"field offsets of {cls.__name__}: C++ {want[1:]}, ctypes {got[1:]}"
        assert len(want) - (1 if which == 4 else 0) == len(got), f"{cls.__name__}: field count differs"
    assert lib.nsr_test_layout(99, (ctypes.c_int64 * 4)(), 4) == -1


def _valid(**kw):
    """A GemmArgs that passes validation (pointers are never dereferenced: M > 0 cases below all fail before the launch)."""
    g = hooks.GemmArgs()
    g.A, g.lda, g.B, g.ldb, g.C, g.ldc = 256, 64, 256, 64, 256, 32
    g.M, g.N, g.K, g.n_valid, g.splits = 0, 32, 64, 32, 1          # M == 0: success without a launch
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_gemm_argument_checks_without_a_device(lib):
    call = lambda **kw: lib.nsr_test_gemm(ctypes.byref(_valid(**kw)), None)
    assert lib.nsr_test_gemm(None, None) == INV
    assert lib.nsr_test_gemm(ctypes.byref(hooks.GemmArgs()), None) == INV          # all null
    assert call() == 0                                                               # the base case is valid (empty batch)
    assert call(b_kmajor=1) == 0
    for K in (1, 16, 31, 33, 48, -32):
        assert call(K=K) == INV, K                                                   # K % 32, K < 0
    assert call(M=-1) == INV and call(N=0) == INV
    assert call(lda=62) == INV and call(ldb=66) == INV and call(Ct=256, ldct=6) == INV
    assert call(A=260) == INV and call(B=264) == INV and call(Ct=258, ldct=8) == INV  # 16-byte alignment
    assert call(A=None) == INV and call(B=None) == INV and call(C=None) == INV
    assert call(C=None, Ct=256, ldct=8) == 0                                         # Ct alone is enough
    assert call(n_valid=33) == INV and call(n_valid=31) == 0
    # K-major operands: the non-K extent is read four at a time
    assert call(a_kmajor=1, b_kmajor=1, M=6) == INV and call(a_kmajor=1, b_kmajor=1, M=2) == INV
    assert call(a_kmajor=1, b_kmajor=1, M=0) == INV                                  # ... so a K-major A has at least four rows
    assert call(b_kmajor=1, N=30, n_valid=30) == INV and call(b_kmajor=1, N=2, n_valid=2) == INV
    # split-K writes raw sums only
    assert call(splits=2, split_stride=1024) == 0
    for extra in ({"bias": 256}, {"mask": 256, "ldm": 32}, {"act": 1}, {"act": 3}, {"Ct": 256, "ldct": 8}, {"col_sums": 256},
                  {"C": None, "Ct": 256, "ldct": 8}):
        assert call(splits=2, split_stride=1024, **extra) == INV, extra
    # the one orientation nobody needs: validated, then refused without a launch
    assert call(a_kmajor=1, b_kmajor=0, M=4) == UNSUP


TILES, STEP_JOBS = hooks.TILES, hooks.STEP_JOBS


def plan(lib, shapes, P, n_wg):
    jobs = hooks.WgradJobs()
    jobs.n = len(shapes)
    for q, (M, N) in zip(jobs.j, shapes):
        q.w.M, q.w.N = M, N
    return jobs, lib.nsr_test_wgrad_plan(ctypes.byref(jobs), P, n_wg)


def _job_lists():
    out = [[t] for t in TILES]                                              # one job of every tile shape
    for n in range(2, 13):
        out.append(STEP_JOBS[:n])                                           # the step's own order, 2 .. 12 products
        out.append([TILES[(i * 3 + n) % 4] for i in range(n)])              # all four shapes mixed
    return out


@pytest.mark.parametrize("P", [32, 128, 4096, 393216])
def test_wgrad_plan_invariants(lib, P):
    for shapes, n_wg in itertools.product(_job_lists(), (1, 2, 7, 255, 256, 1000)):
        jobs, used = plan(lib, shapes, P, n_wg)
        tag = (P, shapes, n_wg)
        n_groups = P // 32
        assert jobs.n_groups == n_groups
        total = sum(n_groups * (M + N) for M, N in shapes)
        assert jobs.total_cost == total
        assert 1 <= used <= n_wg, tag
        assert jobs.per_wg * used >= total, tag                             # the workgroups launched cover the whole list
        assert jobs.per_wg * (used - 1) < total, tag                        # ... and none of them starts behind its end
        c = 0
        prev_last = None
        for q, (M, N) in zip(jobs.j, shapes):
            assert q.cost == M + N and q.cost0 == c, tag
            c0, c1 = c, c + n_groups * (M + N)
            c = c1
            # the workgroups whose cost interval [w per_wg, (w + 1) per_wg) meets [c0, c1): what wgrad_jobs_kernel tests
            meets = [w for w in range(max(0, c0 // jobs.per_wg - 2), min(used, c1 // jobs.per_wg + 3))
                     if w * jobs.per_wg < c1 and (w + 1) * jobs.per_wg > c0]
            assert meets == list(range(q.w_first, q.w_first + q.n_slots)), (tag, M, N)
            if prev_last is not None:
                assert q.w_first in (prev_last, prev_last + 1), tag        # consecutive jobs share at most one workgroup
            prev_last = q.w_first + q.n_slots - 1
            # every point group is swept by exactly one workgroup (the kernel's own rounding: ceil of the cost offsets)
            cover = 0
            for w in meets:
                lo, hi = w * jobs.per_wg, min((w + 1) * jobs.per_wg, total)
                a, b = max(lo, c0) - c0, min(hi, c1) - c0
                g0, g1 = -(-a // q.cost), min(-(-b // q.cost), n_groups)
                assert g0 == cover or g0 >= g1, (tag, w)
                cover = max(cover, g1)
            assert cover == n_groups, tag


def test_wgrad_plan_empty_pass(lib):
    for n_wg in (1, 7, 256):
        jobs, used = plan(lib, STEP_JOBS, 0, n_wg)
        assert used == 0 and jobs.n_groups == 0 and jobs.total_cost == 0
        assert all(q.n_slots == 0 for q in jobs.j[:12])
    jobs, used = plan(lib, STEP_JOBS, 31, 4)                                # less than one point group
    assert used == 0 and all(q.n_slots == 0 for q in jobs.j[:12])
