"""Loader of the test-hook library (ab/libnsr_testhooks.so = the product's objects + tests/csrc/nsr_test_hooks.hip, built by
``nerf_sr_amd.build.build_test_hooks`` / ``__graft_entry__.build()``) and ctypes mirrors of the library-internal argument
structs of csrc/nsr_gemm.h (and FinishJob of csrc/nsr_train_work.h).  The mirrors are checked against the C++ structs (``nsr_test_layout``) when the library is
loaded: a field added or moved in the header fails every test that uses the hooks instead of silently shifting arguments.

There is no fallback: without the library (and without hipcc to make it) ``load()`` raises and the tests that need it fail.
"""
from __future__ import annotations

import ctypes
import os
import shutil
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_int64, c_void_p

import torch  # noqa: F401  -- FIRST: see the load-order note in nerf_sr_amd/_lib.py::load

from nerf_sr_amd import build as nsr_build

NSR_OK, NSR_ERR_INVALID_ARG, NSR_ERR_UNSUPPORTED = 0, -1, -2
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
MAX_WGRAD_JOBS = 16
# the four tile shapes (M, N) of the fp16 weight-gradient kernel, and the order nsr_train_wgrad.hip::chain_weight_grads issues a
# pass's twelve products in
TILES = ((256, 256), (128, 256), (256, 64), (128, 64))
STEP_JOBS = [(128, 256), (128, 64), (256, 256), (256, 256), (256, 256), (256, 256), (256, 256), (256, 64), (256, 256), (256, 256),
             (256, 256), (256, 64)]


class GemmArgs(Structure):
    _fields_ = [("A", c_void_p), ("lda", c_int64), ("a_kmajor", c_int),
                ("B", c_void_p), ("ldb", c_int64), ("b_kmajor", c_int),
                ("C", c_void_p), ("ldc", c_int64), ("Ct", c_void_p), ("ldct", c_int64),
                ("bias", c_void_p), ("mask", c_void_p), ("ldm", c_int64),
                ("M", c_int64), ("N", c_int), ("K", c_int64),
                ("n_valid", c_int), ("act", c_int), ("splits", c_int), ("split_stride", c_int64),
                ("col_sums", c_void_p), ("acc_scale", c_float)]


class ConvGather(Structure):
    _fields_ = [(n, c_int) for n in ("cin", "Hs", "Ws", "Ho", "Wo", "stride", "up")]


class GemmF16Args(Structure):
    _fields_ = [("g", GemmArgs), ("Bh", c_void_p), ("Bl", c_void_p), ("ldbh", c_int64), ("conv", ConvGather),
                ("Ah", c_void_p), ("a_plane", c_int64), ("Ch", c_void_p), ("c_plane", c_int64), ("group", c_int),
                ("Mh", c_void_p), ("m_plane", c_int64), ("ldm", c_int64), ("Bs", c_void_p)]


class WgradArgs(Structure):
    _fields_ = [("A", c_void_p), ("a_gbytes", c_int64), ("M", c_int),
                ("B", c_void_p), ("b_gbytes", c_int64), ("N", c_int),
                ("a_max_bits", c_void_p), ("a_pscale", c_void_p), ("partial", c_void_p),
                ("split_stride", c_int64), ("row_sums", c_void_p)]


class WgradJob(Structure):
    _fields_ = [("w", WgradArgs), ("cost0", c_int64), ("cost", c_int), ("w_first", c_int), ("n_slots", c_int)]


class WgradJobs(Structure):
    _fields_ = [("j", WgradJob * MAX_WGRAD_JOBS), ("n", c_int), ("n_groups", c_int64), ("total_cost", c_int64),
                ("per_wg", c_int64)]


class FinishJob(Structure):      # csrc/nsr_train_work.h: one second pass of finish_jobs
    _fields_ = [("dst", c_void_p), ("partial", c_void_p), ("stride", c_int64)] + \
               [(n, c_int) for n in ("kind", "dst_ld", "dc0", "rows", "cols", "splits", "p_ld", "accumulate", "enc_rows")] + \
               [("scale", c_float)]


MAX_FINISH_JOBS = 32             # kMaxFinishJobs: 32 jobs are launched, 33 refused (tests/test_gpu_train_finish_jobs.py)
# nsr_test_layout's `which`
MIRRORS = {0: GemmArgs, 1: GemmF16Args, 2: WgradArgs, 3: WgradJob, 4: WgradJobs, 5: ConvGather, 6: FinishJob}

SIGNATURES = {
    "nsr_test_gemm": (c_int, [POINTER(GemmArgs), c_void_p]),
    "nsr_test_gemm_f16x3": (c_int, [POINTER(GemmF16Args), c_void_p]),
    "nsr_test_wgrad_plan": (c_int, [POINTER(WgradJobs), c_int64, c_int]),
    "nsr_test_wgrad_jobs": (c_int, [POINTER(WgradJobs), c_int, c_void_p]),
    "nsr_test_layout": (c_int, [c_int, POINTER(c_int64), c_int]),
    "nsr_test_pack_panel": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    # tests/csrc/nsr_test_hooks_conv.hip
    "nsr_test_gemm_f16x3_route": (c_int, [POINTER(GemmF16Args)]),
    "nsr_test_im2col": (c_int, [c_void_p, c_int, c_int64] + [c_int] * 9 + [c_void_p, c_void_p]),
    # tests/csrc/nsr_test_hooks_chain.hip
    "nsr_test_chain_bwd_pack": (c_int, [POINTER(c_void_p), c_void_p, c_int, c_int, c_void_p]),
    "nsr_test_chain_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int,
                                   c_int, c_void_p]),
    "nsr_test_chain_bwd_packed_bytes": (c_int64, []),
    "nsr_test_train_panel_bytes": (c_int64, [c_int64]),
    "nsr_test_train_sign_words": (c_int64, [c_int64]),
    # tests/csrc/nsr_test_hooks_heads.hip
    "nsr_test_composite_bwd": (c_int, [c_void_p] * 4 + [c_int64, c_int, c_int] + [c_void_p] * 7),
    "nsr_test_lr_loss": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_double, c_float, c_void_p, c_void_p, c_void_p, c_float,
                                 c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "nsr_test_loss_finish": (c_int, [c_void_p, c_int, c_double, c_float, c_void_p, c_int, c_void_p, c_float, c_float, c_void_p,
                                     c_void_p]),
    "nsr_test_sigma_noise": (c_int, [c_void_p, c_int, c_void_p, c_float, c_int64, c_void_p, c_void_p]),
    "nsr_test_gamma_points": (c_int, [c_void_p, c_int64, c_void_p]),
    # tests/csrc/nsr_test_hooks_refine_train.hip (the last argument of each but reduce_parts is the stream)
    "nsr_test_refine_col_reduce": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                                           c_void_p, POINTER(c_int), c_void_p]),
    "nsr_test_refine_reduce_parts": (c_int, [c_int64]),
    "nsr_test_refine_fin_mean": (c_int, [c_void_p, c_int, c_int, c_int64, c_float, c_void_p, c_void_p, c_void_p]),
    "nsr_test_refine_fin_var": (c_int, [c_void_p, c_int, c_int, c_int64, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "nsr_test_refine_fin_bn_bwd": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nsr_test_refine_fin_bias": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "nsr_test_refine_bn_relu": (c_int, [c_void_p] * 4 + [c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "nsr_test_refine_bn_bwd": (c_int, [c_void_p, c_void_p, c_int64] + [c_void_p] * 4 + [c_int64, c_int, c_void_p, c_void_p]),
    "nsr_test_refine_relu_bwd": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "nsr_test_refine_tanh_bwd": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "nsr_test_refine_max_idx": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "nsr_test_refine_route": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p]),
    "nsr_test_refine_col2im": (c_int, [c_void_p] + [c_int] * 10 + [c_void_p, c_int64, c_void_p]),
    "nsr_test_refine_wgrad_reduce": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "nsr_test_refine_fwd_reduce": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_int, c_int64, c_void_p, c_int64,
                                           c_void_p]),
    "nsr_test_refine_nhwc3_to_nchw": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    # tests/csrc/nsr_test_hooks_encode.hip (the last argument of each is the stream)
    "nsr_test_sincos": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "nsr_test_encode_arch": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_int, POINTER(c_void_p), c_int, c_int64, c_int,
                                     c_void_p]),
    "nsr_test_f16x3_train_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int] + [c_void_p] * 5),
    # tests/csrc/nsr_test_hooks_reduce.hip (the last argument of each but the scratch query is the stream)
    "nsr_test_place": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "nsr_test_scatter_heads": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "nsr_test_colsum": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "nsr_test_tile_sums": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p]),
    "nsr_test_reduce_place": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                      c_int64, c_void_p]),
    "nsr_test_panel_wsums": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_int, c_void_p, POINTER(c_int), c_void_p]),
    "nsr_test_finish_jobs": (c_int, [POINTER(FinishJob), c_int, c_void_p]),
    "nsr_test_chain_weight_grads": (c_int, [c_void_p] * 8 + [c_int64, c_int64, POINTER(c_void_p), c_int, c_void_p]),
    "nsr_test_chain_weight_grads_scratch": (c_int, [c_int64, POINTER(c_int64)]),
}

# nsr::GemmF16Route (csrc/nsr_gemm.h): the instantiation gemm_f16x3 launches
(ROUTE_NONE, ROUTE_HALO_TAIL, ROUTE_MULTI_S1, ROUTE_MULTI_S2, ROUTE_HALF_S1, ROUTE_HALF_GROUPED_S1, ROUTE_HALF_S2,
 ROUTE_HALF_GROUPED_S2, ROUTE_BIG82_S1, ROUTE_BIG82_GROUPED_S1, ROUTE_BIG44_S1, ROUTE_BIG44_GROUPED_S1, ROUTE_BIG82_S2,
 ROUTE_BIG82_GROUPED_S2, ROUTE_STAGED_WIDE, ROUTE_STAGED_K64_FULL, ROUTE_STAGED_K64, ROUTE_STAGED_K32_FULL, ROUTE_STAGED_K32,
 ROUTE_STAGED_F32A) = range(20)
ROUTE_NAMES = {v: k for k, v in list(globals().items()) if k.startswith("ROUTE_") and isinstance(v, int)}

_lib = None


def layout_of(lib, which):
    """[sizeof, offsetof(field 0), ...] of the C++ struct number `which` (plus trailing constants)."""
    out = (c_int64 * 32)()
    n = lib.nsr_test_layout(which, out, 32)
    assert 0 < n <= 32, (which, n)
    return list(out[:n])


def mirror_layout(cls):
    return [ctypes.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]


def load() -> ctypes.CDLL:
    """dlopen the hook library, building it first if it is missing or older than the sources and hipcc is at hand."""
    global _lib
    if _lib is not None:
        return _lib
    have_hipcc = bool(shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"))
    if nsr_build.hooks_stale() and have_hipcc:
        nsr_build.build_test_hooks(verbose=False)
    path = nsr_build.TEST_HOOKS_LIB
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found and hipcc is not available to build it: run `python -m nerf_sr_amd.build` "
                           "where hipcc is installed. The matrix-kernel unit tests have no other way to reach the kernels.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    for which, cls in MIRRORS.items():
        want, got = layout_of(lib, which), mirror_layout(cls)
        assert want[:len(got)] == got, f"ctypes mirror of {cls.__name__} does not match csrc/nsr_gemm.h: {got} vs {want}"
    assert layout_of(lib, 4)[-1] == MAX_WGRAD_JOBS
    _lib = lib
    return lib


def ptr(t, offset_elems: int = 0):
    """device (or host) address of a tensor, optionally `offset_elems` elements in; None -> null"""
    if t is None:
        return None
    return t.data_ptr() + offset_elems * t.element_size()


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)
