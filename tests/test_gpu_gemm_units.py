"""Unit layer under the training step: the matrix kernels on their own (csrc/nsr_gemm.hip + nsr_gemm_epilogue.h,
nsr_gemm_f16.hip as a plain linear layer, nsr_wgrad_f16.hip), reached through the test-hook library (tests/hooks.py).  The
convolution gather of nsr_gemm_f16.hip -- conv_halo_kernel and the staged gather, every instantiation the dispatch can pick --
has its own unit layer built on the same method: tests/test_gpu_conv_units.py (reference and cases: tests/conv_ref.py).

Method.  The exact-input cases feed operands for which EVERY product and EVERY partial sum is exactly representable in
fp32: small integers (|a|, |b| <= 4, integer bias), for the fp16 kernels times powers of two.  The result then does not
depend on summation order, tile shape, split factor or MFMA term count and must equal the fp64 reference BIT FOR BIT; a
kernel that is off by one unit anywhere has dropped, duplicated or misplaced an element.  The condition that makes this
true -- max_ij sum_k |a_ik| |b_jk| < 2^24 in units of the smallest operand product -- bounds every partial sum in every
order; it is asserted on the reference (`_assert_exact_regime`) before anything is compared, so a later change of a shape
or a range cannot silently leave the exact regime.  These cases use torch.equal only.

The real-input cases (randn data) hold the kernels to bounds that are derived from the arithmetic, not measured; each
derivation is next to its test, and the largest observed err / bound is printed (run with -s) and recorded in DESIGN.md.

Reference everywhere: torch.float64 products on the CPU, written out here line by line.  Padding of every operand is
poisoned with NaN (a kernel that reads past an extent and uses it poisons its result), every output buffer is filled with
a sentinel first and must keep it outside the region the call owns.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import hooks
from tests.hooks import STEP_JOBS, TILES

pytestmark = pytest.mark.gpu

SENT = -3.0e38            # no exact-input result comes near it
NAN = float("nan")
U = 2.0 ** -24            # fp32 unit roundoff


@pytest.fixture(scope="module")
def hk():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    return hooks.load()


@pytest.fixture(scope="module")
def nsr():
    from nerf_sr_amd import _lib      # the PRODUCT library for the public entry points (nsr_linear_f16x3, nsr_split_weights)
    return _lib.load()


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _padded(mat, ld, fill=NAN, extra_rows=0):
    r, c = mat.shape
    buf = torch.full((r + extra_rows, ld), fill, dtype=mat.dtype)
    buf[:r, :c] = mat
    return buf


def _assert_exact_regime(a_abs, b_abs, extra=None, quantum=1.0, what=""):
    """max_ij sum_k |a_ik| |b_jk| (+ |extra_j|) < 2^24 quanta: every partial sum of the product, in any order, is an integer
    number of quanta below 2^24, hence exact in fp32."""
    worst = a_abs.double() @ b_abs.double().T
    if extra is not None:
        worst = worst + extra.double().abs()
    worst = float(worst.max()) / quantum if worst.numel() else 0.0
    assert worst < 2.0 ** 24, f"{what}: left the exact regime (max sum |a||b| = {worst:.3g} quanta)"


def _f32_exact(ref64):
    """the fp64 reference, which must be its own fp32 rounding"""
    r = ref64.float()
    assert torch.equal(r.double(), ref64), "reference is not representable in fp32: the inputs left the exact regime"
    return r


def _activate(pre, act):
    if act == hooks.ACT_RELU:
        return torch.relu(pre)
    if act == hooks.ACT_SIGMOID:
        return torch.sigmoid(pre)
    if act == hooks.ACT_TANH:
        return torch.tanh(pre)
    return pre


def reference(A, B, bias=None, act=0, mask=None, acc_scale=0.0):
    """fp64: act(acc_scale * A B^T + bias) * [mask > 0]"""
    r = A.double() @ B.double().T
    if acc_scale not in (0.0, 1.0):
        r = r * acc_scale
    if bias is not None:
        r = r + bias.double()
    r = _activate(r, act)
    if mask is not None:
        r = torch.where(mask > 0, r, torch.zeros_like(r))
    return r


def tile_col_sums(ref, n_valid):
    """(ceil(M / 128), n_valid) sums of the reference's rows 128 t .. 128 t + 127"""
    M = ref.shape[0]
    return torch.stack([ref[t:t + 128, :n_valid].sum(0) for t in range(0, M, 128)])


def run_gemm(hk, A, B, *, a_kmajor=0, b_kmajor=0, pad=True, bias=None, mask=None, act=0, n_valid=None, out="c", splits=1,
             col_sums=False, acc_scale=0.0, ldb_min=0):
    """One call of nsr::gemm on the logical operands A (M, K), B (N, K) in the requested memory orientations.  Returns the raw
    output buffers (CPU) with their sentinel-filled surroundings."""
    M, K = A.shape
    N = B.shape[0]
    n_valid = N if n_valid is None else n_valid
    p4, p1 = (4, 5) if pad else (0, 0)
    Ab = _padded(A.T.contiguous() if a_kmajor else A, (M if a_kmajor else K) + 2 * p4).cuda()
    Bb = _padded(B.T.contiguous() if b_kmajor else B, max((N if b_kmajor else K) + p4, ldb_min)).cuda()
    g = hooks.GemmArgs()
    g.A, g.lda, g.a_kmajor = hooks.ptr(Ab), Ab.shape[1], a_kmajor
    g.B, g.ldb, g.b_kmajor = hooks.ptr(Bb), Bb.shape[1], b_kmajor
    g.M, g.N, g.K, g.n_valid, g.act, g.splits, g.acc_scale = M, N, K, n_valid, act, splits, acc_scale
    keep = [Ab, Bb]
    res = {}
    ldc = N + p1
    if splits > 1:
        g.split_stride = M * ldc + 16
        Cb = torch.full((splits + 1, g.split_stride), SENT).cuda()           # one guard slice behind the last
        g.C, g.ldc = hooks.ptr(Cb), ldc
    else:
        Cb = torch.full((M + 128, ldc), SENT).cuda() if "c" in out else None  # a whole guard row tile behind row M
        g.C, g.ldc = hooks.ptr(Cb), ldc
    ldct = (M + 3) // 4 * 4 + 2 * p4
    Ctb = torch.full((N + 1, ldct), SENT).cuda() if "t" in out else None
    g.Ct, g.ldct = hooks.ptr(Ctb), ldct
    if bias is not None:
        keep.append(bias.cuda())
        g.bias = hooks.ptr(keep[-1])
    if mask is not None:
        keep.append(_padded(mask, N + 3).cuda())
        g.mask, g.ldm = hooks.ptr(keep[-1]), N + 3
    Sb = torch.full(((M + 127) // 128 + 1, N), SENT).cuda() if col_sums else None
    g.col_sums = hooks.ptr(Sb)
    rc = hk.nsr_test_gemm(ctypes.byref(g), hooks.stream())
    torch.cuda.synchronize()
    assert rc == 0, f"nsr::gemm returned {rc}"
    res["C"] = None if Cb is None else Cb.cpu()
    res["Ct"] = None if Ctb is None else Ctb.cpu()
    res["S"] = None if Sb is None else Sb.cpu()
    res["split_stride"], res["ldc"] = g.split_stride, ldc
    return res


def assert_region(buf, rows, cols, want, what):
    """buf[:rows, :cols] equals `want` bit for bit (as values) and everything else in buf still holds the sentinel"""
    got = buf[:rows, :cols]
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} elements differ; first at {bad[0].tolist()}: "
                             f"got {got[tuple(bad[0])].item()!r}, want {want[tuple(bad[0])].item()!r}; rows "
                             f"{bad[:, 0].min().item()}..{bad[:, 0].max().item()}, columns {bad[:, 1].min().item()}..{bad[:, 1].max().item()}")
    rest = buf.clone()
    rest[:rows, :cols] = SENT
    assert bool((rest == SENT).all()), f"{what}: wrote outside [0, {rows}) x [0, {cols})"


def check_outputs(res, ref32, n_valid, what, col_sums64=None):
    M = ref32.shape[0]
    if res["C"] is not None:
        assert_region(res["C"], M, n_valid, ref32[:, :n_valid], what + " C")
    if res["Ct"] is not None:
        assert_region(res["Ct"], n_valid, M, ref32[:, :n_valid].T, what + " Ct")
    if col_sums64 is not None:
        assert_region(res["S"], col_sums64.shape[0], n_valid, _f32_exact(col_sums64), what + " col_sums")


# ------------------------------------------------------------------------------------------------------------------------
# fp32-MFMA GEMM, exact inputs
# ------------------------------------------------------------------------------------------------------------------------
FWD_M = (1, 4, 127, 128, 129, 300, 4096)
FWD_N = (1, 3, 32, 36, 96, 128, 160, 256, 288, 320, 416)     # < 256: the 128-column tile; >= 256: the 256-column tile
FWD_K = (32, 64, 288, 320)
# bias, ReLU, which n_valid, outputs, acc_scale, padded leading dimensions
FWD_OPTIONS = list(itertools.product((False, True), (0, 1), ("N", "1", "N-1"), ("c", "t", "ct"), (0.0, 2.0 ** -6), (True, False)))


def _forward_case(hk, gen, M, N, K, opt):
    use_bias, act, nv, out, acc_scale, pad = opt
    n_valid = {"N": N, "1": 1, "N-1": N - 1}[nv]
    A, B = _ints(gen, (M, K), -4, 4), _ints(gen, (N, K), -4, 4)
    bias = _ints(gen, (N,), -8, 8) if use_bias else None
    _assert_exact_regime(A.abs(), B.abs(), None if bias is None else 64 * bias.abs(), what="forward")   # x 64: quantum 2^-6 under acc_scale
    ref32 = _f32_exact(reference(A, B, bias, act, None, acc_scale))
    res = run_gemm(hk, A, B, pad=pad, bias=bias, act=act, n_valid=n_valid, out=out, acc_scale=acc_scale)
    check_outputs(res, ref32, n_valid, f"forward M={M} N={N} K={K} bias={use_bias} act={act} n_valid={n_valid} out={out} "
                                       f"acc_scale={acc_scale} pad={pad}")


@pytest.mark.parametrize("M", FWD_M)
def test_gemm_forward_exact_all_shapes(hk, M):
    """Every (M, N, K) of the grid: ragged row tiles, ragged column tiles of both tile widths, 1 .. 20 K tiles.  Each shape
    runs three option sets picked by a stride that is coprime to the 144 combinations, so every value of every option meets
    every M, N and K many times; the full option product runs on the ragged shapes below."""
    gen = torch.Generator().manual_seed(100 + M)
    i = FWD_M.index(M) * 131
    for N, K in itertools.product(FWD_N, FWD_K):
        for _ in range(3):
            _forward_case(hk, gen, M, N, K, FWD_OPTIONS[(i * 35) % len(FWD_OPTIONS)])
            i += 1


@pytest.mark.parametrize("M,N,K", [(129, 36, 64), (300, 288, 320), (127, 416, 32), (4, 1, 32), (1, 160, 288)])
def test_gemm_forward_exact_all_options(hk, M, N, K):
    gen = torch.Generator().manual_seed(7 * M + N)
    for opt in FWD_OPTIONS:
        _forward_case(hk, gen, M, N, K, opt)


def test_gemm_forward_strided_coverage_is_complete():
    """the stride of test_gemm_forward_exact_all_shapes visits every option set (no GPU needed, but it documents the claim)"""
    n = len(FWD_OPTIONS)
    assert n == 144 and len({(i * 35) % n for i in range(n)}) == n


# the step's dgrad products (nsr_train_gemm.hip lin_dgrad): (K, N, ldb at least)
DGRAD_SHAPES = ((32, 128, 0), (128, 256, 288), (288, 256, 0), (256, 256, 0), (256, 64, 0))


@pytest.mark.parametrize("K,N,ldb_min", DGRAD_SHAPES)
def test_gemm_dgrad_exact(hk, K, N, ldb_min):
    """dX = (dY W) * [X > 0] with W read K-major (element (j, k) at p[k * ldb + j]); the mask has its own leading dimension and
    holds both signs and exact zeros (`mask > 0` is strict); col_sums = the per-128-row-tile column sums of what was written
    (the bias gradient) -- on a ragged last tile (M = 132, 300, 4) the clamped duplicate rows must not be summed."""
    gen = torch.Generator().manual_seed(K * 1000 + N)
    for M, use_mask, pad in itertools.product((4, 128, 132, 300), (True, False), (True, False)):
        A, B = _ints(gen, (M, K), -4, 4), _ints(gen, (N, K), -4, 4)
        mask = _ints(gen, (M, N), -2, 2) if use_mask else None
        _assert_exact_regime(A.abs(), B.abs(), what="dgrad")
        ref = reference(A, B, None, 0, mask)
        sums = tile_col_sums(ref, N)
        assert float(tile_col_sums(ref.abs(), N).max()) < 2.0 ** 24
        res = run_gemm(hk, A, B, b_kmajor=1, pad=pad, mask=mask, col_sums=True, ldb_min=ldb_min)
        check_outputs(res, _f32_exact(ref), N, f"dgrad M={M} K={K} N={N} mask={use_mask} pad={pad}", sums)
    # n_valid < N: only the valid columns are written and summed
    M, n_valid = 132, N - 4
    A, B, mask = _ints(gen, (M, K), -4, 4), _ints(gen, (N, K), -4, 4), _ints(gen, (M, N), -2, 2)
    ref = reference(A, B, None, 0, mask)
    res = run_gemm(hk, A, B, b_kmajor=1, mask=mask, col_sums=True, n_valid=n_valid, ldb_min=ldb_min)
    check_outputs(res, _f32_exact(ref), n_valid, f"dgrad n_valid M={M} K={K} N={N}", tile_col_sums(ref, n_valid))


def test_gemm_forward_col_sums_with_bias_and_relu(hk):
    """col_sums sums the values WRITTEN (after bias, activation and mask), also in the forward orientation and on the wide tile"""
    gen = torch.Generator().manual_seed(5)
    for M, N, K in ((129, 96, 64), (300, 288, 32), (4, 256, 320)):
        A, B, bias = _ints(gen, (M, K), -4, 4), _ints(gen, (N, K), -4, 4), _ints(gen, (N,), -8, 8)
        _assert_exact_regime(A.abs(), B.abs(), bias.abs(), what="forward col_sums")
        ref = reference(A, B, bias, hooks.ACT_RELU)
        res = run_gemm(hk, A, B, bias=bias, act=hooks.ACT_RELU, col_sums=True, out="ct")
        check_outputs(res, _f32_exact(ref), N, f"forward col_sums M={M} N={N} K={K}", tile_col_sums(ref, N))


WGRAD_SHAPES = ((32, 128), (128, 288), (256, 256), (256, 64), (32, 256))
WGRAD_SPLITS = (1, 2, 3, 7, 64, 256)


@pytest.mark.parametrize("M,N", WGRAD_SHAPES)
@pytest.mark.parametrize("K", (32, 480, 4096, 393216))
def test_gemm_wgrad_split_k_exact(hk, M, N, K):
    """dW = sum_p dY[p][m] X[p][n], both operands K-major, split-K: slice z holds the sum over the K range
    [z k_chunk, min((z + 1) k_chunk, K)), k_chunk = ceil((K / 32) / splits) * 32 (nsr_gemm.hip::launch); slices past the end
    of K hold zeros (the reduction reads all of them); nothing else of `partial` is touched."""
    gen = torch.Generator().manual_seed(K + M)
    A, B = _ints(gen, (M, K), -4, 4), _ints(gen, (N, K), -4, 4)
    _assert_exact_regime(A.abs(), B.abs(), what="wgrad")
    # segment sums between ALL slice boundaries of all split factors, once; a slice is a sum of whole segments (exact in fp64)
    chunk = {s: -(-(K // 32) // s) * 32 for s in WGRAD_SPLITS}
    cuts = sorted({min(z * chunk[s], K) for s in WGRAD_SPLITS for z in range(s + 1)})
    A64, B64 = A.double(), B.double()
    seg = {(c0, c1): A64[:, c0:c1] @ B64[:, c0:c1].T for c0, c1 in zip(cuts[:-1], cuts[1:])}
    Ab = _padded(A.T.contiguous(), M + 8).cuda()
    Bb = _padded(B.T.contiguous(), N + 4).cuda()
    for splits, pad in itertools.product(WGRAD_SPLITS, (5, 0)):
        ldc = N + pad
        stride = M * ldc + 16
        part = torch.full((splits + 1, stride), SENT).cuda()
        g = hooks.GemmArgs()
        g.A, g.lda, g.a_kmajor, g.B, g.ldb, g.b_kmajor = hooks.ptr(Ab), M + 8, 1, hooks.ptr(Bb), N + 4, 1
        g.C, g.ldc, g.M, g.N, g.K, g.n_valid, g.splits, g.split_stride = hooks.ptr(part), ldc, M, N, K, N, splits, stride
        rc = hk.nsr_test_gemm(ctypes.byref(g), hooks.stream())
        torch.cuda.synchronize()
        assert rc == 0
        part = part.cpu()
        for z in range(splits):
            k0, k1 = min(z * chunk[splits], K), min((z + 1) * chunk[splits], K)
            want = torch.zeros(M, N, dtype=torch.float64)
            for (c0, c1), s in seg.items():
                if k0 <= c0 and c1 <= k1:
                    want = want + s
            buf = part[z, :M * ldc].view(M, ldc)
            assert_region(buf, M, N, _f32_exact(want), f"wgrad M={M} N={N} K={K} splits={splits} slice {z} (k {k0}..{k1})")
            assert bool((part[z, M * ldc:] == SENT).all())
        assert bool((part[splits] == SENT).all()), "wrote behind the last slice"


def test_gemm_empty_batch_and_tanh_exact_zero(hk):
    """M == 0 is a success that launches nothing; tanh (act = 3, which nsr_linear does not expose) of an exact zero is zero"""
    g = hooks.GemmArgs()
    buf = torch.full((4, 64), SENT).cuda()
    g.A, g.lda, g.B, g.ldb, g.C, g.ldc = hooks.ptr(buf), 64, hooks.ptr(buf), 64, hooks.ptr(buf), 64
    g.M, g.N, g.K, g.n_valid, g.act = 0, 32, 64, 32, hooks.ACT_TANH
    assert hk.nsr_test_gemm(ctypes.byref(g), hooks.stream()) == 0
    torch.cuda.synchronize()
    assert bool((buf.cpu() == SENT).all())
    A, B = torch.zeros(5, 32), _ints(torch.Generator().manual_seed(1), (36, 32), -4, 4)
    res = run_gemm(hk, A, B, act=hooks.ACT_TANH, out="ct")
    check_outputs(res, torch.zeros(5, 36), 36, "tanh(0)")


# ------------------------------------------------------------------------------------------------------------------------
# fp32-MFMA GEMM, real inputs: derived bound
# ------------------------------------------------------------------------------------------------------------------------
def _ulp32(x):
    """ulp of the fp32 number nearest to x (x fp64)"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def derived_bound(absprod, bias, K, act, ref, eps_products=0.0):
    """|err| of act(sum_k a b + bias) computed with fp32 fused multiply-adds in ANY order: each of the K accumulations and the
    bias addition rounds once (relative error <= u = 2^-24 each, of partial sums bounded by S = sum_k |a b| + |bias|), so the
    pre-activation is off by at most ((1 + u)^(K + 1) - 1) S <= (K + 4) u S.  `eps_products` adds a relative error of the
    PRODUCTS themselves (the split-fp16 scheme's dropped lo x lo term).  The activations are 1-Lipschitz (ReLU, tanh; sigmoid
    1/4), so the error passes through them undiminished at worst; expf / tanhf and the division add at most 4 ulp of the
    result."""
    S = absprod + (bias.double().abs() if bias is not None else 0.0)
    atol = (eps_products + (K + 4) * U) * S
    if act in (hooks.ACT_SIGMOID, hooks.ACT_TANH):
        atol = atol + 4 * _ulp32(ref)
    return atol


REAL_CASES = ((300, 288, 320, hooks.ACT_NONE), (129, 36, 64, hooks.ACT_RELU), (4096, 256, 256, hooks.ACT_RELU),
              (512, 32, 128, hooks.ACT_SIGMOID), (127, 96, 288, hooks.ACT_SIGMOID), (300, 160, 64, hooks.ACT_TANH),
              (132, 416, 32, hooks.ACT_TANH), (1, 3, 32, hooks.ACT_TANH))


def test_gemm_forward_real_inputs_within_derived_bound(hk):
    gen = torch.Generator().manual_seed(11)
    worst = 0.0
    for M, N, K, act in REAL_CASES:
        A = torch.randn(M, K, generator=gen)
        B = torch.randn(N, K, generator=gen) / K ** 0.5
        bias = torch.randn(N, generator=gen)
        ref = reference(A, B, bias, act)
        res = run_gemm(hk, A, B, bias=bias, act=act, out="ct")
        # atol: derived_bound -- (K + 4) 2^-24 (sum |a b| + |bias|) through a 1-Lipschitz activation, + 4 ulp for expf / tanhf
        atol = derived_bound(A.abs().double() @ B.abs().double().T, bias, K, act, ref)
        err = (res["C"][:M, :N].double() - ref).abs()
        ratio = float((err / atol).max())
        print(f"gemm fp32 real inputs M={M} N={N} K={K} act={act}: max err {float(err.max()):.3e}, max err / bound {ratio:.4f}")
        worst = max(worst, ratio)
        assert bool((err <= atol).all()), (M, N, K, act, ratio)
        assert torch.equal(res["Ct"][:N, :M], res["C"][:M, :N].T.contiguous())
    print(f"gemm fp32 real inputs: largest err / bound {worst:.4f}")


def test_gemm_dgrad_and_wgrad_real_inputs_within_derived_bound(hk):
    """the other two orientations on randn data, same bound (no activation: the pre-activation bound alone)"""
    gen = torch.Generator().manual_seed(12)
    worst = 0.0
    for M, K, N in ((300, 256, 256), (132, 32, 128)):
        A, B = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5
        mask = torch.randn(M, N, generator=gen)
        ref = reference(A, B, None, 0, mask)
        res = run_gemm(hk, A, B, b_kmajor=1, mask=mask)
        atol = derived_bound(A.abs().double() @ B.abs().double().T, None, K, 0, ref)      # (K + 4) 2^-24 sum |a b|
        err = (res["C"][:M, :N].double() - ref).abs()
        worst = max(worst, float((err / atol).max()))
        assert bool((err <= atol).all()), (M, K, N)
    for M, N, K, splits in ((256, 256, 4096, 7), (128, 288, 480, 3)):
        A, B = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen)
        res = run_gemm(hk, A, B, a_kmajor=1, b_kmajor=1, splits=splits)
        ldc = res["ldc"]
        got = sum(res["C"][z, :M * ldc].view(M, ldc)[:, :N].double() for z in range(splits))   # the slices, summed in fp64
        ref = reference(A, B)
        atol = derived_bound(A.abs().double() @ B.abs().double().T, None, K, 0, ref)      # (K + 4) 2^-24 sum |a b|, any split
        err = (got - ref).abs()
        worst = max(worst, float((err / atol).max()))
        assert bool((err <= atol).all()), (M, N, K, splits)
    print(f"gemm fp32 dgrad / wgrad real inputs: largest err / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------------------
# split-fp16 linear
# ------------------------------------------------------------------------------------------------------------------------
def split_weights(nsr, w):
    """nsr_split_weights on a (N, K) fp32 matrix -> (hi, lo) int16 tensors padded to a row stride that is a multiple of 8"""
    hi, lo = torch.empty(w.shape, dtype=torch.int16, device="cuda"), torch.empty(w.shape, dtype=torch.int16, device="cuda")
    wd = w.contiguous().cuda()
    rc = nsr.nsr_split_weights(hooks.ptr(wd), wd.numel(), hooks.ptr(hi), hooks.ptr(lo), hooks.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return hi, lo


def run_linear_f16x3(nsr, hk, X, W, bias, act, pad, n_valid=None, col_sums=False):
    P, K = X.shape
    N = W.shape[0]
    hi, lo = split_weights(nsr, W)
    ldw = K + (8 if pad else 0)
    hib = torch.full((N, ldw), 0x7e00, dtype=torch.int16, device="cuda")      # padding: fp16 NaN
    lob = hib.clone()
    hib[:, :K], lob[:, :K] = hi, lo
    Xb = _padded(X, K + (4 if pad else 0)).cuda()
    ldy = N + (5 if pad else 0)
    Yb = torch.full((P + 128, ldy), SENT).cuda()
    bd = None if bias is None else bias.cuda()
    Sb = None
    if n_valid is None and not col_sums:      # the public entry point
        rc = nsr.nsr_linear_f16x3(hooks.ptr(Xb), Xb.shape[1], hooks.ptr(hib), hooks.ptr(lob), ldw, hooks.ptr(bd), act, hooks.ptr(Yb), ldy,
                                  P, K, N, hooks.stream())
    else:                                     # what it cannot set: n_valid, col_sums
        a = hooks.GemmF16Args()
        a.g.A, a.g.lda, a.g.C, a.g.ldc, a.g.bias = hooks.ptr(Xb), Xb.shape[1], hooks.ptr(Yb), ldy, hooks.ptr(bd)
        a.g.M, a.g.N, a.g.K, a.g.act, a.g.splits, a.g.acc_scale = P, N, K, act, 1, 2.0 ** -6
        a.g.n_valid = N if n_valid is None else n_valid
        Sb = torch.full(((P + 127) // 128 + 1, N), SENT).cuda() if col_sums else None
        a.g.col_sums = hooks.ptr(Sb)
        a.Bh, a.Bl, a.ldbh = hooks.ptr(hib), hooks.ptr(lob), ldw
        rc = hk.nsr_test_gemm_f16x3(ctypes.byref(a), hooks.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return {"C": Yb.cpu(), "Ct": None, "S": None if Sb is None else Sb.cpu()}


F16_P = (1, 5, 127, 128, 129, 1000)
F16_N = (1, 4, 32, 36, 128, 160, 256, 288)
F16_K = (32, 64, 96, 320)
F16_OPTIONS = list(itertools.product((False, True), (0, 1), (True, False)))      # bias, ReLU, padded leading dimensions


@pytest.mark.parametrize("P", F16_P)
def test_linear_f16x3_exact(nsr, hk, P):
    """Integer operands are exact in fp16 (hi = 64 w, lo = 0; x_hi = x, x_lo = 0), so the three-term product is the exact
    product and y = 2^-6 acc + b must equal the fp64 reference bit for bit -- every (P, N, K) of the grid, all eight option
    sets on every shape."""
    gen = torch.Generator().manual_seed(300 + P)
    for N, K in itertools.product(F16_N, F16_K):
        for use_bias, act, pad in F16_OPTIONS:
            X, W = _ints(gen, (P, K), -4, 4), _ints(gen, (N, K), -4, 4)
            bias = _ints(gen, (N,), -8, 8) if use_bias else None
            _assert_exact_regime(X.abs(), 64 * W.abs(), None if bias is None else 64 * bias.abs(), what="f16x3")   # the accumulator holds 64 w x
            ref32 = _f32_exact(reference(X, W, bias, act))
            res = run_linear_f16x3(nsr, hk, X, W, bias, act, pad)
            check_outputs(res, ref32, N, f"f16x3 P={P} N={N} K={K} bias={use_bias} act={act} pad={pad}")


@pytest.mark.parametrize("P,N,K", [(129, 36, 64), (1000, 288, 320), (5, 160, 96), (127, 256, 32)])
def test_linear_f16x3_exact_n_valid_and_col_sums(nsr, hk, P, N, K):
    """through the hook: n_valid < N and the per-row-tile column sums of the shared epilogue on the split-fp16 kernel"""
    gen = torch.Generator().manual_seed(P + N)
    for n_valid, act in itertools.product((N, 1, N - 1), (0, 1)):
        X, W, bias = _ints(gen, (P, K), -4, 4), _ints(gen, (N, K), -4, 4), _ints(gen, (N,), -8, 8)
        _assert_exact_regime(X.abs(), 64 * W.abs(), 64 * bias.abs(), what="f16x3")
        ref = reference(X, W, bias, act)
        assert float(tile_col_sums(ref.abs(), N).max()) < 2.0 ** 24
        res = run_linear_f16x3(nsr, hk, X, W, bias, act, True, n_valid=n_valid, col_sums=True)
        check_outputs(res, _f32_exact(ref), n_valid, f"f16x3 hook P={P} N={N} K={K} n_valid={n_valid} act={act}", tile_col_sums(ref, n_valid))


def test_split_weights_bit_exact(nsr):
    """hi = float16(64 w), lo = float16(64 w - hi), both round-to-nearest-even, bit for bit: magnitudes 2^-20 .. 2^3, both signs,
    zero, and the many values whose lo half is an fp16 subnormal (|lo| < 2^-14 <=> |64 w| < 2^-3 or so)."""
    gen = torch.Generator().manual_seed(21)
    e = torch.randint(-20, 3, (20000,), generator=gen).float()
    w = (1.0 + torch.rand(20000, generator=gen)) * torch.exp2(e) * (torch.randint(0, 2, (20000,), generator=gen).float() * 2 - 1)
    w = torch.cat([w, torch.zeros(8), torch.exp2(torch.arange(-20.0, 4.0)), -torch.exp2(torch.arange(-20.0, 4.0)),
                   torch.tensor([0.02, -0.05, 1.0 / 3.0, 7.999, -7.999, 2.0 ** -20 * 1.0000001])])
    hi, lo = split_weights(nsr, w.view(1, -1))
    v = w.numpy().astype(np.float32) * np.float32(64.0)                       # exact: a power of two
    want_hi = v.astype(np.float16)
    want_lo = (v - want_hi.astype(np.float32)).astype(np.float16)            # the difference is exact in fp32
    assert int((np.abs(want_lo.astype(np.float32)) < 2.0 ** -14).sum() - (want_lo == 0).sum()) > 1000, "no subnormal lo halves in the sample"
    assert np.array_equal(hi.cpu().numpy().view(np.uint16).ravel(), want_hi.view(np.uint16))
    assert np.array_equal(lo.cpu().numpy().view(np.uint16).ravel(), want_lo.view(np.uint16))


def test_linear_f16x3_real_inputs_within_derived_bound(nsr, hk):
    """include/nsr_train.h: "products exact to ~2^-21".  x = xh + xl and 64 w = wh + wl with |xl| <= 2^-11 |x| (fp16 rounding
    of a value in fp16's normal range), |wl| <= 2^-11 |64 w|; what remains after the second rounding is <= 2^-22 of the value.
    Of the four terms of (xh + xl)(wh + wl) the kernel drops xl wl (<= 2^-22 |x w|) and the two residuals contribute
    <= 2 * 2^-22 (1 + 2^-11): together < 2^-21 |x w| + (negligible); the three kept products are exact in the fp32 accumulator's
    input.  The accumulation and the bias then behave as in `derived_bound`.  |x| <= 100 keeps x inside fp16's range."""
    gen = torch.Generator().manual_seed(31)
    worst = 0.0
    for P, N, K, act in ((1000, 288, 320, 0), (129, 36, 64, 1), (127, 256, 96, 1), (5, 160, 32, 2), (1000, 128, 320, 2)):
        X = (torch.randn(P, K, generator=gen) * 3).clamp(-100, 100)
        W = torch.randn(N, K, generator=gen) / K ** 0.5
        bias = torch.randn(N, generator=gen)
        ref = reference(X, W, bias, act)
        res = run_linear_f16x3(nsr, hk, X, W, bias, act, True)
        # atol: (2^-21 + (K + 4) 2^-24) (sum |x w| + |b|), through the activation (+ 4 ulp for the sigmoid's expf / division)
        atol = derived_bound(X.abs().double() @ W.abs().double().T, bias, K, act, ref, eps_products=2.0 ** -21)
        err = (res["C"][:P, :N].double() - ref).abs()
        ratio = float((err / atol).max())
        print(f"f16x3 real inputs P={P} N={N} K={K} act={act}: max err {float(err.max()):.3e}, max err / bound {ratio:.4f}")
        worst = max(worst, ratio)
        assert bool((err <= atol).all()), (P, N, K, act, ratio)
    print(f"f16x3 real inputs: largest err / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------------------
# fp16 weight-gradient launch
# ------------------------------------------------------------------------------------------------------------------------
def pack_panel(hk, mat16, rows_tall=None, row0=0):
    """(P, rows) fp16 -> a panel in the chain kernels' unit layout (nsr_test_pack_panel).  With rows_tall the panel is rows
    [row0, row0 + rows) of a taller one whose other rows hold fp16 NaN.  Returns (buffer, address of the slice, bytes per group)."""
    P, rows = mat16.shape
    rows_tall = rows if rows_tall is None else rows_tall
    assert row0 % 32 == 0 and row0 + rows <= rows_tall
    gbytes = 64 * rows_tall
    buf = torch.full((P // 32 * gbytes // 2,), 0x7e00, dtype=torch.int16, device="cuda")
    src = mat16.contiguous().cuda()
    addr = buf.data_ptr() + 64 * row0
    rc = hk.nsr_test_pack_panel(hooks.ptr(src), rows, P, rows, addr, gbytes, hooks.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return buf, addr, gbytes


def run_wgrad(hk, shapes, P, n_wg, gen, *, amax=4, spread=3, tall=False, k=0, zero=False, row_sums=None):
    """One launch of wgrad_jobs_kernel over `shapes` = [(M, N), ...].  A's stored integers x pscale[p] (powers of two,
    2^-spread .. 2^spread) are the true gradients, *a_max_bits their largest magnitude; k: everything at 2^k times that scale.
    Returns per job (summed slots fp64, summed row sums fp64 or None, reference product, reference row sums)."""
    jobs = hooks.WgradJobs()
    jobs.n = len(shapes)
    keep, host = [], []
    for i, (M, N) in enumerate(shapes):
        A = torch.zeros(P, M) if zero else _ints(gen, (P, M), -amax, amax)
        B = _ints(gen, (P, N), -amax, amax)
        ps = torch.exp2(torch.randint(-spread, spread + 1, (P,), generator=gen).float())
        true_a = A.double() * ps.double()[:, None]
        # exact regime: in quanta of the smallest scale, max_ij sum_p |a_pi| ps_p |b_pj| < 2^24 (row sums: b = 1)
        _assert_exact_regime((A.abs() * ps[:, None]).T, B.abs().T, quantum=2.0 ** -spread, what="wgrad f16")
        assert float(true_a.abs().sum(0).max()) / 2.0 ** -spread < 2.0 ** 24
        # after the kernel's rescale (largest magnitude at 2^13 .. 2^14) the smallest non-zero element is a normal fp16 number
        top = float(true_a.abs().max())
        if top > 0:
            small = float(true_a.abs()[true_a != 0].min())
            assert small / top * 2.0 ** 13 >= 2.0 ** -14
        amax_bits = torch.tensor([top * 2.0 ** k], dtype=torch.float32).view(torch.int32).cuda()
        psd = (ps * 2.0 ** k).cuda()
        ta = pack_panel(hk, A.half().view(torch.int16), M + 64 if tall else None, 32 if tall else 0)
        tb = pack_panel(hk, B.half().view(torch.int16), N + 96 if tall else None, 64 if tall else 0)
        w = jobs.j[i].w
        w.A, w.a_gbytes, w.M, w.B, w.b_gbytes, w.N = ta[1], ta[2], M, tb[1], tb[2], N
        w.a_max_bits, w.a_pscale = hooks.ptr(amax_bits), hooks.ptr(psd)
        w.partial = ta[1]        # placeholder until the plan has handed the slots out (validated non-null)
        keep += [ta, tb, amax_bits, psd]
        host.append((true_a, B.double()))
    used = hk.nsr_test_wgrad_plan(ctypes.byref(jobs), P, n_wg)
    assert 1 <= used <= n_wg
    bufs = []
    for i, (M, N) in enumerate(shapes):
        q = jobs.j[i]
        stride = M * N + 32
        part = torch.full((q.n_slots + 2, stride), SENT).cuda()              # a guard slot on either side
        q.w.partial, q.w.split_stride = hooks.ptr(part, stride), stride
        want_rs = (i % 2 == 0) if row_sums is None else row_sums
        rs = torch.full((q.n_slots + 2, M), SENT).cuda() if want_rs else None
        q.w.row_sums = hooks.ptr(rs, M) if want_rs else None
        bufs.append((part, rs, q.n_slots, stride))
    rc = hk.nsr_test_wgrad_jobs(ctypes.byref(jobs), used, hooks.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    out = []
    for (M, N), (part, rs, n_slots, stride), (true_a, B64) in zip(shapes, bufs, host):
        part = part.cpu()
        what = f"wgrad f16 shapes={shapes} P={P} n_wg={n_wg} job {M}x{N}"
        assert n_slots >= 1
        assert bool((part[0] == SENT).all()) and bool((part[n_slots + 1] == SENT).all()), what + ": wrote a slot it does not own"
        assert bool((part[:, M * N:] == SENT).all()), what + ": wrote between two slots"
        assert bool((part[1:n_slots + 1, :M * N] != SENT).all()), what + ": left part of an owned slot unwritten"
        got = part[1:n_slots + 1, :M * N].double().sum(0).view(M, N)
        got_rs = None
        if rs is not None:
            rs = rs.cpu()
            assert bool((rs[0] == SENT).all()) and bool((rs[n_slots + 1] == SENT).all()), what + ": row sums outside the job's slots"
            got_rs = rs[1:n_slots + 1].double().sum(0)
        out.append((got, got_rs, true_a.T @ B64, true_a.sum(0), what))
    return out


def check_wgrad(out, scale=1.0):
    for got, got_rs, ref, ref_rs, what in out:
        if not torch.equal(got, ref * scale):
            bad = (got != ref * scale).nonzero()
            raise AssertionError(f"{what}: {len(bad)} of {ref.numel()} elements differ, first at {bad[0].tolist()}: "
                                 f"got {got[tuple(bad[0])].item()!r}, want {(ref * scale)[tuple(bad[0])].item()!r}; rows "
                                 f"{bad[:, 0].min().item()}..{bad[:, 0].max().item()}, columns {bad[:, 1].min().item()}..{bad[:, 1].max().item()}")
        if got_rs is not None:
            assert torch.equal(got_rs, ref_rs * scale), what + ": row sums"


@pytest.mark.parametrize("M,N", TILES)
def test_wgrad_f16_single_product_exact(hk, M, N):
    """every tile shape on its own: P from one point group to 128 of them, 1 .. 256 workgroups (n_wg = 7 and 256 exceed the
    3 or 4 point groups of P = 96 / 128: workgroups whose cost interval holds no group start write zeros into their slot)"""
    gen = torch.Generator().manual_seed(M + N)
    for P, n_wg in itertools.product((32, 96, 128, 4096), (1, 2, 7, 256)):
        check_wgrad(run_wgrad(hk, [(M, N)], P, n_wg, gen, row_sums=True))
    check_wgrad(run_wgrad(hk, [(M, N)], 128, 2, gen, tall=True, row_sums=True))     # both panels slices of taller ones
    check_wgrad(run_wgrad(hk, [(M, N)], 4096, 7, gen, tall=True))


@pytest.mark.parametrize("n_jobs", (2, 5, 12))
def test_wgrad_f16_many_products_one_launch_exact(hk, n_jobs):
    """the step's own product list (nsr_train_wgrad.hip chain_weight_grads order, mixed tile shapes) as ONE launch: a workgroup
    starts and ends in the middle of a product, slots are handed out per product; 300 workgroups for 128 point groups x 12
    products leave some without a whole group"""
    gen = torch.Generator().manual_seed(n_jobs)
    shapes = STEP_JOBS[:n_jobs]
    for P, n_wg in itertools.product((32, 96, 128, 4096), (1, 2, 7, 256)):
        check_wgrad(run_wgrad(hk, shapes, P, n_wg, gen))
    check_wgrad(run_wgrad(hk, shapes, 96, 300, gen))
    check_wgrad(run_wgrad(hk, shapes, 4096, 256, gen, tall=True))
    mixed = [TILES[(3 * i + n_jobs) % 4] for i in range(n_jobs)]
    check_wgrad(run_wgrad(hk, mixed, 128, 7, gen))
    check_wgrad(run_wgrad(hk, mixed, 4096, 255, gen))


def test_wgrad_f16_long_contraction_exact(hk):
    """P = 131,072 points with a constant per-point scale and |a|, |b| <= 2: 2 x 2 x 131,072 = 2^19 quanta at most"""
    gen = torch.Generator().manual_seed(77)
    check_wgrad(run_wgrad(hk, STEP_JOBS[:5], 131072, 256, gen, amax=2, spread=0))
    check_wgrad(run_wgrad(hk, [(256, 256)], 131072, 7, gen, amax=2, spread=0, row_sums=True))


def test_wgrad_f16_scale_invariance_and_zero_panel(hk):
    """All of the kernel's factors are powers of two: pscale and *a_max_bits times 2^k give exactly 2^k times the result
    (the same integers: the generator is re-seeded); a panel whose maximum is 0 gives exact zeros."""
    for k in (-40, 30):
        for shapes, P, n_wg in (([(256, 256)], 128, 2), (STEP_JOBS[:5], 4096, 7)):
            check_wgrad(run_wgrad(hk, shapes, P, n_wg, torch.Generator().manual_seed(9), k=k, row_sums=True), scale=2.0 ** k)
    out = run_wgrad(hk, [(128, 64), (256, 256)], 4096, 7, torch.Generator().manual_seed(10), zero=True, row_sums=True)
    for got, got_rs, ref, ref_rs, what in out:
        assert torch.equal(got, torch.zeros_like(got)) and torch.equal(got_rs, torch.zeros_like(got_rs)), what
    check_wgrad(out)
