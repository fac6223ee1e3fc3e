"""numpy restatement of the two kernels of csrc/nsr_train_bwd_f16.hip (precision NSR_F16X3_GEMM_BWD): the (hi, lo) fp16 split at
the stated power-of-two scales, three terms per product (lo hi, hi lo, hi hi: small terms first), fp32 accumulation in steps of
16 along the contraction (one v_mfma_f32_32x32x16_f16 per term and step; the sum inside a step is taken exactly, which an fp16
product allows: 22 bits), the range rules (max -> [2^13, 2^14), clamped to 2^+-100, 0 / NaN -> 1) and the slice boundaries.

tests/test_train_bwd_f16_cpu.py checks it against the fp64 product; tests/test_gpu_train_bwd_f16_units.py uses it."""
import numpy as np

SPLIT_SCALE = 64.0       # csrc/nsr_gemm.h kSplitScale: the weights' 2^6
K_STEP = 16
MAX_SPLITS = 256         # csrc/nsr_train_work.h kMaxSplits


def range_exp(amax):
    """The exponent e of the power of two that takes |amax| into [2^13, 2^14): 13 - floor(log2(amax)), from the float's exponent
    field (a subnormal counts as 2^-127), clamped to +-100; 0 for amax = 0 or NaN."""
    a = np.float32(abs(amax))
    if not a > 0:
        return 0
    e = 13 - (int((a.view(np.uint32) >> 23) & 255) - 127)
    return max(-100, min(100, e))


def split(v):
    """fp32 array -> (hi, lo) fp16 halves as float64 arrays: hi = RNE(v), lo = RNE(v - hi) (the subtraction in fp32)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _three_terms(ah, al, bh, bl):
    """sum_k a[i][k] b[j][k] on the halves: per step of 16 the three terms in the kernel's order, each added in fp32."""
    acc = np.zeros((ah.shape[0], bh.shape[0]), np.float32)
    for k0 in range(0, ah.shape[1], K_STEP):
        s = slice(k0, k0 + K_STEP)
        for x, y in ((al, bh), (ah, bl), (ah, bh)):
            acc = (acc.astype(np.float64) + x[:, s] @ y[:, s].T).astype(np.float32)
    return acc


def dgrad(dy, w, mask=None):
    """dx (P, N) = (dy (P, K) w (K, N)) * [mask > 0]: dy scaled per row, the weights by 2^6, both removed in one multiply."""
    dy, w = np.asarray(dy, np.float32), np.asarray(w, np.float32)
    e = np.array([range_exp(np.abs(r).max()) for r in dy])
    ah, al = split(dy * np.exp2(e).astype(np.float32)[:, None])
    bh, bl = split(np.float32(SPLIT_SCALE) * w.T)
    out = _three_terms(ah, al, bh, bl) * np.exp2(-6.0 - e).astype(np.float32)[:, None]
    if mask is not None:
        out = np.where(np.asarray(mask) > 0, out, np.float32(0))
    return out.astype(np.float32)


def n_splits(P):
    return max(1, min(MAX_SPLITS, (P + 511) // 512))


def slice_len(P, splits):
    groups = (P + 31) // 32
    return (groups + splits - 1) // splits * 32


def wgrad(dy, x, splits):
    """partial (splits, M, N): slice z = sum over its points of dy[p][:, None] x[p][None, :]; dy scaled by ONE power of two."""
    dy, x = np.asarray(dy, np.float32), np.asarray(x, np.float32)
    P = dy.shape[0]
    e = range_exp(np.abs(dy).max()) if dy.size else 0
    L = slice_len(P, splits)
    out = np.zeros((splits, dy.shape[1], x.shape[1]), np.float32)
    for z in range(splits):
        lo, hi = z * L, min((z + 1) * L, P)
        if hi <= lo:
            continue
        n = (hi - lo + 31) // 32 * 32                    # points past the slice: zeros in both operands
        a = np.zeros((n, dy.shape[1]), np.float32)
        b = np.zeros((n, x.shape[1]), np.float32)
        a[:hi - lo], b[:hi - lo] = dy[lo:hi] * np.float32(2.0 ** e), x[lo:hi]
        ah, al = split(a.T)
        bh, bl = split(b.T)
        out[z] = _three_terms(ah, al, bh, bl) * np.float32(2.0 ** -e)
    return out
