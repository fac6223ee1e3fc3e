"""Plain reference of ONE 3 x 3 / pad 1 convolution layer as csrc/nsr_gemm_f16.hip computes it on pre-split fp16 planes
(conv_halo_kernel and the conv-gather mode of gemm_f16x3_kernel), on the CPU in fp64, together with the exact-input operand
builder, the case table and the argument structs the two test files share (tests/test_gpu_conv_units.py runs the cases on the
device, tests/test_conv_units_cpu.py checks this file against itself and the dispatch of every case without a device).

Method (tests/test_gpu_gemm_units.py): operands for which every product and every partial sum is exactly representable in
fp32, so the result does not depend on the order of summation, the tile shape or the kernel, and must equal the reference BIT
FOR BIT.  Here: activations a = ah + al and weights b = bh + bl with ah, bh integers in [-3, 3] and al, bl INDEPENDENT integers
in [-3, 3] x 2^-8.  The kernels treat the planes as opaque fp16 and compute ah bh + ah bl + al bh -- the al bl term is dropped
by design (nsr_gemm.h) -- so the reference is the sum of exactly these three convolutions: a multiple of 2^-8 of magnitude
<= K (9 + 18 / 256) < 2^24 quanta for K = 9 cin up to 4,608.  v = relu(2^-6 acc + bias) with an integer bias is a multiple of
2^-14 below 2^10: fmaf rounds nothing.  The output planes are hi = fp16(v), lo = fp16(fp32(v) - hi), round to nearest even.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from tests import hooks

NAN16 = 0x7e00                                # fp16 quiet NaN: every element a kernel has no business reading
SENT16 = np.uint16(0xBEEF).view(np.int16)     # output sentinel (planes); fp32 outputs use SENT32
SENT32 = -3.0e38
ACC_SCALE = 2.0 ** -6
LO = 2.0 ** -8                                # quantum of the lo planes
GUARD_ROWS = 64                               # sentinel rows before and after the owned output rows


@dataclass(frozen=True)
class Case:
    """One call of gemm_f16x3 in conv-gather mode.  Hs x Ws: source image (before the optional nearest x2 upsample)."""
    name: str
    route: int                  # hooks.ROUTE_* the dispatch must pick
    cin: int
    N: int
    n_img: int
    Hs: int
    Ws: int
    stride: int = 1
    up: int = 0
    group: int = 0              # 8: grouped rows + max planes
    bs: bool = True             # hand the stream-ordered weights over (False: Bs = null forces the staged kernels)
    tail: bool = False          # the network's last layer: tanh, fp32 NHWC output, n_valid real columns
    n_valid: Optional[int] = None
    seed: int = 0

    @property
    def Ho(self):
        return ((2 * self.Hs if self.up else self.Hs) - 1) // self.stride + 1

    @property
    def Wo(self):
        return ((2 * self.Ws if self.up else self.Ws) - 1) // self.stride + 1

    @property
    def M(self):
        return self.n_img * self.Ho * self.Wo

    @property
    def K(self):
        return 9 * self.cin

    @property
    def nv(self):
        return self.N if self.n_valid is None else self.n_valid


# ------------------------------------------------------------------------------------------------------------------------
# fp16 helpers (numpy round-to-nearest-even casts)
# ------------------------------------------------------------------------------------------------------------------------
def f16_bits(x: np.ndarray) -> np.ndarray:
    """values -> fp16 bit patterns as int16 (exact for the operands built here; RNE otherwise)"""
    return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.int16)


def bits_f64(bits) -> torch.Tensor:
    """int16 fp16 bit patterns (numpy or torch) -> fp64 values"""
    b = bits.cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
    return torch.from_numpy(b.view(np.float16).astype(np.float64))


def split_planes(v32: np.ndarray):
    """hi = fp16(v), lo = fp16(v - hi) as int16 bit patterns -- tests/test_gpu_gemm_units.py::test_split_weights_bit_exact"""
    v32 = np.asarray(v32, dtype=np.float32)
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.int16), lo.view(np.int16)


# ------------------------------------------------------------------------------------------------------------------------
# GemmF16Args::Bs, from the layout documented in csrc/nsr_gemm.h
# ------------------------------------------------------------------------------------------------------------------------
def stream_order(Bh: np.ndarray, Bl: np.ndarray, cin: int) -> np.ndarray:
    """[column block of 32][cc * 9 + tap][hi, lo][lane li + 32 h][8 halves], the halves of a lane =
    B[32 nb + li][tap * cin + 16 cc + 8 h .. + 8).  Bh, Bl: (N, 9 cin) 16-bit arrays, N % 32 == 0, cin % 16 == 0."""
    N, K = Bh.shape
    assert Bl.shape == Bh.shape and K == 9 * cin and cin % 16 == 0 and N % 32 == 0
    ncc = cin // 16
    out = np.empty((N // 32, ncc * 9, 2, 64, 8), dtype=Bh.dtype)
    for plane, B in enumerate((Bh, Bl)):
        for nb in range(N // 32):
            for cc in range(ncc):
                for tap in range(9):
                    for h in range(2):
                        k0 = tap * cin + 16 * cc + 8 * h
                        out[nb, cc * 9 + tap, plane, 32 * h:32 * h + 32, :] = B[32 * nb:32 * nb + 32, k0:k0 + 8]
    return out.reshape(-1)


def stream_order_inverse(Bs: np.ndarray, N: int, cin: int):
    """the (Bh, Bl) a stream-ordered copy was made from: the same index map, vectorised and read the other way round"""
    ncc = cin // 16
    s = Bs.reshape(N // 32, ncc, 9, 2, 2, 32, 8)                      # nb, cc, tap, plane, h, li, e
    b = s.transpose(3, 0, 5, 2, 1, 4, 6)                              # plane, nb, li, tap, cc, h, e
    b = np.ascontiguousarray(b).reshape(2, N, 9 * cin)
    return b[0], b[1]


# ------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Operands:
    case: Case
    ah: torch.Tensor            # (n_img, Hs, Ws, cin) fp64 values of the hi plane
    al: torch.Tensor
    bh: torch.Tensor            # (N, K) fp64
    bl: torch.Tensor
    bias: torch.Tensor          # (N,) fp32
    # device-layout buffers (CPU tensors; the GPU test moves them over)
    A: torch.Tensor             # int16 (2, n_img + 2, Hs, Ws, ld): hi | lo planes with one guard image either side
    ld: int = 0
    ch0: int = 0
    Bh: torch.Tensor = None     # int16 (N, ldbh)
    Bl: torch.Tensor = None
    ldbh: int = 0
    Bs: Optional[torch.Tensor] = None
    extra: dict = field(default_factory=dict)


def _ints(gen, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def build_planes(ah, al, ld, ch0):
    """(2, n_img + 2, Hs, Ws, ld) int16: the slice [ch0, ch0 + cin) of images 1 .. n_img holds the values, everything else NaN"""
    n_img, Hs, Ws, cin = ah.shape
    A = np.full((2, n_img + 2, Hs, Ws, ld), NAN16, dtype=np.int16)
    A[0, 1:-1, :, :, ch0:ch0 + cin] = f16_bits(ah.numpy())
    A[1, 1:-1, :, :, ch0:ch0 + cin] = f16_bits(al.numpy())
    return torch.from_numpy(A)


def build_weights(bh, bl, pad=8):
    N, K = bh.shape
    out = []
    for b in (bh, bl):
        buf = np.full((N, K + pad), NAN16, dtype=np.int16)
        buf[:, :K] = f16_bits(b.numpy())
        out.append(torch.from_numpy(buf))
    return out[0], out[1], K + pad


def build_operands(c: Case) -> Operands:
    gen = torch.Generator().manual_seed(1000 + c.seed)
    ah = _ints(gen, (c.n_img, c.Hs, c.Ws, c.cin))
    al = _ints(gen, (c.n_img, c.Hs, c.Ws, c.cin)) * LO
    bh = _ints(gen, (c.N, c.K))
    bl = _ints(gen, (c.N, c.K)) * LO
    bias = _ints(gen, (c.N,), -8, 8).float()
    ch0 = 16 if c.cin <= 64 else 128          # the slice sits inside a wider buffer, as in the concatenated decoder inputs
    ld = ch0 + c.cin + 8
    A = build_planes(ah, al, ld, ch0)
    Bh, Bl, ldbh = build_weights(bh, bl)
    Bs = None
    if c.bs:
        Bs = torch.from_numpy(stream_order(Bh[:, :c.K].numpy(), Bl[:, :c.K].numpy(), c.cin))
    return Operands(c, ah, al, bh, bl, bias, A, ld, ch0, Bh, Bl, ldbh, Bs)


# ------------------------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------------------------
def conv64(x_nhwc: torch.Tensor, w_nk: torch.Tensor, stride: int, up: int) -> torch.Tensor:
    """fp64 3 x 3 / pad 1 convolution of an NHWC tensor (through a nearest x2 upsample if `up`) with weights (N, K), K index =
    (ky * 3 + kx) * cin + c.  Returns the GEMM's (n_img * Ho * Wo, N) matrix, rows image-major then row-major pixels."""
    n_img, Hs, Ws, cin = x_nhwc.shape
    x = x_nhwc.permute(0, 3, 1, 2).double()
    if up:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    w = w_nk.double().view(-1, 3, 3, cin).permute(0, 3, 1, 2).contiguous()
    y = F.conv2d(x, w, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def im2col_numpy(src, nchw, cin, n_img, Hs, Ws, stride, up, Ho, Wo, kp):
    """col[(img, oy, ox)][tap * cin + c] = source pixel (oy stride + ky - 1, ox stride + kx - 1) of the (upsampled) image, zero
    outside it; columns >= 9 cin zero.  src: (n_img, Hs, Ws, >= cin) or (n_img, cin, Hs, Ws)."""
    col = np.zeros((n_img, Ho, Wo, kp), dtype=np.float32)
    Hin, Win = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    oy, ox = np.arange(Ho), np.arange(Wo)
    for tap in range(9):
        iy, ix = oy * stride + tap // 3 - 1, ox * stride + tap % 3 - 1
        vy, vx = (iy >= 0) & (iy < Hin), (ix >= 0) & (ix < Win)
        sy, sx = (iy >> 1 if up else iy)[vy], (ix >> 1 if up else ix)[vx]
        for c in range(cin):
            plane = src[:, c] if nchw else src[..., c]                     # (n_img, Hs, Ws)
            block = col[:, :, :, tap * cin + c]
            block[np.ix_(np.arange(n_img), oy[vy], ox[vx])] = plane[np.ix_(np.arange(n_img), sy, sx)]
    return col.reshape(n_img * Ho * Wo, kp)


def accumulator(o: Operands, four_terms: bool = False) -> torch.Tensor:
    c = o.case
    acc = conv64(o.ah, o.bh, c.stride, c.up) + conv64(o.ah, o.bl, c.stride, c.up) + conv64(o.al, o.bh, c.stride, c.up)
    if four_terms:
        acc = acc + conv64(o.al, o.bl, c.stride, c.up)
    return acc


def assert_exact_regime(o: Operands):
    """tests/test_gpu_gemm_units.py::_assert_exact_regime with quantum 2^-8 on the case's im2col product: max over outputs of
    sum_k (|ah| + |al|)(|bh| + |bl|) + |bias| / acc_scale < 2^24 quanta bounds every partial sum of the three kept terms in any
    order.  The sums over k are formed by a convolution of the absolute values and handed over one row per output column (a
    1 x 1 product): the im2col matrix of the largest cases would take gigabytes."""
    from tests.test_gpu_gemm_units import _assert_exact_regime
    c = o.case
    w = conv64(o.ah.abs() + o.al.abs(), o.bh.abs() + o.bl.abs(), c.stride, c.up).max(dim=0).values
    _assert_exact_regime(w.view(1, -1), torch.eye(c.N, dtype=torch.float64), o.bias.double() / ACC_SCALE, quantum=LO, what=c.name)


def pre_activation(o: Operands, four_terms: bool = False) -> torch.Tensor:
    return accumulator(o, four_terms) * ACC_SCALE + o.bias.double()


def grouped_max(v: torch.Tensor, c: Case) -> torch.Tensor:
    """(n_img * px, N) -> (n_img / 8 * px, N): the maximum over the 8 consecutive images of a group, per pixel"""
    px = c.Ho * c.Wo
    return v.view(c.n_img // 8, 8, px, -1).max(dim=1).values.reshape(-1, v.shape[1])


# ------------------------------------------------------------------------------------------------------------------------
# outputs and argument struct
# ------------------------------------------------------------------------------------------------------------------------
def output_geometry(c: Case):
    """(ldc, column offset, ldm, max-plane column offset): wider than N, even, offset into the row"""
    if c.tail:
        return c.nv, 0, 0, 0              # NHWC rgb: ldc = 3, nothing beside the valid columns
    return c.N + 24, 6, c.N + 10, 4


def empty_outputs(c: Case):
    """sentinel-filled output buffers (CPU): C int16 (2, GUARD + M + GUARD, ldc) or fp32 (GUARD + M + GUARD, ldc); Mx or None"""
    ldc, _, ldm, _ = output_geometry(c)
    rows = c.M + 2 * GUARD_ROWS
    if c.tail:
        C = torch.full((rows, ldc), SENT32, dtype=torch.float32)
    else:
        C = torch.full((2, rows, ldc), int(SENT16), dtype=torch.int16)
    Mx = torch.full((2, c.M // 8 + 2 * GUARD_ROWS, ldm), int(SENT16), dtype=torch.int16) if c.group == 8 else None
    return C, Mx


def expected_outputs(c: Case, v64: torch.Tensor):
    """the buffers of empty_outputs with the owned region filled from the reference values v64 (M, N) (not the tail)"""
    C, Mx = empty_outputs(c)
    _, co, _, mo = output_geometry(c)
    v32 = v64.float()
    assert torch.equal(v32.double(), v64), "reference is not representable in fp32: the inputs left the exact regime"
    hi, lo = split_planes(v32.numpy()[:, :c.nv])
    C[0, GUARD_ROWS:GUARD_ROWS + c.M, co:co + c.nv] = torch.from_numpy(hi)
    C[1, GUARD_ROWS:GUARD_ROWS + c.M, co:co + c.nv] = torch.from_numpy(lo)
    if Mx is not None:
        mh, ml = split_planes(grouped_max(v32, c).numpy()[:, :c.nv])
        Mx[0, GUARD_ROWS:GUARD_ROWS + c.M // 8, mo:mo + c.nv] = torch.from_numpy(mh)
        Mx[1, GUARD_ROWS:GUARD_ROWS + c.M // 8, mo:mo + c.nv] = torch.from_numpy(ml)
    return C, Mx


def fill_args(c: Case, o: Operands, pA, pBh, pBl, pBs, pbias, pC, pMx) -> hooks.GemmF16Args:
    """GemmF16Args of the case; p*: base addresses of the buffers of `o` / empty_outputs (device, or dummy aligned ones)"""
    ldc, co, ldm, mo = output_geometry(c)
    a = hooks.GemmF16Args()
    a.g.M, a.g.N, a.g.K, a.g.n_valid, a.g.splits = c.M, c.N, c.K, c.nv, 1
    a.g.act = hooks.ACT_TANH if c.tail else hooks.ACT_RELU
    a.g.acc_scale = ACC_SCALE
    a.g.bias = pbias
    a.g.lda, a.g.ldc = o.ld, ldc
    plane = (c.n_img + 2) * c.Hs * c.Ws * o.ld
    a.Ah = pA + 2 * (c.Hs * c.Ws * o.ld + o.ch0)          # image 1 (behind the guard image), channel ch0
    a.a_plane = plane
    a.Bh, a.Bl, a.ldbh = pBh, pBl, o.ldbh
    a.Bs = pBs if c.bs else None
    a.conv = hooks.ConvGather(c.cin, c.Hs, c.Ws, c.Ho, c.Wo, c.stride, c.up)
    rows = c.M + 2 * GUARD_ROWS
    if c.tail:
        a.g.C = pC + 4 * GUARD_ROWS * ldc
    else:
        a.Ch = pC + 2 * (GUARD_ROWS * ldc + co)
        a.c_plane = rows * ldc
    if c.group == 8:
        a.group = 8
        a.Mh = pMx + 2 * (GUARD_ROWS * ldm + mo)
        a.m_plane = (c.M // 8 + 2 * GUARD_ROWS) * ldm
        a.ldm = ldm
    return a


def dummy_args(c: Case) -> hooks.GemmF16Args:
    """the case's argument struct over made-up 4-KiB-aligned addresses: all the dispatch looks at (it follows no pointer)"""
    o = Operands(c, None, None, None, None, None, None, ld=(16 if c.cin <= 64 else 128) + c.cin + 8, ch0=16 if c.cin <= 64 else 128,
                 ldbh=c.K + 8)
    base = 0x10000000
    return fill_args(c, o, *(base * (i + 1) for i in range(7)))


def route_of(lib, a: hooks.GemmF16Args) -> int:
    return lib.nsr_test_gemm_f16x3_route(ctypes.byref(a))


# ------------------------------------------------------------------------------------------------------------------------
# the cases (issue table: every route at the smallest shapes at which it can go wrong)
# ------------------------------------------------------------------------------------------------------------------------
R = hooks


def _half_plain_s1():
    out = []
    for cin in (16, 32, 48, 128):                       # 1, 2, 3, 8 channel chunks: ring and buffer parity wrap at odd and even counts
        for (H, W) in ((16, 16), (32, 48)):             # one block with all four borders; interior-side and border-side blocks
            for n_img in (1, 3):
                for up in (0, 1):                       # up: 8 x 8 -> 16 x 16, 16 x 24 -> 32 x 48
                    out.append(Case(f"half_s1_c{cin}_{H}x{W}_n{n_img}_up{up}", R.ROUTE_HALF_S1, cin, 128, n_img, H >> up, W >> up, 1, up,
                                    seed=len(out)))
    return out


HALF_S1 = _half_plain_s1()
HALF_S1_WIDE = [Case(f"half_s1_N{N}", R.ROUTE_HALF_S1, 32, N, 2, 32, 32, seed=40 + i) for i, N in enumerate((256, 384))]   # two / three column tiles: n0 != 0
HALF_GROUPED_S1 = [Case(f"half_g_s1_n{n}_{H}x{W}", R.ROUTE_HALF_GROUPED_S1, 32, 128, n, H, W, group=8, seed=50 + i)
                   for i, (n, H, W) in enumerate(((8, 8, 8), (16, 8, 8), (8, 4, 8), (16, 4, 8), (8, 8, 16), (16, 8, 16)))]
HALF_GROUPED_S1.append(Case("half_g_s1_up", R.ROUTE_HALF_GROUPED_S1, 48, 128, 8, 4, 4, 1, 1, group=8, seed=57))
MULTI_S1 = [Case(f"multi_s1_H{H}_n{n}", R.ROUTE_MULTI_S1, 32, 128, n, H, 8, seed=60 + i)
            for i, (H, n) in enumerate((H, n) for H in (4, 8) for n in (1, 7, 8, 9))]
MULTI_S2 = [Case(f"multi_s2_n{n}", R.ROUTE_MULTI_S2, 128, 128, n, 16, 16, 2, seed=70 + n) for n in (1, 9)]
HALF_S2 = [Case("half_s2", R.ROUTE_HALF_S2, 128, 128, 2, 64, 32, 2, seed=80)]
HALF_GROUPED_S2 = [Case("half_g_s2", R.ROUTE_HALF_GROUPED_S2, 128, 128, 8, 16, 32, 2, group=8, seed=81)]
# the big tiles: only where the half tile costs 1.05 x as many CU-rounds, i.e. 128 < big blocks <= 256
BIG = [
    Case("big82_s1", R.ROUTE_BIG82_S1, 16, 256, 33, 32, 32, seed=90),                        # 132 blocks of 256 x 256
    Case("big82_g_s1", R.ROUTE_BIG82_GROUPED_S1, 16, 256, 16, 32, 72, group=8, seed=91),     # 144
    Case("big44_g_s1", R.ROUTE_BIG44_GROUPED_S1, 16, 128, 16, 64, 72, group=8, seed=92),     # 144 blocks of 512 x 128
    Case("big82_s2", R.ROUTE_BIG82_S2, 128, 256, 33, 64, 64, 2, seed=93),                    # 132
    Case("big82_g_s2", R.ROUTE_BIG82_GROUPED_S2, 128, 256, 16, 64, 144, 2, group=8, seed=94),  # 144
]
TAIL = [Case(f"tail_c{cin}_{H}x16", R.ROUTE_HALO_TAIL, cin, 64, 2, H, 16, tail=True, n_valid=3, seed=100 + i)
        for i, (cin, H) in enumerate((cin, H) for cin in (16, 128) for H in (16, 32))]

_STAGED_VARIANTS = ((R.ROUTE_STAGED_K64_FULL, 64, 128), (R.ROUTE_STAGED_K64, 64, 160), (R.ROUTE_STAGED_K32_FULL, 32, 128),
                    (R.ROUTE_STAGED_K32, 32, 36))


def _staged():
    out = []
    for route, cin, N in _STAGED_VARIANTS:
        tag = f"staged{route}_c{cin}_N{N}"
        s = 110 + 10 * len(out)
        out += [
            Case(tag + "_6x10", route, cin, N, 2, 6, 10, bs=False, seed=s),
            Case(tag + "_12x20", route, cin, N, 3, 12, 20, bs=False, seed=s + 1),
            Case(tag + "_s2_odd", route, cin, N, 5, 5, 7, 2, bs=False, seed=s + 2),                 # 5 x 7 -> 3 x 4
            Case(tag + "_up", route, cin, N, 2, 3, 5, 1, 1, bs=False, seed=s + 3),                   # 3 x 5 -> 6 x 10
            Case(tag + "_grouped_ragged", route, cin, N, 8, 6, 10, group=8, bs=False, seed=s + 4),   # M = 480: the last row tile is ragged
            Case(tag + "_nvalid", route, cin, N, 2, 6, 10, bs=False, n_valid=N - 2, seed=s + 5),     # the general epilogue
        ]
    return out


STAGED = _staged()
STAGED_WIDE = [Case("staged_wide", R.ROUTE_STAGED_WIDE, 32, 512, 64, 32, 32, bs=False, seed=200)]      # M = 65,536: 512 row tiles x 2

EXACT_CASES = (HALF_S1 + HALF_S1_WIDE + HALF_GROUPED_S1 + MULTI_S1 + MULTI_S2 + HALF_S2 + HALF_GROUPED_S2 + BIG + TAIL + STAGED +
               STAGED_WIDE)
# routes that no exact case covers, with the reason (tests/test_conv_units_cpu.py)
UNCOVERED_ROUTES = {
    R.ROUTE_NONE: "launches nothing",
    R.ROUTE_BIG44_S1: "unreachable: a plain non-wide stride-1 layer that fits 512 x 128 fits the paired half tile, which is always taken",
    R.ROUTE_STAGED_F32A: "fp32 A: with a conv gather it has no call site in the product (tests/test_gpu_gemm_units.py covers it as a plain GEMM)",
}
