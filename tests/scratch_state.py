"""Tools for testing that a caller-owned workspace is pure scratch and that its stated size suffices
(tests/test_gpu_scratch_state.py; the logic is checked on CPU tensors in tests/test_scratch_state_cpu.py).

``guarded(nbytes, fill, device)`` hands out exactly ``nbytes`` bytes at the FRONT of a larger allocation, so the base pointer --
and with it the alignment a launcher may rely on -- is the allocation's own; the ``guard`` bytes behind the view hold the
sentinel byte 0xA5 and ``Guarded.damage()`` reports the first and last offset past the view that a call changed.
``guarded_like(shape, dtype, device)`` is the same for a typed output tensor, pre-filled with 0xFF (NaN as fp16 / fp32 / fp64,
-1 as any integer).

Fills of the body:

    ZERO      0x00 -- what a fresh process usually finds
    ONES      0xFF -- NaN as fp16 / fp32 / fp64, -1 as any integer
    LEFTOVER  whatever a previous call left behind: a tensor (or bytes) given as ``leftover=``, repeated to the length

``same_bits(a, b)`` compares the byte content, so NaN payloads and signed zeros count; ``diff(name, got, want)`` is None on equal
bits and otherwise a line with the tensor's name, the number of differing elements and the first index."""
from typing import NamedTuple, Optional, Tuple

import torch

ZERO, ONES, LEFTOVER = "ZERO", "ONES", "LEFTOVER"
FILLS = (ZERO, ONES, LEFTOVER)
SENTINEL = 0xA5
GUARD_BYTES = 1 << 20


def _bytes(t: torch.Tensor) -> torch.Tensor:
    """The byte content of a tensor, flat."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def fill_bytes(view: torch.Tensor, fill: str, leftover: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Set a uint8 view's body to ``fill`` (in place; returns the view)."""
    if view.dtype != torch.uint8 or view.ndim != 1:
        raise TypeError("fill_bytes wants a flat uint8 view")
    if fill == ZERO:
        view.zero_()
    elif fill == ONES:
        view.fill_(0xFF)
    elif fill == LEFTOVER:
        if leftover is None:
            raise ValueError("fill LEFTOVER needs leftover=: the bytes a previous call left behind")
        src = _bytes(leftover).to(view.device)
        if src.numel() == 0:
            raise ValueError("leftover is empty")
        n = view.numel()
        view.copy_(src.repeat(-(-n // src.numel()))[:n] if src.numel() < n else src[:n])
    else:
        raise ValueError(f"unknown fill {fill!r}: one of {FILLS}")
    return view


class Damage(NamedTuple):
    """Changed guard bytes: their number and the first / last offset counted from the END of the view (0 = the byte right
    behind it)."""
    count: int
    first: int
    last: int


class Guarded:
    """``view``: the tensor a call gets; ``base``: the whole allocation (view + guard)."""

    def __init__(self, name: str, base: torch.Tensor, nbytes: int, view: torch.Tensor):
        self.name, self.base, self.nbytes, self.view = name, base, int(nbytes), view

    @property
    def guard(self) -> torch.Tensor:
        return self.base[self.nbytes:]

    def damage(self) -> Optional[Damage]:
        """None while every guard byte holds the sentinel (synchronises: it reads the bytes)."""
        bad = torch.nonzero(self.guard != SENTINEL).reshape(-1)
        if bad.numel() == 0:
            return None
        return Damage(int(bad.numel()), int(bad[0]), int(bad[-1]))

    def check(self) -> Optional[str]:
        """None, or a line that names the buffer and locates the damage."""
        d = self.damage()
        if d is None:
            return None
        return (f"{self.name}: {d.count} guard byte(s) changed behind the stated {self.nbytes} bytes, "
                f"first at +{d.first}, last at +{d.last}")


def guarded(nbytes: int, fill: str, device, guard: int = GUARD_BYTES, leftover: Optional[torch.Tensor] = None,
            name: str = "workspace") -> Guarded:
    """A uint8 view of exactly ``nbytes`` at the front of an allocation of ``nbytes + guard`` bytes: body = ``fill``, the rest
    the sentinel."""
    nbytes, guard = int(nbytes), int(guard)
    if nbytes < 0 or guard <= 0:
        raise ValueError("nbytes >= 0 and guard > 0")
    base = torch.empty(nbytes + guard, dtype=torch.uint8, device=device)
    base[nbytes:].fill_(SENTINEL)
    view = base[:nbytes]
    fill_bytes(view, fill, leftover)
    assert view.data_ptr() == base.data_ptr()
    return Guarded(name, base, nbytes, view)


def guarded_like(shape: Tuple[int, ...], dtype, device, guard: int = GUARD_BYTES, name: str = "output") -> Guarded:
    """A contiguous tensor of ``shape`` / ``dtype`` whose storage is followed by a guard; pre-filled with 0xFF bytes (NaN for the
    float types, -1 for the integer ones) so that an element a call leaves unwritten shows."""
    shape = tuple(int(s) for s in shape)
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    g = guarded(nbytes, ONES, device, guard, name=name)
    g.view = g.base[:nbytes].view(dtype).view(shape)
    assert g.view.data_ptr() == g.base.data_ptr()
    return g


def check_guards(guards) -> list:
    """The damage lines of every guarded buffer in ``guards`` (an empty list: all intact)."""
    return [line for line in (g.check() for g in guards) if line]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal shape, dtype and byte content (0.0 != -0.0; two NaNs are equal only with the same payload)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a).cpu(), _bytes(b).cpu())


def diff(name: str, got: torch.Tensor, want: torch.Tensor) -> Optional[str]:
    """None if ``got`` has the bits of ``want``, else a line: the tensor, how many elements differ, the first index."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{name}: {tuple(got.shape)} {got.dtype} != {tuple(want.shape)} {want.dtype}"
    if got.numel() == 0:
        return None
    size = got.element_size()
    g, w = _bytes(got).cpu().view(-1, size), _bytes(want).cpu().view(-1, size)
    bad = torch.nonzero((g != w).any(1)).reshape(-1)
    if bad.numel() == 0:
        return None
    flat = int(bad[0])
    idx, rem = [], flat
    for s in reversed(got.shape):
        idx.append(rem % s)
        rem //= s
    idx = tuple(reversed(idx))
    gv, wv = got.detach().reshape(-1)[flat].item(), want.detach().reshape(-1)[flat].item()
    return (f"{name}: {bad.numel()} of {got.numel()} elements differ, first at {idx}: got {gv!r} "
            f"(0x{bytes(g[flat].tolist())[::-1].hex()}), want {wv!r} (0x{bytes(w[flat].tolist())[::-1].hex()})")


def diff_all(case: str, got: dict, want: dict) -> list:
    """``diff`` over two dicts of tensors with the same keys; every line is prefixed with ``case``."""
    lines = []
    if set(got) != set(want):
        lines.append(f"{case}: outputs {sorted(got)} != {sorted(want)}")
    for k in want:
        if k in got:
            line = diff(k, got[k], want[k])
            if line:
                lines.append(f"{case}: {line}")
    return lines


def unwritten(name: str, t: torch.Tensor) -> Optional[str]:
    """For an output that was pre-filled with 0xFF bytes and must come back fully overwritten: None, or a line with the number
    of elements that hold those bits and the first of them.  (Arithmetic on a NaN keeps its payload, so a value computed FROM a
    0xFF-filled workspace shows up here too: either way the call did not produce the element from its inputs.)"""
    size = t.element_size()
    b = _bytes(t).view(-1, size)                     # on the tensor's own device
    left = torch.nonzero((b == 0xFF).all(1)).reshape(-1)
    if left.numel() == 0:
        return None
    return f"{name}: {left.numel()} of {t.numel()} elements hold 0xFF bytes (the pre-fill, or a NaN carried out of a 0xFF-filled buffer), first at flat index {int(left[0])}"


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_scratch_state.py, kept here so that tests/test_scratch_state_cpu.py checks their CPU-checkable
# part: every size function returns non-zero for them, and the refinement-training arithmetic below names the ragged sites.
# ---------------------------------------------------------------------------------------------------------------------------
# A. render: (precision, R, N_coarse, N_importance, options of ops.forward_rays)
RENDER_PRECISIONS = ("fp32", "f16x3", "f16", "bf16")
RENDER_CASES = [(p, R, 64, ni, {}) for p in RENDER_PRECISIONS for R in (5, 259) for ni in (64, 128)] + \
    [("f16x3", 259, 64, 64, {"coarse_rgb": False}), ("f16x3", 259, 64, 64, {"early_stop": 1e-4})]
RENDER_SEEDS = (99, 21)    # make_state_dict seeds (coarse, fine) whose fields are neither empty nor opaque on the test's rays
RENDER_REUSE =(("f16x3", 259, 64, 128), ("f16x3", 5, 64, 64))            # property 4: the large call, then the small one

# B. default-network training on the batch of tests/golden/train_llff_rand.npz (96 rays, s2 = 4, 64 + 64 samples):
# unchunked, and 40-ray chunks (a multiple of s2 = 4) that leave a ragged last pass of 16 rays
TRAIN_R, TRAIN_NC, TRAIN_NI, TRAIN_S2 = 96, 64, 64, 4
TRAIN_PRECISIONS = ("f16x3", "f16x3_gemm", "fp32")
TRAIN_CHUNKS = (0, 40)
TRAIN_CASES = [(entry, p, c) for entry in ("fused", "pair") for p in TRAIN_PRECISIONS for c in TRAIN_CHUNKS]

# C. architecture-descriptor training: a skip layer and W = 48 != Wp = 64 (padded columns in every activation and weight panel);
# 7 rays: 448 coarse points are 3.5 tiles of 128; in chunks of 3 rays the passes hold 192 / 384 / 64 / 128 points
ARCH = {"D": 3, "W": 48, "skips": (1,), "deg_pos": 4, "deg_dir": 2, "no_dir": False}
ARCH_R, ARCH_CHUNKS = 7, (0, 3)
ARCH_SEEDS = (3, 6)        # make_state_dict_arch seeds whose coarse AND fine fields are neither empty nor opaque on these rays, under both embedding words
ARCH_CASES = [(p, embed, c) for p in ("fp32", "f16x3_gemm") for embed in (0, 1) for c in ARCH_CHUNKS]      # embed 1: --no_xyz

# D. refinement inference: (precision, with references, (B, R, H, W))
REFINE_SHAPES = ((3, 2, 16, 24), (9, 1, 16, 16))
REFINE_CASES = [(p, ref, s) for p in ("fp32", "f16x3") for ref in (True, False) for s in REFINE_SHAPES]

# E. refinement training: (precision, weight_grad, (B, R, H, W), img_chunk); shapes of fixture cases A and B of
# tests/golden/refine_train.npz
REFINE_TRAIN_COMBOS = (("fp32", "fp32"), ("f16x3_mixed", "fp32"), ("f16x3_mixed", "f16x3"))
REFINE_TRAIN_SHAPES = {"A": (2, 2, 16, 24), "B": (3, 1, 16, 16)}
REFINE_TRAIN_CASES = [(combo, tag, ic) for combo in REFINE_TRAIN_COMBOS for tag in REFINE_TRAIN_SHAPES for ic in (0, 1)]

# F. metrics: the fixtures of tests/golden/metrics.npz
METRIC_TAGS = ("ragged", "tiny")

# output level (0: H x W, 1: / 4, 2: / 16, 3: / 64 pixels) of the refinement network's 19 layers (csrc/nsr_refine_train.hip)
_REFINE_LEVEL = (0, 0, 1, 1, 2, 2, 3, 3, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0, 0)


def refine_train_chunk(B: int, R: int, H: int, W: int, img_chunk: int) -> int:
    """``resolve_chunk`` of csrc/nsr_refine_train.hip: images whose im2col matrix is live at once."""
    c = img_chunk if img_chunk > 0 else (1 << 28) // (H * W * 3456)
    return min(max(c, 1), B * R)


def refine_train_sites(B: int, R: int, H: int, W: int, img_chunk: int):
    """Per site of the train-mode refinement network (0..6 encoder on the synthesised patches, 7..13 encoder on the references,
    14..25 decoder) the rows M = nc * rows_img of every weight-gradient product of the fp32 route: a list of
    (site, layer, [M of each image chunk]).  M % 32 != 0 takes the ``Kp > M`` memset of the col matrix and makes the product
    read the zeroed rows behind dZ."""
    chunk = refine_train_chunk(B, R, H, W, img_chunk)
    sites = []
    for s in range(26):
        layer = s if s < 7 else s - 7
        n_img = B * R if 7 <= s < 14 else B
        rows_img = (H * W) >> (2 * _REFINE_LEVEL[layer])
        sites.append((s, layer, [min(chunk, n_img - i0) * rows_img for i0 in range(0, n_img, chunk)]))
    return sites


def ragged_sites(B: int, R: int, H: int, W: int, img_chunk: int):
    """The sites of ``refine_train_sites`` with a chunk whose M is not a multiple of 32."""
    return [s for s, _, ms in refine_train_sites(B, R, H, W, img_chunk) if any(m % 32 for m in ms)]
