"""The helper of the workspace tests (tests/scratch_state.py) on CPU tensors, and the CPU-checkable part of the cases of
tests/test_gpu_scratch_state.py: every size function returns non-zero for the chosen arguments, and the arithmetic of the
refinement-training cases names the sites whose weight-gradient product has M = nc * rows_img not a multiple of 32."""
import struct

import pytest
import torch

from nerf_sr_amd import _lib
from nerf_sr_amd import refine as rf
from tests import scratch_state as ss


# ---- the guard ------------------------------------------------------------------------------------------------------------
def test_guarded_view_keeps_the_base_pointer_and_the_fill():
    for fill, byte in ((ss.ZERO, 0x00), (ss.ONES, 0xFF)):
        g = ss.guarded(1000, fill, "cpu", guard=4096)
        assert g.view.dtype == torch.uint8 and g.view.numel() == 1000 and g.view.data_ptr() == g.base.data_ptr()
        assert g.base.numel() == 1000 + 4096
        assert bool((g.view == byte).all()) and bool((g.guard == ss.SENTINEL).all())
        assert g.damage() is None and g.check() is None


def test_a_write_one_byte_past_the_view_is_detected_and_located():
    g = ss.guarded(1000, ss.ZERO, "cpu", guard=4096, name="ws")
    g.base[1000] = 0                                  # the first byte behind the view
    assert g.damage() == ss.Damage(1, 0, 0)
    assert "ws" in g.check() and "+0" in g.check() and "1000 bytes" in g.check()
    g.base[1000 + 4095] = 7                           # ... and the last byte of the guard
    assert g.damage() == ss.Damage(2, 0, 4095)
    g2 = ss.guarded(24, ss.ONES, "cpu", guard=64)
    g2.base[24 + 17: 24 + 21] = 0
    assert g2.damage() == ss.Damage(4, 17, 20)


def test_a_write_inside_the_view_is_not_reported():
    g = ss.guarded(1000, ss.ONES, "cpu", guard=4096)
    g.view[0] = 1
    g.view[999] = 2                                   # the last byte of the view
    g.view[17:400] = ss.SENTINEL
    assert g.damage() is None and ss.check_guards([g]) == []


def test_a_sentinel_valued_write_into_the_guard_is_the_only_blind_spot():
    """The checker compares bytes: a stray store of the sentinel's own value cannot show.  Floats and indices are never
    0xA5A5A5A5 by accident (-2.9e-16), which is why that byte was chosen."""
    assert struct.unpack("<f", bytes([ss.SENTINEL] * 4))[0] == pytest.approx(-2.8731e-16, rel=1e-3)


def test_typed_output_views():
    g = ss.guarded_like((5, 3), torch.float32, "cpu", guard=256, name="rgb")
    assert g.view.shape == (5, 3) and g.view.dtype == torch.float32 and g.view.is_contiguous()
    assert g.view.data_ptr() == g.base.data_ptr() and g.nbytes == 60
    assert bool(torch.isnan(g.view).all())
    assert "15 of 15" in ss.unwritten("rgb", g.view)
    g.view.copy_(torch.arange(15.0).view(5, 3))
    assert ss.unwritten("rgb", g.view) is None and g.damage() is None
    g.view[4, 2] = float("nan")                       # a computed NaN has another payload than the pre-fill
    assert ss.unwritten("rgb", g.view) is None
    g.base[60] = 0
    assert g.damage() == ss.Damage(1, 0, 0)
    i = ss.guarded_like((7,), torch.int32, "cpu", guard=64)
    assert bool((i.view == -1).all())
    d = ss.guarded_like((2,), torch.float64, "cpu", guard=64)
    assert bool(torch.isnan(d.view).all()) and d.nbytes == 16


# ---- the fills --------------------------------------------------------------------------------------------------------------
def test_ones_is_nan_in_every_float_type_and_minus_one_in_every_integer_type():
    v = ss.guarded(64, ss.ONES, "cpu", guard=64).view
    for dt in (torch.float32, torch.float16, torch.float64, torch.bfloat16):
        assert bool(torch.isnan(v.view(dt)).all()), dt
    for dt in (torch.int8, torch.int16, torch.int32, torch.int64):
        assert bool((v.view(dt) == -1).all()), dt
    z = ss.guarded(64, ss.ZERO, "cpu", guard=64).view
    assert not bool(z.any()) and bool((z.view(torch.float32) == 0).all())


def test_leftover_is_the_given_bytes_cut_or_repeated():
    src = torch.arange(10, dtype=torch.float32)                       # 40 bytes
    short = ss.guarded(16, ss.LEFTOVER, "cpu", guard=64, leftover=src)
    assert torch.equal(short.view.view(torch.float32), src[:4])
    long = ss.guarded(100, ss.LEFTOVER, "cpu", guard=64, leftover=src)
    assert torch.equal(long.view[:40], src.view(torch.uint8)) and torch.equal(long.view[40:80], src.view(torch.uint8))
    assert torch.equal(long.view[80:], src.view(torch.uint8)[:20]) and long.damage() is None
    with pytest.raises(ValueError):
        ss.guarded(16, ss.LEFTOVER, "cpu", guard=64)
    with pytest.raises(ValueError):
        ss.guarded(16, "GARBAGE", "cpu", guard=64)


# ---- bit comparison ---------------------------------------------------------------------------------------------------------
def _f32_from_bits(*words):
    import numpy as np
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32))


def test_same_bits_tells_signed_zeros_and_nan_payloads_apart():
    pz, nz = torch.tensor([0.0]), torch.tensor([-0.0])
    assert bool(pz == nz) and not ss.same_bits(pz, nz) and ss.same_bits(nz, nz.clone())
    a, b = _f32_from_bits(0x7FC00000), _f32_from_bits(0x7FC00001)
    assert bool(torch.isnan(a)) and bool(torch.isnan(b))
    assert not torch.equal(a, a)                                      # what == makes of a NaN
    assert ss.same_bits(a, a.clone()) and not ss.same_bits(a, b)
    assert not ss.same_bits(torch.zeros(2), torch.zeros(3)) and not ss.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
    assert ss.same_bits(torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))


def test_the_reporter_names_tensor_count_and_first_index():
    want = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    assert ss.diff("w", want.clone(), want) is None
    got = want.clone()
    got[1, 0, 2] = -14.0
    got[1, 2, 3] = float("nan")
    line = ss.diff("grad.rgb", got, want)
    assert line.startswith("grad.rgb: 2 of 24 elements differ, first at (1, 0, 2): got -14.0") and "want 14.0" in line
    assert "0xc1600000" in line and "0x41600000" in line
    z = torch.zeros(3)
    nz = z.clone()
    nz[1] = -0.0
    assert "1 of 3" in ss.diff("z", nz, z) and "(1,)" in ss.diff("z", nz, z)
    assert "float64" in ss.diff("t", z.double(), z)
    lines = ss.diff_all("case fp32 ONES", {"a": got, "b": z}, {"a": want, "b": z})
    assert len(lines) == 1 and lines[0].startswith("case fp32 ONES: a: 2 of 24")
    assert ss.diff_all("c", {"a": z}, {"a": z, "b": z})[0].startswith("c: outputs")


# ---- the cases of the GPU tests: size functions ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_render_sizes(lib):
    seen = set()
    for prec, R, nc, ni, _ in ss.RENDER_CASES:
        need = lib.nsr_forward_rays_workspace_bytes_for(_lib.PRECISIONS[prec], R, nc, ni)
        assert need > 0, (prec, R, nc, ni)
        seen.add((prec, R, ni))
    assert len(seen) == 16                                           # four precisions x two ray counts x two importance counts
    for prec, R, nc, ni in ss.RENDER_REUSE:
        assert lib.nsr_forward_rays_workspace_bytes_for(_lib.PRECISIONS[prec], R, nc, ni) > 0
    big, small = (lib.nsr_forward_rays_workspace_bytes_for(_lib.PRECISIONS[p], R, nc, ni) for p, R, nc, ni in ss.RENDER_REUSE)
    assert big > small                                               # the small call really runs in a larger buffer


def _rays_per_pass(chunk, R):
    return chunk if 0 < chunk < R else R


def test_train_sizes(lib):
    R, nc, ni = ss.TRAIN_R, ss.TRAIN_NC, ss.TRAIN_NI
    for chunk in ss.TRAIN_CHUNKS:
        assert chunk % ss.TRAIN_S2 == 0
        if chunk:
            last = R % chunk
            assert 0 < last < chunk and last % ss.TRAIN_S2 == 0       # a ragged last pass of whole LR pixels
            assert (last * nc) % 32 == 0 and (chunk * nc) % 32 == 0   # ... inside the 32-point rule
    for _, prec, chunk in ss.TRAIN_CASES:
        p = _lib.TRAIN_PRECISIONS[prec]
        ws = lib.nsr_train_workspace_bytes_for(p, _rays_per_pass(chunk, R), nc, ni)
        sv = lib.nsr_train_saved_bytes(p, R, nc, ni, chunk)
        assert ws > 64 and sv > 0, (prec, chunk)
        assert ws <= lib.nsr_train_workspace_bytes(_rays_per_pass(chunk, R), nc, ni)
    # the patch of the reuse test: 64 rays in a buffer sized for 96
    for prec in ss.TRAIN_PRECISIONS:
        p = _lib.TRAIN_PRECISIONS[prec]
        assert 0 < lib.nsr_train_workspace_bytes_for(p, 64, nc, ni) < lib.nsr_train_workspace_bytes_for(p, 96, nc, ni)


def test_arch_sizes(lib):
    import ctypes
    from nerf_sr_amd.weights import normalize_arch
    arch = _lib.NsrArch.from_arch(normalize_arch(dict(ss.ARCH)))
    assert ss.ARCH["W"] % 32 != 0 and ss.ARCH["skips"]                # W != Wp and a skip layer
    R, nc, ni = ss.ARCH_R, 64, 64
    assert (R * nc) % 128 != 0                                        # ragged against the 128-point tiles
    for prec, embed, chunk in ss.ARCH_CASES:
        p = _lib.TRAIN_PRECISIONS[prec]
        ws = lib.nsr_train_arch_workspace_bytes_e(ctypes.byref(arch), embed, p, _rays_per_pass(chunk, R), nc, ni)
        sv = lib.nsr_train_arch_saved_bytes_e(ctypes.byref(arch), embed, p, R, nc, ni, chunk)
        assert ws > 64 and sv > 0, (prec, embed, chunk)
        if not embed:
            assert ws == lib.nsr_train_arch_workspace_bytes(ctypes.byref(arch), p, _rays_per_pass(chunk, R), nc, ni)
            assert sv == lib.nsr_train_arch_saved_bytes(ctypes.byref(arch), p, R, nc, ni, chunk)


def test_refine_sizes(lib):
    for prec, with_ref, (B, R, H, W) in ss.REFINE_CASES:
        need = lib.nsr_refine_workspace_bytes_for(_lib.PRECISIONS[prec], B, R if with_ref else 1, H, W)
        assert need > 0, (prec, with_ref, B, R, H, W)
    (B3, R3, H3, W3), (B9, R9, H9, W9) = ss.REFINE_SHAPES
    assert B3 % 8 != 0 and (B3 * R3) % 8 != 0 and (B9 * R9) % 8 == 1  # incomplete eight-image blocks
    for prec in ("fp32", "f16x3"):
        p = _lib.PRECISIONS[prec]
        assert lib.nsr_refine_workspace_bytes_for(p, B9, R9, H9, W9) > lib.nsr_refine_workspace_bytes_for(p, B3, R3, H3, W3)


def test_refine_train_sizes_and_ragged_sites(lib):
    for (prec, wgrad), tag, ic in ss.REFINE_TRAIN_CASES:
        B, R, H, W = ss.REFINE_TRAIN_SHAPES[tag]
        assert prec in rf.TRAIN_PRECISIONS and wgrad in rf.WEIGHT_GRADS
        assert lib.nsr_refine_train_workspace_bytes(B, R, H, W, ic) > 0 and lib.nsr_refine_train_saved_bytes(B, R, H, W) > 0
    # Which sites have M = nc * rows_img not a multiple of 32 (the `Kp > M` rows of the col matrix and the 32 zeroed rows behind
    # dZ are then read).  Sites 0..6: encoder on the synthesised patches (layers 0..6), 7..13: on the references, 14..25: decoder
    # (layers 7..18).  The deepest level (1 / 64 of the pixels: layer 6 and 7, 8) and the level above it (layers 4, 5, 9..11):
    deep = {6, 13, 14, 15}                       # E.conv7 (both calls), D.conv1, D.conv2
    mid = {4, 5, 11, 12, 16, 17, 18}             # E.conv5, E.conv6 (both calls), D.conv2_up, D.conv3, D.conv4
    # case A (2, 2, 16, 24), img_chunk 0 -> 4 images at once: rows per image 384 / 96 / 24 / 6.  Synthesised call and decoder
    # (2 images): M = 12 at the deepest level, 48 one above; reference call (4 images): M = 24 deepest, 96 above (a multiple)
    assert ss.refine_train_chunk(2, 2, 16, 24, 0) == 4
    assert set(ss.ragged_sites(2, 2, 16, 24, 0)) == deep | (mid - {11, 12})
    # img_chunk 1: M = 6 and 24 per image: every deep and mid site, the reference call's included
    assert set(ss.ragged_sites(2, 2, 16, 24, 1)) == deep | mid
    # case B (3, 1, 16, 16): rows per image 256 / 64 / 16 / 4; img_chunk 0 -> 3 images: M = 12 and 48; img_chunk 1: M = 4 and 16
    assert ss.refine_train_chunk(3, 1, 16, 16, 0) == 3
    assert set(ss.ragged_sites(3, 1, 16, 16, 0)) == deep | mid
    assert set(ss.ragged_sites(3, 1, 16, 16, 1)) == deep | mid
    ms = dict((s, m) for s, _, m in ss.refine_train_sites(3, 1, 16, 16, 0))
    assert ms[14] == [12] and ms[16] == [48] and ms[25] == [768] and ms[0] == [768]
    ms = dict((s, m) for s, _, m in ss.refine_train_sites(2, 2, 16, 24, 1))
    assert ms[13] == [6, 6, 6, 6] and ms[6] == [6, 6] and ms[12] == [24] * 4
    # the reuse test's first shape, fixture case C (2, 8, 16, 16), needs the larger workspace
    assert lib.nsr_refine_train_workspace_bytes(2, 8, 16, 16, 0) > lib.nsr_refine_train_workspace_bytes(3, 1, 16, 16, 0)


def test_metric_sizes(lib, golden_dir):
    import os
    import numpy as np
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    for tag in ss.METRIC_TAGS:
        B, C, H, W = g[f"x_{tag}"].shape
        assert lib.nsr_ssim_workspace_bytes(B, C, H, W) > 0
        assert lib.nsr_psnr_workspace_bytes(B, C * H * W) > 0
    for kind, (n_img, C) in ((_lib.NSR_LOSS_TV, (1, 3)), (_lib.NSR_LOSS_GRADIENT, (2, 3)), (_lib.NSR_LOSS_LAPLACIAN, (2, 1))):
        assert lib.nsr_loss_workspace_bytes(kind, n_img, C, 45, 70) > 0
    # the reuse test: a loss at 70 x 45 leaves more partial sums than SSIM at the `tiny` shape reads
    assert lib.nsr_loss_workspace_bytes(_lib.NSR_LOSS_LAPLACIAN, 2, 1, 45, 70) > lib.nsr_ssim_workspace_bytes(*g["x_tiny"].shape)
