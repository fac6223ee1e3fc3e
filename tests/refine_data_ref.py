"""numpy restatement of the refinement patch batches (include/nsr_refine_data.h): Pillow's 8-bit PERSPECTIVE + BILINEAR
transform operation by operation in double, the bounding-box rule, the reference's position ranges and the mapping of raw
random words onto them, the assembly of a sample.  The CPU tests hold it against Pillow itself and against what the reference's
own dataset class produced (tests/golden/refine_data.npz); the GPU tests hold the kernels against it."""
import numpy as np

IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
TRAIN, VAL = 0, 1


def warp_u8(img, coeffs):
    """``Image.fromarray(img).transform((W, H), Image.PERSPECTIVE, coeffs, Image.BILINEAR, fillcolor=0)`` of an (H, W, C) uint8
    image: every line below is one IEEE double operation per element (numpy never contracts)."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    a = [np.float64(v) for v in coeffs]
    xin = np.arange(W, dtype=np.float64)[None, :] + 0.5
    yin = np.arange(H, dtype=np.float64)[:, None] + 0.5
    with np.errstate(all="ignore"):
        den = a[6] * xin + a[7] * yin + 1.0
        xs = (a[0] * xin + a[1] * yin + a[2]) / den
        ys = (a[3] * xin + a[4] * yin + a[5]) / den
        inside = (xs >= 0.0) & (xs < W) & (ys >= 0.0) & (ys < H)
    xs = np.where(inside, xs, 0.5) - 0.5
    ys = np.where(inside, ys, 0.5) - 0.5
    fx, fy = np.floor(xs), np.floor(ys)
    dx, dy = (xs - fx)[..., None], (ys - fy)[..., None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    y0, y1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    p = img.astype(np.int64)
    p00, p01, p10, p11 = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
    v1 = p00 + (p01 - p00) * dx
    v2 = p10 + (p11 - p10) * dx
    v = v1 + (v2 - v1) * dy
    return np.where(inside[..., None], v.astype(np.int64), 0).astype(np.uint8)       # (UINT8) v: truncation


def normalize(u8):
    """ToTensor + Normalize(0.5, 0.5) of (..., H, W, 3) bytes -> (..., 3, H, W) fp32: three fp32 operations per value."""
    t = np.moveaxis(np.asarray(u8), -1, -3).astype(np.float32)
    return (t / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)


def aug_bbox(img, coeffs):
    """x0, y0, x1 + 1, y1 + 1 around the destination pixels whose warped pixel has a non-zero channel; zeros if there is none."""
    nz = warp_u8(img, coeffs).any(axis=2)
    if not nz.any():
        return np.zeros(4, dtype=np.int32)
    ys, xs = np.nonzero(nz)
    return np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], dtype=np.int32)


def start_ranges(box, P):
    wl, hl, wh, hh = (int(v) for v in box)
    return (wl, wh - P), (hl, hh - P)


def ref_ranges(box, x, y, P, off, mode):
    """[lo, hi) of a reference patch's ref_x and ref_y (llff_refine_dataset.py:227-234; 'val': :247-252 with get_start_pos's
    extra ``- patch_len``)."""
    wl, hl, wh, hh = (int(v) for v in box)
    if mode == VAL:
        off, cut = P, P
    else:
        cut = 0
    return (max(wl, x - off), min(wh - P, x + off) - cut), (max(hl, y - off), min(hh - P, y + off) - cut)


def all_ranges(box, x, y, P, R, off, mode, with_gt):
    """The 2 + 2R + 1 ranges of a sample's position words given its x, y; the last one is None without with_gt_patch."""
    rx, ry = ref_ranges(box, x, y, P, off, mode)
    return list(start_ranges(box, P)) + [rx, ry] * R + [(0, R) if with_gt else None]


def positions_from_draws(words, box, P, R, off, mode, with_gt):
    """lo + word % (hi - lo) per word, in the reference's order; None where a range is empty or a word negative."""
    words = [int(w) for w in words]
    out = []
    for k, (lo, hi) in enumerate(start_ranges(box, P)):
        if words[k] < 0 or hi <= lo:
            return None
        out.append(lo + words[k] % (hi - lo))
    for k, rng in enumerate(all_ranges(box, out[0], out[1], P, R, off, mode, with_gt)[2:], start=2):
        if rng is None:
            out.append(-1)
            continue
        lo, hi = rng
        if words[k] < 0 or hi <= lo:
            return None
        out.append(lo + words[k] % (hi - lo))
    return np.array(out, dtype=np.int32)


def starts_valid(starts, box, P, R, off, mode, with_gt, W, H):
    wl, hl, wh, hh = (int(v) for v in box)
    if not (0 <= wl <= wh <= W and 0 <= hl <= hh <= H):
        return False
    s = [int(v) for v in starts]
    (xl, xh), (yl, yh) = start_ranges(box, P)
    if not (xl <= s[0] < xh and yl <= s[1] < yh):
        return False
    for v, rng in zip(s, all_ranges(box, s[0], s[1], P, R, off, mode, with_gt)):
        if rng is not None and not rng[0] <= v < rng[1]:
            return False
    return True


def sample(gt_u8, sr_u8, ref_u8, coeffs, starts, P, R, with_gt, warped=None):
    """One sample from explicit positions: sr_patch, gt_patch (3, P, P), ref_patches (R, 3, P, P).  ``warped``: the pair of warped
    8-bit images if the caller already has them."""
    s = [int(v) for v in starts]
    wgt, wsr = warped if warped is not None else (warp_u8(gt_u8, coeffs), warp_u8(sr_u8, coeffs))
    x, y = s[0], s[1]
    sr_patch, gt_patch = normalize(wsr[y:y + P, x:x + P]), normalize(wgt[y:y + P, x:x + P])
    refs = [normalize(ref_u8[s[3 + 2 * k]:s[3 + 2 * k] + P, s[2 + 2 * k]:s[2 + 2 * k] + P]) for k in range(R)]
    if with_gt:
        refs[s[2 + 2 * R]] = gt_patch
    return sr_patch, gt_patch, np.stack(refs)


def perspective_coeffs(startpoints, endpoints):
    a = np.zeros((8, 8), dtype=np.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i] = [p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]]
        a[2 * i + 1] = [0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]]
    return np.linalg.solve(a, np.asarray(startpoints, dtype=np.float64).reshape(8))
