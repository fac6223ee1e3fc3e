"""Python mirrors of the encoding panels' row order (csrc/nsr_mlp_layout.h, csrc/nsr_panels.h), shared by
tests/test_gpu_encoding.py (the TRAIN forward writes the panels) and tests/train_reduce_ref.py (the weight gradients read them)."""
import numpy as np


def pecol(t, h):                 # csrc/nsr_mlp_layout.h: the column register t of lane half h holds (None: padding)
    if t == 0:
        return 0 if h == 0 else 2
    if t == 1:
        return 1 if h == 0 else None
    return 3 + 30 * h + (t - 2)


def dircol(t, h):
    if t == 0:
        return 0 if h == 0 else 2
    if t == 1:
        return 1 if h == 0 else None
    if t >= 14:
        return None
    return 3 + 12 * h + (t - 2)


def enc_row(t, h):               # csrc/nsr_panels.h
    return 32 * (t >> 4) + 16 * ((t >> 3) & 1) + 8 * ((t >> 2) & 1) + 4 * h + (t & 3)


def panel_rows(rows, n_regs, col_of, col0):
    """(P, 64) float16: the encoding panel's rows in enc_row() order; rows no register maps to stay zero."""
    out = np.zeros((rows.shape[0], 64), dtype=np.float16)
    used = set()
    for t in range(n_regs):
        for h in (0, 1):
            c = col_of(t, h)
            r = enc_row(t, h)
            assert r not in used
            used.add(r)
            if c is not None:
                out[:, r] = rows[:, col0 + c].astype(np.float16)
    return out, used
