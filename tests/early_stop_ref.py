"""Emulation of the early-ray-termination rule of include/nsr.h on the (rgb, sigma, z) of WHOLE rays, independent of any kernel
(numpy, fp32): used by tests/test_early_stop_cpu.py on the oracle's own render to pin the derivation of the bound, by
tests/test_gpu_early_stop.py to predict the kernel's counter from the raw densities of the two-call route, and by
scripts/early_stop_stats.py.

The rule.  Rays are taken in groups of four consecutive ones (the last group may hold fewer) and walked front to back in
windows of 32 samples.  After window w (w + 1 < N / 32) a ray's optical depth is
``tau_w = sum_{k < 32 (w + 1)} relu(sigma_k) (z_{k+1} - z_k)`` (fp32; the last delta reaches into the next window); the group
ends when ``tau_w >= -ln(eps)`` for every ray present.  NaN never terminates.  The windows behind the cut are not evaluated:
their (r, g, b, sigma) become 0.

Summation order is left open by the definition, so a comparison that lands within ``MARGINAL`` (relative) of the threshold
is not decided by it: such (group, window) pairs are reported as *marginal*, and ``n_cut_lo`` / ``n_cut_hi`` are the counts
with every comparison inside that band resolved against / for a cut.  (fp32 sums of 128 non-negative terms in two orders
differ by < 128 * 2^-24 = 8e-6 relative, far inside the band.)"""
from __future__ import annotations

import math
from typing import NamedTuple, Set, Tuple

import numpy as np

MARGINAL = 1e-4
GROUP, WINDOW = 4, 32


class Truncated(NamedTuple):
    rgb: np.ndarray          # (R, N, 3), zero behind every group's cut
    sigma: np.ndarray        # (R, N), the same
    n_cut: int               # windows not evaluated, over all groups
    n_cut_lo: int            # ... with every marginal comparison resolved against the cut
    n_cut_hi: int            # ... and for it
    marginal: Set[Tuple[int, int]]   # (group, window) with |tau_w / -ln(eps) - 1| < MARGINAL for a ray present
    last_window: np.ndarray  # (ceil(R / 4),): index of the last window each group evaluates
    n_cut_single_ray: int    # for contrast: windows of SINGLE rays (32 samples) a per-ray rule would not evaluate


def threshold(eps: float) -> np.float32:
    """-ln(eps) made in double and rounded to fp32, as the entry points make it."""
    if not (0.0 < float(eps) < 1.0):
        raise ValueError("eps must be in (0, 1)")
    return np.float32(-math.log(float(eps)))


def optical_depth(sigma: np.ndarray, z: np.ndarray) -> np.ndarray:
    """(R, N / 32 - 1): tau_w for w = 0 .. N / 32 - 2, fp32, relu that keeps a NaN."""
    sigma, z = np.asarray(sigma, np.float32), np.asarray(z, np.float32)
    R, N = sigma.shape
    assert z.shape == (R, N) and N % WINDOW == 0
    dens = np.where(sigma <= 0, np.float32(0), sigma)                    # NaN <= 0 is False: a NaN stays
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (dens[:, :N - 1] * (z[:, 1:] - z[:, :-1])).astype(np.float32)
        tau = np.cumsum(terms, axis=1, dtype=np.float32)
    return tau[:, WINDOW - 1::WINDOW][:, :N // WINDOW - 1]


def _first_done(done: np.ndarray, n_windows: int) -> np.ndarray:
    """index of the last window evaluated, from the (G, W - 1) table "the group is finished after window w" """
    any_done = done.any(axis=1)
    return np.where(any_done, done.argmax(axis=1), n_windows - 1)


def truncate(rgb, sigma, z, eps: float) -> Truncated:
    rgb = np.array(rgb, dtype=np.float32, copy=True)
    sigma = np.array(sigma, dtype=np.float32, copy=True)
    z = np.asarray(z, np.float32)
    R, N = sigma.shape
    W = N // WINDOW
    thr = threshold(eps)
    tau = optical_depth(sigma, z)                                        # (R, W - 1)
    pad = (-R) % GROUP
    if pad:                                                              # a ray past the end of the batch counts as terminated
        tau = np.concatenate([tau, np.full((pad, W - 1), np.inf, np.float32)])
    G = tau.shape[0] // GROUP
    tau_g = tau.reshape(G, GROUP, W - 1)
    with np.errstate(invalid="ignore"):
        done = (tau_g >= thr).all(axis=1)                                # NaN >= thr is False
        done_lo = (tau_g >= thr * np.float32(1 + MARGINAL)).all(axis=1)
        done_hi = (tau_g >= thr * np.float32(1 - MARGINAL)).all(axis=1)
        near = np.abs(tau_g.astype(np.float64) / float(thr) - 1.0) < MARGINAL
        single = (tau[:R] >= thr)
    marginal = {(int(g), int(w)) for g, w in zip(*np.nonzero(near.any(axis=1)))}
    last = _first_done(done, W)
    for g in range(G):
        if last[g] + 1 < W:
            rows = slice(GROUP * g, min(GROUP * g + GROUP, R))
            rgb[rows, WINDOW * (last[g] + 1):] = 0
            sigma[rows, WINDOW * (last[g] + 1):] = 0
    n = lambda l: int((W - 1 - l).sum())
    return Truncated(rgb, sigma, n(last), n(_first_done(done_lo, W)), n(_first_done(done_hi, W)), marginal, last,
                     n(_first_done(single, W)))


def bounds(eps: float, z) -> Tuple[float, float]:
    """(bound on |d comp_rgb| and |d opacity|, per-ray bound on |d depth|) of include/nsr.h for threshold eps."""
    b = float(eps) + 2e-6
    return b, b * np.abs(np.asarray(z, np.float64)).max(axis=1)
