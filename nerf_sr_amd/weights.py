"""Weight interface of the render hot path.

The reference hands the NeRF MLP to the path as the 24-tensor ``state_dict()``
of ``VanillaMLP`` (reference ``models/networks.py:131-180``; checkpoint writer
``models/base_model.py:181-196``).  nn.Linear layout: ``weight`` is
``(out, in)`` row-major, ``y = x @ W.T + b``.

This module owns
  * the key/shape table of that state_dict for any architecture (``arch_spec``; ``STATE_DICT_SPEC`` is the default's),
  * a deterministic, seedable generator for synthetic weights (no checkpoints
    can be downloaded), used by tests, the golden-vector script and
    ``bench.py`` so that no weight blob has to be committed.

Everything here is numpy; nothing touches the GPU.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

# Architecture constants of the path (reference defaults):
#   D=8, W=256, skips=[4]  (models/networks.py:124-126)
#   deg_pos=10, deg_dir=4  (models/nerf_model.py:56-57)
D_LAYERS = 8
WIDTH = 256
SKIP_LAYER = 4            # 0-based index of the trunk layer whose input is cat([pe, h])
DEG_POS = 10
DEG_DIR = 4
POS_CH = 3 + 3 * 2 * DEG_POS   # 63
DIR_CH = 3 + 3 * 2 * DEG_DIR   # 27
IN_CH = POS_CH + DIR_CH        # 90
MACS_PER_POINT = 593_408
FLOP_PER_POINT = 2 * MACS_PER_POINT


# ---------------------------------------------------------------------------------------------------------------------
# The architecture flags of VanillaMLP (models/networks.py:124-128 --D --W --skips --no_dir; models/nerf_model.py:53-57
# --dim_rgb --deg_pos --deg_dir).  The fused kernels are laid out for the defaults above; any other value runs layer by
# layer (ops.GenericMLP).
# ---------------------------------------------------------------------------------------------------------------------
def arch_of(opt=None) -> dict:
    """The architecture values of an options object (absent ones = the reference's defaults)."""
    g = (lambda k, d: getattr(opt, k, d)) if opt is not None else (lambda k, d: d)
    return {"D": int(g("D", D_LAYERS)), "W": int(g("W", WIDTH)), "skips": tuple(int(s) for s in g("skips", (SKIP_LAYER,))),
            "deg_pos": int(g("deg_pos", DEG_POS)), "deg_dir": int(g("deg_dir", DEG_DIR)), "dim_rgb": int(g("dim_rgb", 3)),
            "no_dir": bool(g("no_dir", False))}


EMBED_NO_XYZ, EMBED_LINEAR_FREQS = 1, 2      # include/nsr.h: NSR_EMBED_NO_XYZ, NSR_EMBED_LINEAR_FREQS


def embed_of(opt=None) -> int:
    """The embedding's option word of an options object (models/embedding.py:17-18 ``--no_xyz``, ``--no_logscale``; absent
    options = 0, the reference's defaults).  It travels NEXT TO the architecture dict, whose keys stay as they are."""
    if opt is None:
        return 0
    return (EMBED_NO_XYZ if bool(getattr(opt, "no_xyz", False)) else 0) | \
        (EMBED_LINEAR_FREQS if bool(getattr(opt, "no_logscale", False)) else 0)


def embed_names(embed: int) -> str:
    """The reference's flag names of an option word, for messages."""
    return " ".join(n for bit, n in ((EMBED_NO_XYZ, "--no_xyz"), (EMBED_LINEAR_FREQS, "--no_logscale")) if embed & bit)


def check_embed(embed: int, arch: dict) -> int:
    """``ValueError`` for a word the library refuses (include/nsr.h): an unknown bit, ``--no_xyz`` on an encoding of degree 0 that
    the network reads.  Host only; returns the word."""
    embed = int(embed)
    if embed & ~(EMBED_NO_XYZ | EMBED_LINEAR_FREQS):
        raise ValueError(f"embed={embed:#x}: an OR of EMBED_NO_XYZ (1) and EMBED_LINEAR_FREQS (2)")
    if embed & EMBED_NO_XYZ and (arch["deg_pos"] == 0 or (arch["deg_dir"] == 0 and not arch["no_dir"])):
        raise ValueError("no_xyz with an encoding of degree 0 leaves a layer without input columns "
                         "(deg_pos must be >= 1, and deg_dir unless no_dir): the reference cannot build that network either")
    return embed


def is_default_arch(arch: dict) -> bool:
    """True when the fused kernels cover it (``no_dir`` rides them too: weights.pad_no_dir)."""
    return all(arch[k] == v for k, v in (("D", D_LAYERS), ("W", WIDTH), ("skips", (SKIP_LAYER,)), ("deg_pos", DEG_POS),
                                          ("deg_dir", DEG_DIR), ("dim_rgb", 3)))


def arch_spec(D=D_LAYERS, W=WIDTH, skips=(SKIP_LAYER,), deg_pos=DEG_POS, deg_dir=DEG_DIR, dim_rgb=3, no_dir=False, no_xyz=False):
    """key -> shape of ``VanillaMLP(opt).state_dict()`` for these flags, in the module's own order (models/networks.py:131-180).
    ``no_xyz`` (models/embedding.py:17): the encodings lose their 3 identity columns (models/networks.py:143-163)."""
    if D < 1 or W < 2 or W % 2 or deg_pos < 0 or deg_dir < 0 or dim_rgb < 1 or any(s < 1 or s >= D for s in skips):
        raise ValueError("D >= 1, even W >= 2, degrees >= 0, dim_rgb >= 1 and skip layers inside 1 .. D - 1 "
                         "(a skip at layer 0 would double the input: the reference's constructor gives layer 0 the plain width)")
    in_xyz, in_dir = (0 if no_xyz else 3) + 6 * deg_pos, (0 if no_xyz else 3) + 6 * deg_dir
    spec = OrderedDict()
    for i in range(D):
        fan_in = in_xyz if i == 0 else (W + in_xyz if i in skips else W)
        spec[f"xyz_encoding_{i + 1}.0.weight"] = (W, fan_in)
        spec[f"xyz_encoding_{i + 1}.0.bias"] = (W,)
    spec["xyz_encoding_final.weight"] = (W, W)
    spec["xyz_encoding_final.bias"] = (W,)
    spec["dir_encoding.0.weight"] = (W // 2, W + (0 if no_dir else in_dir))
    spec["dir_encoding.0.bias"] = (W // 2,)
    spec["sigma.weight"] = (1, W)
    spec["sigma.bias"] = (1,)
    spec["rgb.0.weight"] = (dim_rgb, W // 2)
    spec["rgb.0.bias"] = (dim_rgb,)
    return spec


def normalize_arch(arch=None, **overrides) -> dict:
    """The dict ``arch_spec`` takes, from a dict with any of its keys or an options object carrying the reference's flags
    (absent ones = the reference's defaults), then ``overrides``: ints, skips sorted and de-duplicated; validated
    (``ValueError``) through ``arch_spec``."""
    a = {**arch_of(None), **arch} if isinstance(arch, dict) else arch_of(arch)
    a.update(overrides)
    for k in ("D", "W", "deg_pos", "deg_dir", "dim_rgb"):
        a[k] = int(a[k])
    a["skips"] = tuple(sorted(set(int(s) for s in a["skips"])))
    a["no_dir"] = bool(a["no_dir"])
    arch_spec(**a)
    return a


def arch_key(arch: dict, no_dir: bool = False) -> tuple:
    """What the warn-once sets remember an architecture by: (D, W, skips, deg_pos, deg_dir), plus ``no_dir`` if asked."""
    key = (arch["D"], arch["W"], tuple(arch["skips"]), arch["deg_pos"], arch["deg_dir"])
    return key + (bool(arch["no_dir"]),) if no_dir else key


#: key -> shape, in the order ``VanillaMLP.state_dict()`` yields them: the default architecture's table
STATE_DICT_SPEC = arch_spec()
N_PARAMS = sum(int(np.prod(s)) for s in STATE_DICT_SPEC.values())
assert N_PARAMS == 595_844
assert sum(int(np.prod(s)) for k, s in STATE_DICT_SPEC.items() if k.endswith("weight")) == MACS_PER_POINT

DIR_W = "dir_encoding.0.weight"          # (128, 256 + 27); (128, 256) in a --no_dir network (models/networks.py:160-169)


def _check(sd, spec, note: str) -> None:
    missing = [k for k in spec if k not in sd]
    if missing:
        raise ValueError(f"state_dict is missing keys: {missing}")
    for k, shape in spec.items():
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"state_dict[{k!r}] has shape {tuple(sd[k].shape)}, expected {tuple(shape)}{note}")


def check_state_dict_arch(sd, no_xyz: bool = False, **arch) -> None:
    """Raise ``ValueError`` unless ``sd`` has exactly the keys and shapes of ``arch_spec(**arch)`` (``no_xyz``: of the ``--no_xyz``
    network, and the message says so)."""
    _check(sd, arch_spec(no_xyz=no_xyz, **arch), f" for {arch}" + (" with --no_xyz" if no_xyz else ""))


def check_state_dict(sd, no_dir: bool = False) -> None:
    """Raise ``ValueError`` unless ``sd`` has exactly the 24 keys/shapes of the path (``no_dir``: of the ``--no_dir``
    variant, whose ``dir_encoding`` layer sees ``xyz_encoding_final`` alone)."""
    _check(sd, arch_spec(no_dir=no_dir), " (no_dir network)" if no_dir else "")


def pad_no_dir(w):
    """``--no_dir`` (models/networks.py:160-169, 213-216): ``dir_encoding`` is Linear(256, 128) on ``xyz_encoding_final``
    alone.  The kernels are laid out for the (128, 283) layer over ``cat([final, dir_pe])``: the same function with 27
    ZERO columns behind the 256 -- every product with them is an exact 0, so the outputs are those of the narrow layer
    bit for bit in any accumulation order.  Works on numpy arrays and torch tensors."""
    if isinstance(w, np.ndarray):
        return np.concatenate([w, np.zeros((w.shape[0], 27), dtype=w.dtype)], 1)
    import torch
    return torch.cat([w, torch.zeros(w.shape[0], 27, dtype=w.dtype, device=w.device)], 1)


#: synthetic density-field presets: (spectral decay of the PE input columns, sigma.weight scale, sigma.bias)
FIELDS = {
    "plain": (0.0, 1.0, None),     # kaiming only: fog everywhere, every ray saturates
    "smooth": (1.0, 10.0, -3.0),   # default: 1/f spectrum, ~45 % empty samples, opacity varies ray to ray
    "sharp": (0.0, 30.0, -40.0),   # stress: white spectrum x30 density head, chaotic under fp32 rounding
}


def _generate(seed: int, field: str, bias_scale: float, arch: dict, no_xyz: bool = False):
    """One draw per tensor in ``arch_spec`` order (so a seed's arrays never change), then the field preset."""
    if field not in FIELDS:
        raise ValueError(f"field must be one of {list(FIELDS)}")
    decay, sigma_scale, sigma_bias = FIELDS[field]
    a = normalize_arch(arch)
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for key, shape in arch_spec(no_xyz=no_xyz, **a).items():
        scale = np.sqrt(2.0 / shape[1]) if key.endswith("weight") else bias_scale
        sd[key] = (rng.standard_normal(shape, dtype=np.float64) * scale).astype(np.float32)
    if decay > 0:
        c0 = 0 if no_xyz else 3                 # first band column
        for i in (0,) + a["skips"]:             # the layers that read the positional encoding, in their first columns
            for k in range(a["deg_pos"]):
                sd[f"xyz_encoding_{i + 1}.0.weight"][:, c0 + 6 * k: c0 + 6 + 6 * k] *= np.float32(2.0 ** (-decay * k))
    sd["sigma.weight"] = (sd["sigma.weight"] * np.float32(sigma_scale)).astype(np.float32)
    if sigma_bias is not None:
        sd["sigma.bias"] = np.full((1,), sigma_bias, dtype=np.float32)
    return sd


def make_state_dict(seed: int = 99, field: str = "smooth", bias_scale: float = 0.05):
    """Deterministic synthetic ``VanillaMLP`` weights as ``{key: float32 ndarray}``.

    ``W ~ N(0, 2/fan_in)`` mirrors ``init_type=kaiming`` of the reference
    (``models/networks.py:31-38``: kaiming_normal_, fan_in, a=0).  The reference
    zero-inits biases; a small non-zero bias (``bias_scale``) is used here so
    that bias handling of the kernels is actually exercised by the parity tests.

    ``field`` shapes the random density field so that renders are non-trivial
    (no dataset or checkpoint is reachable offline):

    * ``"smooth"`` (default) scales the positional-encoding columns of octave k in
      the two layers that read them (``xyz_encoding_1``, ``xyz_encoding_5``) by
      ``2^-k`` — a 1/f spectrum, band-limited at the sample spacing like a trained
      scene — and sets ``sigma.weight *= 10, sigma.bias = -3``: ~45 % of the
      samples are empty, opacity mean 0.3-0.9 with std ~0.3 across rays.  On this
      field the reference algorithm itself is well conditioned (fp32 vs fp64
      oracle differ by < 1e-5 RGB), so an all-rays 1e-4 parity bound is meaningful.
    * ``"sharp"`` (white spectrum, ``sigma.weight *= 30, sigma.bias = -40``) is a
      stress field: the reference's ``denom < 1e-5 -> 1`` snap
      (``models/utils.py:87-88``) and the 1/pdf amplification of the inverse CDF
      make its own fp32 and fp64 results differ by > 1e-2 on ~5 % of the rays, so
      only statistical parity can be asked of it.
    * ``"plain"``: kaiming weights only.
    """
    return _generate(seed, field, bias_scale, {})


def make_state_dict_arch(seed: int, bias_scale: float = 0.05, no_xyz: bool = False, **arch):
    """``make_state_dict``'s "smooth" field for any architecture ``arch_spec`` describes: kaiming weights, small biases, the
    density head (``sigma.weight`` x 10, ``sigma.bias`` -3) and 1/f positional-encoding columns.  ``no_xyz``: the shapes of the
    ``--no_xyz`` network (one draw per tensor in the same order)."""
    return _generate(seed, "smooth", bias_scale, arch, no_xyz)
