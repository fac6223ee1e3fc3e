"""The one network descriptor of the Python layer (nerf_sr_amd/weights.py, ``_lib.NsrArch.from_arch``): the default network
is ``arch_spec()`` at its defaults, one generator draws every synthetic network, one function normalises an architecture.

The SHA-256 digests below were computed with the two separate generators this module replaced (``make_state_dict`` over its own
24-entry table, ``make_state_dict_arch`` over ``arch_spec``), one commit before they were merged: a seed's arrays must never
change, since every golden fixture names its networks by seed."""
import hashlib

import numpy as np
import pytest

from nerf_sr_amd import _lib
from nerf_sr_amd.weights import (DIR_W, STATE_DICT_SPEC, arch_spec, check_state_dict, make_state_dict, make_state_dict_arch,
                                 normalize_arch)
from tests import arch_util as au

DEFAULT_TABLE = [
    ("xyz_encoding_1.0.weight", (256, 63)), ("xyz_encoding_1.0.bias", (256,)),
    ("xyz_encoding_2.0.weight", (256, 256)), ("xyz_encoding_2.0.bias", (256,)),
    ("xyz_encoding_3.0.weight", (256, 256)), ("xyz_encoding_3.0.bias", (256,)),
    ("xyz_encoding_4.0.weight", (256, 256)), ("xyz_encoding_4.0.bias", (256,)),
    ("xyz_encoding_5.0.weight", (256, 319)), ("xyz_encoding_5.0.bias", (256,)),
    ("xyz_encoding_6.0.weight", (256, 256)), ("xyz_encoding_6.0.bias", (256,)),
    ("xyz_encoding_7.0.weight", (256, 256)), ("xyz_encoding_7.0.bias", (256,)),
    ("xyz_encoding_8.0.weight", (256, 256)), ("xyz_encoding_8.0.bias", (256,)),
    ("xyz_encoding_final.weight", (256, 256)), ("xyz_encoding_final.bias", (256,)),
    ("dir_encoding.0.weight", (128, 283)), ("dir_encoding.0.bias", (128,)),
    ("sigma.weight", (1, 256)), ("sigma.bias", (1,)),
    ("rgb.0.weight", (3, 128)), ("rgb.0.bias", (3,)),
]

FIELD_DIGESTS = {
    (99, "plain"): "ca4357b603b33e649030134e3af2acc0a683ebb2dda9d32e2ef514eb6c5dfd5e",
    (99, "smooth"): "4a7f56ddd5237591c3494f3ea2e334e307599ad3cbd2db2542c8c1bc8468a26f",
    (99, "sharp"): "1927af29fd32c54ccc3d339cb1f372286c11ccec96d813df75a0da7c031c2db9",
    (100, "plain"): "297ecc7ac89cb8fa9fa67c247b90cf444955f30f410dd068250eec05c2e9ed2d",
    (100, "smooth"): "b01bf9390136020e5a883d2a26558c57e342d37fca3adda9721b05147eddbb3f",
    (100, "sharp"): "ad17efb82f1641fe2861b4488b71bdaab0269def34cd7ebffe73452f33a3a7ee",
}
# tests/arch_util.CASES with the seeds of tests/golden/train_arch.npz (coarse, fine)
ARCH_DIGESTS = {
    ("small", 21): "017ce7fb22fc3722ef4a5eade5524fa0ad6df095c95675e3c1bdbeb83a886bdd",
    ("small", 22): "91be59a39e21c743de935124d3f27f9bec067b4ec1a86c601039859150f7ba5d",
    ("odd", 21): "5bb883c6bcd90a0bf401d2b55b877f8ea85595690b3848f09f5c7d9706ed4627",
    ("odd", 22): "35c35cc9e332baf578e483d6ac3af01ecd3a515d74979022fc2c638b28ecd6f5",
    ("nodir", 21): "255a38f1d9cf6c4e662fdfe05f4e1e723aa541d1eb46e75ba6d1aa21660f59c8",
    ("nodir", 22): "47b366a90aa55115397b3edcbc4d48793665396e2937de1437d4b64d81ae5a25",
    ("odd_dense", 22): "35c35cc9e332baf578e483d6ac3af01ecd3a515d74979022fc2c638b28ecd6f5",
    ("odd_dense", 23): "836e721137b3399d1402600fb36cea8f3d3c506ec52c9f6b4ddbc7694cf98e77",
}
DEFAULT_NO_DIR_99 = "ecd1137d5edc91115cd244f9293afc8a5dba9882244446d2e43018bd2a03c40f"     # make_state_dict_arch(99, no_dir=True)


def digest(sd):
    """SHA-256 over the concatenated bytes of all arrays, in key order."""
    return hashlib.sha256(b"".join(np.ascontiguousarray(v).tobytes() for v in sd.values())).hexdigest()


def test_default_spec_is_the_literal_table():
    assert list(arch_spec().items()) == DEFAULT_TABLE
    assert list(STATE_DICT_SPEC.items()) == DEFAULT_TABLE


@pytest.mark.parametrize("seed,field", list(FIELD_DIGESTS))
def test_default_weights_keep_their_bits(seed, field):
    sd = make_state_dict(seed, field)
    assert [(k, v.shape, v.dtype) for k, v in sd.items()] == [(k, s, np.float32) for k, s in DEFAULT_TABLE]
    assert digest(sd) == FIELD_DIGESTS[(seed, field)]


@pytest.mark.parametrize("tag", au.CASES)
def test_arch_weights_keep_their_bits(golden_dir, tag):
    g = au.load_case(golden_dir, tag)
    for seed in (g["seed_coarse"], g["seed_fine"]):
        sd = make_state_dict_arch(seed, **g["arch"])
        assert [(k, v.shape) for k, v in sd.items()] == list(arch_spec(**g["arch"]).items())
        assert digest(sd) == ARCH_DIGESTS[(tag, seed)]


def test_default_and_no_dir_fronts_of_the_one_generator():
    assert digest(make_state_dict_arch(99)) == FIELD_DIGESTS[(99, "smooth")]       # the default architecture = make_state_dict
    nd = make_state_dict_arch(99, no_dir=True)
    assert nd[DIR_W].shape == (128, 256) and digest(nd) == DEFAULT_NO_DIR_99


def test_normalize_arch():
    a = normalize_arch({"D": 6, "W": 192, "skips": [4, 4, 2]})
    assert a["skips"] == (2, 4) and a == {"D": 6, "W": 192, "skips": (2, 4), "deg_pos": 10, "deg_dir": 4, "dim_rgb": 3, "no_dir": False}
    assert normalize_arch(None) == normalize_arch({}) and list(arch_spec(**normalize_arch(None)).items()) == DEFAULT_TABLE
    assert normalize_arch(None, no_dir=1, skips=[3])["no_dir"] is True and normalize_arch(None, skips=[3])["skips"] == (3,)
    for D in (4, 8):
        for bad in (0, D):
            with pytest.raises(ValueError):
                normalize_arch({"D": D, "skips": [bad]})
            with pytest.raises(ValueError):
                normalize_arch(None, D=D, skips=(2, bad))


def test_descriptor_struct_from_arch():
    d = _lib.NsrArch.from_arch(normalize_arch(None))
    assert (d.D, d.W, d.skips, d.deg_pos, d.deg_dir, d.no_dir) == (8, 256, 1 << 4, 10, 4, 0)
    d = _lib.NsrArch.from_arch(normalize_arch({"D": 6, "W": 192, "skips": [3, 1], "no_dir": True}))
    assert d.skips == (1 << 1) | (1 << 3) and d.no_dir == 1


def test_check_state_dict_is_the_arch_check_at_the_default():
    full = make_state_dict(3)
    narrow = dict(full)
    narrow[DIR_W] = full[DIR_W][:, :256].copy()
    check_state_dict(full)
    check_state_dict(narrow, no_dir=True)
    for sd, kw in ((narrow, {}), (full, {"no_dir": True})):
        with pytest.raises(ValueError, match="dir_encoding.0.weight"):
            check_state_dict(sd, **kw)
    with pytest.raises(ValueError, match=r"\(128, 283\).*\(128, 256\).*no_dir network"):      # found, expected, the suffix
        check_state_dict(full, no_dir=True)
    short = dict(full)
    del short["sigma.bias"]
    with pytest.raises(ValueError, match="missing keys.*sigma.bias"):
        check_state_dict(short)
