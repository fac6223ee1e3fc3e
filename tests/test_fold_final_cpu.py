"""The identity behind the fold of ``xyz_encoding_final`` into ``dir_encoding`` (csrc/nsr_mlp_layout.h), in torch
fp64, and the emulation of the folded kernel that scripts/study_fold_final.py evaluates.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from nerf_sr_amd.weights import make_state_dict
from oracle import nerf_oracle as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def study():
    spec = importlib.util.spec_from_file_location("study_fold_final", os.path.join(REPO, "scripts", "study_fold_final.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _points(n=96, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.cat([oc.posenc(torch.rand(n, 3, generator=gen) * 2 - 1, 10),
                      oc.posenc(torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1), 4)], -1).double()


def _structured(kind):
    sd = make_state_dict(7)
    if kind == "zero":
        sd["xyz_encoding_final.weight"] = np.zeros((256, 256), np.float32)
    elif kind == "identity":
        sd["xyz_encoding_final.weight"] = np.eye(256, dtype=np.float32)
    elif kind == "no_dir":
        sd["dir_encoding.0.weight"] = np.ascontiguousarray(sd["dir_encoding.0.weight"][:, :256])
    elif kind != "random":
        raise ValueError(kind)
    return sd


@pytest.mark.parametrize("kind", ["random", "zero", "identity", "no_dir"])
def test_fold_identity_fp64(kind):
    """relu(W' h8 + W_dir[:, 256:] de + b') is dir_encoding(cat([W_f h8 + b_f, de])): the whole network's output in fp64."""
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in _structured(kind).items()}
    wd, wf = sd["dir_encoding.0.weight"], sd["xyz_encoding_final.weight"]
    folded = dict(sd)
    folded["dir_encoding.0.weight"] = torch.cat([wd[:, :256] @ wf, wd[:, 256:]], 1)
    folded["dir_encoding.0.bias"] = sd["dir_encoding.0.bias"] + wd[:, :256] @ sd["xyz_encoding_final.bias"]
    folded["xyz_encoding_final.weight"] = torch.eye(256, dtype=torch.float64)
    folded["xyz_encoding_final.bias"] = torch.zeros(256, dtype=torch.float64)
    assert folded["dir_encoding.0.weight"].shape == wd.shape
    x = _points()
    want, got = oc.mlp_forward(sd, x), oc.mlp_forward(folded, x)
    assert torch.equal(got[:, 3], want[:, 3])                      # the density never sees the colour branch
    assert float((got[:, :3] - want[:, :3]).abs().max()) <= 1e-14
    if kind == "zero":                                             # b' alone carries the layer
        assert float(folded["dir_encoding.0.weight"][:, :256].abs().max()) == 0.0


def test_study_fold_matches_fp64(study):
    sd = make_state_dict(7)
    w64, b64 = study.fold(sd, "fp64")
    w32, b32 = study.fold(sd, "fp32")
    wd, wf = sd["dir_encoding.0.weight"][:, :256].astype(np.float64), sd["xyz_encoding_final.weight"].astype(np.float64)
    exact = wd @ wf
    assert w64.dtype == np.float32 and np.array_equal(w64, exact.astype(np.float32))          # one rounding
    assert np.abs(w32 - exact).max() >= np.abs(w64 - exact).max()
    assert np.abs(b64 - (sd["dir_encoding.0.bias"] + wd @ sd["xyz_encoding_final.bias"].astype(np.float64))).max() <= 1e-7
    assert b32.shape == b64.shape == (128,)


def test_study_emulation_of_the_folded_scheme(study):
    """Scheme (b) on 64 mid-frame rays: finite colours inside the contract against the fp64 oracle."""
    rays = study.mid_frame_rays(64)
    sd_c, sd_f = make_state_dict(99), make_state_dict(100)
    got = study.render("fold64", sd_c, sd_f, rays).double()
    ref64 = study.emu.run("oracle", sd_c, sd_f, rays, torch.float64)
    assert got.shape == (64, 3) and bool(torch.isfinite(got).all())
    assert float((got - ref64).abs().max()) <= 1e-4
    assert torch.nn.functional.linear is study.emu._orig_linear    # the emulation put the real linear back
