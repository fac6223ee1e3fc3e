"""CPU study in front of folding xyz_encoding_final into dir_encoding in the f16x3 render kernels ("The fold").

xyz_encoding_final is a bare Linear(256, 256) whose output feeds only dir_encoding's Linear(256 + 27, 128): two linear maps
with nothing between them are one,

    W' = W_dir[:, :256] W_f,   b' = b_dir + W_dir[:, :256] b_f,   dir_encoding(cat([W_f h8 + b_f, de])) = relu(W' h8 + W_dir[:, 256:] de + b').

Schemes, all in the operand arithmetic of scripts/study_fp8_cross.py ("f16x3": a = 2^6 W and the layer input are split into
hi = RN_f16(v), lo = RN_f16(v - hi); y = a_hi b_hi + a_hi b_lo + a_lo b_hi in fp32):
  (a) "current":    the network as it is, xyz_encoding_final evaluated and its output re-split;
  (b) "fold64":     the folded network, W' / b' summed in fp64 and rounded once to fp32 (what the fold kernel does);
  (c) "fold32":     the folded network, W' / b' accumulated term by term in fp32 (what the fp64 sum buys).
The folded network is handed to the unmodified oracle as a state dict whose xyz_encoding_final is the identity with a zero
bias: in the emulated arithmetic that layer returns hi(h8) + lo(h8) exactly (a = 64 is its own hi), and the re-split of that
sum in front of dir_encoding gives hi(h8), lo(h8) back -- the operand registers relu(h8) already sits in, which is what the
folded kernel multiplies.

Reported per scheme and field, for the fine colours of N consecutive mid-frame rays of BASELINE config #2 (504 x 378, 2 x 2
sub-pixels, NDC, 64 + 64 samples) against the fp64 oracle: median, p99.9 and max |dRGB| and the number of rays over
max(1e-4, 2 x the fp32 oracle's own gap to fp64).  Acceptance as the study was specified: (b) has no ray over the bound, and
its median and p99.9 are at most twice (a)'s.  That line cannot tell the fold from what is upstream of it: the trunk, the
density and the resampler are the same arithmetic in all three schemes, and on a chaotic field (`sharp`) the resampler alone
puts rays over the bound under (a) already.  So a second, fold-specific criterion is reported beside it, and it is the one the
decision to build the kernel rested on: no ray is over the bound under (b) that is not over it under (a), and (b)'s median
and p99.9 are at most twice (a)'s.  Both verdicts are printed; the exit status follows the first, as specified.

usage: python scripts/study_fold_final.py [N=4096] [out.txt]
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nerf_sr_amd.weights import make_state_dict  # noqa: E402  (numpy on the host)
from oracle import nerf_oracle as oc  # noqa: E402  (test infrastructure; this script is a study, not the product)
import study_fp8_cross as emu  # noqa: E402  (the operand-arithmetic emulation)

SCHEMES = ("current", "fold64", "fold32")
FINAL_W, FINAL_B, DIR_W, DIR_B = "xyz_encoding_final.weight", "xyz_encoding_final.bias", "dir_encoding.0.weight", "dir_encoding.0.bias"


def fold(sd, acc="fp64"):
    """(W', b') as fp32 numpy arrays from a numpy state dict; ``acc``: "fp64" (one rounding) or "fp32" (term by term)."""
    wd, wf = np.asarray(sd[DIR_W])[:, :256], np.asarray(sd[FINAL_W])
    bd, bf = np.asarray(sd[DIR_B]), np.asarray(sd[FINAL_B])
    if acc == "fp64":
        w = wd.astype(np.float64) @ wf.astype(np.float64)
        b = bd.astype(np.float64) + wd.astype(np.float64) @ bf.astype(np.float64)
        return w.astype(np.float32), b.astype(np.float32)
    if acc != "fp32":
        raise ValueError(acc)
    w = np.zeros((wd.shape[0], wf.shape[1]), np.float32)
    b = bd.astype(np.float32).copy()
    for k in range(wd.shape[1]):                       # fixed order, one fp32 rounding per product and per sum
        w = (w + wd[:, k:k + 1].astype(np.float32) * wf[k:k + 1, :].astype(np.float32)).astype(np.float32)
        b = (b + wd[:, k].astype(np.float32) * np.float32(bf[k])).astype(np.float32)
    return w, b


def folded_state_dict(sd, acc="fp64"):
    """The folded network as a state dict the oracle evaluates unchanged (identity xyz_encoding_final, see the header)."""
    w, b = fold(sd, acc)
    out = dict(sd)
    out[FINAL_W] = np.eye(256, dtype=np.float32)
    out[FINAL_B] = np.zeros(256, np.float32)
    out[DIR_W] = np.concatenate([w, np.asarray(sd[DIR_W])[:, 256:]], 1).astype(np.float32)
    out[DIR_B] = b
    return out


def scheme_state_dicts(scheme, sd_c, sd_f):
    if scheme == "current":
        return sd_c, sd_f
    acc = {"fold64": "fp64", "fold32": "fp32"}[scheme]
    return folded_state_dict(sd_c, acc), folded_state_dict(sd_f, acc)


def mid_frame_rays(n):
    from nerf_sr_amd import cameras                    # pure host code (no GPU, no library)
    wh, s = (504, 378), 2
    c2w = torch.as_tensor(np.asarray(cameras.spiral_pose(0.4)), dtype=torch.float32)
    rays = oc.subpixel_ray_grid(c2w, wh[1], wh[0], cameras.llff_focal(wh[0]), s, True, 0.0, 1.0).reshape(-1, 8)
    lo = (rays.shape[0] // 2) - (rays.shape[0] // 2) % (s * s)
    return rays[lo:lo + n].contiguous()


def render(scheme, sd_c, sd_f, rays):
    """Fine colours of ``scheme`` in the emulated f16x3 arithmetic."""
    a, b = scheme_state_dicts(scheme, sd_c, sd_f)
    return emu.run("f16x3", a, b, rays)


def study(n, fields=("smooth", "sharp")):
    rays = mid_frame_rays(n)
    lines = [f"fold of xyz_encoding_final into dir_encoding, {n} rays of config #2 (mid-frame), 64 + 64 samples, fine colours against the fp64 oracle"]
    ok = ok_fold = True
    for field in fields:
        sd_c, sd_f = make_state_dict(99, field), make_state_dict(100, field)
        ref64 = emu.run("oracle", sd_c, sd_f, rays, torch.float64)
        gap = (emu.run("oracle", sd_c, sd_f, rays).double() - ref64).abs().amax(-1)
        bound = torch.maximum(torch.full_like(gap, 1e-4), 2 * gap)
        lines.append(f"field {field}: fp32 oracle vs fp64: median {gap.median():.3e}  p99.9 {torch.quantile(gap, 0.999):.3e}  max {gap.max():.3e}")
        lines.append("  scheme    median     p99.9      max        rays>max(1e-4, 2 x oracle gap)")
        stat, over, rgb = {}, {}, {}
        for scheme in SCHEMES:
            rgb[scheme] = render(scheme, sd_c, sd_f, rays).double()
            d = (rgb[scheme] - ref64).abs().amax(-1)
            over[scheme] = d > bound
            stat[scheme] = (float(d.median()), float(torch.quantile(d, 0.999)), float(d.max()), int((d > bound).sum()))
            lines.append("  %-8s  %.3e  %.3e  %.3e  %d" % ((scheme,) + stat[scheme]))
            print(lines[-1], flush=True)
        a, b = stat["current"], stat["fold64"]
        good = b[3] == 0 and b[0] <= 2 * a[0] and b[1] <= 2 * a[1]
        ok = ok and good
        lines.append(f"  acceptance (fold64: 0 rays over the bound, median and p99.9 <= 2 x current): {'PASS' if good else 'FAIL'}")
        # what the fold itself moves: the trunk, the density and with them the resampled depths are the same arithmetic in
        # all three schemes, so a ray the resampler amplifies past the bound is past it in every scheme alike
        added = int((over['fold64'] & ~over['current']).sum())
        good_fold = added == 0 and b[0] <= 2 * a[0] and b[1] <= 2 * a[1]
        ok_fold = ok_fold and good_fold
        lines.append(f"  fold-specific criterion (no ray over the bound under fold64 that is not over it under current, median and "
                     f"p99.9 <= 2 x current): {'PASS' if good_fold else 'FAIL'}")
        lines.append(f"  rays over the bound under fold64 but not under current: {added}"
                     f"   max |fold64 - current| {float((rgb['fold64'] - rgb['current']).abs().max()):.3e}"
                     f"   max |fold32 - current| {float((rgb['fold32'] - rgb['current']).abs().max()):.3e}")
    lines.append("verdict, acceptance as specified: " + ("PASS" if ok else "FAIL"))
    lines.append("verdict, fold-specific criterion (the one the kernel was built on): " + ("PASS" if ok_fold else "FAIL"))
    return ok, "\n".join(lines) + "\n"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    ok, text = study(n)
    print(text)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
