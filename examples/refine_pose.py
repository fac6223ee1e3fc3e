#!/usr/bin/env python3
"""Refine a camera pose against a frozen field through the gradient with respect to the rays (needs an MI355X).

A teacher view of the synthetic field of nerf_sr_amd.weights is rendered from a known pose; the pose is then perturbed by a
small se(3) offset (a rotation vector and a translation) and, with both networks frozen, the offset is recovered by Adam on the
photometric loss, BARF / NeRF-- style: pose -> ``cameras.rays_from_pose`` (torch, differentiable) -> ``train.forward_rays_train``
with rays that require grad (``precision='fp32'``: the layer-by-layer pair, ``nsr_train_arch_backward_r``) -> MSE against the
teacher's colours -> ``loss.backward()`` fills the offset's gradient.  Prints the rotation / translation error before and after,
and the iterations per second of the loop.

``--chain`` runs the same recovery on ``precision='f16x3'`` with ``chain_ray_grad=True``: the chain pair, whose backward
(``nsr_train_backward_r``) takes the ray gradient from the backward chain's panels and -- the field being frozen, no weight
requires grad -- skips the weight-gradient launches (``NSR_BACKWARD_NO_WEIGHT_GRADS``).

``--precision`` names the layer-by-layer pair's arithmetic: 'fp32', 'f16x3_gemm' (forward products split-fp16) or
'f16x3_gemm_bwd' (the gradient products split-fp16 as well).

    python examples/refine_pose.py [--iters 300] [--batch 512] [--rot 0.02] [--trans 0.02] [--chain | --precision f16x3_gemm_bwd]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_sr_amd import cameras, train  # noqa: E402
from nerf_sr_amd.weights import make_state_dict  # noqa: E402


def skew(w):
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def compose(c2w0, xi):
    """[exp(omega^) R0 | c0 + t] of the offset xi = (omega, t); on the host, (3, 4)."""
    R = torch.linalg.matrix_exp(skew(xi[:3])) @ c2w0[:, :3]
    return torch.cat([R, (c2w0[:, 3] + xi[3:])[:, None]], 1)


def errors(c2w, c2w_true):
    """(rotation error in degrees, translation error) between two poses."""
    dR = c2w[:, :3] @ c2w_true[:, :3].T
    cos = ((torch.trace(dR) - 1.0) / 2.0).clamp(-1.0, 1.0)
    return float(torch.rad2deg(torch.acos(cos))), float((c2w[:, 3] - c2w_true[:, 3]).norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batch", type=int, default=512, help="LR pixels per step (x4 sub-rays)")
    ap.add_argument("--rot", type=float, default=0.02, help="norm of the rotation offset (radians)")
    ap.add_argument("--trans", type=float, default=0.02, help="norm of the translation offset")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--chain", action="store_true", help="the chain pair under precision 'f16x3' (chain_ray_grad=True)")
    ap.add_argument("--precision", default="fp32", choices=train.ARCH_PRECISIONS,
                    help="the layer-by-layer pair's arithmetic (without --chain)")
    a = ap.parse_args()
    W, H, s = 96, 72, 2
    focal = cameras.llff_focal(504) * W / 504
    field = [{k: torch.from_numpy(v).cuda() for k, v in make_state_dict(seed).items()} for seed in (99, 100)]
    route = dict(precision="f16x3", chain_ray_grad=True) if a.chain else dict(precision=a.precision)
    render = lambda rays: train.forward_rays_train(field[0], field[1], rays, None, ray_chunk=4096, **route)
    c2w_true = torch.from_numpy(cameras.spiral_pose(0.5)).float()
    with torch.no_grad():      # the teacher: the deterministic train-mode forward from the true pose
        out = render(cameras.rays_from_pose(c2w_true.cuda(), H, W, focal, s, True, 0.0, 1.0))
        teacher = torch.cat([out["coarse_comp_rgbs"], out["fine_comp_rgbs"]], 1)
    gen = torch.Generator().manual_seed(0)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(3, generator=gen), dim=0) * n
    with torch.no_grad():      # the starting pose: the true one moved by a small se(3) offset
        c2w0 = compose(c2w_true, torch.cat([unit(a.rot), unit(a.trans)]))
    xi = torch.zeros(6, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=a.lr)
    r0, t0 = errors(c2w0, c2w_true)
    print(f"before: rotation error {r0:.4f} deg, translation error {t0:.5f}")
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for it in range(a.iters):
        rows = torch.randint(0, (H // s) * (W // s), (a.batch,), generator=gen)
        rows = (rows[:, None] * (s * s) + torch.arange(s * s)[None, :]).reshape(-1).cuda()      # whole LR pixels
        rays = cameras.rays_from_pose(compose(c2w0, xi).cuda(), H, W, focal, s, True, 0.0, 1.0, rows=rows)
        out = render(rays)
        loss = torch.nn.functional.mse_loss(torch.cat([out["coarse_comp_rgbs"], out["fine_comp_rgbs"]], 1), teacher[rows])
        opt.zero_grad()
        loss.backward()
        opt.step()
        if it % 50 == 0 or it == a.iters - 1:
            r, t = errors(compose(c2w0, xi.detach()), c2w_true)
            print(f"iter {it:4d}  loss {float(loss):.3e}  rotation error {r:.4f} deg  translation error {t:.5f}")
    torch.cuda.synchronize()
    print(f"{a.iters / (time.perf_counter() - t_start):.2f} iterations/s ({'chain pair, f16x3' if a.chain else 'layer-by-layer pair, fp32'})")
    r1, t1 = errors(compose(c2w0, xi.detach()), c2w_true)
    print(f"after:  rotation error {r1:.4f} deg, translation error {t1:.5f}")


if __name__ == "__main__":
    main()
