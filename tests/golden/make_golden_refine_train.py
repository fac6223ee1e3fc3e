#!/usr/bin/env python3
"""Golden vectors of the reference's refinement network in TRAIN mode: ``models/networks.py::MaxPoolingModel`` under
``.train()``, weights ``nerf_sr_amd.refine.make_refine_state_dict(7)``, three small cases, each run in fp32 AND with the
module in ``.double()``.  Stored per case: inputs, y (fp32, fp64), the loss, the 34 running-statistics tensors after the
forward, and per gradient tensor its fp64 norm, 64 fp64 entries at seeded indices and the reference's own
fp32-vs-fp64 relative gap; plus the whole-gradient gap and max |y32 - y64|.

A ReLU / max kink event (an activation a rounding error away from 0, or two references a rounding error apart) makes the
reference's fp32 gradients differ from its fp64 ones by orders more than rounding: a case is only stored if every one of
the 55 non-cancelled tensors of the fp32 run is within 2e-5 of fp64, otherwise the next input seed is tried.

Also the loss of 20 iterations of the reference's ``optimize_parameters`` (models/refine_model.py:141-149: forward,
zero_grad, backward of the L1 loss, Adam(lr 5e-4, betas (0.9, 0.999)).step) on case A's fixed batch, fp32.
Development container only; data only.

    python tests/golden/make_golden_refine_train.py      # rewrites tests/golden/refine_train.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

from nerf_sr_amd.refine import RUNNING_KEYS, TRAIN_PARAM_KEYS, make_refine_state_dict  # noqa: E402

# tag -> (B, R, H, W), lambda L1, lambda MSE, first input seed
CASES = {"A": ((2, 2, 16, 24), 1.0, 0.0, 5), "B": ((3, 1, 16, 16), 1.0, 10.0, 5), "C": ((2, 8, 16, 16), 0.0, 10.0, 6)}
CLEAN = 2e-5
N_ENTRIES = 64


def build(dtype):
    from models.networks import MaxPoolingModel
    net = MaxPoolingModel(types.SimpleNamespace(not_use_ref=False))
    sd = {k: torch.from_numpy(v) for k, v in make_refine_state_dict(7).items()}
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    net.to(dtype).train()
    params = dict(net.named_parameters())
    assert list(params) == TRAIN_PARAM_KEYS, "parameter order differs from nerf_sr_amd.refine.TRAIN_PARAM_KEYS"
    return net, params


def loss_of(y, gt, l1, mse):
    tot = 0.0
    if l1:
        tot = tot + l1 * torch.nn.L1Loss(reduction="mean")(y, gt)
    if mse:
        tot = tot + mse * torch.nn.MSELoss(reduction="mean")(y, gt)
    return tot


def run(dtype, x, c, gt, l1, mse):
    net, params = build(dtype)
    y = net(x.to(dtype), c.to(dtype))
    loss = loss_of(y, gt.to(dtype), l1, mse)
    loss.backward()
    bufs = dict(net.named_buffers())
    return y.detach(), loss.detach(), {k: p.grad.double() for k, p in params.items()}, {k: bufs[k].double() for k in RUNNING_KEYS}


def rel(a, b):
    return float((a - b).norm() / b.norm())


def main():
    mg.install_shim()
    out = {"weights_seed": 7, "param_keys": np.array(TRAIN_PARAM_KEYS), "running_keys": np.array(RUNNING_KEYS)}
    cancelled = [k for k in TRAIN_PARAM_KEYS if k.endswith(".bias") and k.replace(".bias", "_bnorm.bias") in TRAIN_PARAM_KEYS]
    live = [k for k in TRAIN_PARAM_KEYS if k not in cancelled]
    assert len(cancelled) == 17 and len(live) == 55
    for tag, ((B, R, H, W), l1, mse, seed0) in CASES.items():
        for seed in range(seed0, seed0 + 50):
            gen = torch.Generator().manual_seed(seed)
            x = torch.rand(B, 3, H, W, generator=gen) * 2 - 1
            c = torch.rand(B, R, 3, H, W, generator=gen) * 2 - 1
            gt = torch.rand(B, 3, H, W, generator=gen) * 2 - 1
            y32, loss32, g32, r32 = run(torch.float32, x, c, gt, l1, mse)
            y64, loss64, g64, r64 = run(torch.float64, x, c, gt, l1, mse)
            gaps = {k: rel(g32[k], g64[k]) for k in live}
            worst = max(gaps.values())
            if worst <= CLEAN:
                break
            print(f"case {tag} seed {seed}: NOT clean, {sum(v > CLEAN for v in gaps.values())} tensors over {CLEAN:g}, worst {worst:.2e}")
        else:
            raise SystemExit(f"case {tag}: no clean input seed found")
        whole = float(torch.cat([(g32[k] - g64[k]).flatten() for k in live]).norm() / torch.cat([g64[k].flatten() for k in live]).norm())
        idx_gen = np.random.default_rng(1000 + seed)
        out[f"{tag}_shape"], out[f"{tag}_lambdas"], out[f"{tag}_seed"] = np.array([B, R, H, W]), np.array([l1, mse]), seed
        out[f"{tag}_x"], out[f"{tag}_c"], out[f"{tag}_gt"] = mg.np32(x), mg.np32(c), mg.np32(gt)
        out[f"{tag}_y32"], out[f"{tag}_y64"] = mg.np32(y32), y64.numpy()
        out[f"{tag}_loss64"], out[f"{tag}_loss32"] = float(loss64), float(loss32)
        out[f"{tag}_dy_max"] = float((y32.double() - y64).abs().max())
        out[f"{tag}_running64"] = np.concatenate([r64[k].numpy() for k in RUNNING_KEYS])
        out[f"{tag}_running_gap"] = max(float((r32[k] - r64[k]).abs().max()) for k in RUNNING_KEYS)
        out[f"{tag}_grad_norm64"] = np.array([float(g64[k].norm()) for k in TRAIN_PARAM_KEYS])
        out[f"{tag}_grad_gap"] = np.array([gaps.get(k, 0.0) for k in TRAIN_PARAM_KEYS])
        out[f"{tag}_cancelled_max64"] = max(float(g64[k].abs().max()) for k in cancelled)
        out[f"{tag}_whole_gap"] = whole
        idx = np.stack([idx_gen.integers(0, g64[k].numel(), N_ENTRIES) for k in TRAIN_PARAM_KEYS])
        out[f"{tag}_grad_idx"] = idx
        out[f"{tag}_grad_entries64"] = np.stack([g64[k].flatten().numpy()[idx[i]] for i, k in enumerate(TRAIN_PARAM_KEYS)])
        print(f"case {tag} seed {seed}: worst per-tensor gap {worst:.2e}, whole gradient {whole:.2e}, max |dy| {out[f'{tag}_dy_max']:.1e}, "
              f"running gap {out[f'{tag}_running_gap']:.1e}, cancelled biases (fp64) <= {out[f'{tag}_cancelled_max64']:.1e}")
    # the reference's training iteration on case A's batch
    x, c, gt = (torch.from_numpy(out[f"A_{k}"]) for k in ("x", "c", "gt"))
    net, _ = build(torch.float32)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.9, 0.999))
    curve = []
    for _ in range(20):
        y = net(x, c)
        opt.zero_grad()
        loss = loss_of(y, gt, 1.0, 0.0)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    out["A_curve"] = np.array(curve)
    print("curve", " ".join(f"{v:.4f}" for v in curve))
    path = os.path.join(HERE, "refine_train.npz")
    np.savez_compressed(path, **out)
    print("->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
