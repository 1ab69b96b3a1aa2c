#!/usr/bin/env python3
"""Generate tests/golden/g15_unet_cond.npz from the REFERENCE's own ``ConditionalUnet1D`` with ``global_cond_dim > 0``.

In the style of make_golden.py: the reference class is imported at generation time only (the reference tree does not exist where the
tests run), weights come from ``dgdm_amd.synth`` so the fixture carries seeds, and only arrays are written.

Forward: ``ConditionalUnet1D(1, gc, [128, 256], 32)`` for gc in {1, 6, 16}, L in {14, 42}, B = 4, per-sample timesteps (0, 3, 12, 999),
condition rows uniform in [-1, 1] with row 3 all zero.
Training: gc = 6 in train mode, cases (L = 14, B = 5) and (L = 42, B = 6), three Adam steps as in g12_unet_train (lr 1e-4, the cosine
schedule stepped once before the third) on the generator's own loss with a condition - the reference's ``get_stats`` never passes one:
``noisy = add_noise(x0, noise, t); mse_loss(net(noisy, t, global_cond=c), noise)``, one condition row all zero.  Kept: the inputs and
draws, the three losses, g12's sampled entries plus sum / sum of squares of every parameter's step-1 gradient and step-3 value, and the
FULL step-1 gradient of two cond_encoder weights (the global columns' gradient is ~7 % of the step columns' in norm and is checked
on its own).

Usage:  python tests/golden/make_golden_cond.py      (from the repository root, ~1 min on the CPU)"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")
OUT = os.path.dirname(os.path.abspath(__file__))

from dgdm_amd import synth                      # noqa: E402
from oracle import dgdm_oracle as orc           # noqa: E402  (only its DDIM restatement is used here)
from tests.util import sample_idx               # noqa: E402

# `generator` must resolve to the REFERENCE (a namespace package under its root), not to this repository's shim of the same name
sys.path.remove(REPO)
assert "generator" not in sys.modules
from generator.diffusion_utils import ConditionalUnet1D     # noqa: E402

assert ConditionalUnet1D.__module__ == "generator.diffusion_utils" and sys.modules["generator.diffusion_utils"].__file__.startswith(REF)

UNET_SEED = 11
FULL_GRADS = ("mid_modules.0.cond_encoder.1.weight", "down_modules.0.0.cond_encoder.1.weight")


def make_unet(gc):
    net = ConditionalUnet1D(input_dim=1, global_cond_dim=gc, down_dims=[128, 256], diffusion_step_embed_dim=32)
    spec = synth.unet_spec(global_cond_dim=gc)
    ref_sd = net.state_dict()
    assert sorted(ref_sd.keys()) == sorted(k for k, _ in spec), "spec keys differ from the reference module"
    for k, shp in spec:
        assert tuple(ref_sd[k].shape) == tuple(shp), (k, ref_sd[k].shape, shp)
    net.load_state_dict(synth.synth_state_dict(spec, UNET_SEED))
    return net.eval()


def cond_rows(seed, B, gc, zero_row):
    c = np.random.RandomState(seed).uniform(-1, 1, (B, gc)).astype(np.float32)
    c[zero_row] = 0.0
    return c


def forward(out):
    ts = torch.tensor([0, 3, 12, 999], dtype=torch.int64)
    out["fwd_t"] = ts.numpy()
    for gc in (1, 6, 16):
        net = make_unet(gc)
        for L in (14, 42):
            x = synth.synth_noise(200 + L + gc, 4, L)
            c = cond_rows(300 + L + gc, 4, gc, 3)
            with torch.no_grad():
                y = net(x, ts, global_cond=torch.from_numpy(c))
            out[f"fwd_gc{gc}_L{L}_x"], out[f"fwd_gc{gc}_L{L}_cond"], out[f"fwd_gc{gc}_L{L}_y"] = x.numpy(), c, y.numpy()


def training(out):
    gc, T, lr0, E = 6, 15, 1e-4, 100
    out.update({"train_gc": np.int64(gc), "torch_seed": np.int64(4321), "lr": np.float64(lr0), "num_epochs": np.int64(E),
                "num_train_timesteps": np.int64(T)})
    sched = orc.DDIM(T)
    for tag, L, B in (("p2", 14, 5), ("p3", 42, 6)):
        net = make_unet(gc).train()
        for p_ in net.parameters():
            p_.requires_grad_(True)
        opt = torch.optim.Adam(net.parameters(), lr=lr0)                                   # generator/diffusion.py:712
        lrs = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=E, eta_min=0.0)        # :713
        x0 = torch.from_numpy(np.random.RandomState(77 + L).uniform(-1, 1, (B, L, 1)).astype(np.float32))
        c = torch.from_numpy(cond_rows(88 + L, B, gc, 1))
        out[f"{tag}_x0"], out[f"{tag}_cond"], out[f"{tag}_dims"] = x0.numpy(), c.numpy(), np.array([B, L])
        torch.manual_seed(4321)
        for step in range(3):
            if step == 2:
                lrs.step()
            noise = torch.randn((B, L, 1))                                                 # get_stats' draws, in its order (:139-142)
            ts = torch.randint(0, T, (B,)).long()
            noisy = sched.add_noise(x0, noise, ts)
            loss = F.mse_loss(net(noisy, ts, global_cond=c), noise)
            opt.zero_grad()
            loss.backward()
            if step == 0:
                for k, prm in net.named_parameters():
                    g = prm.grad.detach().double().flatten()
                    out[f"{tag}_grad/{k}"] = g[sample_idx(k, g.numel())].float().numpy()
                    out[f"{tag}_gradsum/{k}"] = np.array([float(g.sum()), float((g * g).sum())])
                    if k in FULL_GRADS:
                        out[f"{tag}_fullgrad/{k}"] = prm.grad.detach().numpy().copy()
            out[f"{tag}_lr{step}"] = np.float64(opt.param_groups[0]["lr"])
            opt.step()
            out[f"{tag}_loss{step}"] = np.float64(float(loss))
            out[f"{tag}_noise{step}"], out[f"{tag}_t{step}"] = noise.numpy(), ts.numpy()
        for k, v in net.state_dict().items():
            f = v.detach().double().flatten()
            out[f"{tag}_final/{k}"] = f[sample_idx(k, f.numel())].float().numpy()
            out[f"{tag}_finalsum/{k}"] = np.array([float(f.sum()), float((f * f).sum())])
        print("g15", tag, [out[f"{tag}_loss{i}"] for i in range(3)], flush=True)


if __name__ == "__main__":
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    out = {"seed": np.int64(UNET_SEED)}
    forward(out)
    training(out)
    np.savez_compressed(os.path.join(OUT, "g15_unet_cond.npz"), **out)
    print("wrote g15_unet_cond.npz", os.path.getsize(os.path.join(OUT, "g15_unet_cond.npz")), "bytes")
