"""tests/cond_oracle.py against the reference's own ConditionalUnet1D with global_cond_dim > 0 (tests/golden/g15_unet_cond.npz, written by
tests/golden/make_golden_cond.py).  This is what pins the yardstick the GPU tests of the conditional eps-net use: the restatement runs the
same torch CPU kernels as the reference class, so equal bits are expected; the bounds are those tests/test_oracle_golden.py holds the
unconditional fixtures (g2, g12) to."""
import math

import numpy as np
import pytest
import torch

from dgdm_amd import synth
from tests import cond_oracle as co
from tests import util
from tests.util import sample_idx

FULL_GRADS = ("mid_modules.0.cond_encoder.1.weight", "down_modules.0.0.cond_encoder.1.weight")


def _sd(g, gc):
    return synth.synth_state_dict(synth.unet_spec(global_cond_dim=gc), int(g["seed"]))


@pytest.mark.parametrize("gc", [1, 6, 16])
@pytest.mark.parametrize("L", [14, 42])
def test_cond_forward_matches_reference(gc, L):
    g = util.load("g15_unet_cond.npz")
    sd = _sd(g, gc)
    assert co.global_cond_dim(sd) == gc
    x, c, t = torch.from_numpy(g[f"fwd_gc{gc}_L{L}_x"]), torch.from_numpy(g[f"fwd_gc{gc}_L{L}_cond"]), torch.from_numpy(g["fwd_t"])
    assert float(c[3].abs().max()) == 0.0 and float(c[:3].abs().min()) > 0.0          # the fixture's all-zero row
    with torch.no_grad():
        y = co.unet1d_forward_cond(sd, x, t, c)
    ref = g[f"fwd_gc{gc}_L{L}_y"]
    assert util.rel_l2(y, ref) <= 1e-6
    # the condition matters: rows rolled by one give another answer (the reference's own sensitivity is 0.19-0.37)
    with torch.no_grad():
        y2 = co.unet1d_forward_cond(sd, x, t, torch.roll(c, 1, 0))
    assert util.rel_l2(y2, ref) > 1e-2


def test_cond_forward_without_condition_is_the_oracle():
    """gc = 0: the restatement is oracle.unet1d_forward."""
    from oracle import dgdm_oracle as orc
    sd = util.unet_sd(2)
    x = synth.synth_noise(5, 3, 14)
    t = torch.tensor([0, 7, 999])
    with torch.no_grad():
        assert torch.equal(co.unet1d_forward_cond(sd, x, t, None), orc.unet1d_forward(sd, x, t))


@pytest.mark.parametrize("tag", ["p2", "p3"])
def test_cond_training_matches_reference(tag):
    """Three Adam steps on the recorded draws: losses, the sampled gradients of step 1 and parameters after step 3 at the tolerances of
    test_unet_trainer_matches_reference (g12); the two full cond_encoder gradients, step columns and global columns separately."""
    g = util.load("g15_unet_cond.npz")
    gc, T, lr0, E = int(g["train_gc"]), int(g["num_train_timesteps"]), float(g["lr"]), int(g["num_epochs"])
    o = co.CondTrainer(_sd(g, gc), T, lr0)
    x0, c = torch.from_numpy(g[f"{tag}_x0"]), torch.from_numpy(g[f"{tag}_cond"])
    assert int((c.abs().max(dim=1).values == 0).sum()) == 1
    for step in range(3):
        if step == 2:
            o.lr = lr0 * (1 + math.cos(math.pi / E)) / 2
        assert abs(o.lr - float(g[f"{tag}_lr{step}"])) < 1e-12
        loss, _ = o.step(x0, torch.from_numpy(g[f"{tag}_noise{step}"]), torch.from_numpy(g[f"{tag}_t{step}"]), c)
        assert abs(loss - float(g[f"{tag}_loss{step}"])) < 1e-6
        if step == 0:
            for k, v in o.grads.items():
                f = v.double().flatten().numpy()
                rms = math.sqrt(float(g[f"{tag}_gradsum/{k}"][1]) / f.size)
                assert np.abs(f[sample_idx(k, f.size)] - g[f"{tag}_grad/{k}"]).max() < 2e-5 * rms, k
            for k in FULL_GRADS:
                ref = g[f"{tag}_fullgrad/{k}"]
                assert ref.shape[1] == 32 + gc
                assert util.rel_l2(o.grads[k][:, :32], ref[:, :32]) < 2e-5, k
                assert util.rel_l2(o.grads[k][:, 32:], ref[:, 32:]) < 2e-5, k
    for k, v in o.sd.items():
        f = v.double().flatten().numpy()
        assert np.abs(f[sample_idx(k, f.size)] - g[f"{tag}_final/{k}"]).max() < 4e-6, k
