"""Resampling by the squeeze simulator's objective, host side: the oracle's start grid against the torch.meshgrid
statement of cond_fn's grid, what Resample / check_resample / the entry point's flags refuse, and that a Resample without `potential`
is the one of old.  No GPU."""
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import sampler
from dgdm_amd.dynamics.parser import parse
from dgdm_amd.goal import Goal
from dgdm_amd.resample import Resample, SqueezePotential, resample_from_args, squeeze_potential_from_args, start_grid
from tests import resample_squeeze_oracle as rso


def _square(n=2):
    return np.stack([np.array([[-0.02, -0.02], [0.02, -0.02], [0.02, 0.02], [-0.02, 0.02]]) * (1 + i) for i in range(n)])


@pytest.mark.parametrize("G,P,ori", [(8, 3, (-0.5, 0.25)), (4, 1, (-1.0, 1.0)), (1, 2, (0.0, 0.5)), (5, 4, (-1.0, 1.0))])
def test_start_grid_is_cond_fns_grid(G, P, ori):
    """generator/diffusion.py:478: meshgrid(linspace(ori), linspace(-1, 1, P), linspace(-1, 1, P)), flattened - the model's (ori, x, y)
    inputs per cell; the starts are those in the simulator's units.  torch's linspace is float32, the starts float64: equal to a few
    float32 ulps of the largest magnitudes (2 pi and 0.03), 2e-6 and 1e-8 being more than ten of them."""
    so, sx, sy = torch.meshgrid(torch.linspace(ori[0], ori[1], G), torch.linspace(-1, 1, P), torch.linspace(-1, 1, P), indexing="ij")
    want = np.stack([(so.reshape(-1).double().numpy() + 1.0) * np.pi, sx.reshape(-1).double().numpy() * 0.03,
                     sy.reshape(-1).double().numpy() * 0.03], axis=1)
    got = rso.start_grid(G, P, ori)
    assert got.shape == (G * P * P, 3) and got.dtype == np.float64
    assert np.abs(got[:, 0] - want[:, 0]).max() <= 2e-6 and np.abs(got[:, 1:] - want[:, 1:]).max() <= 1e-8
    assert np.array_equal(got.view(np.int64), start_grid(G, P, ori).view(np.int64))        # the package builds the oracle's grid, bit for bit
    if P > 1:
        assert got[1, 2] > got[0, 2] and got[P, 1] > got[0, 1] and got[1, 1] == got[0, 1]   # y runs fastest, then x
    if G > 1:
        assert got[P * P, 0] > got[0, 0] and got[P * P - 1, 0] == got[0, 0]                 # the orientation slowest


def test_resample_without_potential_is_the_one_of_old():
    r = Resample(2, 0.5)
    assert repr(r) == "Resample(every=2, beta=0.5, ess_frac=0.5)" and (r.every, r.beta, r.ess_frac) == (2, 0.5, 0.5)
    assert r.potential == 'model' and r.squeeze is None
    assert repr(Resample(1, 1.0, 2.0, potential='model')) == "Resample(every=1, beta=1.0, ess_frac=2.0)"
    assert r.evaluations(5) == [1, 3]


def test_resample_potential_validation():
    pot = SqueezePotential(_square(), theta_cells=24, x_cells=9)
    r = Resample(1, 1.0, 2.0, potential='squeeze', squeeze=pot)
    assert r.potential == 'squeeze' and r.squeeze is pot and "potential='squeeze'" in repr(r) and pot.n_objects == 2
    with pytest.raises(ValueError, match="SqueezePotential"):
        Resample(1, 1.0, potential='squeeze')
    with pytest.raises(ValueError, match="SqueezePotential"):
        Resample(1, 1.0, potential='squeeze', squeeze=object())
    with pytest.raises(ValueError, match="potential"):
        Resample(1, 1.0, potential='mujoco')
    with pytest.raises(ValueError, match="squeeze"):
        Resample(1, 1.0, squeeze=pot)
    for bad in (np.zeros((2, 4)), np.zeros((0, 4, 2)), np.zeros((1, 2, 2)), np.zeros((1, 4, 3))):
        with pytest.raises(ValueError, match="contours"):
            SqueezePotential(bad)
    with pytest.raises(ValueError, match="score_std"):
        SqueezePotential(_square(), score_std=(0.05, 0.0, 0.004))
    with pytest.raises(ValueError, match="unknown"):
        SqueezePotential(_square(), cells=3)


class _Handle:
    """What check_resample reads of a guidance handle."""

    def __init__(self, kind=2, n_objects=2, contraction_dtype="f32"):
        self.dyn = type("Dyn", (), {"kind": kind})()
        self.n_objects, self.contraction_dtype = n_objects, contraction_dtype


def test_check_resample_refusals():
    pot = SqueezePotential(_square(2))
    rs = Resample(1, 1.0, potential='squeeze', squeeze=pot)
    ok = dict(eta=0.5, guid=_Handle(), n_grad=1)
    sampler.check_resample(rs, **ok)
    sampler.check_resample(rs, **dict(ok, guid=_Handle(contraction_dtype="bf16")))          # needs no forward-only trunk
    with pytest.raises(ValueError, match="bf16"):
        sampler.check_resample(Resample(1, 1.0), **dict(ok, guid=_Handle(contraction_dtype="bf16")))
    with pytest.raises(ValueError, match="2-D only"):
        sampler.check_resample(rs, **dict(ok, guid=_Handle(kind=3)))
    sampler.check_resample(Resample(1, 1.0), **dict(ok, guid=_Handle(kind=3)))               # the model's potential has a 3-D form
    with pytest.raises(ValueError, match="contours"):
        sampler.check_resample(rs, **dict(ok, guid=_Handle(n_objects=3)))
    goal = Goal(ori=0.25, pos=(0.3, -0.2))
    with pytest.raises(ValueError, match="goal"):
        sampler.check_resample(rs, objectives=['rotate', goal], **ok)
    field = type("Objective", (), {"use_rowcoef": 2})()
    with pytest.raises(ValueError, match="goal"):
        sampler.check_resample(rs, objectives=[field], **ok)
    sampler.check_resample(rs, objectives=['rotate', 'convergence'], **ok)
    # the refusals that do not depend on the potential are unchanged
    with pytest.raises(ValueError, match="eta"):
        sampler.check_resample(rs, **dict(ok, eta=0.0))
    with pytest.raises(ValueError, match="bounds"):
        sampler.check_resample(rs, bounds=(0, 1), **ok)
    with pytest.raises(ValueError, match="global_cond"):
        sampler.check_resample(rs, global_cond=object(), **ok)
    with pytest.raises(ValueError, match="n_grad"):
        sampler.check_resample(rs, **dict(ok, n_grad=0))
    with pytest.raises(ValueError, match="n_grad"):
        sampler.check_resample(rs, **dict(ok, guid=None))
    with pytest.raises(ValueError, match="scales"):
        sampler.check_resample(rs, scales=[0.001, 10.0], **dict(ok, n_grad=2))


def test_flag_rules():
    base = "--mode=test --num_fingers=2 --batch_size=2 --classifier_guidance --eta 0.5"
    on = base + " --resample_every 2 --resample_beta 0.7"
    args = parse(shlex.split(on))
    assert args.resample_potential == 'model' and squeeze_potential_from_args(args) is None and resample_from_args(args).potential == 'model'
    assert squeeze_potential_from_args(parse(shlex.split(on + " --resample_potential squeeze"))) == {}
    got = squeeze_potential_from_args(parse(shlex.split(on + " --resample_potential squeeze --resample_squeeze_cells 360,121 "
                                                             "--squeeze_closing_steps 4 --squeeze_window 1")))
    assert got == dict(theta_cells=360, x_cells=121, closing_steps=4, window=1)
    assert isinstance(resample_from_args(parse(shlex.split(on + " --resample_potential squeeze"))), Resample)
    for flags, what in ((base + " --resample_potential squeeze", "resample_every"),
                        (on + " --resample_potential squeeze --fingers_3d", "2-D only"),
                        (on + " --resample_potential squeeze --goal_pose 90,0,0", "goal"),
                        (on + " --resample_potential mujoco", "resample_potential"),
                        (on + " --resample_squeeze_cells 360,121", "resample_squeeze_cells"),
                        (on + " --resample_potential squeeze --resample_squeeze_cells 360", "resample_squeeze_cells"),
                        (on + " --resample_potential squeeze --resample_squeeze_cells 0,5", "resample_squeeze_cells"),
                        (on + " --resample_potential squeeze --squeeze_window 0", "window"),
                        (on + " --resample_potential squeeze --squeeze_closing_steps -1", "closing_steps")):
        with pytest.raises(ValueError, match=what):
            resample_from_args(parse(shlex.split(flags)))
    # --squeeze_closing_steps / --squeeze_window are honoured by the potential, and still refused where nothing reads them
    from dgdm_amd.generator.train import squeeze_from_args
    assert squeeze_from_args(parse(shlex.split(on + " --resample_potential squeeze --squeeze_window 1"))) is None
    with pytest.raises(ValueError, match="squeeze_window"):
        squeeze_from_args(parse(shlex.split(on + " --squeeze_window 1")))
