"""Resampling 3-D fingers by the sliced squeeze's objective, host side (DESIGN.md 4.3e "potential: squeeze_3d"): what Resample,
SqueezePotential3D, check_resample and the entry point's flags accept and refuse, and that the library exports the new entry.  No GPU."""
import os
import shlex

import numpy as np
import pytest

from dgdm_amd import _lib, sampler
from dgdm_amd.dynamics.parser import parse
from dgdm_amd.goal import Goal
from dgdm_amd.resample import (POTENTIALS, Resample, SqueezePotential, SqueezePotential3D, resample_from_args, squeeze_potential_from_args)
from tests.test_resample_squeeze_host import _Handle, _square


def tetra(scale=0.03):
    v = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 3.0]]) * scale
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)
    return v, f


def meshes(n=2):
    return [tetra(0.02 * (1 + i)) for i in range(n)]


def test_the_library_and_the_table_name_the_entry():
    assert 'squeeze_3d' in POTENTIALS and POTENTIALS[:2] == ('model', 'squeeze')
    for name in ("dgdm_squeeze_values_3d", "dgdm_squeeze_values_3d_workspace_bytes"):
        assert name in _lib.PROTOTYPES
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dgdm_hip.h")).read()
    assert "int dgdm_squeeze_values_3d(" in hdr and "int64_t dgdm_squeeze_values_3d_workspace_bytes(" in hdr
    assert len(_lib.PROTOTYPES["dgdm_squeeze_values_3d"][1]) == 26


def test_resample_and_potential_validation():
    pot3 = SqueezePotential3D(meshes(), theta_cells=24, x_cells=9, closing_steps=3)
    pot2 = SqueezePotential(_square(), theta_cells=24, x_cells=9)
    r = Resample(1, 1.0, 2.0, potential='squeeze_3d', squeeze=pot3)
    assert r.potential == 'squeeze_3d' and r.squeeze is pot3 and "potential='squeeze_3d'" in repr(r) and pot3.n_objects == 2
    assert pot3.sample_size == 25 and pot3.width == 0.1 and len(pot3.score_std) == 3
    from dgdm_amd.dynamics.dataloader import SCORE_STD
    assert pot3.score_std == tuple(float(v) for v in SCORE_STD[0])
    # the wrong class for either potential
    with pytest.raises(ValueError, match="SqueezePotential3D"):
        Resample(1, 1.0, potential='squeeze_3d')
    with pytest.raises(ValueError, match="SqueezePotential3D"):
        Resample(1, 1.0, potential='squeeze_3d', squeeze=pot2)
    with pytest.raises(ValueError, match="SqueezePotential"):
        Resample(1, 1.0, potential='squeeze', squeeze=pot3)
    with pytest.raises(ValueError, match="squeeze"):
        Resample(1, 1.0, squeeze=pot3)
    # no FPS draws for a squeeze potential; the model's draws at every evaluation
    assert r.evaluations(5) == [0, 1, 2, 3] and r.fps_evaluations(5) == 0
    assert Resample(1, 1.0).fps_evaluations(5) == 4 and Resample(2, 1.0, potential='squeeze', squeeze=pot2).fps_evaluations(5) == 0
    # a rank's local bank
    sub = r.for_objects([1])
    assert sub.potential == 'squeeze_3d' and sub.squeeze.n_objects == 1 and np.array_equal(sub.squeeze.meshes[0][0], pot3.meshes[1][0])
    assert sub.squeeze.config == pot3.config and (sub.every, sub.beta, sub.ess_frac) == (1, 1.0, 2.0)
    assert Resample(1, 1.0).for_objects([0]).squeeze is None
    two = Resample(1, 1.0, potential='squeeze', squeeze=pot2).for_objects([1, 0]).squeeze
    assert np.array_equal(two.contours, pot2.contours[[1, 0]])
    # bad meshes
    v, f = tetra()
    for bad in ([], [(v[:, :2], f)], [(v, f[:, :2])], [(v, f + 2)], [(v, f - 1)], [(np.zeros((0, 3)), f)], [(v * np.nan, f)], [v], 3):
        with pytest.raises(ValueError, match="mesh"):
            SqueezePotential3D(bad)
    for std in ((0.05, 0.0, 0.004), (0.05, 0.002), (0.05, 0.002, float("nan")), (-1.0, 0.002, 0.004)):
        with pytest.raises(ValueError, match="score_std"):
            SqueezePotential3D(meshes(), score_std=std)
    with pytest.raises(ValueError, match="unknown"):
        SqueezePotential3D(meshes(), cells=3)
    with pytest.raises(ValueError, match="sample_size"):
        SqueezePotential3D(meshes(), sample_size=1)
    from dgdm_amd.sim.squeeze import FRICTION_2D_ONLY
    for mu in (0.0, 0.3):
        with pytest.raises(ValueError) as e:
            SqueezePotential3D(meshes(), friction=mu)
        assert FRICTION_2D_ONLY in str(e.value)


def test_check_resample():
    pot3 = SqueezePotential3D(meshes(2))
    rs = Resample(1, 1.0, potential='squeeze_3d', squeeze=pot3)
    ok = dict(eta=0.5, guid=_Handle(kind=3), n_grad=1)
    sampler.check_resample(rs, **ok)
    sampler.check_resample(rs, **dict(ok, guid=_Handle(kind=3, contraction_dtype="bf16")))      # needs no forward-only trunk
    sampler.check_resample(rs, **dict(ok, n_grad=2))
    sampler.check_resample(rs, objectives=['rotate', 'convergence'], **ok)
    with pytest.raises(ValueError, match="3-D fingers"):
        sampler.check_resample(rs, **dict(ok, guid=_Handle(kind=2)))
    with pytest.raises(ValueError, match="goal"):
        sampler.check_resample(rs, objectives=['rotate', Goal(ori=0.25, pos=(0.3, -0.2))], **ok)
    with pytest.raises(ValueError, match="goal"):
        sampler.check_resample(rs, objectives=[type("Objective", (), {"use_rowcoef": 2})()], **ok)
    with pytest.raises(ValueError, match="2 meshes"):
        sampler.check_resample(rs, **dict(ok, guid=_Handle(kind=3, n_objects=3)))
    # a caller whose handle is a spec without objects names the count itself (dist.guided_chains_sharded)
    spec = type("Spec", (), {"dyn": type("Dyn", (), {"kind": 3})(), "contraction_dtype": "f32"})()
    sampler.check_resample(rs, **dict(ok, guid=spec), n_objects=2)
    with pytest.raises(ValueError, match="meshes"):
        sampler.check_resample(rs, **dict(ok, guid=spec), n_objects=4)
    # 'squeeze' on a 3-D handle is still refused, and now says where to go
    rs2 = Resample(1, 1.0, potential='squeeze', squeeze=SqueezePotential(_square(2)))
    with pytest.raises(ValueError, match="2-D only") as e:
        sampler.check_resample(rs2, **ok)
    assert "squeeze_3d" in str(e.value)
    # what does not depend on the potential
    with pytest.raises(ValueError, match="eta"):
        sampler.check_resample(rs, **dict(ok, eta=0.0))
    with pytest.raises(ValueError, match="bounds"):
        sampler.check_resample(rs, bounds=(0, 1), **ok)
    with pytest.raises(ValueError, match="global_cond"):
        sampler.check_resample(rs, global_cond=object(), **ok)


def test_flag_rules(tmp_path):
    from dgdm_amd.generator.train import squeeze_friction_from_args, squeeze_from_args, train
    from dgdm_amd.sim.squeeze import FRICTION_2D_ONLY, NO_MESHES_3D
    base = "--mode=test --num_fingers=2 --batch_size=2 --classifier_guidance --eta 0.5 --fingers_3d --ctrlpts_dim=42"
    on = base + " --resample_every 2 --resample_beta 0.7"
    p3 = on + " --resample_potential squeeze_3d"
    assert squeeze_potential_from_args(parse(shlex.split(p3))) == {}
    got = squeeze_potential_from_args(parse(shlex.split(p3 + " --resample_squeeze_cells 24,9 --squeeze_closing_steps 4 --squeeze_window 1")))
    assert got == dict(theta_cells=24, x_cells=9, closing_steps=4, window=1)
    r = resample_from_args(parse(shlex.split(p3)))
    assert isinstance(r, Resample) and r.potential == 'model'       # the potential is attached where the meshes are known (train)
    assert squeeze_from_args(parse(shlex.split(p3 + " --squeeze_window 1"))) is None       # honoured: not "nothing reads them"
    two_d = on.replace(" --fingers_3d --ctrlpts_dim=42", "")
    for flags, what in ((base + " --resample_potential squeeze_3d", "resample_every"),
                        (two_d + " --resample_potential squeeze_3d", "needs --fingers_3d"),
                        (p3 + " --goal_pose 90,0,0", "goal"),
                        (p3 + " --squeeze_friction 0.3", "friction is 2-D only"),
                        (p3 + " --resample_squeeze_cells 24", "resample_squeeze_cells"),
                        (p3 + " --resample_squeeze_cells 0,5", "resample_squeeze_cells"),
                        (p3 + " --squeeze_window 0", "window"),
                        (p3 + " --squeeze_closing_steps -1", "closing_steps"),
                        (on + " --resample_potential squeeze", "2-D only"),
                        (on + " --resample_squeeze_cells 24,9", "resample_squeeze_cells")):
        with pytest.raises(ValueError, match=what):
            resample_from_args(parse(shlex.split(flags)))
    with pytest.raises(ValueError) as e:
        squeeze_friction_from_args(parse(shlex.split(p3 + " --squeeze_friction 0.3")))
    assert FRICTION_2D_ONLY in str(e.value)
    with pytest.raises(ValueError) as e:
        resample_from_args(parse(shlex.split(on + " --resample_potential squeeze")))
    assert "squeeze_3d" in str(e.value)
    # the run's objects must be mesh files: refused before anything is built (an empty object_dir means synthetic clouds)
    with pytest.raises(ValueError) as e:
        train(parse(shlex.split(p3 + f" --object_dir {tmp_path}")))
    assert NO_MESHES_3D in str(e.value)
