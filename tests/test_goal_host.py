"""Host side of the goal-pose objectives: the Goal dataclass, goal_objective, objective_directions, the parser flags, the draw order."""
import numpy as np
import pytest
import torch

from dgdm_amd import _lib, dist as ddist, sampler
from dgdm_amd.dynamics import metrics, predicted
from dgdm_amd.dynamics.parser import parse
from dgdm_amd.goal import Goal, goal_from_args, is_goal


def test_abi_has_the_goal_entry_points():
    lib = _lib.lib()
    assert hasattr(lib, "dgdm_guidance_set_row_field") and hasattr(lib, "dgdm_guidance_goal_field")
    import ctypes as C
    assert C.sizeof(_lib.GoalSpec) == 24 and _lib.OBJ_ROWFIELD == 2


def test_goal_units_and_validation():
    g = Goal.from_physical(30.0, 0.015, -0.003)
    assert g.ori == pytest.approx(30.0 / 180.0 - 1.0) and g.pos == pytest.approx((0.5, -0.1)) and g.theta_deg == pytest.approx(30.0)
    assert (g.weight, g.ori_window, g.pos_window, g.profile, g.scale) == ((1.0, 0.0, 0.0), 0.5, 1.0, 'sign', None)
    assert Goal.from_physical(390.0).ori == pytest.approx(Goal.from_physical(30.0).ori) and Goal.from_physical(-90.0).theta_deg == pytest.approx(270.0)
    w = Goal.from_physical(0.0, window_deg=45.0, window_m=0.015, profile='linear', scale=2.0)
    assert w.ori == -1.0 and w.ori_window == pytest.approx(0.25) and w.pos_window == pytest.approx(0.5) and w.scale == 2.0
    assert str(g) == g.name == "goal_30.0deg_1.50_-0.30cm" and f"multi/{g}" == "multi/goal_30.0deg_1.50_-0.30cm"
    assert is_goal(g) and not is_goal('rotate') and sampler.Goal is Goal
    assert (g == 'convergence') is False and (g != 'convergence') is True and g in {g}
    t = g.triples(4)
    assert t.shape == (4, 3) and t.dtype == torch.float32 and torch.equal(t[0], torch.tensor([g.ori, 0.5, -0.1], dtype=torch.float32))
    pf = Goal.per_finger(torch.tensor([[0.1, 0.0, 0.0], [-0.2, 0.5, 0.5]]))
    assert torch.equal(pf.triples(2), torch.tensor([[0.1, 0.0, 0.0], [-0.2, 0.5, 0.5]])) and pf.name == "goal_per_finger"
    with pytest.raises(ValueError, match="2 fingers"):
        pf.triples(3)
    for kw in (dict(ori=1.5), dict(ori=float("nan")), dict(pos=(0.0,)), dict(pos=(0.0, float("inf"))), dict(weight=(1.0, 0.0)),
               dict(weight=(1.0, 0.0, float("nan"))), dict(ori_window=0.0), dict(ori_window=1.01), dict(pos_window=0.0), dict(pos_window=-1.0),
               dict(profile='cubic'), dict(scale=float("inf")), dict(fingers=torch.zeros(3)), dict(fingers=torch.full((2, 3), 2.0))):
        with pytest.raises(ValueError, match="Goal"):
            Goal(**kw)
    with pytest.raises(ValueError, match="finite"):
        Goal.from_physical(float("nan"))
    n = Goal(ori=np.float32(0.25), pos=(np.float64(0.5), np.float32(0.0)), weight=tuple(np.array([1, 0, 0], dtype=np.float32)), scale=np.float32(2))
    assert n.ori == 0.25 and n.triples(1).tolist() == [[0.25, 0.5, 0.0]] and Goal.from_physical(np.float32(30.0)).theta_deg == pytest.approx(30.0)


def test_goal_field_host_restatement():
    """Goal.field: the definition on a grid small enough to check by hand (G = 4 orientations -1, -1/3, 1/3, 1; P = 3; B = 2)."""
    g = Goal(ori=1.0 / 3.0, pos=(0.0, 1.0), weight=(2.0, 1.0, -1.0), ori_window=0.7, pos_window=1.0)
    f = g.field(2, 4, 3).reshape(4, 3, 3, 2, 3)
    grid = torch.linspace(-1.0, 1.0, 4)
    u0 = 1.0 / 3.0 - grid.double()
    assert float(u0[2].abs()) < 1e-7                          # (the float32 grid value is within rounding of the goal: a pull of +-1 or 0)
    assert f[0, 0, 0, 0, 0] == -2.0 and f[1, 0, 0, 0, 0] == 2.0 and f[3, 0, 0, 1, 0] == -2.0      # at ori -1, 4/3 wraps to -2/3: inside the window, backwards
    assert torch.equal(f[0, :, 0, 0, 1], torch.tensor([1.0, 0.0, -1.0])) and torch.equal(f[0, 0, :, 0, 2], torch.tensor([0.0, -1.0, 0.0]))
    lin = Goal(ori=0.0, weight=(1.0, 1.0, 1.0), ori_window=0.5, pos_window=2.0, profile='linear').field(1, 5, 3).reshape(5, 3, 3, 3)
    assert torch.equal(lin[:, 0, 0, 0], torch.tensor([1.0, 1.0, 0.0, -1.0, -1.0])) and torch.equal(lin[0, :, 0, 1], torch.tensor([0.5, 0.0, -0.5]))


def _metric(final_theta, final_pos_cm, **extra):
    n = len(final_theta)
    pos = np.concatenate([np.asarray(final_pos_cm, dtype=np.float64).reshape(n, 2), np.zeros((n, 1))], axis=1)
    return {'final_theta': np.asarray(final_theta, dtype=np.float64), 'final_pos': pos, 'predicted': True, 'rollout_interactions': 3, **extra}


def test_goal_objective_hand_made():
    goal = Goal.from_physical(30.0, 0.01, 0.0)
    m = _metric([30.0, 32.9, 34.0, 26.0, 41.0, 200.0], [[1.0, 0.0]] * 5 + [[4.0, 4.0]])
    o = predicted.goal_objective(m, goal)
    assert (o['goal_basin_3deg'], o['goal_basin_5deg'], o['goal_basin_10deg']) == (2, 4, 4)
    assert all(o[k].dtype == np.int16 for k in ('goal_basin_3deg', 'goal_basin_5deg', 'goal_basin_10deg'))
    assert o['goal_error_deg'] == pytest.approx((0 + 2.9 + 4 + 4 + 11 + 170) / 6) and o['goal_pos_error_cm'] == pytest.approx(5.0 / 6)
    assert o['predicted'] is True
    # the wrap at +-180 degrees: a goal at 359 and finals at 1, 358.5, 4.5 and 179 (the far side)
    o = predicted.goal_objective(_metric([1.0, 358.5, 4.5, 179.0, 359.0 + 360.0], [[0.0, 0.0]] * 5), Goal.from_physical(359.0))
    assert (o['goal_basin_3deg'], o['goal_basin_5deg'], o['goal_basin_10deg']) == (3, 3, 4)
    assert o['goal_error_deg'] == pytest.approx((2 + 0.5 + 5.5 + 180 + 0) / 5)
    o = predicted.goal_objective(_metric([0.5, 359.5], [[0.0, 0.0]] * 2), Goal.from_physical(0.0))
    assert o['goal_basin_3deg'] == 2 and o['goal_error_deg'] == pytest.approx(0.5)
    assert metrics.metric2objective(m, goal) == predicted.goal_objective(m, goal)
    one_step = {k: v for k, v in m.items() if k != 'rollout_interactions'}
    with pytest.raises(ValueError, match="no settled pose"):
        predicted.goal_objective(one_step, goal)
    with pytest.raises(ValueError, match="per-finger"):
        predicted.goal_objective(m, Goal.per_finger(torch.zeros((2, 3))))
    assert metrics.metric2objective({'profile': np.array([0, 1, 2]), 'delta_theta': np.zeros(3), 'final_delta_theta': np.zeros(3)}, 'rotate')['num_zero_classes'] == 1


def test_objective_directions_of_a_goal():
    d, primary = metrics.objective_directions(Goal.from_physical(10.0))
    assert primary == 'goal_basin_5deg'
    assert d == {'goal_basin_3deg': 1, 'goal_basin_5deg': 1, 'goal_basin_10deg': 1, 'goal_error_deg': -1, 'goal_pos_error_cm': -1}
    assert metrics.objective_directions('convergence')[1] == 'max_convergence_range_5deg'
    from dgdm_amd.generator import artefacts
    assert artefacts.profile_family(Goal.from_physical(10.0)) == 'profiles' and artefacts.profile_family('shift_up') == 'profiles_x'


def test_parser_goal_flags():
    a = parse([])
    assert a.goal_pose is None and goal_from_args(a) is None
    a = parse(["--goal_pose=30,1.5,-0.3", "--goal_weight=1,0.5,0.25", "--goal_window_deg=45", "--goal_window_cm=1.5", "--goal_profile=linear",
               "--goal_scale=0.2"])
    g = goal_from_args(a)
    assert g.theta_deg == pytest.approx(30.0) and g.pos == pytest.approx((0.5, -0.1)) and g.weight == (1.0, 0.5, 0.25)
    assert g.ori_window == pytest.approx(0.25) and g.pos_window == pytest.approx(0.5) and g.profile == 'linear' and g.scale == 0.2
    d = goal_from_args(parse(["--goal_pose", "180,0,0"]))
    assert d.ori == 0.0 and d.weight == (1.0, 0.0, 0.0) and d.ori_window == pytest.approx(0.5) and d.pos_window == pytest.approx(1.0)
    assert d.profile == 'sign' and d.scale is None
    for bad in (["--goal_pose=30,1"], ["--goal_pose=a,b,c"], ["--goal_pose=0,0,0", "--goal_weight=1,1"], ["--goal_pose=0,0,0", "--goal_window_deg=0"],
                ["--goal_pose=0,0,0", "--goal_profile=cubic"]):
        with pytest.raises(ValueError):
            goal_from_args(parse(bad))


def test_scales_and_draw_order_of_goal_chains():
    """The default scale is 'convergence''s; a Goal chain consumes the FPS start stream exactly as 'rotate' does (no centre sweep)."""
    g = Goal.from_physical(90.0)
    for mode in ('point', 'point_3d'):
        for multi in (False, True):
            assert sampler.chain_scale(mode, g, multi) == sampler.classifier_scale(mode, 'convergence', multi)
            assert sampler.chain_scale(mode, 'shift_up', multi) == sampler.classifier_scale(mode, 'shift_up', multi)
    assert sampler.chain_scale('point', Goal.from_physical(90.0, scale=0.3)) == 0.3
    spec = ddist.GuidanceSpec(None, 2, 3, 2, (-1.0, 1.0), 15, 64, 5)
    drawn = {}
    for tag, o in (("goal", g), ("rotate", 'rotate'), ("convergence", 'convergence')):
        gen = torch.Generator().manual_seed(11)
        sweep, step = sampler.draw_chain_starts(spec, [(0, o), (1, 'shift_up')], 3, sampler.StartStream(64, 5, generator=gen))
        drawn[tag] = (sweep, step, gen.get_state())
    assert drawn["goal"][0] == [None, None] and np.array_equal(drawn["goal"][1], drawn["rotate"][1]) and torch.equal(drawn["goal"][2], drawn["rotate"][2])
    assert drawn["convergence"][0][0] is not None and not np.array_equal(drawn["convergence"][1], drawn["goal"][1])
    mine, local_objects, local_chains = ddist.shard_chains([(0, 'rotate'), (2, g), (2, 'shift_up'), (1, g)], 1, 2)
    assert list(mine) == [2, 3] and local_objects == [2, 1] and local_chains[0] == (0, 'shift_up') and local_chains[1][0] == 1 and local_chains[1][1] is g
