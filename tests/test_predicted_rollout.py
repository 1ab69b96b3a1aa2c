"""The host side of predicted roll-outs (dynamics/predicted.py build_metric with a settled pose, the --predicted_rollout flag): the
formulas stated by hand, and the 'convergence' objective on a hand-made funnel."""
import numpy as np
import pytest

from dgdm_amd.dynamics import predicted
from dgdm_amd.dynamics.dataloader import POS_NORM, SCORE_STD, SCORE_THRESHOLD
from dgdm_amd.dynamics.metrics import metric2objective
from dgdm_amd.dynamics.parser import parse

STD = [float(v) for v in SCORE_STD[1]]
THR = [float(t / s) for t, s in zip(SCORE_THRESHOLD[1], SCORE_STD[1])]


def logits(g):
    rs = np.random.RandomState(5)
    return rs.randn(g, 3).astype(np.float32)


def test_pos_norm_is_the_dataset_divisor():
    assert POS_NORM == 0.03


def test_parser_default_is_zero():
    assert parse([]).predicted_rollout == 0
    assert parse(["--predicted_rollout=40"]).predicted_rollout == 40


def test_build_metric_without_a_final_pose_is_unchanged():
    """Same keys and values as the one-interaction metric stated by hand (the rule the function had before roll-outs)."""
    l = logits(5)
    m = predicted.build_metric(l, THR, STD, (-1.0, 1.0))
    dt = l[:, 0].astype(np.float64) * STD[0] * 180.0 / np.pi
    dp = np.stack([l[:, 1].astype(np.float64) * STD[1] * 100.0, l[:, 2].astype(np.float64) * STD[2] * 100.0, np.zeros(5)], axis=1)
    initial = (np.linspace(-1.0, 1.0, 5) + 1.0) * 180.0
    cls = predicted.classes(l, THR)
    want = {'delta_theta': dt, 'delta_pos': dp, 'profile': cls[:, 0], 'profile_x': cls[:, 1], 'profile_y': cls[:, 2], 'final_theta': initial + dt,
            'final_delta_theta': dt, 'final_pos': dp, 'predicted': True}
    assert list(m.keys()) == list(want.keys())
    for k, v in want.items():
        assert np.array_equal(m[k], v), k


def test_build_metric_with_a_final_pose():
    """final_theta = (ori_K + 1) x 180; final_delta_theta = final - initial folded once by 360 when it leaves [-180, 180]
    (continuous_signed_delta in degrees); final_pos = pos_K x 0.03 x 100 cm, third column 0; one-step keys untouched."""
    l = logits(5)
    #            initial 0      90      180      270      360 degrees
    ori = np.array([0.95, -0.5, 0.0, 0.5 + 1e-3, -0.9])      # final 351, 90, 180, 270.18, 18 degrees
    pos = np.array([[0.5, -0.25], [1.5, 0.0], [0.0, 0.0], [-2.0, 1.0], [0.1, 0.2]])
    left = np.array([-1, 2, -1, 0, -1], dtype=np.int32)
    m = predicted.build_metric(l, THR, STD, (-1.0, 1.0), final_pose=np.concatenate([ori[:, None], pos], axis=1), left=left, rollout_interactions=7)
    one = predicted.build_metric(l, THR, STD, (-1.0, 1.0))
    for k in ('delta_theta', 'delta_pos', 'profile', 'profile_x', 'profile_y'):
        assert np.array_equal(m[k], one[k]), k
    assert m['predicted'] is True and m['rollout_interactions'] == 7 and m['rollout_left_range'] == 2 and isinstance(m['rollout_left_range'], int)
    assert np.allclose(m['final_theta'], [351.0, 90.0, 180.0, 270.18, 18.0], rtol=0, atol=1e-9)
    # 351 - 0 = 351 > 180 -> -9 (crosses +180); 18 - 360 = -342 < -180 -> 18 (crosses -180); the others are plain differences
    assert np.allclose(m['final_delta_theta'], [-9.0, 0.0, 0.0, 0.18, 18.0], rtol=0, atol=1e-9)
    assert np.allclose(m['final_pos'], np.concatenate([pos * 3.0, np.zeros((5, 1))], axis=1), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        predicted.build_metric(l, THR, STD, (-1.0, 1.0), final_pose=np.zeros((5, 3)))
    with pytest.raises(ValueError):
        predicted.build_metric(l, THR, STD, (-1.0, 1.0), final_pose=np.zeros((4, 3)), left=left, rollout_interactions=7)
    with pytest.raises(ValueError, match="rollout_interactions"):
        predicted.build_metric(l, THR, STD, (-1.0, 1.0), final_pose=np.zeros((5, 3)), left=left)


def test_convergence_on_a_funnel():
    """Orientations 4 .. 13 of 24 settle within 3 degrees of each other (a funnel), the rest stay where they started, 15 degrees apart:
    the longest 3-degree run spans 9 steps; 5 and 10 degrees see the same funnel."""
    G = 24
    initial = (np.linspace(-1.0, 1.0, G) + 1.0) * 180.0
    ori = np.linspace(-1.0, 1.0, G).copy()
    ori[4:14] = 100.0 / 180.0 - 1.0 + np.linspace(0.0, 2.5, 10) / 180.0        # 100 .. 102.5 degrees
    pose = np.stack([ori, np.zeros(G), np.zeros(G)], axis=1)
    m = predicted.build_metric(logits(G), THR, STD, (-1.0, 1.0), final_pose=pose, left=np.full(G, -1), rollout_interactions=40)
    assert float(np.diff(initial).min()) > 10.0
    obj = metric2objective(m, 'convergence')
    assert int(obj['max_convergence_range_3deg']) == 9 and int(obj['max_convergence_range_5deg']) == 9 and int(obj['max_convergence_range_10deg']) == 9
    one = metric2objective(predicted.build_metric(logits(G), THR, STD, (-1.0, 1.0)), 'convergence')
    assert int(one['max_convergence_range_3deg']) < 9            # one interaction of a random model funnels nothing like it


def test_rollout_flag_needs_predicted_sim():
    from dgdm_amd.generator.train import train
    with pytest.raises(ValueError, match="--predicted_sim"):
        train(parse(["--mode=test", "--predicted_rollout=3"]))
    with pytest.raises(ValueError, match="negative"):
        predicted.PredictedSimulator(None, rollout_interactions=-1)
