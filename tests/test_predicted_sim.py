"""Host side of the predicted scores (dgdm_amd/dynamics/predicted.py): the dicts built from the dynamics model's grid tally / centre-row
logits equal what the harness's own ``metric2objective`` gives on the equivalent hand-made simulator ``metric``, for all 16 objectives,
and the selection helpers of ``Diffusion`` run on them.  No GPU."""
import numpy as np
import pytest

from dgdm_amd.dynamics import predicted as pr
from dgdm_amd.dynamics.metrics import metric2objective
from dgdm_amd.generator.diffusion import OBJECTIVE_SWEEP, Diffusion

SIGNED = ['rotate_clockwise', 'rotate_counterclockwise', 'shift_up', 'shift_down', 'shift_left', 'shift_right'] + \
         [f'{r}_{s}' for r in ('clockwise', 'counterclockwise') for s in ('up', 'down', 'left', 'right')]
ALL16 = ['rotate', 'convergence'] + SIGNED
THR = [0.53, 0.77, 0.64]                 # threshold / std
STD = [0.0565, 0.0026, 0.0047]           # rad, m, m (the 2-D dataset's)


def hand_logits(seed, n):
    """Normalised outputs with all three classes in every column and a few values exactly ON a threshold (class 1 on both sides)."""
    rs = np.random.RandomState(seed)
    l = (rs.randn(n, 3) * 1.2).astype(np.float32)
    l[0], l[1] = np.float32(THR), -np.float32(THR)
    return l


def hand_metric(l, ori_range=(-1.0, 1.0)):
    """The simulator's metric dict (dynamics/sim_test_mj.py:209-218) written out by hand for motions that ARE the un-normalised
    logits: degrees, centimetres, profiles = class + 1 of the -1 / 0 / 1 rule of :198-200, finals by the one-step convention."""
    l = np.asarray(l, dtype=np.float32)
    dth = np.array([float(v) * STD[0] * 180.0 / np.pi for v in l[:, 0]])
    dpos = np.array([[float(a) * STD[1] * 100.0, float(b) * STD[2] * 100.0, 0.0] for a, b in l[:, 1:]])
    prof = [np.array([1 if v > np.float32(THR[k]) else -1 if v < -np.float32(THR[k]) else 0 for v in l[:, k]]) + 1 for k in range(3)]
    init = (np.linspace(ori_range[0], ori_range[1], len(l)) + 1.0) * 180.0
    return {'delta_theta': dth, 'delta_pos': dpos, 'profile': prof[0], 'profile_x': prof[1], 'profile_y': prof[2],
            'final_theta': init + dth, 'final_delta_theta': dth, 'final_pos': dpos}


def tally(l):
    cls = [hand_metric(l)[k] for k in ('profile', 'profile_x', 'profile_y')]
    counts = np.zeros((3, 3, 3), dtype=np.int32)
    for a, b, c in zip(*cls):
        counts[a, b, c] += 1
    sums = np.array([l[:, 0].sum(dtype=np.float64), np.abs(l[:, 0]).sum(dtype=np.float64), l[:, 1].sum(dtype=np.float64),
                     l[:, 2].sum(dtype=np.float64)], dtype=np.float32)
    return counts, sums


def same(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert np.asarray(a[k]).dtype.kind == np.asarray(b[k]).dtype.kind, k
        if np.asarray(b[k]).dtype.kind in 'iu':
            assert a[k] == b[k], k
        else:
            assert a[k] == pytest.approx(b[k], rel=1e-6, abs=1e-9), k      # float32 sums of the tally against float64 means


def test_all_16_objectives_are_covered():
    assert len(ALL16) == 16 and set(OBJECTIVE_SWEEP) <= set(ALL16)


@pytest.mark.parametrize("opt_obj", ['rotate'] + SIGNED)
def test_predicted_objective_equals_metric2objective(opt_obj):
    l = hand_logits(1, 45)
    counts, sums = tally(l)
    same(pr.predicted_objective(counts, sums, len(l), STD, opt_obj), metric2objective(hand_metric(l), opt_obj))


def test_predicted_objective_rejects_what_a_histogram_cannot_say():
    counts, sums = tally(hand_logits(1, 45))
    with pytest.raises(ValueError, match="convergence"):
        pr.predicted_objective(counts, sums, 45, STD, 'convergence')
    with pytest.raises(ValueError, match="n_cells"):
        pr.predicted_objective(counts, sums, 44, STD, 'rotate')
    with pytest.raises(ValueError, match="opt obj not supported"):
        pr.predicted_objective(counts, sums, 45, STD, 'wiggle')


@pytest.mark.parametrize("opt_obj", ALL16)
def test_metric_builder_equals_hand_made_metric(opt_obj):
    rng = (-0.5, 1.0)
    l = hand_logits(2, 60)
    m = pr.build_metric(l, THR, STD, rng)
    assert m['predicted'] is True
    hand = hand_metric(l, rng)
    for k in hand:
        assert m[k].shape == hand[k].shape and np.allclose(m[k], hand[k], rtol=1e-12, atol=0), k
    same(metric2objective(m, opt_obj), metric2objective(hand, opt_obj))


def test_center_rows_and_even_grid():
    B, G, P = 3, 4, 5
    cell = np.arange(G * P * P)
    rows = np.repeat(cell, B) * 10 + np.tile(np.arange(B), G * P * P)          # row = cell * B + finger
    logits = np.stack([rows, rows, rows], axis=-1)[None].astype(np.float32)
    c = pr.center_rows(logits, B, G, P)
    assert c.shape == (1, B, G, 3)
    for b in range(B):
        for g in range(G):
            assert c[0, b, g, 0] == ((g * P + 2) * P + 2) * 10 + b
    with pytest.raises(ValueError, match="even"):
        pr.center_rows(logits[:, :B * G * 16], B, G, 4)
    with pytest.raises(ValueError, match="even"):
        pr.center_index(2)


@pytest.mark.parametrize("opt_obj", ALL16)
def test_selection_helpers_run_on_predicted_scores(opt_obj):
    n_obj, n_grip = 2, 3
    objs = [metric2objective(pr.build_metric(hand_logits(10 + i, 36), THR, STD), opt_obj) for i in range(n_obj * n_grip)]
    best = Diffusion.get_best_ids_all_metrics(None, objs[:n_grip], opt_obj=opt_obj)
    assert best and all(0 <= int(v) < n_grip for v in best.values())
    per_obj = Diffusion.get_best_ids(Diffusion.__new__(Diffusion), objs, n_grip, n_obj, opt_obj=opt_obj)
    assert len(per_obj) == n_obj and all(n_grip <= int(v) < 2 * n_grip for v in per_obj[1].values())
    assert 0 <= int(Diffusion.get_average_best_ids(None, objs[:n_grip], opt_obj=opt_obj)) < n_grip


def test_tables_accept_predicted_metrics_and_leave_simulator_tables_alone(tmp_path):
    """The three table builders take the predicted simulator's output (plot slots None, no videos, metrics flagged) and mark the scores;
    a simulator's metrics (no flag) give the same tables as before."""
    import json
    from dgdm_amd.generator import artefacts
    n_obj, n_grip = 2, 2
    model = Diffusion.__new__(Diffusion)
    for flagged in (True, False):
        metrics = [pr.build_metric(hand_logits(20 + i, 360), THR, STD) for i in range(n_obj * n_grip)]
        if not flagged:
            for m in metrics:
                del m['predicted']
        none = [None] * (n_obj * n_grip)
        sim = (list(none), metrics, list(none), list(none), list(none), list(none), [[] for _ in none], list(none))
        log = artefacts.TableLog(str(tmp_path / str(flagged)))
        artefacts.unguided_table(model, log, sim, [None] * n_grip, n_obj, n_grip, 'shift_up', [-1.0, 1.0], False)
        per_obj = [tuple(s[i * n_grip:(i + 1) * n_grip] for s in sim) for i in range(n_obj)]
        artefacts.guided_table(model, log, per_obj, 'rotate', [-1.0, 1.0])
        per_grip = [tuple([s[g], s[n_grip + g]] for s in sim) for g in range(n_grip)]
        artefacts.multi_object_table(model, log, per_grip, n_obj, 'clockwise_left', [-1.0, 1.0])
        assert len(log.keys) == 3
        for key in log.keys:
            t = json.load(open(tmp_path / str(flagged) / "tables" / (key.replace("/", "__") + ".json")))
            oc = t["columns"].index("objective")
            marks = [row[oc].get("predicted") for row in t["data"] if isinstance(row[oc], dict) and "success_rate" in row[oc] and row[0] != -1]
            assert marks and all(v is (True if flagged else None) for v in marks), key
