"""Host side of the squeeze simulator: the contract as tests/squeeze_oracle.py states it against closed-form results of frictionless
squeezing (Goldberg's diameter function for flat jaws, a disc in a V), its edge rules (loose objects, snapping, k = 0, k past every path),
the dataset writer's files through DynamicsDataset, and the command line's refusals.  No GPU."""
import json
import os

import numpy as np
import pytest

from tests import squeeze_oracle as so

M = 200
FLAT = np.stack([np.full(M, -0.12), np.full(M, 0.15)])         # control values such that yl = yr = 0
RECT = np.array([[-0.03, -0.015], [0.03, -0.015], [0.03, 0.015], [-0.03, 0.015]])       # 0.06 x 0.03 m


def grid_starts(T, X, x_half, y0=0.0):
    return np.array([[2.0 * np.pi * a / T, -x_half + b * (2.0 * x_half / (X - 1)), y0] for a in range(T) for b in range(X)])


@pytest.fixture(scope="module")
def rect_run():
    T, X = 360, 5
    return T, X, so.squeeze_pair(FLAT[0], FLAT[1], RECT, so.rotation_table(T), grid_starts(T, X, 0.06), X, 0.06, 1, 6, 0.2)


def test_rectangle_settles_as_the_diameter_function_says(rect_run):
    """Between flat jaws S = (0.27 - w(theta)) / 2 with the width w = 0.06 |sin| + 0.03 |cos|: four stable orientations, basins edged by
    atan 2 = 63.43 degrees and its mirrors.  All 360 x 5 rows, none excluded."""
    T, X, r = rect_run
    a0, af = r["cells"][:, 0] // X, r["cells"][:, 2] // X
    assert np.array_equal(r["cells"][:, 0], np.arange(T * X))
    assert sorted(set(af.tolist())) == [0, 90, 180, 270]
    edge = np.degrees(np.arctan(2.0))
    want = np.where((a0 < edge) | (a0 > 360 - edge), 0, np.where(a0 < 180 - edge, 90, np.where(a0 < 180 + edge, 180, 270)))
    assert np.array_equal(af, want)
    th = 2.0 * np.pi * np.arange(T) / T
    w = 0.06 * np.abs(np.sin(th)) + 0.03 * np.abs(np.cos(th))
    assert np.allclose(r["S"], ((0.27 - w) / 2.0)[:, None], rtol=0, atol=1e-15)
    assert not (r["flags"] & 3).any()


def test_rectangle_never_changes_its_x_cell(rect_run):
    """S does not depend on x here, so every neighbour in x ties: the visiting order must prefer the pure rotation."""
    T, X, r = rect_run
    assert np.array_equal(r["cells"][:, 1] % X, r["cells"][:, 0] % X) and np.array_equal(r["cells"][:, 2] % X, r["cells"][:, 0] % X)
    assert np.allclose(r["y"], 0.015, rtol=0, atol=1e-15)          # centred between L = -0.12 and U = 0.15


def test_disc_settles_in_the_v():
    T, X = 8, 81
    u = -0.12 + np.arange(M) * (0.24 / (M - 1))
    lower, upper = -0.12 + 0.5 * np.abs(u - 0.04), 0.15 - 0.5 * np.abs(u - 0.04)
    ang = 2.0 * np.pi * np.arange(60) / 60
    disc = 0.04 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    r = so.squeeze_pair(lower, upper, disc, so.rotation_table(T), grid_starts(T, X, 0.06), X, 0.06, 2, 6, 0.2)
    _, x = so.cell_pose(r["cells"][:, 2], T, X, 0.06)
    assert np.abs(x - 0.04).max() <= 0.0015 + 1e-12
    assert not r["flags"].any()


def test_loose_object_stays_where_it_is():
    """Default travel_max = 0.1: the jaws close fully before both touch the 3 cm rectangle (S >= 0.1015 everywhere)."""
    T, X = 360, 5
    st = grid_starts(T, X, 0.06)
    st[:, 2] = np.where(np.arange(len(st)) % 3 == 0, 0.2, np.where(np.arange(len(st)) % 3 == 1, -0.2, 0.015))
    r = so.squeeze_pair(FLAT[0], FLAT[1], RECT, so.rotation_table(T), st, X, 0.06, 1, 6, 0.1)
    assert r["S"].min() >= 0.1014 and (r["flags"] & 3 == 3).all()
    assert np.array_equal(r["cells"][:, 1], r["cells"][:, 0]) and np.array_equal(r["cells"][:, 2], r["cells"][:, 0])
    tl, tr = r["touch_l"].reshape(-1)[r["cells"][:, 0]], r["touch_r"].reshape(-1)[r["cells"][:, 0]]
    assert np.array_equal(r["y"][:, 0], np.clip(st[:, 2], 0.1 - tl, tr - 0.1)) and np.array_equal(r["y"][:, 0], r["y"][:, 1])
    assert (r["y"][2::3, 0] == 0.015).all() and (r["y"][0::3, 0] < 0.2).all() and (r["y"][1::3, 0] > -0.2).all()


def test_starts_snap_to_the_nearest_cell():
    T, X, xh = 48, 17, 0.06
    dth, dx = so.TWO_PI / T, 0.12 / 16
    st = np.array([[0.49 * dth, 0.0, 0], [0.5 * dth, 0.0, 0], [-0.5 * dth, 0.0, 0], [-0.51 * dth, 0.0, 0], [so.TWO_PI + 3.2 * dth, 0.0, 0],
                   [-so.TWO_PI - 3.2 * dth, 0.0, 0], [47.6 * dth, 0.0, 0], [0, -1.0, 0], [0, 1.0, 0], [0, -xh + 2.5 * dx, 0], [0, -xh + 2.49 * dx, 0],
                   [0, np.nan, 0], [np.nan, 0, 0], [np.inf, np.inf, 0]])
    c = so.snap(st, T, X, xh)
    assert (c // X).tolist() == [0, 1, 0, 47, 3, 45, 0, 0, 0, 0, 0, 0, 0, 0]
    assert (c % X).tolist() == [8, 8, 8, 8, 8, 8, 8, 0, 16, 3, 2, 0, 8, 16]


def lobes():
    a = 2.0 * np.pi * np.arange(40) / 40
    r = 0.035 * (1.0 + 0.25 * np.cos(3 * a))
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


def test_closing_steps_zero_is_the_identity_and_many_is_settled():
    T, X = 48, 17
    rs = np.random.RandomState(0)
    u = np.linspace(-1, 1, 50)
    lower, upper = -0.12 + 0.01 * np.cos(2.5 * u + rs.uniform(0, 6)), 0.15 + 0.01 * np.cos(3.5 * u + rs.uniform(0, 6))
    st = grid_starts(T, X, 0.06)
    kw = dict(x_cells=X, x_half=0.06, window=2, travel_max=0.1)
    r0 = so.squeeze_pair(lower, upper, lobes(), so.rotation_table(T), st, closing_steps=0, **kw)
    r3 = so.squeeze_pair(lower, upper, lobes(), so.rotation_table(T), st, closing_steps=3, **kw)
    rN = so.squeeze_pair(lower, upper, lobes(), so.rotation_table(T), st, closing_steps=10 ** 6, **kw)
    assert np.array_equal(r0["cells"][:, 1], r0["cells"][:, 0])
    assert np.array_equal(rN["cells"][:, 1], rN["cells"][:, 2]) and np.array_equal(rN["y"][:, 0], rN["y"][:, 1])
    succ = r3["succ"].astype(np.int64)
    assert np.array_equal(r3["cells"][:, 1], succ[succ[succ[r3["cells"][:, 0]]]])
    S = r3["S"].reshape(-1)
    moved = succ != np.arange(T * X)
    assert moved.any() and (S[succ[moved]] > S[moved]).all()                   # S rises strictly along a path
    assert np.array_equal(succ[r3["cells"][:, 2]], r3["cells"][:, 2])          # settled cells are fixed points
    assert (so.candidates(1)[:2] == [(-1, 0), (1, 0)]) and len(so.candidates(2)) == 24


def fake_pair(T=360, X=41):
    from dgdm_amd.sim import sim_2d
    starts = sim_2d.pose_grid()
    r = so.squeeze_pair(FLAT[0] + 0.01 * np.cos(np.linspace(0, 5, M)), FLAT[1], lobes(), so.rotation_table(T), starts, X, 0.06, 2, 6, 0.1)
    th, x = so.cell_pose(r["cells"], T, X, 0.06)
    start = np.stack([th[:, 0], x[:, 0]], axis=1)
    closed = np.stack([th[:, 1], x[:, 1], r["y"][:, 0]], axis=1)
    ctrl = np.stack([np.tile(np.linspace(-0.12, 0.12, 7), 2), np.zeros(14)], axis=1)
    allpts = np.stack([np.tile(np.linspace(-0.12, 0.12, M), 2), np.zeros(2 * M)], axis=1)
    return sim_2d.pair_record(ctrl, allpts, lobes(), starts, start, closed), starts


def test_writer_files_go_through_the_dataset(tmp_path):
    from dgdm_amd import engine
    from dgdm_amd.dynamics.dataloader import SCORE_STD, DynamicsDataset, load_score_stats
    from dgdm_amd.sim import sim_2d
    rec, starts = fake_pair()
    assert list(rec) == ["ctrlpts", "allpts", "object_vertices", "obj_pos", "obj_theta", "delta_theta", "delta_pos"]
    shapes = {k: (v.shape, v.dtype) for k, v in rec.items()}
    assert shapes == {"ctrlpts": ((14, 2), np.float64), "allpts": ((400, 2), np.float64), "object_vertices": ((40, 2), np.float64),
                      "obj_pos": ((9000, 3), np.float64), "obj_theta": ((9000,), np.float32), "delta_theta": ((9000,), np.float32),
                      "delta_pos": ((9000, 3), np.float64)}
    # pose order: theta-major, then x, then y, by the reference's formulae (sim/sim_2d.py:139-146)
    z_rots, locs = np.arange(0.0, 2 * np.pi, 2 * np.pi / 360), -0.03 + 0.06 * np.arange(5) / 4
    k, i, j = 217, 3, 1
    row = (k * 5 + i) * 5 + j
    assert rec["obj_theta"][row] == np.float32(z_rots[k]) and rec["obj_pos"][row].tolist() == [locs[i], locs[j], 0.0]
    assert np.abs(rec["delta_theta"]).max() <= np.pi and rec["delta_theta"].any() and (rec["delta_pos"][:, 2] == 0).all()
    files = sim_2d.write_dataset(str(tmp_path), [(7, 3, rec), (7, 4, rec)], engine.squeeze_config(theta_cells=360, x_cells=41), 5)
    assert [os.path.basename(f) for f in files] == ["7_3.npz", "7_4.npz"]
    stats = json.load(open(tmp_path / "stats.json"))
    assert stats["simulated"] == "squeeze" and stats["config"]["x_cells"] == 41 and stats["config"]["closing_steps"] == 6 and stats["loose_starts"] == 5
    std = np.array([rec["delta_theta"].astype(np.float64).std(), rec["delta_pos"][:, 0].std(), rec["delta_pos"][:, 1].std()])
    assert np.allclose(stats["score_std"], std, rtol=1e-12)
    d = np.load(files[0], allow_pickle=True)['arr_0'].item()
    assert list(d) == list(rec) and all(np.array_equal(d[k], rec[k]) for k in rec)
    plain, own = DynamicsDataset(str(tmp_path), object_max_num_vertices=40), DynamicsDataset(str(tmp_path), object_max_num_vertices=40,
                                                                                             **load_score_stats(str(tmp_path / "stats.json")))
    assert len(plain) == 2 and np.array_equal(plain.std, SCORE_STD[1]) and np.allclose(own.std, std) and np.array_equal(own.threshold, plain.threshold)
    a, b = plain[0], own[0]
    assert a['scores'].shape == (9000, 3) and a['input_ori'].shape == (9000,) and a['input_pos'].shape == (9000, 2) and a['object_vertices'].shape == (40, 2)
    assert np.allclose(b['scores'].numpy() * std, a['scores'].numpy() * SCORE_STD[1], rtol=1e-5, atol=1e-9)
    assert np.allclose(b['scores'].numpy().std(axis=0), 1.0, atol=1e-3)
    assert float(a['input_ori'].min()) == -1.0 and float(a['input_pos'].abs().max()) == 1.0
    with pytest.raises(ValueError, match="score_std"):
        DynamicsDataset(str(tmp_path), score_std=[1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="score_threshold"):
        DynamicsDataset(str(tmp_path), score_threshold=[1.0, 2.0])


def test_flag_refusals():
    from dgdm_amd.generator.train import squeeze_from_args, train
    from dynamics.parser import parse
    base = "--mode=test --classifier_guidance --ctrlpts_dim=14 --object_max_num_vertices=100 --num_fingers=2 --batch_size=2"
    assert squeeze_from_args(parse(base.split())) is None
    assert squeeze_from_args(parse((base + " --squeeze_sim").split())) == {}
    assert squeeze_from_args(parse((base + " --squeeze_sim --squeeze_closing_steps 9 --squeeze_window 3").split())) == {"closing_steps": 9, "window": 3}
    for extra, why in ((" --squeeze_sim --fingers_3d", "2-D only"), (" --squeeze_sim --predicted_sim", "choose one"),
                       (" --squeeze_window 2", "need --squeeze_sim"), (" --squeeze_sim --squeeze_window 0", "at least 1"),
                       (" --squeeze_sim --squeeze_closing_steps -1", "negative"),
                       (" --squeeze_sim --goal_pose=30,0,0", "--goal_pose")):
        with pytest.raises(ValueError, match=why):
            train(parse((base + extra).split()))                  # refused before anything is built: no device is touched
    with pytest.raises(ValueError, match="--mode=test"):
        squeeze_from_args(parse((base.replace("--mode=test", "--mode=train") + " --squeeze_sim").split()))
    with pytest.raises(ValueError, match="--classifier_guidance"):
        squeeze_from_args(parse((base.replace(" --classifier_guidance", "") + " --squeeze_sim").split()))


def test_simulated_mark_travels_through_the_tables(tmp_path):
    """The table builders mark scores made from squeeze metrics 'simulated': 'squeeze' and never 'predicted'."""
    from dgdm_amd.generator import artefacts
    from dgdm_amd.generator.diffusion import Diffusion
    from dgdm_amd.sim.squeeze import squeeze_metric
    rs = np.random.RandomState(3)
    n = 360

    def metric():
        st = np.stack([np.linspace(0, 2 * np.pi, n, endpoint=False), np.zeros(n)], axis=1)
        cl = np.concatenate([st + rs.normal(0, [0.05, 0.003], (n, 2)), rs.normal(0, 0.004, (n, 1))], axis=1)
        return squeeze_metric(st, cl, cl, rs.randint(0, 8, n))
    metrics = [metric() for _ in range(4)]
    assert all('predicted' not in m and m['simulated'] == 'squeeze' for m in metrics)
    none = [None] * 4
    sim = (list(none), metrics, list(none), list(none), list(none), list(none), [[] for _ in none], list(none))
    model, log = Diffusion.__new__(Diffusion), artefacts.TableLog(str(tmp_path))
    artefacts.unguided_table(model, log, sim, [None] * 2, 2, 2, 'shift_up', [-1.0, 1.0], False)
    artefacts.guided_table(model, log, [tuple(s[i * 2:(i + 1) * 2] for s in sim) for i in range(2)], 'rotate', [-1.0, 1.0])
    artefacts.multi_object_table(model, log, [tuple([s[g], s[2 + g]] for s in sim) for g in range(2)], 2, 'clockwise_left', [-1.0, 1.0])
    for key in log.keys:
        t = json.load(open(tmp_path / "tables" / (key.replace("/", "__") + ".json")))
        oc = t["columns"].index("objective")
        rows = [row[oc] for row in t["data"] if isinstance(row[oc], dict) and "success_rate" in row[oc] and row[0] != -1]
        assert rows and all(r.get("simulated") == "squeeze" and "predicted" not in r for r in rows), key
