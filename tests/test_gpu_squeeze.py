"""The squeeze simulator on the device (csrc/squeeze.hip) against its float64 CPU restatement tests/squeeze_oracle.py.

Every operation of the contract (include/dgdm_hip.h "squeeze simulator") is a basic IEEE float64 one or an int32 one, so nothing here
has a tolerance: the three tables and y are compared bit for bit, the successor array, the three cells per start and the flags as
integers, with no row excluded.  Shapes: 48 orientations; 17 and 70 x cells (no multiples of 64, 70 > one wave); 200 and 9 surface
samples; 3, 4, 12 and 100 vertices; two fingers x three objects in two chunks (the workspace holds four pairs); windows 1 and 3;
closings of 0, 1 and 7 steps.  The object sets hold a polygon with vertical edges, one large enough (with x_half = 0.1) that vertices and
edge spans pass the finger ends, and one wholly beyond the finger ends at some cells (S = +inf)."""
import ctypes as C
import functools
import json
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine
from tests import squeeze_oracle as so

pytestmark = pytest.mark.gpu

THETA = 48
HL = 0.12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def ngon(n, radius, lobes=0, depth=0.0, centre=(0.0, 0.0), phase=0.0, reverse=False):
    a = phase + 2.0 * np.pi * np.arange(n) / n
    r = radius * (1.0 + depth * np.cos(lobes * a))
    p = np.stack([centre[0] + r * np.cos(a), centre[1] + r * np.sin(a)], axis=1)
    return p[::-1].copy() if reverse else p


def surfaces(m, seed):
    """Two smooth random jaw surfaces around the flat ones (L = -0.12, U = 0.15)."""
    rs = np.random.RandomState(seed)
    u = np.linspace(-1.0, 1.0, m)
    bump = lambda: sum(rs.uniform(-0.012, 0.012) * np.cos(k * np.pi * u + rs.uniform(0, 6)) for k in range(1, 4))      # noqa: E731
    return np.stack([-0.12 + bump(), 0.15 + bump()])


def objects(nv):
    if nv == 4:          # an axis-aligned rectangle (vertical edges at theta = 0, clockwise), a square, a rectangle off its origin
        rect = np.array([[-0.03, -0.015], [-0.03, 0.015], [0.03, 0.015], [0.03, -0.015]])
        return np.stack([rect, ngon(4, 0.02, phase=np.pi / 4), np.array([[0.0, 0.0], [0.05, 0.0], [0.05, 0.02], [0.0, 0.02]])])
    if nv == 3:          # the second spans every finger sample, the third lies past the finger ends at some orientations
        return np.stack([ngon(3, 0.03), ngon(3, 0.2, phase=0.3), ngon(3, 0.02, centre=(0.2, 0.0), reverse=True)])
    # a lobed contour, one that passes the finger ends, one wholly beyond them at theta near 0 and pi
    return np.stack([ngon(nv, 0.035, 3, 0.25), ngon(nv, 0.15, 2, 0.3, phase=0.2), ngon(nv, 0.03, 5, 0.2, centre=(0.21, 0.01), reverse=True)])


def starts(x_half, n=40, seed=5):
    rs = np.random.RandomState(seed)
    st = np.stack([rs.uniform(-7.0, 14.0, n), rs.uniform(-1.3 * x_half, 1.3 * x_half, n), rs.uniform(-0.05, 0.05, n)], axis=1)
    dth = so.TWO_PI / THETA
    st[0] = (0.5 * dth, 0.0, 0.0)                      # halves round up
    st[1] = (-0.5 * dth, -x_half, 0.2)
    st[2] = (so.TWO_PI - 0.25 * dth, x_half, -0.2)     # wraps to cell 0
    st[3] = (np.nan, np.nan, 0.0)                      # non-finite starts land on cell 0, no index leaves the table
    st[4] = (np.inf, -np.inf, 0.01)
    st[5] = (1e300, 1e300, np.nan)
    return st


# name: (nv, m, X, x_half, R, k)
CASES = {"rect_k0": (4, 200, 17, 0.06, 1, 0), "lobes_k7": (100, 200, 70, 0.1, 3, 7), "tri_k1": (3, 9, 17, 0.1, 3, 1),
         "dodecagon_k7": (12, 9, 70, 0.1, 1, 7), "settles": (12, 200, 17, 0.06, 3, 1 << 20)}
PAIRS = [(f, o) for o in range(3) for f in range(2)]


def case_inputs(name):
    nv, m, X, x_half, R, k = CASES[name]
    cfg = dict(theta_cells=THETA, x_cells=X, x_half=x_half, window=R, closing_steps=k, travel_max=0.1, finger_half_len=HL)
    return np.stack([surfaces(m, 1), surfaces(m, 2)]), objects(nv), starts(x_half), cfg


@functools.lru_cache(maxsize=None)
def reference(name):
    sf, ob, st, cfg = case_inputs(name)
    return so.squeeze_map(sf, ob, PAIRS, so.rotation_table(THETA), st, x_cells=cfg["x_cells"], x_half=cfg["x_half"], window=cfg["window"],
                          closing_steps=cfg["closing_steps"], travel_max=cfg["travel_max"], half_len=HL)


def run(name, chunk_pairs=4, slack=0):
    """slack: bytes on top of the size the library gives for chunk_pairs, which must still hold no further pair."""
    sf, ob, st, cfg = case_inputs(name)
    ws = _lib.lib().dgdm_squeeze_workspace_bytes(C.byref(engine.squeeze_config(**cfg)), chunk_pairs) + slack
    assert slack == 0 or ws < _lib.lib().dgdm_squeeze_workspace_bytes(C.byref(engine.squeeze_config(**cfg)), chunk_pairs + 1)
    out = engine.squeeze_tables(sf, ob, PAIRS, st, rot=so.rotation_table(THETA), tables=True, workspace_bytes=int(ws), **cfg)
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", list(CASES))
def test_tables_and_maps_equal_the_oracle(dev, name):
    got, ref = run(name), reference(name)
    if name == "lobes_k7":                            # the case is what its docstring says it is
        assert np.isinf(ref["S"][4]).any() and np.isfinite(ref["S"][4]).any() and (ref["flags"] & 1).any()
    for k in ("touch_l", "touch_r", "S"):
        bad = np.argwhere(bits(got[k]) != bits(ref[k]))
        assert len(bad) == 0, f"{k}: {len(bad)} cells differ, first (pair, a, b) = {bad[0]}: {got[k][tuple(bad[0])]!r} vs {ref[k][tuple(bad[0])]!r}"
    assert np.array_equal(got["succ"], ref["succ"])
    assert np.array_equal(got["cells"], ref["cells"])
    assert np.array_equal(bits(got["y"]), bits(ref["y"]))
    assert np.array_equal(got["flags"], ref["flags"])


def test_repeated_calls_and_chunkings_are_bit_identical(dev):
    a, b, c = run("lobes_k7"), run("lobes_k7"), run("lobes_k7", chunk_pairs=1)
    d = run("lobes_k7", slack=1000)                       # still chunks of 4 pairs, in a workspace of no size the library returns
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), k
        assert np.array_equal(a[k].view(np.uint8), d[k].view(np.uint8)), k


def test_rectangle_between_flat_jaws_follows_the_diameter_function(dev):
    """0.06 x 0.03 m rectangle, flat jaws (control values 0 in metres): every start settles as the diameter function
    0.06 |sin| + 0.03 |cos| says - basins edged by atan 2 = 63.43 degrees and its mirrors - and none changes its x cell."""
    from dgdm_amd.sim import squeeze
    T, X = 360, 5
    rect = np.array([[-0.03, -0.015], [0.03, -0.015], [0.03, 0.015], [-0.03, 0.015]])
    st = np.array([[2.0 * np.pi * a / T, -0.06 + b * 0.03, 0.0] for a in range(T) for b in range(X)])
    out = squeeze.squeeze_map(torch.zeros(1, 14), rect[None], st, scale=1.0, offset=0.0, theta_cells=T, x_cells=X, travel_max=0.2, window=1)
    cells, flags = out["cells"].cpu().numpy()[0], out["flags"].cpu().numpy()[0]
    assert np.array_equal(cells[:, 0], np.arange(T * X))
    edge_cell = (cells[:, 0] % X == 0) | (cells[:, 0] % X == X - 1)
    assert np.array_equal(flags, np.where(edge_cell, 4, 0))    # nothing loose; the outer x cells say that the table ends there
    deg = cells[:, 0] // X
    edge = np.degrees(np.arctan(2.0))
    want = np.where((deg < edge) | (deg > 360 - edge), 0, np.where(deg < 180 - edge, 90, np.where(deg < 180 + edge, 180, 270)))
    assert np.array_equal(cells[:, 2] // X, want)
    assert np.array_equal(cells[:, 2] % X, cells[:, 0] % X) and np.array_equal(cells[:, 1] % X, cells[:, 0] % X)
    # default travel_max: the 3 cm rectangle is loose everywhere - theta and x unchanged, y clamped as defined
    st2 = st.copy()
    st2[:, 2] = np.where(np.arange(len(st)) % 2 == 0, 0.2, -0.2)
    loose = squeeze.squeeze_map(torch.zeros(1, 14), rect[None], st2, scale=1.0, offset=0.0, theta_cells=T, x_cells=X, window=1, tables=True)
    lc, S = loose["cells"].cpu().numpy()[0], loose["S"].cpu().numpy()[0]
    assert S.min() >= 0.1 and (loose["flags"].cpu().numpy()[0] & 3 == 3).all()
    assert np.array_equal(lc[:, 1], lc[:, 0]) and np.array_equal(lc[:, 2], lc[:, 0])
    tl, tr = loose["touch_l"].cpu().numpy()[0].reshape(-1), loose["touch_r"].cpu().numpy()[0].reshape(-1)
    want_y = np.clip(st2[:, 2], 0.1 - tl[lc[:, 0]], tr[lc[:, 0]] - 0.1)
    assert np.array_equal(loose["y"].cpu().numpy()[0][:, 1], want_y)


def test_disc_settles_in_the_v(dev):
    """A 60-gon disc of radius 0.04 under V-shaped jaws with their apex at x = 0.04: every start settles within one cell of it."""
    m, T, X = 200, 8, 81
    u = -HL + np.arange(m) * (2 * HL / (m - 1))
    sf = np.stack([-0.12 + 0.5 * np.abs(u - 0.04), 0.15 - 0.5 * np.abs(u - 0.04)])[None]
    st = np.array([[2.0 * np.pi * a / T, -0.06 + b * 0.0015, 0.0] for a in range(T) for b in range(X)])
    out = engine.squeeze_tables(sf, ngon(60, 0.04)[None], [(0, 0)], st, theta_cells=T, x_cells=X, x_half=0.06, travel_max=0.2)
    _, x = so.cell_pose(out["cells"].cpu().numpy()[0, :, 2], T, X, 0.06)
    assert np.abs(x - 0.04).max() <= 0.0015 + 1e-12 and not out["flags"].cpu().numpy().any()


def test_every_bad_argument_is_refused_before_a_launch(dev):
    lib = _lib.lib()
    sf = torch.zeros(2, 2, 8, dtype=torch.float64, device=dev)
    ob = torch.zeros(3, 4, 2, dtype=torch.float64, device=dev)
    rot = torch.zeros(8, 2, dtype=torch.float64, device=dev)
    st = torch.zeros(2, 3, dtype=torch.float64, device=dev)
    cells = torch.full((1, 2, 3), -7, dtype=torch.int32, device=dev)
    y = torch.zeros(1, 2, 2, dtype=torch.float64, device=dev)
    flags = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    good = dict(theta_cells=8, x_cells=5, window=1, closing_steps=2, x_half=0.06, travel_max=0.1, finger_half_len=0.12)
    ws_bytes = int(lib.dgdm_squeeze_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def call(cfg=None, m=8, nv=4, pair=(1, 2), n_pairs=1, nf=2, no=3, surf=sf, ws_b=ws_bytes, cells_out=cells):
        c = engine.squeeze_config(**dict(good, **(cfg or {})))
        pr = np.array([pair], dtype=np.int32)
        return lib.dgdm_squeeze_map(C.byref(c), _lib.dptr(surf), nf, m, _lib.dptr(ob), no, nv, pr.ctypes.data, n_pairs, _lib.dptr(rot), _lib.dptr(st), 2,
                                    _lib.dptr(cells_out), _lib.dptr(y), _lib.dptr(flags), None, None, None, None, _lib.dptr(ws), ws_b, None)

    bad = [dict(cfg=dict(theta_cells=0)), dict(cfg=dict(x_cells=1)), dict(cfg=dict(theta_cells=1 << 20, x_cells=1 << 11)), dict(cfg=dict(window=0)),
           dict(cfg=dict(closing_steps=-1)), dict(cfg=dict(x_half=0.0)), dict(cfg=dict(x_half=float("nan"))), dict(cfg=dict(x_half=float("inf"))),
           dict(cfg=dict(travel_max=float("inf"))), dict(cfg=dict(finger_half_len=-0.1)), dict(m=1), dict(m=4096), dict(nv=2), dict(nv=4096),
           dict(pair=(2, 0)), dict(pair=(0, 3)), dict(pair=(-1, 0)), dict(n_pairs=0), dict(nf=0), dict(no=0), dict(surf=None),
           dict(ws_b=ws_bytes - 1), dict(cells_out=None)]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.dgdm_last_error()
    torch.cuda.synchronize()
    assert (cells.cpu() == -7).all()                          # nothing was launched
    assert call() == _lib.OK and (cells.cpu() >= 0).all()
    assert lib.dgdm_squeeze_workspace_bytes(C.byref(engine.squeeze_config(**dict(good, window=0))), 1) == _lib.EINVAL
    assert lib.dgdm_squeeze_workspace_bytes(C.byref(engine.squeeze_config(**good)), 0) == _lib.EINVAL
    with pytest.raises(ValueError, match="window"):
        engine.squeeze_tables(sf, ob, [(0, 0)], st, window=0)


def test_squeeze_simulator_fills_the_tables(dev, tmp_path):
    """--squeeze_sim through the command-line entry point on a synthetic 2-D model: the unguided / guided / multi-object tables are
    written, every score carries 'simulated': 'squeeze' and none 'predicted'; the sampled designs are bit-identical with the flag on and
    off and the global CPU generator is left where the sampling left it."""
    from dgdm_amd.generator.train import train
    from dynamics.parser import parse
    common = ("--mode=test --classifier_guidance --object_max_num_vertices=100 --ctrlpts_dim=14 --num_fingers=2 --batch_size=2 --grid_size=3 "
              "--num_pos=3 --num_train_timesteps=15 --num_inference_steps=2")
    runs, states = {}, {}
    for tag, extra in (("off", ""), ("on", " --squeeze_sim --squeeze_closing_steps 4 --squeeze_window 1")):
        torch.manual_seed(7)
        _, runs[tag] = train(parse(shlex.split(common + extra + f" --save_dir={tmp_path / tag}")))
        states[tag] = torch.get_rng_state()
    assert runs["on"][0].keys() == runs["off"][0].keys()
    for k, v in runs["off"][0].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, runs["on"][0][k]), k
    assert torch.equal(states["on"], states["off"])
    tables = sorted(os.listdir(tmp_path / "on" / "tables"))
    assert "SKIPPED.txt" not in tables and len(tables) == 35
    for t in tables:
        tab = json.load(open(tmp_path / "on" / "tables" / t))
        oc = tab["columns"].index("objective")
        scores = [row[oc] for row in tab["data"] if isinstance(row[oc], dict) and row[0] != -1]      # -1: the rows of averages, which carry no mark
        assert tab["data"] and scores, t
        assert all(s.get("simulated") == "squeeze" and "predicted" not in s for s in scores), t


def test_squeeze_simulator_metrics(dev):
    """The callable itself: build_metric's keys over num_rot orientations, object-major, and the marks."""
    from dgdm_amd import synth
    from dgdm_amd.dynamics.predicted import build_metric
    from dgdm_amd.sim.squeeze import SqueezeSimulator

    class Holder:
        mode = 'point'
        object_vertices = torch.stack([synth.synth_object_2d(i, 100) for i in range(2)])

        def _object_ids(self):
            return [11, 12]

    sim = SqueezeSimulator(Holder(), closing_steps=3, theta_cells=90, x_cells=33)
    samples = np.random.RandomState(0).uniform(-1, 1, (3, 14, 1)).astype(np.float32)
    out = sim(samples, [12, 11], None, num_rot=45, ori_range=(-0.5, 1.0))
    assert len(out) == 8 and len(out[1]) == 6 and all(v is None for v in out[0] + out[2] + out[3] + out[4] + out[5] + out[7])
    want = build_metric(np.zeros((45, 3), dtype=np.float32), [1, 1, 1], [1, 1, 1], (-0.5, 1.0))
    for m in out[1]:
        assert 'predicted' not in m and m['simulated'] == 'squeeze' and 0 <= m['squeeze_cut'] <= 45 and 0 <= m['squeeze_loose'] <= 45
        for k, v in want.items():
            if k != 'predicted':
                assert np.asarray(m[k]).shape == np.asarray(v).shape and np.asarray(m[k]).dtype == np.asarray(v).dtype, k
        assert set(np.unique(m['profile'])) <= {0, 1, 2}
    with pytest.raises(ValueError, match="2-D only"):
        Holder.mode = 'point_3d'
        SqueezeSimulator(Holder())


def test_generate_writes_files_the_dataset_reads(dev, tmp_path):
    """sim_2d.generate at 2 grippers x 2 objects: the files go through DynamicsDataset, the deltas equal the oracle's on the same pair."""
    from dgdm_amd.dynamics.dataloader import DynamicsDataset, load_score_stats
    from dgdm_amd.sim import sim_2d
    contours = np.stack([ngon(100, 0.03, 3, 0.3), ngon(100, 0.025, 2, 0.4, phase=0.5)])
    files = sim_2d.generate(str(tmp_path), [3, 4], contours, [7, 9], theta_cells=360, x_cells=41)
    assert sorted(os.path.basename(f) for f in files) == ["7_3.npz", "7_4.npz", "9_3.npz", "9_4.npz"]
    stats = load_score_stats(str(tmp_path / "stats.json"))
    ds = DynamicsDataset(str(tmp_path), object_max_num_vertices=100, **stats)
    assert len(ds) == 4
    item = ds[0]
    assert item['scores'].shape == (9000, 3) and item['ctrlpts'].shape == (14, 2) and item['object_vertices'].shape == (100, 2)
    d = np.load(tmp_path / "7_3.npz", allow_pickle=True)['arr_0'].item()
    sf = np.stack([d['allpts'][:200, 1] - 0.12, d['allpts'][200:, 1] + 0.15])
    ref = so.squeeze_pair(sf[0], sf[1], contours[0], so.rotation_table(360), sim_2d.pose_grid(), 41, 0.06, 2, 6, 0.1)
    th, x = so.cell_pose(ref["cells"], 360, 41, 0.06)
    assert np.array_equal(d['delta_pos'][:, 0], x[:, 1] - x[:, 0]) and np.array_equal(d['delta_pos'][:, 1], ref["y"][:, 0] - d['obj_pos'][:, 1])
    assert np.array_equal(d['delta_theta'], sim_2d.fold(th[:, 1] - th[:, 0], 2.0 * np.pi).astype(np.float32))
