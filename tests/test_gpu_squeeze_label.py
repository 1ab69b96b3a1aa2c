"""Condition rows from the squeeze simulator on the device (csrc/squeeze.hip, dgdm_squeeze_label) against the float64 CPU restatement
tests/squeeze_label_oracle.py, through the C ABI and through the layers above it (engine.squeeze_label, label.label_fingers_squeeze,
--mode=label --label_source squeeze, --cond_stats / --cond_target).

Every operation of the contract (include/dgdm_hip.h "squeeze-simulator labels") but sqrt is a basic IEEE float64 or an integer one, and
the order of every sum is fixed, so columns 0-9, 11, 12 and 14 and the counts are compared bit for bit with no row excluded; columns 10
and 13 pass through sqrt and get one float32 ulp, DESIGN.md 4.1b's allowance for settled columns.  Shapes: 24 orientations x 9 x cells,
16 surface samples, 8 vertices, window 2, 3 steps; 5 fingers; 1 and 3 objects out of a bank of 4, not in bank order; 150 tally starts
(more than one stride of the 64 lanes and no multiple of it), 64 and 1; 6 settle starts and none."""
import ctypes as C
import functools
import json
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine
from dgdm_amd import label as lb
from dgdm_amd.dynamics.dataloader import POS_NORM, SCORE_STD, SCORE_THRESHOLD
from dgdm_amd.sim import squeeze
from tests import resample_squeeze_oracle as rso
from tests import squeeze_friction_oracle as fo
from tests import squeeze_label_oracle as slo
from tests import squeeze_oracle as so

pytestmark = pytest.mark.gpu

T, X, M_PTS, NV, HL, XH, TM = 24, 9, 16, 8, 0.12, 0.06, 0.1
CFG = dict(theta_cells=T, x_cells=X, x_half=XH, window=2, closing_steps=3, travel_max=TM, finger_half_len=HL)
G, P, ORI = 6, 5, (-1.0, 1.0)
THR, STD = [float(v) for v in SCORE_THRESHOLD[1]], [float(v) for v in SCORE_STD[1]]
OBJECTS = {1: [1], 3: [2, 0, 3]}
SENTINEL = -77.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def surfaces(n=5, seed=3):
    """Random jaw pairs about L = -0.05 and U = 0.05: a tilt, a bow and a sample-wise jitter each - the bank's polygons are gripped on
    most cells (S < travel_max)."""
    rs = np.random.RandomState(seed)
    u = np.linspace(-1.0, 1.0, M_PTS)
    return np.stack([np.stack([off + rs.uniform(-0.01, 0.01) * u + rs.uniform(-0.01, 0.01) * np.cos(2.0 * u + rs.uniform(0, 6)) + rs.uniform(-0.002, 0.002, M_PTS)
                               for off in (-0.05, 0.05)]) for _ in range(n)])


def bank(seed=29):
    """Four random star-shaped polygons about their origin, one of them clockwise."""
    rs = np.random.RandomState(seed)
    out = []
    for k, stretch in enumerate(((0.045, 0.02), (0.03, 0.035), (0.04, 0.03), (0.025, 0.04))):
        ang = np.sort(rs.uniform(0, 2 * np.pi / NV, NV) + 2 * np.pi * np.arange(NV) / NV)
        p = np.stack([np.cos(ang), np.sin(ang)], axis=1) * rs.uniform(0.7, 1.0, (NV, 1)) * np.array(stretch)
        out.append(p[::-1].copy() if k == 2 else p)
    return np.stack(out)


def all_starts():
    return np.concatenate([rso.start_grid(G, P, ORI), squeeze.start_orientations(G, ORI)])


@functools.lru_cache(maxsize=None)
def maps(M, mu=0.0):
    """The oracle's map of every (finger, object) pair, finger-major, over all 150 + 6 starts: made once, never changed."""
    pairs = [(f, o) for f in range(5) for o in OBJECTS[M]]
    kw = dict(x_cells=X, x_half=XH, window=2, closing_steps=3, travel_max=TM, half_len=HL)
    if mu > 0.0:
        return fo.squeeze_map(surfaces(), bank(), pairs, so.rotation_table(T), all_starts(), mu=mu, **kw)
    return so.squeeze_map(surfaces(), bank(), pairs, so.rotation_table(T), all_starts(), **kw)


def pick(n_tally, n_settle):
    """Columns of all_starts(): the first n_tally grid cells, then the first n_settle start orientations."""
    return np.concatenate([np.arange(n_tally), G * P * P + np.arange(n_settle)])


def reference(M, n_tally, n_settle, layout, mu=0.0):
    ref, idx = maps(M, mu), pick(n_tally, n_settle)
    return slo.label_rows(ref["cells"][:, idx], ref["y"][:, idx], ref["flags"][:, idx], all_starts()[idx], n_tally, M, so.rotation_table(T), T, X, XH,
                          THR, STD, POS_NORM, layout)


def run(M, n_tally, n_settle, layout, mu=0.0, fingers_per_chunk=5, **kw):
    cfg = engine.squeeze_config(**CFG)
    ws = int(_lib.lib().dgdm_squeeze_label_workspace_bytes(C.byref(cfg), fingers_per_chunk, M, int(mu > 0.0)))
    rows, counts = engine.squeeze_label(surfaces(), bank(), OBJECTS[M], all_starts()[pick(n_tally, n_settle)], n_tally, THR, STD, POS_NORM, layout=layout,
                                        friction=mu, rot=so.rotation_table(T), workspace_bytes=ws, **CFG, **kw)
    return rows.cpu().numpy(), counts.cpu().numpy()


def compare(got, ref, cols):
    """got, ref [F][blocks * cols] float32: bit equality but for columns 10 and 13 of every block, which get one float32 ulp."""
    assert got.shape == ref.shape and got.dtype == np.float32 and ref.dtype == np.float32
    gi, ri = got.view(np.int32).astype(np.int64), ref.view(np.int32).astype(np.int64)
    ulp = np.zeros(got.shape[1], dtype=np.int64)
    for b in range(got.shape[1] // cols):
        ulp[[b * cols + c for c in (10, 13) if c < cols]] = 1
    assert np.isfinite(ref).all() and (ref[:, ulp == 1] > 0).all()
    bad = np.argwhere(np.abs(gi - ri) > ulp[None])
    assert len(bad) == 0, f"{len(bad)} entries differ, first (finger, column) = {bad[0]}: {got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}"


@pytest.mark.parametrize("n_tally,n_settle", [(150, 6), (150, 0), (64, 6), (1, 6)])
@pytest.mark.parametrize("layout", ["mean", "per_object"])
@pytest.mark.parametrize("M", [1, 3])
def test_rows_and_counts_equal_the_oracle(dev, M, layout, n_tally, n_settle):
    ref, ref_counts = reference(M, n_tally, n_settle, layout)
    got, counts = run(M, n_tally, n_settle, layout)
    cols = 15 if n_settle else 10
    compare(got, ref, cols)
    assert np.array_equal(counts, ref_counts) and counts.dtype == np.int32
    if n_tally == 150 and M == 3:                                         # the case exercises the classes, not one value
        assert len(np.unique(ref[:, :6])) > 6 and (ref[:, 6:8] != 0).all()


@pytest.mark.parametrize("layout", ["mean", "per_object"])
def test_placement_leaves_every_other_float_alone(dev, layout):
    """object_stride 17 > 15 and column_offset 3 in rows 60 floats wide: the blocks land where the header says, bit for bit what the
    packed call writes, and every float outside them keeps its bytes."""
    M = 3
    packed, _ = run(M, 150, 6, layout)
    out = torch.full((5, 60), SENTINEL, dtype=torch.float32, device=dev)
    got, _ = run(M, 150, 6, layout, out=out, column_offset=3, object_stride=17)
    assert got.shape == (5, 60)
    written = np.zeros(60, dtype=bool)
    for b in range(M if layout == "per_object" else 1):
        written[3 + 17 * b:3 + 17 * b + 15] = True
    assert np.array_equal(got[:, written].view(np.int32), packed.view(np.int32))
    assert (got[:, ~written] == SENTINEL).all()


def test_chunking_does_not_change_a_bit(dev):
    """A workspace of two fingers: N = 5 runs as chunks of 2, 2 and 1 fingers."""
    cfg, lib = engine.squeeze_config(**CFG), _lib.lib()
    size = [int(lib.dgdm_squeeze_label_workspace_bytes(C.byref(cfg), n, 3, 0)) for n in (1, 2, 3, 5)]
    assert 0 < size[0] < size[1] < size[2] < size[3]                       # two fingers' bytes hold no third
    for layout in ("mean", "per_object"):
        small, small_counts = run(3, 150, 6, layout, fingers_per_chunk=2)
        whole, whole_counts = run(3, 150, 6, layout, fingers_per_chunk=5)
        assert np.array_equal(small.view(np.int32), whole.view(np.int32)) and np.array_equal(small_counts, whole_counts)
        compare(small, reference(3, 150, 6, layout)[0], 15)


def test_fractions_equal_squeeze_metrics_class_counts(dev):
    """Independent of the oracle: columns 0-5 are float32(K / (M n)) with K counted from sim.squeeze.squeeze_metric's profiles over
    sim.squeeze.squeeze_map of the same pairs and starts."""
    rs = np.random.RandomState(17)
    fingers = torch.from_numpy(rs.uniform(-1, 1, (5, 14)).astype(np.float32))
    contours, objects = bank(), [2, 0, 3]
    cfg = dict(theta_cells=48, x_cells=17, travel_max=0.2, closing_steps=3)
    rows, counts = lb.label_fingers_squeeze(fingers, contours, objects, G, P, ORI, THR, STD, settled=True, layout="per_object", **cfg)
    mean_rows, _ = lb.label_fingers_squeeze(fingers, contours, objects, G, P, ORI, THR, STD, layout="mean", **cfg)
    rows, counts, mean_rows = rows.cpu().numpy(), counts.cpu().numpy(), mean_rows.cpu().numpy()
    assert rows.shape == (5, 45) and mean_rows.shape == (5, 10) and np.isfinite(rows).all()
    starts = rso.start_grid(G, P, ORI)
    pairs = [(f, o) for f in range(5) for o in objects]
    out = squeeze.squeeze_map(fingers, contours, starts, pairs=pairs, **cfg)
    start, closed, settled, flags = (out[k].cpu().numpy() for k in ("start", "closed", "settled", "flags"))
    n = len(starts)
    K = np.zeros((5, 3, 6), dtype=np.int64)
    for p, (f, _) in enumerate(pairs):
        met = squeeze.squeeze_metric(start[p], closed[p], settled[p], flags[p], starts[:, 2], THR)
        for j, key in enumerate(("profile", "profile_x", "profile_y")):
            K[f, p % 3, 2 * j], K[f, p % 3, 2 * j + 1] = np.count_nonzero(met[key] == 0), np.count_nonzero(met[key] == 2)
    assert len(np.unique(K)) > 4
    want = (K.astype(np.float64) / float(n)).astype(np.float32)
    assert np.array_equal(rows.reshape(5, 3, 15)[:, :, :6].view(np.int32), want.view(np.int32))
    want_mean = (K.sum(axis=1).astype(np.float64) / float(3 * n)).astype(np.float32)
    assert np.array_equal(mean_rows[:, :6].view(np.int32), want_mean.view(np.int32))
    fl = flags.reshape(5, 3 * n)
    assert np.array_equal(counts, np.stack([np.count_nonzero(fl & b, axis=1) for b in (1, 2, 4)], axis=1))


def test_friction_rows_equal_the_friction_oracle(dev):
    ref, ref_counts = reference(3, 150, 6, "per_object", mu=0.5)
    assert (maps(3, 0.5)["flags"] & 24).any()                              # some starts begin or settle on a jammed cell
    got, counts = run(3, 150, 6, "per_object", mu=0.5)
    compare(got, ref, 15)
    assert np.array_equal(counts, ref_counts)
    assert not np.array_equal(got.view(np.int32), run(3, 150, 6, "per_object")[0].view(np.int32))


def test_zero_friction_is_the_frictionless_entry(dev):
    """mu = 0 through the friction argument: the frictionless rows, bit for bit (and so is a workspace sized for the jam table)."""
    plain, plain_counts = run(3, 150, 6, "mean")
    cfg = engine.squeeze_config(**CFG)
    ws = int(_lib.lib().dgdm_squeeze_label_workspace_bytes(C.byref(cfg), 5, 3, 1))
    rows, counts = engine.squeeze_label(surfaces(), bank(), OBJECTS[3], all_starts(), 150, THR, STD, POS_NORM, layout="mean", friction=0.0,
                                        rot=so.rotation_table(T), workspace_bytes=ws, **CFG)
    assert np.array_equal(rows.cpu().numpy().view(np.int32), plain.view(np.int32)) and np.array_equal(counts.cpu().numpy(), plain_counts)


def test_rectangle_between_flat_jaws_closed_form(dev):
    """The 0.06 x 0.03 m rectangle between flat jaws (L = -0.12, U = 0.15), 360 x 5 cells, travel_max 0.2, 37 start orientations within
    +-54 degrees of 180, all in its basin: a start d cells away turns min(d, k R) cells toward it."""
    rect = np.array([[-0.03, -0.015], [0.03, -0.015], [0.03, 0.015], [-0.03, 0.015]])
    flat = np.stack([np.full(M_PTS, -0.12), np.full(M_PTS, 0.15)])[None]
    Gc, ori = 37, (-0.3, 0.3)
    starts = np.concatenate([rso.start_grid(Gc, 1, ori), squeeze.start_orientations(Gc, ori)])
    d = 3 * np.abs(np.arange(Gc) - 18)
    for k, R in ((6, 2), (3, 1)):
        rows, counts = engine.squeeze_label(flat, rect[None], [0], starts, Gc, THR, STD, POS_NORM, theta_cells=360, x_cells=5, x_half=0.06, travel_max=0.2,
                                            closing_steps=k, window=R)
        r = rows.cpu().numpy()[0].astype(np.float64)
        f = float(np.float32(18.0 / 37.0))
        assert r[0] == f and r[1] == f and r[2] == 0 and r[3] == 0 and r[4] == 0 and r[5] == 1
        assert abs(r[6]) < 1e-6                                           # the two sides cancel
        want = np.minimum(d, k * R).sum() * (2.0 * np.pi / 360.0) / 0.0565 / 37.0
        assert abs(r[7] - want) <= 1e-6 * want and r[8] == 0
        assert abs(r[9] - (0.015 + POS_NORM) / STD[2]) <= 1e-6 * r[9]       # P = 1: the grid's only position is (-POS_NORM, -POS_NORM)
        assert abs(r[10] - 1.0) < 1e-6 and r[11] == -1.0 and abs(r[12]) < 1e-12 and abs(r[13] - 0.5) < 1e-6 and r[14] == 0
        assert not counts.cpu().numpy().any()


def test_every_bad_argument_is_refused_before_a_launch(dev):
    lib = _lib.lib()
    sf = torch.zeros(2, 2, 8, dtype=torch.float64, device=dev)
    ob = torch.zeros(3, 4, 2, dtype=torch.float64, device=dev)
    rot = torch.zeros(8, 2, dtype=torch.float64, device=dev)
    st = torch.zeros(7, 3, dtype=torch.float64, device=dev)
    rows = torch.full((2, 40), SENTINEL, dtype=torch.float32, device=dev)
    counts = torch.full((2, 3), -7, dtype=torch.int32, device=dev)
    good = dict(theta_cells=8, x_cells=5, window=1, closing_steps=2, x_half=0.06, travel_max=0.1, finger_half_len=0.12)
    size = lambda mu: int(lib.dgdm_squeeze_label_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1, 2, int(mu > 0)))      # noqa: E731
    ws = torch.empty(size(1.0), dtype=torch.uint8, device=dev)
    nan, inf = float("nan"), float("inf")

    def call(cfg=None, m=8, nv=4, objects=(2, 0), M=2, nf=2, no=3, surf=sf, n_tally=5, n_settle=2, mu=0.0, thr=(0.03, 0.002, 0.003),
             std=(0.0565, 0.0026, 0.0047), pos_norm=0.03, layout=1, out=rows, row_stride=40, column_offset=3, object_stride=17, ws_b=None, starts=st):
        c = engine.squeeze_config(**dict(good, **(cfg or {})))
        oi = np.array(objects, dtype=np.int32)
        return lib.dgdm_squeeze_label(C.byref(c), _lib.dptr(surf), nf, m, _lib.dptr(ob), no, nv, oi.ctypes.data, M, _lib.dptr(rot), _lib.dptr(starts),
                                      n_tally, n_settle, mu, (C.c_double * 3)(*thr), (C.c_double * 3)(*std), pos_norm, layout, _lib.dptr(out), row_stride,
                                      column_offset, object_stride, _lib.dptr(counts), _lib.dptr(ws), size(mu) if ws_b is None else ws_b, None)

    bad = [dict(cfg=dict(theta_cells=0)), dict(cfg=dict(x_cells=1)), dict(cfg=dict(theta_cells=1 << 20, x_cells=1 << 11)), dict(cfg=dict(window=0)),
           dict(cfg=dict(closing_steps=-1)), dict(cfg=dict(x_half=0.0)), dict(cfg=dict(x_half=nan)), dict(cfg=dict(travel_max=inf)),
           dict(cfg=dict(finger_half_len=-0.1)), dict(m=1), dict(m=4096), dict(nv=2), dict(nv=4096), dict(nf=0), dict(no=0), dict(surf=None),
           dict(mu=-0.5), dict(mu=nan), dict(mu=inf),
           dict(M=0), dict(objects=(3, 0)), dict(objects=(0, -1)), dict(n_tally=0), dict(n_settle=-1),
           dict(std=(0.0, 0.1, 0.1)), dict(std=(0.1, -0.1, 0.1)), dict(std=(0.1, 0.1, nan)), dict(std=(inf, 0.1, 0.1)),
           dict(pos_norm=0.0), dict(pos_norm=-1.0), dict(pos_norm=nan), dict(pos_norm=inf),
           dict(thr=(-0.01, 0.0, 0.0)), dict(thr=(0.0, nan, 0.0)), dict(thr=(0.0, 0.0, inf)),
           dict(layout=2), dict(layout=-1), dict(object_stride=14), dict(row_stride=3 + 17 + 14), dict(layout=0, row_stride=17), dict(column_offset=-1),
           dict(out=None), dict(starts=None), dict(ws_b=size(0.0) - 1), dict(mu=0.5, ws_b=size(0.5) - 1), dict(mu=0.5, ws_b=size(0.0))]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.dgdm_last_error()
    torch.cuda.synchronize()
    assert bool((rows == SENTINEL).all()) and bool((counts == -7).all())     # nothing was launched
    assert call() == _lib.OK and call(mu=0.5) == _lib.OK and call(n_settle=0, object_stride=10, row_stride=3 + 10 + 10) == _lib.OK
    torch.cuda.synchronize()
    assert bool((counts >= 0).all()) and bool(torch.isfinite(rows).all())
    cfg = C.byref(engine.squeeze_config(**good))
    assert lib.dgdm_squeeze_label_workspace_bytes(C.byref(engine.squeeze_config(**dict(good, window=0))), 1, 2, 0) == _lib.EINVAL
    for fingers, M in ((0, 2), (1, 0), (1, 65536), (32768, 2)):
        assert lib.dgdm_squeeze_label_workspace_bytes(cfg, fingers, M, 0) == _lib.EINVAL
    assert lib.dgdm_squeeze_label_workspace_bytes(cfg, 1, 2, 1) > lib.dgdm_squeeze_label_workspace_bytes(cfg, 1, 2, 0) > 0
    with pytest.raises(ValueError, match="window"):
        engine.squeeze_label(sf, ob, [0], st, 5, (0.03, 0.002, 0.003), (0.0565, 0.0026, 0.0047), window=0)
    with pytest.raises(ValueError, match="layout"):
        engine.squeeze_label(sf, ob, [0], st, 5, (0.03, 0.002, 0.003), (0.0565, 0.0026, 0.0047), layout="median")


def test_nan_settled_columns_name_the_finger(dev, monkeypatch):
    """Jaws at L = +inf and U = -inf leave every cell at S = -inf, its own successor, with y = (-inf + inf) / 2: the finger's settled
    columns 10-13 are NaN, left_range is not, the other fingers are untouched, and label_fingers_squeeze says which finger it was."""
    sf = surfaces()
    sf[3, 0], sf[3, 1] = np.inf, -np.inf
    rows, _ = engine.squeeze_label(sf, bank(), [1], all_starts(), 150, THR, STD, POS_NORM, rot=so.rotation_table(T), **CFG)
    r = rows.cpu().numpy()
    assert np.isnan(r[3, 10:14]).all() and np.isfinite(r[3, 14]) and np.isfinite(np.delete(r, 3, axis=0)).all()
    clean, _ = run(1, 150, 6, "mean")
    assert np.array_equal(np.delete(r, 3, axis=0).view(np.int32), np.delete(clean, 3, axis=0).view(np.int32))
    monkeypatch.setattr(squeeze, "finger_surfaces", lambda x, num_points: torch.from_numpy(sf[2:2 + len(x)]).to(dev))
    with pytest.raises(ValueError, match="finger 1 "):
        lb.label_fingers_squeeze(torch.zeros(3, 14), bank(), [1], G, P, ORI, THR, STD, settled=True, **CFG)


def test_label_cli_squeeze_end_to_end(dev, tmp_path, capsys):
    """--mode=label --label_source squeeze on 12 synthetic fingers and 2 synthetic contours, with no checkpoint anywhere: the three files,
    marked 'simulated': 'squeeze'; then --mode=test --cond_stats --cond_target reports what the unguided samples achieve, scored by the
    same simulator under the stored recipe."""
    from dgdm_amd.dynamics.parser import parse
    from dgdm_amd.generator import train as gtrain
    from dgdm_amd.generator.dataloader import GripperDataset
    ang = 2 * np.pi * np.arange(20) / 20
    contours = np.stack([np.stack([0.04 * np.cos(ang), 0.02 * np.sin(ang)], axis=1),
                         np.stack([(0.03 + 0.008 * np.cos(3 * ang)) * np.cos(ang), (0.03 + 0.008 * np.cos(3 * ang)) * np.sin(ang)], axis=1)])
    np.save(tmp_path / "objects.npy", contours.astype(np.float32))
    shape = (f"--object_dir={tmp_path} --object_max_num_vertices=20 --ctrlpts_dim=14 --num_fingers=12 --batch_size=4 --num_train_timesteps=15 "
             "--num_inference_steps=2 --num_workers=0")
    out = tmp_path / "rows.npy"
    flags = "--label_source squeeze --label_settled --label_squeeze_cells 90,33 --squeeze_closing_steps 4 --grid_size=5 --num_pos=3"
    stats, raw = gtrain.train(parse(shlex.split(f"--mode=label {shape} {flags} --label_out={out}")))
    assert "loose" in capsys.readouterr().out
    rows, raw_file, js = gtrain.load_global_cond(str(out), 12), np.load(tmp_path / "rows_raw.npy"), json.load(open(tmp_path / "rows.json"))
    assert rows.shape == (12, 15) and raw_file.shape == (12, 15) and np.array_equal(raw_file, raw) and np.array_equal(rows, stats.apply(raw_file))
    assert js["simulated"] == "squeeze" and "predicted" not in js and js["source"] == "squeeze" and js["settled"] is True and js["friction"] == 0.0
    assert js["columns"] == lb.TALLY_COLUMNS + lb.SETTLED_COLUMNS and js["G"] == 5 and js["P"] == 3 and js["object_ids"] == [0, 1]
    assert js["squeeze_config"]["theta_cells"] == 90 and js["squeeze_config"]["x_cells"] == 33 and js["squeeze_config"]["closing_steps"] == 4
    assert js["threshold"] == THR and js["score_std"] == STD
    # the raw rows are label_fingers_squeeze on the dataset's fingers
    fingers = torch.from_numpy(np.stack(list(GripperDataset(gtrain.finger_control_points(12, False), 0.12, -0.12, 0.015, -0.045)._items)))
    bank_m = torch.from_numpy(contours.astype(np.float32)).double().numpy()      # objects.npy holds float32
    objs, _ = gtrain._objects(parse(shlex.split(shape)), False)
    direct, _ = lb.label_fingers_squeeze(fingers, objs.double() * squeeze.OBJECT_HALF_BOX_2D, [0, 1], 5, 3, ORI, THR, STD, settled=True,
                                         theta_cells=90, x_cells=33, closing_steps=4)
    assert np.array_equal(direct.cpu().numpy().view(np.int32), raw_file.view(np.int32)) and np.abs(objs.double().numpy() * 0.05 - bank_m).max() < 1e-6
    # sampling under a target: no --classifier_guidance, no dynamics model; the object flags alone
    torch.manual_seed(7)
    _, results = gtrain.train(parse(shlex.split(f"--mode=test {shape} --cond_stats={tmp_path / 'rows.json'} --cond_target=frac_clockwise=0.9")))
    rep = results[0]["cond_target"]
    assert rep["simulated"] == "squeeze" and "predicted" not in rep and rep["requested"] == {"frac_clockwise": 0.9}
    assert rep["achieved_mean"].shape == (15,) and np.isfinite(rep["achieved_mean"]).all() and np.isfinite(rep["achieved_std"]).all()
    achieved, _ = lb.label_fingers_squeeze(results[0]["unguided"], objs.double() * squeeze.OBJECT_HALF_BOX_2D, [0, 1], 5, 3, ORI, THR, STD, settled=True,
                                           **js["squeeze_config"])
    assert np.array_equal(rep["achieved_mean"], achieved.cpu().numpy().astype(np.float64).mean(axis=0))
    # another object count than the recipe's
    js["object_ids"] = [0]
    json.dump(js, open(tmp_path / "one.json", "w"))
    with pytest.raises(ValueError, match="1 objects"):
        gtrain.train(parse(shlex.split(f"--mode=test {shape} --cond_stats={tmp_path / 'one.json'} --cond_target=frac_up=0.7")))
