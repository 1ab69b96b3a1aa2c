"""Condition rows of 3-D fingers from the sliced squeeze on the device (csrc/squeeze.hip: dgdm_squeeze_label_3d, table3d_fingers_kernel)
against the composition of the two CPU restatements that already exist: tests/squeeze3d_oracle.squeeze_map_3d, then
tests/squeeze_label_oracle.label_rows on its cells / y / flags.

The tables are float64 operations in a fixed order and are compared bit for bit, as int64 views with no cell excluded, with the oracle's
and with table3d_kernel's (engine.squeeze_tables_3d); the rows follow tests/test_gpu_squeeze_label.py's rule: columns 0-9, 11, 12, 14
and the counts bit for bit, columns 10 and 13 (sqrt) within one float32 ulp.  Shapes: tests/test_gpu_squeeze3d.py's 5 non-uniform
abscissae, 3 levels, 12 orientations and four meshes; 19 fingers = two full blocks of 8 and a tail of 3; objects [1, 3, 0, 1] out of
the bank of 4.  The cylinder's 400 segments per level fit one 512-segment LDS tile, so one more test has a 300-gon whose 600 segments
per level take two."""
import ctypes as C
import functools
import json
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine
from dgdm_amd import label as lb
from dgdm_amd.dynamics.dataloader import POS_NORM, SCORE_STD, SCORE_THRESHOLD
from dgdm_amd.sim import squeeze
from tests import resample_squeeze_oracle as rso
from tests import squeeze3d_oracle as so3
from tests import squeeze_label_oracle as slo
from tests import squeeze_oracle as so
from tests.test_gpu_squeeze3d import GX, GZ, THETA, meshes, prism, rect, surfaces

pytestmark = pytest.mark.gpu

OBJECTS = [1, 3, 0, 1]
M = len(OBJECTS)
THR, STD = [float(v) for v in SCORE_THRESHOLD[0]], [float(v) for v in SCORE_STD[0]]
THR2, STD2 = [float(v) for v in SCORE_THRESHOLD[1]], [float(v) for v in SCORE_STD[1]]     # the closed form's, as the 2-D test states it
ORI = (-1.0, 1.0)
# name: (X, x_half, R, k, fingers)
CASES = {"k3": (9, 0.06, 2, 3, 19), "settles": (9, 0.06, 1, 1 << 20, 19), "wide": (300, 0.1, 1, 1, 3)}
# name: (grid cells G, positions P): 54 tally starts leave lanes idle, 81 are more than one stride of the wave
STARTS = {"54": (6, 3), "81": (9, 3)}
SENTINEL = -77.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def config(case):
    X, x_half, R, k, _ = CASES[case]
    return dict(theta_cells=THETA, x_cells=X, x_half=x_half, window=R, closing_steps=k, travel_max=0.15)


@functools.lru_cache(maxsize=None)
def fingers(n):
    return np.stack([surfaces(s) for s in range(1, n + 1)])


def all_starts(which):
    G, P = STARTS[which]
    return np.concatenate([rso.start_grid(G, P, ORI), squeeze.start_orientations(6, ORI)])


def pick(which, settle):
    G, P = STARTS[which]
    return np.arange(G * P * P + (6 if settle else 0))


@functools.lru_cache(maxsize=None)
def sliced():
    return so3.slice_meshes(meshes(), GZ)


@functools.lru_cache(maxsize=None)
def maps(case, which):
    """The oracle's map of every (finger, object) pair, finger-major, over the tally and the settle starts: made once, never changed."""
    cfg = config(case)
    seg, off = sliced()
    pairs = [(f, o) for f in range(CASES[case][4]) for o in OBJECTS]
    return so3.squeeze_map_3d(fingers(CASES[case][4]), GX, seg, off, pairs, so.rotation_table(THETA), all_starts(which), x_cells=cfg["x_cells"],
                              x_half=cfg["x_half"], window=cfg["window"], closing_steps=cfg["closing_steps"], travel_max=cfg["travel_max"])


def label_of(ref, starts, n_tally, n_objects, cfg, layout):
    return slo.label_rows(ref["cells"], ref["y"], ref["flags"], starts, n_tally, n_objects, so.rotation_table(cfg["theta_cells"]), cfg["theta_cells"],
                          cfg["x_cells"], cfg["x_half"], THR, STD, POS_NORM, layout)


def reference(case, which, settle, layout):
    ref, idx = maps(case, which), pick(which, settle)
    G, P = STARTS[which]
    return label_of({k: ref[k][:, idx] for k in ("cells", "y", "flags")}, all_starts(which)[idx], G * P * P, M, config(case), layout)


def workspace(case, fingers_per_chunk):
    cfg = engine.squeeze_config(**config(case))
    return int(_lib.lib().dgdm_squeeze_label_3d_workspace_bytes(C.byref(cfg), fingers_per_chunk, M, len(GX), len(GZ), 4))


def run(case, which="54", settle=True, layout="mean", fingers_per_chunk=None, slack=0, tables=False, **kw):
    n = CASES[case][4]
    G, P = STARTS[which]
    sl = engine.squeeze_slice(meshes(), GZ)
    out = engine.squeeze_label_3d(fingers(n), GX, sl["segments"], sl["offsets"], OBJECTS, all_starts(which)[pick(which, settle)], G * P * P, THR, STD,
                                  POS_NORM, layout=layout, rot=so.rotation_table(THETA), tables=tables,
                                  workspace_bytes=workspace(case, fingers_per_chunk or n) + slack, **config(case), **kw)
    rows, counts = out[0].cpu().numpy(), out[1].cpu().numpy()
    return (rows, counts, {k: v.cpu().numpy() for k, v in out[2].items()}) if tables else (rows, counts)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def compare(got, ref, cols):
    """got, ref [F][blocks * cols] float32: bit equality but for columns 10 and 13 of every block, which get one float32 ulp."""
    assert got.shape == ref.shape and got.dtype == np.float32 and ref.dtype == np.float32
    gi, ri = got.view(np.int32).astype(np.int64), ref.view(np.int32).astype(np.int64)
    ulp = np.zeros(got.shape[1], dtype=np.int64)
    for b in range(got.shape[1] // cols):
        ulp[[b * cols + c for c in (10, 13) if c < cols]] = 1
    assert np.isfinite(ref).all()
    bad = np.argwhere(np.abs(gi - ri) > ulp[None])
    assert len(bad) == 0, f"{len(bad)} entries differ, first (finger, column) = {bad[0]}: {got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}"


@pytest.mark.parametrize("settle", [True, False])
@pytest.mark.parametrize("layout", ["mean", "per_object"])
@pytest.mark.parametrize("which", ["54", "81"])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_and_counts_equal_the_oracle(dev, case, which, layout, settle):
    ref, ref_counts = reference(case, which, settle, layout)
    got, counts = run(case, which, settle, layout)
    compare(got, ref, 15 if settle else 10)
    assert np.array_equal(counts, ref_counts) and counts.dtype == np.int32
    if case == "k3" and layout == "mean":                                 # the case tells the fingers apart
        assert len(np.unique(ref, axis=0)) == 19


def test_tables_equal_table3d_kernel_and_the_oracle(dev):
    """S, touch_l and touch_r of all 76 pairs: the finger-shared kernel against table3d_kernel on the same pairs and against the oracle,
    as int64 views, no cell excluded."""
    _, _, tab = run("k3", tables=True)
    cfg = config("k3")
    sl = engine.squeeze_slice(meshes(), GZ)
    pairs = [(f, o) for f in range(19) for o in OBJECTS]
    per_pair = engine.squeeze_tables_3d(fingers(19), GX, sl["segments"], sl["offsets"], pairs, None, rot=so.rotation_table(THETA), tables=True, **cfg)
    ref = maps("k3", "54")
    for k in ("S", "touch_l", "touch_r"):
        assert tab[k].shape == (76, THETA, 9)
        assert np.array_equal(bits(tab[k]), bits(per_pair[k].cpu().numpy())), k
        assert np.array_equal(bits(tab[k]), bits(ref[k])), k
    assert np.isfinite(tab["S"]).all() and len(np.unique(tab["S"])) > 76 * THETA


def test_a_level_of_more_than_one_segment_tile(dev):
    """A 300-gon prism: 600 segments on each level, two LDS tiles of the finger-shared kernel, the second one partly filled; 9 fingers (a
    full block and a single-finger block).  Tables against the oracle's and table3d_kernel's, bit for bit."""
    from tests.test_gpu_squeeze3d import ngon
    mesh = [prism(ngon(300, 0.05, 0.2), -0.01, 0.06)]
    seg, off = so3.slice_meshes(mesh, GZ)
    assert (np.diff(off, axis=1) == 600).all()
    cfg = dict(theta_cells=4, x_cells=7, x_half=0.06, window=1, closing_steps=2, travel_max=0.15)
    starts = rso.start_grid(4, 2, ORI)
    pairs = [(f, 0) for f in range(9)]
    ref = so3.squeeze_map_3d(fingers(9), GX, seg, off, pairs, so.rotation_table(4), starts, x_cells=7, x_half=0.06, window=1, closing_steps=2,
                             travel_max=0.15)
    sl = engine.squeeze_slice(mesh, GZ)
    rows, counts, tab = engine.squeeze_label_3d(fingers(9), GX, sl["segments"], sl["offsets"], [0], starts, 16, THR, STD, POS_NORM, tables=True, **cfg)
    per_pair = engine.squeeze_tables_3d(fingers(9), GX, sl["segments"], sl["offsets"], pairs, None, tables=True, **cfg)
    want, want_counts = label_of(ref, starts, 16, 1, cfg, "mean")
    compare(rows.cpu().numpy(), want, 10)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    for k in ("S", "touch_l", "touch_r"):
        assert np.array_equal(bits(tab[k].cpu().numpy()), bits(ref[k])), k
        assert np.array_equal(bits(tab[k].cpu().numpy()), bits(per_pair[k].cpu().numpy())), k


def test_chunking_and_blocking_change_no_bit(dev):
    """Workspaces of 19, 7 and 1 fingers and one size the library never returned: full blocks of fingers, tails and single-finger blocks;
    and the same call twice."""
    sizes = [workspace("k3", n) for n in (1, 7, 19)]
    assert 0 < sizes[0] < sizes[1] < sizes[2]
    whole = run("k3", tables=True)
    compare(whole[0], reference("k3", "54", True, "mean")[0], 15)
    for kw in (dict(fingers_per_chunk=7), dict(fingers_per_chunk=1), dict(fingers_per_chunk=7, slack=12345), dict()):
        rows, counts, tab = run("k3", tables=True, **kw)
        assert np.array_equal(rows.view(np.int32), whole[0].view(np.int32)) and np.array_equal(counts, whole[1]), kw
        for k in ("S", "touch_l", "touch_r"):
            assert np.array_equal(bits(tab[k]), bits(whole[2][k])), (kw, k)


@pytest.mark.parametrize("mu,mv", [(128, 8), (2, 512)])
def test_the_lds_limits(dev, mu, mv):
    """mu mv = 1024 both ways, 17 fingers (two blocks and a tail of one), T = 4, X = 5, a box prism that crosses every level."""
    rs = np.random.RandomState(mu)
    gx = np.sort(rs.uniform(-0.12, 0.12, mu)) if mu > 2 else np.array([-0.12, 0.12])
    gx[0], gx[-1] = -0.12, 0.12
    gz = np.linspace(0.0, 0.05, mv)
    sf = np.stack([np.stack([-0.1 + rs.uniform(-0.01, 0.01, (mv, mu)), 0.1 + rs.uniform(-0.01, 0.01, (mv, mu))]) for _ in range(17)])
    box = [prism(rect(0.03, 0.015), -0.01, 0.06)]
    cfg = dict(theta_cells=4, x_cells=5, x_half=0.06, window=1, closing_steps=2, travel_max=0.15)
    starts = np.concatenate([rso.start_grid(4, 2, ORI), squeeze.start_orientations(4, ORI)])
    seg, off = so3.slice_meshes(box, gz)
    assert (np.diff(off, axis=1) == 8).all()
    pairs = [(f, 0) for f in range(17)]
    ref = so3.squeeze_map_3d(sf, gx, seg, off, pairs, so.rotation_table(4), starts, x_cells=5, x_half=0.06, window=1, closing_steps=2, travel_max=0.15)
    want, want_counts = label_of(ref, starts, 16, 1, cfg, "mean")
    sl = engine.squeeze_slice(box, gz)
    rows, counts, tab = engine.squeeze_label_3d(sf, gx, sl["segments"], sl["offsets"], [0], starts, 16, THR, STD, POS_NORM, tables=True, **cfg)
    compare(rows.cpu().numpy(), want, 15)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    for k in ("S", "touch_l", "touch_r"):
        assert np.array_equal(bits(tab[k].cpu().numpy()), bits(ref[k])), k


def closed_form_inputs():
    """The 0.06 x 0.03 m rectangle as a prism through every level of GZ, between flat faces L = -0.12 and U = 0.15 on GX x GZ."""
    flat = np.stack([np.full((len(GZ), len(GX)), -0.12), np.full((len(GZ), len(GX)), 0.15)])[None]
    Gc, ori = 37, (-0.3, 0.3)
    starts = np.concatenate([rso.start_grid(Gc, 1, ori), squeeze.start_orientations(Gc, ori)])
    return flat, [prism(rect(0.03, 0.015), -0.01, 0.06)], starts, Gc


def assert_closed_form(r, counts, k, R):
    """test_rectangle_between_flat_jaws_closed_form's assertions (tests/test_squeeze_label_host.py), unchanged: threshold and std THR2, STD2."""
    d = 3 * np.abs(np.arange(37) - 18)
    f = float(np.float32(18.0 / 37.0))
    assert r[0] == f and r[1] == f and r[2] == 0 and r[3] == 0 and r[4] == 0 and r[5] == 1
    want = np.minimum(d, k * R).sum() * (2.0 * np.pi / 360.0) / 0.0565 / 37.0
    assert abs(r[6]) < 1e-6 and abs(r[7] - want) <= 1e-6 * want and r[8] == 0
    assert abs(r[9] - (0.015 + POS_NORM) / STD2[2]) <= 1e-6 * r[9]            # P = 1: the grid's only position is (-POS_NORM, -POS_NORM)
    assert abs(r[10] - 1.0) < 1e-6 and r[11] == -1.0 and abs(r[12]) < 1e-12 and abs(r[13] - 0.5) < 1e-6 and r[14] == 0
    assert not counts.any()


@pytest.mark.parametrize("k,R", [(6, 2), (3, 1)])
def test_rectangle_prism_between_flat_faces_closed_form(dev, k, R):
    flat, box, starts, Gc = closed_form_inputs()
    sl = engine.squeeze_slice(box, GZ)
    rows, counts = engine.squeeze_label_3d(flat, GX, sl["segments"], sl["offsets"], [0], starts, Gc, THR2, STD2, POS_NORM, theta_cells=360, x_cells=5,
                                           x_half=0.06, travel_max=0.2, closing_steps=k, window=R)
    assert_closed_form(rows.cpu().numpy()[0].astype(np.float64), counts.cpu().numpy(), k, R)


def test_an_object_with_no_segment_is_loose_everywhere(dev):
    above = [prism(rect(0.03, 0.015), 0.06, 0.08)]                          # over every level of GZ
    sl = engine.squeeze_slice(above, GZ)
    assert len(sl["segments"]) == 0
    starts = all_starts("54")
    rows, counts = engine.squeeze_label_3d(fingers(3), GX, sl["segments"], sl["offsets"], [0, 0], starts, 54, THR, STD, POS_NORM, **config("k3"))
    r, c = rows.cpu().numpy(), counts.cpu().numpy()
    assert (r[:, :6] == 0).all() and np.isfinite(r).all()
    assert (c[:, 0] == 2 * 54).all() and (c[:, 1] == 2 * 54).all()


@pytest.mark.parametrize("layout", ["mean", "per_object"])
def test_placement_leaves_every_other_float_alone(dev, layout):
    packed, _ = run("k3", layout=layout)
    out = torch.full((19, 80), SENTINEL, dtype=torch.float32, device=dev)
    got, _ = run("k3", layout=layout, out=out, column_offset=3, object_stride=17)
    assert got.shape == (19, 80)
    written = np.zeros(80, dtype=bool)
    for b in range(M if layout == "per_object" else 1):
        written[3 + 17 * b:3 + 17 * b + 15] = True
    assert np.array_equal(got[:, written].view(np.int32), packed.view(np.int32))
    assert (got[:, ~written] == SENTINEL).all()


def test_every_bad_argument_is_refused_before_a_launch(dev):
    lib = _lib.lib()
    mu, mv = 5, 3
    sf = torch.zeros(2, 2, mv, mu, dtype=torch.float64, device=dev)
    seg = torch.zeros(6, 4, dtype=torch.float64, device=dev)
    rot = torch.zeros(8, 2, dtype=torch.float64, device=dev)
    st = torch.zeros(7, 3, dtype=torch.float64, device=dev)
    rows = torch.full((2, 40), SENTINEL, dtype=torch.float32, device=dev)
    counts = torch.full((2, 3), -7, dtype=torch.int32, device=dev)
    tab = torch.full((4, 8, 5), SENTINEL, dtype=torch.float64, device=dev)
    good = dict(theta_cells=8, x_cells=5, window=1, closing_steps=2, x_half=0.06, travel_max=0.1, finger_half_len=0.12)
    size = lambda: int(lib.dgdm_squeeze_label_3d_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1, 2, mu, mv, 3))      # noqa: E731
    ws = torch.empty(size(), dtype=torch.uint8, device=dev)
    nan, inf = float("nan"), float("inf")
    offsets = np.array([[0, 1, 2, 2], [2, 2, 3, 4], [4, 5, 6, 6]], dtype=np.int32)

    def call(cfg=None, gx=tuple(GX), mu_=mu, mv_=mv, n_seg=6, off=offsets, objects=(2, 0), M_=2, nf=2, nb=3, surf=sf, segs=seg, n_tally=5, n_settle=2,
             thr=(0.03, 0.002, 0.003), std=(0.0565, 0.0026, 0.0047), pos_norm=0.03, layout=1, out=rows, row_stride=40, column_offset=3, object_stride=17,
             ws_b=None, starts=st, rot_=rot, gx_null=False, off_null=False):
        c = engine.squeeze_config(**dict(good, **(cfg or {})))
        oi = np.array(objects, dtype=np.int32)
        g = np.array(gx, dtype=np.float64)
        of = np.ascontiguousarray(off, dtype=np.int32)
        return lib.dgdm_squeeze_label_3d(C.byref(c), _lib.dptr(surf), nf, None if gx_null else g.ctypes.data, mu_, mv_, _lib.dptr(segs), n_seg,
                                         None if off_null else of.ctypes.data, nb, oi.ctypes.data, M_, _lib.dptr(rot_), _lib.dptr(starts), n_tally,
                                         n_settle, (C.c_double * 3)(*thr), (C.c_double * 3)(*std), pos_norm, layout, _lib.dptr(out), row_stride,
                                         column_offset, object_stride, _lib.dptr(counts), _lib.dptr(tab), None, None, _lib.dptr(ws),
                                         size() if ws_b is None else ws_b, None)

    down = offsets.copy()
    down[1, 1] = 1
    late = offsets.copy()
    late[0, 0] = 1
    bad = [dict(cfg=dict(theta_cells=0)), dict(cfg=dict(x_cells=1)), dict(cfg=dict(theta_cells=1 << 20, x_cells=1 << 11)), dict(cfg=dict(window=0)),
           dict(cfg=dict(closing_steps=-1)), dict(cfg=dict(x_half=0.0)), dict(cfg=dict(x_half=nan)), dict(cfg=dict(travel_max=inf)),
           dict(cfg=dict(finger_half_len=-0.1)),
           # what dgdm_squeeze_map_3d refuses
           dict(mu_=1), dict(mu_=129), dict(mv_=0), dict(mv_=513), dict(mu_=128, mv_=9), dict(nb=0), dict(nb=(1 << 20) + 1), dict(nf=0), dict(surf=None),
           dict(gx_null=True), dict(off_null=True), dict(rot_=None), dict(gx=(-0.12, -0.07, -0.07, 0.03, 0.12)), dict(gx=(-0.12, -0.07, nan, 0.03, 0.12)),
           dict(gx=(0.12, 0.03, 0.0, -0.07, -0.12)), dict(n_seg=-1), dict(n_seg=5), dict(segs=None), dict(off=down), dict(off=late),
           # what dgdm_squeeze_label refuses, friction and the 2-D sizes apart
           dict(M_=0), dict(M_=65536), dict(objects=(3, 0)), dict(objects=(0, -1)), dict(n_tally=0), dict(n_settle=-1),
           dict(std=(0.0, 0.1, 0.1)), dict(std=(0.1, -0.1, 0.1)), dict(std=(0.1, 0.1, nan)), dict(std=(inf, 0.1, 0.1)),
           dict(pos_norm=0.0), dict(pos_norm=-1.0), dict(pos_norm=nan), dict(pos_norm=inf),
           dict(thr=(-0.01, 0.0, 0.0)), dict(thr=(0.0, nan, 0.0)), dict(thr=(0.0, 0.0, inf)),
           dict(layout=2), dict(layout=-1), dict(object_stride=14), dict(row_stride=3 + 17 + 14), dict(layout=0, row_stride=17), dict(column_offset=-1),
           dict(out=None), dict(starts=None), dict(ws_b=size() - 1), dict(ws_b=0)]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.dgdm_last_error()
    torch.cuda.synchronize()
    assert bool((rows == SENTINEL).all()) and bool((counts == -7).all()) and bool((tab == SENTINEL).all())     # nothing was launched
    assert call() == _lib.OK and call(n_settle=0, object_stride=10, row_stride=3 + 10 + 10) == _lib.OK
    torch.cuda.synchronize()
    assert bool((counts >= 0).all()) and bool(torch.isfinite(rows).all()) and bool((tab != SENTINEL).all())
    cfg = C.byref(engine.squeeze_config(**good))
    assert lib.dgdm_squeeze_label_3d_workspace_bytes(C.byref(engine.squeeze_config(**dict(good, window=0))), 1, 2, mu, mv, 3) == _lib.EINVAL
    for fingers_, M_, mu_, mv_, nb in ((0, 2, 5, 3, 3), (1, 0, 5, 3, 3), (1, 65536, 5, 3, 3), (32768, 2, 5, 3, 3), (1, 2, 1, 3, 3), (1, 2, 129, 3, 3),
                                       (1, 2, 5, 0, 3), (1, 2, 5, 513, 3), (1, 2, 128, 9, 3), (1, 2, 5, 3, 0)):
        assert lib.dgdm_squeeze_label_3d_workspace_bytes(cfg, fingers_, M_, mu_, mv_, nb) == _lib.EINVAL, (fingers_, M_, mu_, mv_, nb)
    assert lib.dgdm_squeeze_label_3d_workspace_bytes(cfg, 2, 2, mu, mv, 3) > lib.dgdm_squeeze_label_3d_workspace_bytes(cfg, 1, 2, mu, mv, 3) > 0
    with pytest.raises(ValueError, match="window"):
        engine.squeeze_label_3d(sf, GX, seg, offsets, [0], st, 5, (0.03, 0.002, 0.003), (0.0565, 0.0026, 0.0047), window=0)
    with pytest.raises(ValueError, match="layout"):
        engine.squeeze_label_3d(sf, GX, seg, offsets, [0], st, 5, (0.03, 0.002, 0.003), (0.0565, 0.0026, 0.0047), layout="median")


def test_nan_settled_columns_name_the_finger(dev, monkeypatch):
    """Faces at L = +inf and U = -inf over a box that covers the abscissa gx = 0 at every cell (x_half = 0.01 < the box's half-width):
    every cell of that finger has S = -inf and y = (-inf + inf) / 2, its settled columns are NaN and label_fingers_squeeze_3d says which
    finger it was."""
    sf = fingers(3).copy()
    sf[1, 0], sf[1, 1] = np.inf, -np.inf
    monkeypatch.setattr(squeeze, "finger_surfaces_3d", lambda x, n, w: (GX, GZ, torch.from_numpy(sf[:len(x)]).to(dev)))
    with pytest.raises(ValueError, match="finger 1 "):
        lb.label_fingers_squeeze_3d(torch.zeros(3, 42), [meshes()[1]], [0], 6, 3, ORI, THR, STD, settled=True, sample_size=5, **dict(config("k3"), x_half=0.01))


def test_label_cli_squeeze_3d_end_to_end(dev, tmp_path, capsys):
    """--mode=label --label_source squeeze_3d --fingers_3d on 4 synthetic 3-D fingers and the six mesh files, with no checkpoint anywhere:
    the three files, marked 'source': 'squeeze_3d' and 'simulated': 'squeeze'; the raw rows are engine.squeeze_label_3d's on the same
    fingers; then --mode=test --cond_stats --cond_target reports what the unguided samples achieve by the same simulator."""
    from dgdm_amd.dynamics.parser import parse
    from dgdm_amd.generator import train as gtrain
    from dgdm_amd.generator.dataloader import GripperDataset
    from tests.test_gpu_squeeze3d import write_meshes
    write_meshes(str(tmp_path / "objects"), gtrain.OBJECT_NAMES_3D)
    shape = (f"--fingers_3d --object_dir={tmp_path / 'objects'} --object_max_num_vertices=512 --ctrlpts_dim=42 --sub_bs=40 --num_fingers=4 --batch_size=2 "
             "--num_train_timesteps=15 --num_inference_steps=2 --num_workers=0")
    out = tmp_path / "rows.npy"
    flags = "--label_source squeeze_3d --label_settled --label_squeeze_cells 90,33 --squeeze_closing_steps 4 --grid_size=3 --num_pos=3"
    stats, raw = gtrain.train(parse(shlex.split(f"--mode=label {shape} {flags} --label_out={out}")))
    assert "loose" in capsys.readouterr().out
    rows, raw_file, js = gtrain.load_global_cond(str(out), 4), np.load(tmp_path / "rows_raw.npy"), json.load(open(tmp_path / "rows.json"))
    assert rows.shape == (4, 15) and raw_file.shape == (4, 15) and np.array_equal(raw_file, raw) and np.array_equal(rows, stats.apply(raw_file))
    assert js["source"] == "squeeze_3d" and js["simulated"] == "squeeze" and "predicted" not in js and "friction" not in js
    assert js["settled"] is True and js["sample_size"] == 25 and js["width"] == squeeze.FINGER_WIDTH_3D
    assert js["columns"] == lb.TALLY_COLUMNS + lb.SETTLED_COLUMNS and js["G"] == 3 and js["P"] == 3 and js["object_ids"] == list(gtrain.OBJECT_NAMES_3D)
    assert js["squeeze_config"]["theta_cells"] == 90 and js["squeeze_config"]["x_cells"] == 33 and js["squeeze_config"]["closing_steps"] == 4
    assert js["threshold"] == THR and js["score_std"] == STD
    # the raw rows are a direct engine.squeeze_label_3d call on the dataset's fingers
    fing = torch.from_numpy(np.stack(list(GripperDataset(gtrain.finger_control_points(4, True), 0.12, -0.12, 0.0, -0.1)._items)))
    mesh = [engine.read_obj(os.path.join(tmp_path, "objects", n, "model.obj")) for n in gtrain.OBJECT_NAMES_3D]
    gx, gz, sf = squeeze.finger_surfaces_3d(fing.reshape(4, -1).float().to(dev), 25)
    sl = engine.squeeze_slice(mesh, gz)
    starts = np.concatenate([rso.start_grid(3, 3, ORI), squeeze.start_orientations(3, ORI)])
    direct, _ = engine.squeeze_label_3d(sf, gx, sl["segments"], sl["offsets"], list(range(len(mesh))), starts, 27, THR, STD, theta_cells=90, x_cells=33,
                                        closing_steps=4)
    assert np.array_equal(direct.cpu().numpy().view(np.int32), raw_file.view(np.int32))
    # sampling under a target: no --classifier_guidance, no dynamics model; the mesh files alone
    torch.manual_seed(7)
    _, results = gtrain.train(parse(shlex.split(f"--mode=test {shape} --cond_stats={tmp_path / 'rows.json'} --cond_target=frac_up=0.7")))
    rep = results[0]["cond_target"]
    assert rep["simulated"] == "squeeze" and "predicted" not in rep and rep["requested"] == {"frac_up": 0.7}
    assert rep["achieved_mean"].shape == (15,) and np.isfinite(rep["achieved_mean"]).all() and np.isfinite(rep["achieved_std"]).all()
    achieved, _ = lb.label_fingers_squeeze_3d(results[0]["unguided"], mesh, list(range(len(mesh))), 3, 3, ORI, THR, STD, settled=True,
                                              **js["squeeze_config"])
    assert np.array_equal(rep["achieved_mean"], achieved.cpu().numpy().astype(np.float64).mean(axis=0))
    # the refusals that need the files: no meshes under --object_dir
    with pytest.raises(ValueError, match="model.obj"):
        gtrain.train(parse(shlex.split(f"--mode=label {shape.replace(str(tmp_path / 'objects'), str(tmp_path / 'none'))} {flags} --label_out={out}")))
