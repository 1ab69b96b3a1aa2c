"""The sliced squeeze on the device (csrc/squeeze.hip: slice_kernel, table3d_kernel) against its float64 CPU restatement
tests/squeeze3d_oracle.py.

Every operation of the contract (include/dgdm_hip.h "squeeze simulator, 3-D fingers") is a basic IEEE float64 one or an int32 one, so
nothing here has a tolerance but the prism test, which says why: segments, the three tables and y are compared bit for bit, offsets,
the successor array, the three cells per start and the flags as integers, with no row excluded.  Shapes: 5 non-uniform abscissae, 3
levels, 12 orientations, 9 x cells (and 300: the strided lane loop); four objects of 1200, 16, 16 and 8 segments in one chunk - a
200-sided cylinder (more than one 1024-segment LDS tile, not a multiple of it, reaching past the finger ends at x cells far from 0), a box
(P_x == Q_x on its walls at theta = 0, end points exactly on gx = 0.03 at x = 0), two boxes apart in z (an empty level between two full
ones, the upper one wider than the fingers) and a pyramid whose apex lies exactly on a level."""
import ctypes as C
import functools
import json
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine
from tests import squeeze3d_oracle as so3
from tests import squeeze_oracle as so
from tests import test_squeeze3d_host as host

pytestmark = pytest.mark.gpu

THETA = 12
GX = np.array([-0.12, -0.07, 0.0, 0.03, 0.12])
GZ = np.array([0.0, 0.02, 0.05])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def prism(poly, z0, z1, caps=True):
    """The polygon extruded from z0 to z1: two triangles per wall, corner edges vertical; caps as fans."""
    n = len(poly)
    v = np.concatenate([np.c_[poly, np.full(n, z0)], np.c_[poly, np.full(n, z1)]])
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [[i, j, n + j], [i, n + j, n + i]]
    if caps:
        f += [[0, i + 1, i] for i in range(1, n - 1)] + [[n, n + i, n + i + 1] for i in range(1, n - 1)]
    return v, np.array(f, dtype=np.int32)


def rect(a, b, centre=(0.0, 0.0)):
    return np.array([[-a, -b], [a, -b], [a, b], [-a, b]]) + np.asarray(centre)


def ngon(n, radius, phase=0.0):
    a = phase + 2.0 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1)


def merge(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


@functools.lru_cache(maxsize=None)
def meshes():
    cylinder = prism(ngon(200, 0.07, 0.1), -0.01, 0.06)
    box = prism(rect(0.03, 0.015), -0.005, 0.03)
    apart = merge(prism(rect(0.02, 0.01, (0.01, 0.0)), -0.01, 0.01), prism(rect(0.14, 0.012, (0.0, 0.005)), 0.04, 0.06))
    base = np.c_[ngon(4, 0.04, 0.3), np.full(4, -0.01)]
    pyramid = (np.concatenate([base, [[0.01, 0.0, GZ[1]]]]), np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]], dtype=np.int32))
    return cylinder, box, apart, pyramid


def surfaces(seed):
    """Two smooth random jaw faces [2][mv][mu] around the flat ones (L = -0.13, U = 0.23), leaning with z."""
    rs = np.random.RandomState(seed)
    u, z = GX[None, :] / 0.12, GZ[:, None] / 0.12
    bump = lambda: sum(rs.uniform(-0.012, 0.012) * np.cos(k * np.pi * u + rs.uniform(0, 6)) for k in range(1, 4)) + rs.uniform(-0.05, 0.05) * z     # noqa: E731
    return np.stack([-0.13 + bump(), 0.23 + bump()])


def starts(x_half, n=40, seed=5):
    rs = np.random.RandomState(seed)
    st = np.stack([rs.uniform(-7.0, 14.0, n), rs.uniform(-1.3 * x_half, 1.3 * x_half, n), rs.uniform(-0.05, 0.05, n)], axis=1)
    st[0] = (0.5 * so.TWO_PI / THETA, 0.0, 0.0)
    st[1] = (np.nan, np.nan, 0.0)
    st[2] = (np.inf, -np.inf, 0.01)
    st[3] = (1e300, 1e300, np.nan)
    return st


# name: (X, x_half, R, k, pairs)
ALL = tuple((f, o) for o in range(4) for f in range(2))
CASES = {"all_k3": (9, 0.06, 2, 3, ALL), "wide_k1": (300, 0.1, 1, 1, ((0, 1), (1, 3), (1, 0))), "settles": (9, 0.06, 1, 1 << 20, ALL)}


def case_inputs(name):
    X, x_half, R, k, pairs = CASES[name]
    cfg = dict(theta_cells=THETA, x_cells=X, x_half=x_half, window=R, closing_steps=k, travel_max=0.15)
    return np.stack([surfaces(1), surfaces(2)]), starts(x_half), cfg, pairs


@functools.lru_cache(maxsize=None)
def sliced():
    return so3.slice_meshes(meshes(), GZ)


@functools.lru_cache(maxsize=None)
def reference(name):
    sf, st, cfg, pairs = case_inputs(name)
    seg, off = sliced()
    return so3.squeeze_map_3d(sf, GX, seg, off, pairs, so.rotation_table(THETA), st, x_cells=cfg["x_cells"], x_half=cfg["x_half"], window=cfg["window"],
                              closing_steps=cfg["closing_steps"], travel_max=cfg["travel_max"])


def workspace(name, chunk_pairs):
    return int(_lib.lib().dgdm_squeeze_map_3d_workspace_bytes(C.byref(engine.squeeze_config(**case_inputs(name)[2])), chunk_pairs, len(GX), len(GZ), 4))


def run(name, chunk_pairs=4, slack=0):
    """slack: bytes on top of the size the library gives for chunk_pairs - a workspace that is no size it returned."""
    sf, st, cfg, pairs = case_inputs(name)
    sl = engine.squeeze_slice(meshes(), GZ)
    out = engine.squeeze_tables_3d(sf, GX, sl["segments"], sl["offsets"], pairs, st, rot=so.rotation_table(THETA), tables=True,
                                   workspace_bytes=workspace(name, chunk_pairs) + slack, **cfg)
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_the_cases_are_what_the_docstring_says():
    seg, off = sliced()
    counts = np.diff(off, axis=1)
    assert counts.tolist() == [[400, 400, 400], [8, 8, 0], [8, 0, 8], [4, 4, 0]]
    assert counts[0].sum() > 1024 and counts[0].sum() % 1024
    apex = seg[off[3, 1]:off[3, 2]]
    assert len(apex) == 4 and np.abs(apex - [0.01, 0.0, 0.01, 0.0]).max() <= 1e-16                   # r = 1: segments of no length, at the apex
    walls = seg[off[1, 0]:off[1, 1]]
    assert (walls[:, 0] == walls[:, 2]).sum() == 4 and (np.abs(walls[:, [0, 2]]) == 0.03).any()       # P_x == Q_x; end points on gx = 0.03 at x = 0
    assert np.abs(seg[off[2, 2]:off[2, 3], [0, 2]]).max() > 0.12                                      # past the finger ends
    ref = reference("all_k3")
    assert np.isfinite(ref["S"]).all() and (ref["flags"] & 1).any() and not (ref["flags"] & 1).all()


def test_slices_equal_the_oracle(dev):
    seg, off = sliced()
    sl = engine.squeeze_slice(meshes(), GZ)
    assert sl["offsets"].dtype == np.int32 and np.array_equal(sl["offsets"], off)
    assert np.array_equal(bits(sl["segments"].cpu().numpy()), bits(seg))
    one = engine.squeeze_slice(meshes()[3:], GZ[1:2])                                                   # one object, one level
    s1, o1 = so3.slice_meshes(meshes()[3:], GZ[1:2])
    assert np.array_equal(one["offsets"], o1) and np.array_equal(bits(one["segments"].cpu().numpy()), bits(s1))
    none = engine.squeeze_slice(meshes()[3:], [0.5])                                                    # above everything: no segment
    assert none["segments"].shape == (0, 4) and none["offsets"].tolist() == [[0, 0]]


@pytest.mark.parametrize("name", list(CASES))
def test_tables_and_maps_equal_the_oracle(dev, name):
    got, ref = run(name), reference(name)
    for k in ("touch_l", "touch_r", "S"):
        bad = np.argwhere(bits(got[k]) != bits(ref[k]))
        assert len(bad) == 0, f"{k}: {len(bad)} cells differ, first (pair, a, b) = {bad[0]}: {got[k][tuple(bad[0])]!r} vs {ref[k][tuple(bad[0])]!r}"
    assert np.array_equal(got["succ"], ref["succ"])
    assert np.array_equal(got["cells"], ref["cells"])
    assert np.array_equal(bits(got["y"]), bits(ref["y"]))
    assert np.array_equal(got["flags"], ref["flags"])


def test_repeated_calls_and_chunkings_are_bit_identical(dev):
    a, b, c = run("all_k3"), run("all_k3"), run("all_k3", chunk_pairs=1)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), k
    # 8 pairs in chunks of 3, 3, 2: a shorter last chunk beside the entry's extra block (gx, level offsets); then 1000 bytes more, which
    # is still 3 pairs and no size the library returns
    assert workspace("all_k3", 4) - workspace("all_k3", 3) > 1000
    for got in (run("all_k3", chunk_pairs=3), run("all_k3", chunk_pairs=3, slack=1000)):
        assert set(got) == set(a)
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), got[k].view(np.uint8)), k


def test_an_object_without_segments_is_loose_everywhere(dev):
    sl = engine.squeeze_slice(meshes()[1:2], [0.5, 0.6, 0.7])
    out = engine.squeeze_tables_3d(np.stack([surfaces(1)]), GX, sl["segments"], sl["offsets"], [(0, 0)], starts(0.06), tables=True, theta_cells=THETA,
                                   x_cells=9)
    assert torch.isinf(out["S"]).all() and (out["flags"].cpu().numpy() & 3 == 3).all()
    assert np.array_equal(out["cells"][0, :, 0].cpu().numpy(), out["cells"][0, :, 2].cpu().numpy())


@pytest.mark.parametrize("name", ["box", "frustum", "lifted"])
def test_closed_forms_hold_on_the_device(dev, name):
    """The three closed forms of tests/test_squeeze3d_host.py, over all 1800 starts, from the device's tables."""
    verts, tris = {"box": host.box(top=1.0, height=float(host.GZ[5])), "frustum": host.box(top=0.5), "lifted": host.box(top=0.5, lift=0.003)}[name]
    lower, upper = host.flat_jaws(1.0 if name == "lifted" else 0.0)
    sl = engine.squeeze_slice([(verts, tris)], host.GZ)
    assert np.diff(sl["offsets"][0]).tolist() == [0, 8, 8, 8, 8, 8] + [0] * 7 or name == "frustum"
    out = engine.squeeze_tables_3d(np.stack([lower, upper])[None], host.GX, sl["segments"], sl["offsets"], [(0, 0)], host.grid_starts(), tables=True,
                                   theta_cells=host.T, x_cells=host.X, x_half=host.X_HALF, window=host.WINDOW, closing_steps=host.STEPS,
                                   travel_max=host.TRAVEL)
    r = {k: v.cpu().numpy()[0] for k, v in out.items()}
    host.assert_box_basins(r)
    ref = host.case(name)[2]
    assert np.array_equal(bits(r["S"]), bits(ref["S"])) and np.array_equal(r["cells"], ref["cells"])
    if name == "lifted":
        assert abs(r["S"][0, 2] - 0.14205) <= 1e-12


def test_prism_agrees_with_the_2d_entry(dev):
    """An extruded 8-gon (corner edges vertical) between jaws that are constant in z, gx built as the 2-D entry builds it (-hl + j h): every
    level's cross-section is the polygon, so touch_l / touch_r must agree with dgdm_squeeze_map on the polygon within 1e-12 m.  Not
    bitwise: the 2-D entry's interpolation weight is t - floor(t) with t = (x + hl) / h, this entry's is (x - gx_i) / (gx_{i+1} - gx_i),
    rounded differently, and a wall's two triangles cut each polygon edge in two at a point that is only collinear up to rounding.  The
    values are about 0.1 m and the weights multiply profile differences below 0.02 m: the difference is a few ulp of 0.1, 1e-16, far
    inside the bound; an error of the model (a missed candidate) would be of the order of the profile's relief, 1e-3."""
    m, hl, T, X = 33, 0.12, 24, 17
    h = 2.0 * hl / (m - 1)
    gx = -hl + np.arange(m, dtype=np.float64) * h
    rs = np.random.RandomState(4)
    u = np.linspace(-1.0, 1.0, m)
    prof = np.stack([-0.12 + sum(rs.uniform(-0.01, 0.01) * np.cos(k * np.pi * u + rs.uniform(0, 6)) for k in range(1, 4)),
                     0.15 + sum(rs.uniform(-0.01, 0.01) * np.cos(k * np.pi * u + rs.uniform(0, 6)) for k in range(1, 4))])
    poly = ngon(8, 0.04, 0.2) * np.array([1.0, 0.6]) + np.array([0.005, 0.0])
    cfg = dict(theta_cells=T, x_cells=X, x_half=0.06, finger_half_len=hl)
    flat = engine.squeeze_tables(prof[None], poly[None], [(0, 0)], None, tables=True, **cfg)
    sl = engine.squeeze_slice([prism(poly, -0.01, 0.07, caps=False)], GZ)
    assert np.diff(sl["offsets"][0]).tolist() == [16, 16, 16]
    sf3 = np.repeat(prof[:, None, :], len(GZ), axis=1)[None]
    sliced3 = engine.squeeze_tables_3d(sf3, gx, sl["segments"], sl["offsets"], [(0, 0)], None, tables=True, **cfg)
    for k in ("touch_l", "touch_r"):
        a, b = flat[k].cpu().numpy(), sliced3[k].cpu().numpy()
        assert np.isfinite(a).all() and np.isfinite(b).all()
        print(k, "max |3-D - 2-D| =", np.abs(a - b).max())
        assert np.abs(a - b).max() <= 1e-12, k


def test_every_bad_argument_is_refused_before_a_launch(dev):
    lib = _lib.lib()
    mu, mv = len(GX), len(GZ)
    sf = torch.zeros(2, 2, mv, mu, dtype=torch.float64, device=dev)
    sl = engine.squeeze_slice(meshes()[1:3], GZ)
    seg, off = sl["segments"], sl["offsets"]
    rot = torch.zeros(8, 2, dtype=torch.float64, device=dev)
    st = torch.zeros(2, 3, dtype=torch.float64, device=dev)
    cells = torch.full((1, 2, 3), -7, dtype=torch.int32, device=dev)
    y = torch.zeros(1, 2, 2, dtype=torch.float64, device=dev)
    flags = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    good = dict(theta_cells=8, x_cells=5, window=1, closing_steps=2, x_half=0.06, travel_max=0.1, finger_half_len=0.12)
    ws_bytes = int(lib.dgdm_squeeze_map_3d_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1, mu, mv, 2))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def call(cfg=None, gx=GX, mu_=mu, mv_=mv, offsets=off, n_seg=len(seg), pair=(1, 1), n_pairs=1, nf=2, no=2, surf=sf, segs=seg, ws_b=ws_bytes,
             cells_out=cells):
        c = engine.squeeze_config(**dict(good, **(cfg or {})))
        pr = np.array([pair], dtype=np.int32)
        g = None if gx is None else np.ascontiguousarray(gx, dtype=np.float64)
        of = np.ascontiguousarray(offsets, dtype=np.int32)
        return lib.dgdm_squeeze_map_3d(C.byref(c), _lib.dptr(surf), nf, None if g is None else g.ctypes.data, mu_, mv_, _lib.dptr(segs), n_seg,
                                       of.ctypes.data, no, pr.ctypes.data, n_pairs, _lib.dptr(rot), _lib.dptr(st), 2, _lib.dptr(cells_out), _lib.dptr(y),
                                       _lib.dptr(flags), None, None, None, None, _lib.dptr(ws), ws_b, None)

    down, late, past = off.copy(), off.copy(), off.copy()
    down[0, 1] = down[0, 2] + 1
    late[0, 0] = 1
    past[1, 3] = len(seg) + 1
    nan_gx, flat_gx = GX.copy(), GX.copy()
    nan_gx[2] = np.nan
    flat_gx[3] = flat_gx[2]
    bad = [dict(cfg=dict(theta_cells=0)), dict(cfg=dict(x_cells=1)), dict(cfg=dict(theta_cells=1 << 20, x_cells=1 << 11)), dict(cfg=dict(window=0)),
           dict(cfg=dict(closing_steps=-1)), dict(cfg=dict(x_half=0.0)), dict(cfg=dict(x_half=float("nan"))), dict(cfg=dict(travel_max=float("inf"))),
           dict(cfg=dict(finger_half_len=-0.1)), dict(mu_=1), dict(mu_=129), dict(mv_=0), dict(mv_=513), dict(mu_=128, mv_=9), dict(gx=nan_gx),
           dict(gx=flat_gx), dict(gx=GX[::-1]), dict(gx=np.r_[GX[:4], np.inf]), dict(gx=None), dict(offsets=down), dict(offsets=late), dict(offsets=past),
           dict(n_seg=len(seg) - 1), dict(n_seg=-1), dict(segs=None), dict(pair=(2, 0)), dict(pair=(0, 2)), dict(pair=(-1, 0)), dict(n_pairs=0), dict(nf=0),
           dict(no=0), dict(surf=None), dict(ws_b=ws_bytes - 1), dict(cells_out=None)]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.dgdm_last_error()
    torch.cuda.synchronize()
    assert (cells.cpu() == -7).all()                          # nothing was launched
    assert call() == _lib.OK and (cells.cpu() >= 0).all()
    assert lib.dgdm_squeeze_map_3d_workspace_bytes(C.byref(engine.squeeze_config(**good)), 0, mu, mv, 2) == _lib.EINVAL
    assert lib.dgdm_squeeze_map_3d_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1, 1, mv, 2) == _lib.EINVAL
    assert lib.dgdm_squeeze_map_3d_workspace_bytes(C.byref(engine.squeeze_config(**dict(good, window=0))), 1, mu, mv, 2) == _lib.EINVAL

    # the slicer
    v, f = meshes()[1]
    v = np.ascontiguousarray(v, dtype=np.float64)
    voff, toff = np.array([0, len(v)], dtype=np.int64), np.array([0, len(f)], dtype=np.int64)
    out = torch.full((len(f) * mv, 4), -7.0, dtype=torch.float64, device=dev)
    offs = np.zeros((1, mv + 1), dtype=np.int32)

    def cut(verts=v, tris=f, vo=voff, to=toff, n=1, gz=GZ, mv_=mv, dst=out, cap=None, offsets=offs):
        cnt = C.c_int64(-1)
        z = None if gz is None else np.ascontiguousarray(gz, dtype=np.float64)
        p = lambda a: None if a is None else a.ctypes.data       # noqa: E731
        rc = lib.dgdm_squeeze_slice(p(verts), p(vo), p(tris), p(to), n, p(z), mv_, _lib.dptr(dst), len(dst) if cap is None else cap, p(offsets),
                                    C.byref(cnt), None)
        return rc, cnt.value

    f_bad, f_neg, v_nan = f.copy(), f.copy(), v.copy()
    f_bad[3, 1] = len(v)
    f_neg[0, 0] = -1
    v_nan[2, 2] = np.nan
    for kw in (dict(verts=None), dict(tris=None), dict(vo=None), dict(to=None), dict(gz=None), dict(offsets=None), dict(n=0), dict(mv_=0), dict(mv_=1025),
               dict(gz=GZ[::-1]), dict(gz=np.array([0.0, 0.0, 0.05])), dict(gz=np.array([0.0, np.nan, 0.05])), dict(tris=f_bad), dict(tris=f_neg),
               dict(verts=v_nan), dict(vo=np.array([1, len(v)], dtype=np.int64)), dict(vo=np.array([0, 0], dtype=np.int64)),
               dict(to=np.array([0, -1], dtype=np.int64)), dict(cap=-1), dict(dst=None, cap=4)):
        assert cut(**kw)[0] == _lib.EINVAL, kw
        assert lib.dgdm_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == -7.0).all()
    rc, need = cut(cap=15)                                     # a capacity too small: refused after the count, which it reports; nothing emitted
    assert rc == _lib.EINVAL and need == 16 and b"16" in lib.dgdm_last_error() and (out.cpu() == -7.0).all()
    assert cut(dst=None, cap=0) == (_lib.OK, 16)               # count only
    assert cut() == (_lib.OK, 16) and offs.tolist() == [[0, 8, 16, 16]] and (out[:16].cpu() != -7.0).all() and (out[16:].cpu() == -7.0).all()
    with pytest.raises(ValueError, match="triangle"):
        engine.squeeze_slice([(v, f_bad)], GZ)
    with pytest.raises(ValueError, match="ascending"):
        engine.squeeze_tables_3d(sf, flat_gx, seg, off, [(0, 0)], st)


def write_meshes(root, names):
    for k, name in enumerate(names):
        v, f = prism(rect(0.03 + 0.004 * k, 0.02 - 0.002 * k, (0.002 * k, 0.0)), 0.0, 0.05 + 0.01 * k)
        os.makedirs(os.path.join(root, name))
        engine.write_obj(os.path.join(root, name, "model.obj"), v, f)


def test_squeeze_simulator_3d_metrics(dev, tmp_path):
    """The callable itself: build_metric's keys over num_rot orientations, object-major, the marks, and the oracle's poses."""
    from dgdm_amd.dynamics.dataloader import SCORE_THRESHOLD
    from dgdm_amd.dynamics.predicted import build_metric
    from dgdm_amd.sim import squeeze
    write_meshes(str(tmp_path), ["alpha", "beta"])

    class Holder:
        mode = 'point_3d'
        object_mesh_dir = str(tmp_path)

    sim = squeeze.SqueezeSimulator3D(Holder(), closing_steps=3, theta_cells=90, x_cells=33, travel_max=0.2)
    samples = np.random.RandomState(0).uniform(-1, 1, (3, 42, 1)).astype(np.float32)
    out = sim(samples, ["beta", "alpha"], None, num_rot=45, ori_range=(-0.5, 1.0))
    assert len(out) == 8 and len(out[1]) == 6 and all(v is None for v in out[0] + out[2] + out[3] + out[4] + out[5] + out[7]) and out[6] == [[]] * 6
    want = build_metric(np.zeros((45, 3), dtype=np.float32), [1, 1, 1], [1, 1, 1], (-0.5, 1.0))
    for m in out[1]:
        assert 'predicted' not in m and m['simulated'] == 'squeeze' and 0 <= m['squeeze_loose'] <= 45 and 0 <= m['squeeze_cut'] <= 45
        for k, v in want.items():
            if k != 'predicted':
                assert np.asarray(m[k]).shape == np.asarray(v).shape and np.asarray(m[k]).dtype == np.asarray(v).dtype, k
        assert set(np.unique(m['profile'])) <= {0, 1, 2}
    # pair 4 = (object 'alpha', gripper 1): the same poses from the oracle on the decoded faces, classes with the 3-D thresholds
    gx, gz, sf = squeeze.finger_surfaces_3d(torch.as_tensor(samples[:, :, 0]))
    assert gx.shape == gz.shape == (25,) and sf.shape == (3, 2, 25, 25) and (np.diff(gx) > 0).all() and np.allclose(gz, 0.12 * np.arange(25) / 24, atol=1e-8)
    assert np.ptp(np.diff(gx)) > 1e-4                                                               # the abscissae are not uniform
    pts = engine.finger_decode_3d(torch.as_tensor(samples[1:2]).to(dev), 25).double().cpu().numpy()[0]
    assert np.array_equal(sf[1, 0].cpu().numpy(), pts[0, :, 1].reshape(25, 25).T - 0.23 + 0.1) and np.array_equal(sf[1, 1].cpu().numpy(), pts[1, :, 1].reshape(25, 25).T + 0.23)
    seg, off = so3.slice_meshes([engine.read_obj(str(tmp_path / "alpha" / "model.obj"))], gz)
    theta0 = (np.linspace(-0.5, 1.0, 45) + 1.0) * np.pi
    st = np.stack([theta0, np.zeros(45), np.zeros(45)], axis=1)
    sfh = sf[1].cpu().numpy()
    ref = so3.squeeze_pair_3d(sfh[0], sfh[1], gx, seg, off[0], so.rotation_table(90), st, 33, 0.06, 2, 3, 0.2)
    th, x = so.cell_pose(ref["cells"], 90, 33, 0.06)
    m = out[1][4]
    d_theta = squeeze.fold(th[:, 1] - th[:, 0], 2.0 * np.pi)
    # a cell's angle is a multiple of 4 degrees made on the device in another operation order than cell_pose's: equal to rounding, 1e-9
    # degrees, where a wrong cell would be 4 degrees off
    assert np.abs(m['delta_theta'] - d_theta * squeeze.DEG).max() <= 1e-9 and np.abs(m['final_theta'] - th[:, 2] * squeeze.DEG).max() <= 1e-9
    assert np.array_equal(m['delta_pos'][:, 1], ref["y"][:, 0] * squeeze.CM)
    thr = SCORE_THRESHOLD[0][0]
    assert np.array_equal(m['profile'], np.where(d_theta > thr, 2, np.where(d_theta < -thr, 0, 1)))
    with pytest.raises(ValueError, match="no mesh"):
        sim(samples[:1], ["gamma"], None, num_rot=4)


def test_squeeze_sim_3d_fills_the_tables(dev, tmp_path):
    """--squeeze_sim_3d through the command-line entry point on a synthetic 3-D model with mesh-backed objects: the tables are written,
    every score carries 'simulated': 'squeeze' and none 'predicted'; the sampled designs are bit-identical with the flag on and off."""
    from dgdm_amd.generator.train import OBJECT_NAMES_3D, train
    from dynamics.parser import parse
    write_meshes(str(tmp_path / "objects"), OBJECT_NAMES_3D)
    common = (f"--mode=test --classifier_guidance --fingers_3d --object_max_num_vertices=512 --ctrlpts_dim=42 --sub_bs=40 --num_fingers=2 --batch_size=2 "
              f"--grid_size=3 --num_pos=3 --num_train_timesteps=15 --num_inference_steps=2 --object_dir={tmp_path / 'objects'}")
    runs, states = {}, {}
    for tag, extra in (("off", ""), ("on", " --squeeze_sim_3d --squeeze_closing_steps 4 --squeeze_window 1")):
        torch.manual_seed(7)
        _, runs[tag] = train(parse(shlex.split(common + extra + f" --save_dir={tmp_path / tag}")))
        states[tag] = torch.get_rng_state()
    assert runs["on"][0].keys() == runs["off"][0].keys()
    for k, v in runs["off"][0].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, runs["on"][0][k]), k
    assert torch.equal(states["on"], states["off"])
    tables = sorted(os.listdir(tmp_path / "on" / "tables"))
    assert "SKIPPED.txt" not in tables and tables
    for t in tables:
        tab = json.load(open(tmp_path / "on" / "tables" / t))
        oc = tab["columns"].index("objective")
        scores = [row[oc] for row in tab["data"] if isinstance(row[oc], dict) and row[0] != -1]
        assert tab["data"] and scores, t
        assert all(s.get("simulated") == "squeeze" and "predicted" not in s for s in scores), t
    with pytest.raises(ValueError, match="mesh files"):
        train(parse(shlex.split(common.split(" --object_dir")[0] + f" --squeeze_sim_3d --save_dir={tmp_path / 'none'}")))


def test_generate_writes_files_the_dataset_reads(dev, tmp_path):
    """sim_3d.generate at 2 grippers x 2 objects: the files go through DynamicsDataset(fingers_3d=True), the deltas equal the oracle's on
    the same pair."""
    from dgdm_amd.dynamics.dataloader import DynamicsDataset, load_score_stats
    from dgdm_amd.sim import sim_2d, sim_3d
    write_meshes(str(tmp_path / "objects"), ["0", "1"])
    meshes_ = [engine.read_obj(str(tmp_path / "objects" / n / "model.obj")) for n in ("0", "1")]
    cfg = dict(theta_cells=360, x_cells=41, travel_max=0.2)
    files = sim_3d.generate(str(tmp_path / "data"), [3, 4], meshes_, [0, 1], ["0", "1"], **cfg)
    assert sorted(os.path.basename(f) for f in files) == ["0_3.npz", "0_4.npz", "1_3.npz", "1_4.npz"]
    stats = load_score_stats(str(tmp_path / "data" / "stats.json"))
    ds = DynamicsDataset(str(tmp_path / "data"), object_max_num_vertices=128, fingers_3d=True, object_mesh_dir=str(tmp_path / "objects"), **stats)
    item = ds[0]
    assert len(ds) == 4 and item['scores'].shape == (9000, 3) and item['ctrlpts'].shape == (42, 3) and item['object_vertices'].shape == (128, 3)
    assert torch.isfinite(item['scores']).all()
    d = np.load(tmp_path / "data" / "1_4.npz", allow_pickle=True)['arr_0'].item()
    assert d["object_name"] == "1" and d["allpts"].shape == (1250, 3) and d["delta_theta"].any()
    yl, yr = sim_3d.gripper_design(4)
    assert np.array_equal(d["ctrlpts"][:, 1], np.concatenate([yl, yr]))
    gx, gz = d["allpts"][:625].reshape(25, 25, 3)[:, 0, 0], d["allpts"][:625].reshape(25, 25, 3)[0, :, 2]
    lower, upper = d["allpts"][:625, 1].reshape(25, 25).T - 0.23 + 0.1, d["allpts"][625:, 1].reshape(25, 25).T + 0.23
    seg, off = so3.slice_meshes(meshes_[1:], gz)
    ref = so3.squeeze_pair_3d(lower, upper, gx, seg, off[0], so.rotation_table(360), sim_2d.pose_grid(), 41, 0.06, 2, 6, 0.2)
    th, x = so.cell_pose(ref["cells"], 360, 41, 0.06)
    assert np.array_equal(d['delta_pos'][:, 0], x[:, 1] - x[:, 0]) and np.array_equal(d['delta_pos'][:, 1], ref["y"][:, 0] - d['obj_pos'][:, 1])
    assert np.array_equal(d['delta_theta'], sim_2d.fold(th[:, 1] - th[:, 0], 2.0 * np.pi).astype(np.float32))
    # the command line: the reference's seven arguments, the objects under MODEL_ROOT/objects
    os.makedirs(tmp_path / "root")
    os.symlink(tmp_path / "objects", tmp_path / "root" / "objects")
    sim_3d.main([str(tmp_path / "root"), "3", "1", "1", "1", str(tmp_path / "cli"), "0", "--squeeze_closing_steps", "6"])
    assert os.listdir(tmp_path / "cli") and np.array_equal(np.load(tmp_path / "cli" / "1_3.npz", allow_pickle=True)['arr_0'].item()["delta_theta"].shape, (9000,))
