"""The sliced squeeze with Coulomb friction on the device (csrc/squeeze.hip: dgdm_squeeze_slice_normals, dgdm_squeeze_map_3d_friction)
against its float64 CPU restatement tests/squeeze3d_friction_oracle.py, through the C ABI and through the layers above it.

Every operation of the contract (include/dgdm_hip.h "squeeze simulator, 3-D fingers, with Coulomb friction") is a basic IEEE float64 one
or an int32 one, so nothing here has a tolerance: the slicer's normals, the three tables and y are compared bit for bit; the successors,
the three cells per start, the flags, the jam table and the contact codes as integers, with no row excluded.  Shapes: at most 24
orientations; (mv, mu) = (1, 2), (3, 5) and (5, 9) levels x abscissae, not uniform; a tetrahedron, a lobed vase of 40 triangles and that
vase with two levels exactly on its vertex rings; windows 1 and 2; closings of 0 and 3 steps; coefficients 0.1, 0.5 and 1; 40 starts, some
beyond the x range and non-finite ones; two fingers x two objects, all four pairs.  One case runs with a workspace of a single pair (the
chunk loop) and one with 300 x cells (the lanes' stride over the x cells).  Every parameter set holds jammed and free cells, which is
asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine
from tests import squeeze3d_friction_oracle as f3
from tests import squeeze3d_oracle as so3
from tests import test_squeeze3d_friction_host as host
from tests.test_gpu_squeeze_friction import starts

pytestmark = pytest.mark.gpu

XH, TM = 0.05, 0.1
PAIRS = [(f, o) for o in range(2) for f in range(2)]
# name: (levels mv, abscissae mu, the two meshes, theta cells, x cells)
SHAPES = {"flat": (1, 2, ("tetrahedron", "vase"), 24, 9), "mid": (3, 5, ("vase", "tetrahedron"), 24, 9), "rings": (5, 9, ("on_level", "vase"), 16, 9),
          "wide": (5, 9, ("vase", "on_level"), 2, 300)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def levels(mv, mesh_names):
    """mv levels inside the meshes' height; with the mesh 'on_level', the second and the fourth are exactly two of the vase's vertex rings."""
    gz = 0.004 + 0.06 * (np.arange(mv) + 0.3) / mv
    if "on_level" in mesh_names:
        ring_z = np.unique(host.vase(3)[0][:, 2])
        gz = np.array([0.01, ring_z[1], 0.03, ring_z[2], 0.05])[:mv]
    return gz


@functools.lru_cache(maxsize=None)
def scene(shape):
    """(surfaces [2][2][mv][mu], gx, gz, the two meshes) of a shape: two uneven jaw pairs, abscissae not uniform.  With mu = 2 the jaws are
    narrower than the object: end points beyond them are no candidates, and some cells have no contact at all (code -1, S = +inf)."""
    mv, mu, names, _, _ = SHAPES[shape]
    rs = np.random.RandomState(100 * mv + mu)
    gx = np.sort(rs.uniform(-0.1, 0.1, mu))
    gx[0], gx[-1] = (-0.1, 0.1) if mu > 2 else (-0.03, 0.045)         # two abscissae: under the object, so that set B has candidates at all
    gz = levels(mv, names)
    make = {"tetrahedron": host.tetrahedron, "vase": lambda: host.vase(1), "on_level": lambda: host.vase(3)}
    sf = np.stack([np.stack(host.wavy_jaws(gx, gz, seed, amp=amp)) for seed, amp in ((7, 0.012), (8, 0.003))])
    return sf, gx, gz, [make[n]() for n in names]


@functools.lru_cache(maxsize=None)
def contact_reference(shape):
    """The oracle's slices and tables per pair: they depend on neither the coefficient, the window nor the number of steps."""
    sf, gx, gz, meshes = scene(shape)
    _, _, _, T, X = SHAPES[shape]
    seg, off, nrm = f3.slice_meshes(meshes, gz)
    rot = so3.rotation_table(T)
    return seg, off, nrm, [f3.contact_tables_3d(sf[f][0], sf[f][1], gx, gz, seg, nrm, off[o], rot, X, XH) for f, o in PAIRS]


def reference(shape, window, k, mu):
    sf, gx, gz, _ = scene(shape)
    _, _, _, T, X = SHAPES[shape]
    seg, off, nrm, tabs = contact_reference(shape)
    rot, st = so3.rotation_table(T), starts(T, XH)
    outs = [f3.squeeze_pair_3d(sf[f][0], sf[f][1], gx, gz, seg, nrm, off[o], rot, st, X, XH, window, k, TM, mu=mu, tables=tab)
            for (f, o), tab in zip(PAIRS, tabs)]
    return {key: np.stack([o[key] for o in outs]) for key in outs[0]}


def run(shape, window, k, mu, chunk_pairs=4, entry="friction", slack=0):
    sf, gx, gz, meshes = scene(shape)
    mv, nu, _, T, X = SHAPES[shape]
    cfg = dict(theta_cells=T, x_cells=X, x_half=XH, window=window, closing_steps=k, travel_max=TM)
    size = _lib.lib().dgdm_squeeze_map_3d_friction_workspace_bytes if entry == "friction" else _lib.lib().dgdm_squeeze_map_3d_workspace_bytes
    ws = int(size(C.byref(engine.squeeze_config(**cfg)), chunk_pairs, nu, mv, 2)) + slack
    assert slack == 0 or ws < int(size(C.byref(engine.squeeze_config(**cfg)), chunk_pairs + 1, nu, mv, 2))
    sl = engine.squeeze_slice(meshes, gz, normals=True)
    kw = dict(friction_3d=mu, gz=gz, normals=sl["normals"], jam=True, contact=True) if entry == "friction" else {}
    out = engine.squeeze_tables_3d(sf, gx, sl["segments"], sl["offsets"], PAIRS, starts(T, XH), rot=so3.rotation_table(T), tables=True, workspace_bytes=ws,
                                   **cfg, **kw)
    return {key: v.cpu().numpy() for key, v in out.items()}


def compare(got, ref):
    for key in ("touch_l", "touch_r", "S"):
        bad = np.argwhere(bits(got[key]) != bits(ref[key]))
        assert len(bad) == 0, f"{key}: {len(bad)} cells differ, first (pair, a, b) = {bad[0]}: {got[key][tuple(bad[0])]!r} vs {ref[key][tuple(bad[0])]!r}"
    bad = np.argwhere(got["contact"] != ref["contact"])
    assert len(bad) == 0, f"contact: {len(bad)} differ, first (pair, a, b, side) = {bad[0]}: {got['contact'][tuple(bad[0])]} vs {ref['contact'][tuple(bad[0])]}"
    bad = np.argwhere(got["jam"] != ref["jam"])
    assert len(bad) == 0, f"jam: {len(bad)} cells differ, first (pair, a, b) = {bad[0]}, contacts {ref['contact'][tuple(bad[0])]}"
    assert np.array_equal(got["succ"], ref["succ"])
    assert np.array_equal(got["cells"], ref["cells"])
    assert np.array_equal(bits(got["y"]), bits(ref["y"]))
    assert np.array_equal(got["flags"], ref["flags"])


def holds_both(ref, shape):
    """Jammed and free cells, and contacts of both sets (k < 2: an end point on a jaw's patch; k >= 2: an abscissa under a segment)."""
    k = ref["contact"] % (SHAPES[shape][1] + 2)
    have = ref["contact"] >= 0
    return bool((ref["jam"] == 1).any() and (ref["jam"] == 0).any() and (have & (k < 2)).any() and (have & (k >= 2)).any())


def test_slice_normals_equal_the_oracle_and_the_segments_are_the_plain_slicer_s(dev):
    for shape in ("mid", "rings"):
        _, _, gz, meshes = scene(shape)
        seg, off, nrm = contact_reference(shape)[:3]
        plain, with_n = engine.squeeze_slice(meshes, gz), engine.squeeze_slice(meshes, gz, normals=True)
        assert set(plain) == {"segments", "offsets"} and set(with_n) == {"segments", "offsets", "normals"}
        assert np.array_equal(bits(plain["segments"].cpu().numpy()), bits(with_n["segments"].cpu().numpy())) and np.array_equal(plain["offsets"], with_n["offsets"])
        assert np.array_equal(bits(with_n["segments"].cpu().numpy()), bits(seg)) and np.array_equal(with_n["offsets"], off)
        got = with_n["normals"].cpu().numpy()
        assert got.shape == nrm.shape and len(nrm) > 20 and np.array_equal(bits(got), bits(nrm))
    assert (np.diff(off[0]) > 0).all()                             # 'rings': the two levels on vertex rings cut triangles too


@pytest.mark.parametrize("mu", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("shape", ["flat", "mid", "rings"])
def test_tables_and_maps_equal_the_oracle(dev, shape, mu):
    for window in (1, 2):
        for k in (0, 3):
            ref = reference(shape, window, k, mu)
            assert holds_both(ref, shape)
            compare(run(shape, window, k, mu), ref)
    assert (ref["flags"] & 8).any() and (ref["flags"] & 16).any() and (ref["cells"][..., 2] != ref["cells"][..., 0]).any()


def test_a_workspace_of_one_pair_runs_the_chunk_loop(dev):
    ref = reference("mid", 2, 3, 0.5)
    one, four = run("mid", 2, 3, 0.5, chunk_pairs=1), run("mid", 2, 3, 0.5)
    compare(one, ref)
    assert {"jam", "contact"} <= set(four)
    for got in (one, run("mid", 2, 3, 0.5, chunk_pairs=3), run("mid", 2, 3, 0.5, chunk_pairs=3, slack=1000)):      # 3 + 1: a shorter last chunk
        assert set(got) == set(four)
        for key in four:
            assert np.array_equal(four[key].view(np.uint8), got[key].view(np.uint8)), key


def test_more_x_cells_than_lanes(dev):
    """300 x cells on 256 lanes, 2 orientations: the second pass of the lanes over the x cells."""
    ref = reference("wide", 2, 3, 0.5)
    assert holds_both(ref, "wide") and (ref["jam"][:, :, 256:] == 1).any() and (ref["jam"][:, :, 256:] == 0).any() and (ref["jam"][:, :, :256] == 1).any()
    compare(run("wide", 2, 3, 0.5), ref)


def test_mu_zero_is_the_frictionless_entry_bit_for_bit(dev):
    new, old = run("mid", 2, 3, 0.0), run("mid", 2, 3, 0.0, entry="plain")
    assert set(new) - set(old) == {"jam", "contact"}
    for key in old:
        assert np.array_equal(new[key].view(np.uint8), old[key].view(np.uint8)), key
    assert not new["jam"].any()
    assert np.array_equal(new["contact"], reference("mid", 2, 3, 0.0)["contact"]) and (new["contact"] >= 0).any()
    assert not (new["flags"] & 24).any()


def device_pair(lower, upper, gx, gz, mesh, rot, st, mu, **cfg):
    sl = engine.squeeze_slice([mesh], gz, normals=True)
    out = engine.squeeze_tables_3d(np.stack([lower, upper])[None], gx, sl["segments"], sl["offsets"], [(0, 0)], st, rot=rot, tables=True, friction_3d=mu,
                                   gz=gz, normals=sl["normals"], **cfg)
    return {k: v.cpu().numpy()[0] for k, v in out.items()}


@pytest.mark.parametrize("mu, jams", [(0.10, False), (0.15, False), (0.20, True), (0.25, True)])
def test_prism_between_jaws_tilted_in_z_jams_when_mu_exceeds_tan_of_the_tilt(dev, mu, jams):
    """tests/test_squeeze3d_friction_host.py's closed form for the z component of the jaw's normal, on the device."""
    lower, upper, seg, off, nrm, rot, T, X, xh, tab = host.prism_case()
    n = 60
    ang = 2.0 * np.pi * (np.arange(n) + 0.5) / n
    ring = 0.03 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    verts = np.concatenate([np.c_[ring, np.zeros(n)], np.c_[ring, np.full(n, 0.06)]])
    tris = np.array([t for i in range(n) for t in ([i, (i + 1) % n, n + (i + 1) % n], [i, n + (i + 1) % n, n + i])], dtype=np.int32)
    st = host.grid_starts(T, X, xh)
    cfg = dict(theta_cells=T, x_cells=X, x_half=xh, window=2, closing_steps=6, travel_max=0.1)
    r = device_pair(lower, upper, host.GX5, host.GZ3, (verts, tris), rot, st, mu, **cfg)
    assert np.array_equal(r["contact"], tab["contact"]) and (r["S"] < 0.1).all()
    if jams:
        assert (r["jam"] == 1).all() and np.array_equal(r["cells"][:, 2], r["cells"][:, 0]) and (r["flags"] & 24 == 24).all()
    else:
        sl = engine.squeeze_slice([(verts, tris)], host.GZ3)
        free = engine.squeeze_tables_3d(np.stack([lower, upper])[None], host.GX5, sl["segments"], sl["offsets"], [(0, 0)], st, rot=rot, **cfg)
        assert (r["jam"] == 0).all() and np.array_equal(r["cells"], free["cells"].cpu().numpy()[0]) and (r["flags"] & 24 == 0).all()


@pytest.mark.parametrize("reverse", [False, True])
def test_frustum_face_on_a_ridge_jams_when_mu_exceeds_tan_of_the_lean(dev, reverse):
    """tests/test_squeeze3d_friction_host.py's closed form for the z component of the triangle's normal, on the device: the cell theta = 0,
    x = the ridge is free at 0.10 and 0.15 and jammed at 0.20 and 0.25, whichever way the mesh is wound."""
    lower, upper, seg, off, nrm, rot, T, X, xh, tab = host.frustum_case(reverse)
    top = (0.03 - 0.06 * host.TAN10) / 0.03
    base = np.array([[-0.03, -0.03], [0.03, -0.03], [0.03, 0.03], [-0.03, 0.03]])
    verts = np.concatenate([np.c_[base, np.zeros(4)], np.c_[base * top, np.full(4, 0.06)]])
    tris = host.BOX_F[:, ::-1].copy() if reverse else host.BOX_F
    cfg = dict(theta_cells=T, x_cells=X, x_half=xh, window=1, closing_steps=1, travel_max=0.1)
    for mu, jams in ((0.10, 0), (0.15, 0), (0.20, 1), (0.25, 1)):
        r = device_pair(lower, upper, host.GX5, host.GZ3, (verts, tris), rot, None, mu, **cfg)
        assert np.array_equal(r["contact"], tab["contact"]) and r["contact"][0, 2].tolist() == tab["contact"][0, 2].tolist()
        assert r["jam"][0, 2] == jams and np.array_equal(r["jam"], f3.jam_table_3d(tab, mu, 0.1))


def test_every_bad_argument_is_refused_before_a_launch(dev):
    lib = _lib.lib()
    sf_h, gx, gz, meshes = scene("mid")
    mv, mu = 3, 5
    sf = torch.as_tensor(sf_h).to(dev)
    sl = engine.squeeze_slice(meshes, gz, normals=True)
    seg, off, nrm = sl["segments"], sl["offsets"], sl["normals"]
    rot = torch.as_tensor(so3.rotation_table(8)).to(dev)
    st = torch.zeros(2, 3, dtype=torch.float64, device=dev)
    cells = torch.full((1, 2, 3), -7, dtype=torch.int32, device=dev)
    jam = torch.full((1, 8, 5), -7, dtype=torch.int32, device=dev)
    contact = torch.full((1, 8, 5, 2), -7, dtype=torch.int32, device=dev)
    y = torch.zeros(1, 2, 2, dtype=torch.float64, device=dev)
    flags = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    good = dict(theta_cells=8, x_cells=5, window=1, closing_steps=2, x_half=0.05, travel_max=0.1, finger_half_len=0.12)
    ws_bytes = int(lib.dgdm_squeeze_map_3d_friction_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1, mu, mv, 2))
    assert ws_bytes > int(lib.dgdm_squeeze_map_3d_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1, mu, mv, 2))      # the jam table and gz live there
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def call(cfg=None, gx_=gx, gz_=gz, mu_=mu, mv_=mv, offsets=off, n_seg=len(seg), pair=(1, 1), n_pairs=1, nf=2, no=2, surf=sf, segs=seg, normals=nrm,
             ws_b=ws_bytes, cells_out=cells, fmu=0.5):
        c = engine.squeeze_config(**dict(good, **(cfg or {})))
        pr = np.array([pair], dtype=np.int32)
        g = None if gx_ is None else np.ascontiguousarray(gx_, dtype=np.float64)
        z = None if gz_ is None else np.ascontiguousarray(gz_, dtype=np.float64)
        of = np.ascontiguousarray(offsets, dtype=np.int32)
        return lib.dgdm_squeeze_map_3d_friction(C.byref(c), _lib.dptr(surf), nf, None if g is None else g.ctypes.data, mu_, mv_, _lib.dptr(segs), n_seg,
                                                of.ctypes.data, no, pr.ctypes.data, n_pairs, _lib.dptr(rot), _lib.dptr(st), 2, _lib.dptr(cells_out),
                                                _lib.dptr(y), _lib.dptr(flags), None, None, None, None, _lib.dptr(ws), ws_b, None,
                                                None if z is None else z.ctypes.data, _lib.dptr(normals), fmu, _lib.dptr(jam), _lib.dptr(contact))

    down, past = off.copy(), off.copy()
    down[0, 1] = down[0, 2] + 1
    past[1, 3] = len(seg) + 1
    huge = np.array([[0, 0, 0, 2 ** 31 - 1], [2 ** 31 - 1] * 4], dtype=np.int32)      # 2^31 - 1 segments x (mu + 2): a code would pass int32
    nan_gz, flat_gz, flat_gx = gz.copy(), gz.copy(), gx.copy()
    nan_gz[1] = np.nan
    flat_gz[2] = flat_gz[1]
    flat_gx[3] = flat_gx[2]
    bad = [dict(fmu=-0.1), dict(fmu=float("nan")), dict(fmu=float("inf")), dict(fmu=-float("inf")), dict(gz_=None), dict(gz_=nan_gz), dict(gz_=flat_gz),
           dict(gz_=gz[::-1]), dict(gz_=np.r_[gz[:2], np.inf]), dict(normals=None), dict(offsets=huge, n_seg=2 ** 31 - 1),
           dict(cfg=dict(theta_cells=0)), dict(cfg=dict(x_cells=1)), dict(cfg=dict(window=0)), dict(cfg=dict(closing_steps=-1)), dict(cfg=dict(x_half=0.0)),
           dict(cfg=dict(travel_max=float("inf"))), dict(mu_=1), dict(mu_=129), dict(mv_=0), dict(mv_=513), dict(gx_=flat_gx), dict(gx_=None),
           dict(offsets=down), dict(offsets=past), dict(n_seg=len(seg) - 1), dict(segs=None), dict(pair=(2, 0)), dict(pair=(0, 2)), dict(n_pairs=0),
           dict(nf=0), dict(no=0), dict(surf=None), dict(ws_b=ws_bytes - 1), dict(cells_out=None)]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.dgdm_last_error()
    torch.cuda.synchronize()
    assert (cells.cpu() == -7).all() and (jam.cpu() == -7).all() and (contact.cpu() == -7).all()       # nothing was launched
    assert call() == _lib.OK and (cells.cpu() >= 0).all() and ((jam.cpu() == 0) | (jam.cpu() == 1)).all() and (contact.cpu() >= -1).all()
    assert call(fmu=0.0) == _lib.OK and (jam.cpu() == 0).all()
    assert lib.dgdm_squeeze_map_3d_friction_workspace_bytes(C.byref(engine.squeeze_config(**good)), 0, mu, mv, 2) == _lib.EINVAL
    assert lib.dgdm_squeeze_map_3d_friction_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1, 1, mv, 2) == _lib.EINVAL
    assert lib.dgdm_squeeze_map_3d_friction_workspace_bytes(C.byref(engine.squeeze_config(**dict(good, window=0))), 1, mu, mv, 2) == _lib.EINVAL

    # the slicer with normals: segments_dev without normals_dev is refused, nothing emitted
    v, f = meshes[0]
    v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int32)
    voff, toff = np.array([0, len(v)], dtype=np.int64), np.array([0, len(f)], dtype=np.int64)
    out = torch.full((len(f) * mv, 4), -7.0, dtype=torch.float64, device=dev)
    nout = torch.full((len(f) * mv, 3), -7.0, dtype=torch.float64, device=dev)
    offs = np.zeros((1, mv + 1), dtype=np.int32)
    z = np.ascontiguousarray(gz)
    cnt = C.c_int64(-1)
    cut = lambda dst, cap, nd, zz=z: lib.dgdm_squeeze_slice_normals(v.ctypes.data, voff.ctypes.data, f.ctypes.data, toff.ctypes.data, 1, zz.ctypes.data, mv,      # noqa: E731
                                                                    _lib.dptr(dst), cap, offs.ctypes.data, C.byref(cnt), None, _lib.dptr(nd))
    assert cut(out, len(out), None) == _lib.EINVAL and cut(out, len(out), nout, np.ascontiguousarray(z[::-1])) == _lib.EINVAL
    torch.cuda.synchronize()
    assert (out.cpu() == -7.0).all() and (nout.cpu() == -7.0).all()
    assert cut(None, 0, None) == _lib.OK and cnt.value == int(off[0, -1])                       # count only
    assert cut(out, len(out), nout) == _lib.OK and (nout[:cnt.value].cpu() != -7.0).any() and (nout[cnt.value:].cpu() == -7.0).all()
    with pytest.raises(ValueError, match="finite non-negative"):
        engine.squeeze_tables_3d(sf, gx, seg, off, [(0, 0)], st, friction_3d=-1.0)
    with pytest.raises(ValueError, match="needs gz and normals"):
        engine.squeeze_tables_3d(sf, gx, seg, off, [(0, 0)], st, friction_3d=0.5)


def test_squeeze_simulator_3d_with_friction(dev, tmp_path):
    """SqueezeSimulator3D(friction_3d=0.5) on a tiny mesh directory: the metric keys and marks, and the jam counts are the oracle's; without
    the argument the metrics carry today's keys only."""
    from dgdm_amd.sim import squeeze
    from tests.test_gpu_squeeze3d import write_meshes
    write_meshes(str(tmp_path), ["alpha", "beta"])

    class Holder:
        mode = 'point_3d'
        object_mesh_dir = str(tmp_path)

    cfg = dict(closing_steps=3, theta_cells=24, x_cells=9, travel_max=0.2)
    samples = np.random.RandomState(0).uniform(-1, 1, (2, 42, 1)).astype(np.float32)
    plain = squeeze.SqueezeSimulator3D(Holder(), **cfg)(samples, ["beta", "alpha"], None, num_rot=12, ori_range=(-0.5, 1.0))[1]
    out = squeeze.SqueezeSimulator3D(Holder(), friction_3d=0.5, **cfg)(samples, ["beta", "alpha"], None, num_rot=12, ori_range=(-0.5, 1.0))
    assert len(out) == 8 and len(out[1]) == 4
    gx, gz, sf = squeeze.finger_surfaces_3d(torch.as_tensor(samples[:, :, 0]))
    sfh = sf.cpu().numpy()
    st = squeeze.start_orientations(12, (-0.5, 1.0))
    seg, off, nrm = f3.slice_meshes([engine.read_obj(str(tmp_path / n / "model.obj")) for n in ("beta", "alpha")], gz)
    jammed = 0
    for p, (met, base) in enumerate(zip(out[1], plain)):
        assert set(met) - set(base) == {'squeeze_friction_3d', 'squeeze_jammed'} and set(base) <= set(met)
        assert 'predicted' not in met and met['simulated'] == 'squeeze' and met['squeeze_friction_3d'] == 0.5 and 'squeeze_friction' not in met
        assert 'squeeze_friction_3d' not in base and 'squeeze_jammed' not in base
        o, f = divmod(p, 2)                              # object-major, gripper-minor
        ref = f3.squeeze_pair_3d(sfh[f][0], sfh[f][1], gx, gz, seg, nrm, off[o], so3.rotation_table(24), st, 9, 0.06, 2, 3, 0.2, mu=0.5)
        assert met['squeeze_jammed'] == int(np.count_nonzero(ref["flags"] & 16))
        assert np.array_equal(np.rint(met['final_theta'] / 15.0).astype(np.int64) % 24, ref["cells"][:, 2] // 9)
        jammed += met['squeeze_jammed']
    assert jammed > 0
