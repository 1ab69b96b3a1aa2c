"""Designed fingers as watertight meshes, convex collision pieces and gripper directories on the GPU (csrc/finger_mesh.hip,
dgdm_amd/assets/finger_mesh.py) against the numpy oracle of tests/finger_mesh_oracle.py.

No test loads the output into MuJoCo (it is not a dependency).  What is asserted is what a simulator needs from the files: meshes that are
closed and outward-oriented, pieces that are convex, and model files whose structure is the reference's (tests/test_finger_mesh_host.py)."""
import glob
import json
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

from dgdm_amd import engine, synth
from dgdm_amd.assets import finger_3d, finger_sampler, save_grippers
from tests import finger_mesh_oracle as fmo

pytestmark = pytest.mark.gpu

W2, H2, W3 = 0.03, 0.02, 0.1
VOL2, VOL3 = W2 * H2 * 0.24, W3 * 0.24 * 0.12            # the extrusion is a shear: the volume does not depend on the design
HALF_ULP = 2.0 ** -28                                     # half a float32 ulp at 0.12 m, the largest coordinate: 3.7e-9 m


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def designs(batch, L, seed):
    """Random designs in [-1, 1]; with a batch of 3 the second is all +1 and the third all -1."""
    s = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (batch, L, 1)).astype(np.float32))
    if batch >= 3:
        s[1], s[2] = 1.0, -1.0
    return s


def check_stats(verts, faces, st, vol, worst):
    """Device statistics against the float64 recomputation (both float64, differing by summation order: 1e-12) and the shear invariant."""
    v = verts.cpu().numpy().reshape(-1, verts.shape[-2], 3)
    for m, row in zip(v, st.cpu().numpy().reshape(-1, 4)):
        rv, ra, rmin = fmo.volume_area(m, faces)
        assert abs(row[0] - rv) <= 1e-12 * abs(rv) and abs(row[1] - ra) <= 1e-12 * ra and abs(row[2] - rmin) <= 1e-12 * rmin
        assert row[3] == 0
        worst[0] = max(worst[0], abs(row[0] / vol - 1))
        assert abs(row[0] - vol) <= 1e-5 * vol, (row[0], vol)


@pytest.mark.parametrize("L", [8, 14])
@pytest.mark.parametrize("batch,n", [(1, 2), (3, 5), (3, 200), (1, 200)])
def test_mesh_2d(dev, batch, n, L):
    s = designs(batch, L, n + L).to(dev)
    v = engine.finger_mesh_2d(s, n)
    curve = engine.finger_decode_2d(s, n)
    assert v.shape == (batch, 2, 4 * n, 3) and v.dtype == torch.float32
    r = v.reshape(batch, 2, 4, n, 3)
    yw = curve[..., 1] + torch.tensor(W2, dtype=torch.float32, device=dev)
    zero, h = torch.zeros_like(yw), torch.full_like(yw, H2)
    for ring, (y, z) in enumerate(((curve[..., 1], zero), (yw, zero), (yw, h), (curve[..., 1], h))):
        want = torch.stack([curve[..., 0], y, z], -1)
        assert torch.equal(r[:, :, ring].contiguous().view(torch.int32), want.contiguous().view(torch.int32)), ring         # bit for bit
    faces = engine.finger_mesh_faces(2, n)
    worst = [0.0]
    st = engine.finger_mesh_stats(v, faces, 1e-12)
    assert st.shape == (batch, 2, 4) and st.dtype == torch.float64
    check_stats(v, faces, st, VOL2, worst)
    print(f"2-D n={n} L={L} batch={batch}: worst |volume / (width height 0.24) - 1| = {worst[0]:.3e}")
    # the epsilon counts: every triangle is below 1 m^2; other widths and heights scale the volume
    assert (engine.finger_mesh_stats(v, faces, 1.0)[..., 3] == len(faces)).all()
    v2 = engine.finger_mesh_2d(s, n, width=0.05, height=0.01)
    assert abs(float(engine.finger_mesh_stats(v2, faces)[0, 0, 0]) / (0.05 * 0.01 * 0.24) - 1) <= 1e-5


@pytest.mark.parametrize("batch,n", [(1, 2), (3, 4), (3, 25)])
def test_mesh_3d(dev, batch, n):
    s = designs(batch, 42, n).to(dev)
    v = engine.finger_mesh_3d(s, n)
    sheet = engine.finger_decode_3d(s, n)
    N = n * n
    assert v.shape == (batch, 2, 2 * N, 3)
    assert torch.equal(v[:, :, :N].contiguous().view(torch.int32), sheet.view(torch.int32))
    shifted = torch.stack([sheet[..., 0], sheet[..., 1] + torch.tensor(W3, dtype=torch.float32, device=dev), sheet[..., 2]], -1)
    assert torch.equal(v[:, :, N:].contiguous().view(torch.int32), shifted.contiguous().view(torch.int32))
    faces = engine.finger_mesh_faces(3, n)
    worst = [0.0]
    check_stats(v, faces, engine.finger_mesh_stats(v, faces, 1e-12), VOL3, worst)
    print(f"3-D n={n} batch={batch}: worst |volume / (width 0.24 0.12) - 1| = {worst[0]:.3e}")


def check_pieces(pieces, pfaces, pstats, vol):
    p = pieces.cpu().numpy()
    assert fmo.is_closed(pfaces)
    for finger, st in zip(p.reshape(-1, *p.shape[2:]), pstats.cpu().numpy().reshape(-1, p.shape[2], 4)):
        total = 0.0
        for piece in finger:
            assert fmo.convexity_excess(piece, pfaces) <= 1e-9
            total += fmo.volume_area(piece, pfaces)[0]
        assert abs(total - vol) <= 1e-5 * vol and abs(st[:, 0].sum() - vol) <= 1e-5 * vol
        assert (st[:, 0] > 0).all()


@pytest.mark.parametrize("batch,n,P", [(1, 2, 1), (3, 5, 2), (3, 5, 4), (3, 200, 16), (1, 200, 199)])
def test_pieces_2d(dev, batch, n, P):
    v = engine.finger_mesh_2d(designs(batch, 14, 7 * n + P).to(dev), n)
    pieces, chord = engine.finger_pieces_2d(v, P)
    assert pieces.shape == (batch, 2, P, 8, 3) and chord.shape == (batch, 2) and chord.dtype == torch.float64
    vh = v.cpu().numpy()
    want = np.array([[fmo.pieces_2d(vh[b, f], n, P) for f in range(2)] for b in range(batch)])
    assert np.array_equal(pieces.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    pfaces = engine.finger_mesh_faces(12)
    check_pieces(pieces, pfaces, engine.finger_mesh_stats(pieces, pfaces), VOL2)
    c = chord.cpu().numpy()
    for b in range(batch):
        for f in range(2):
            assert abs(c[b, f] - fmo.chord_2d(vh[b, f], n, P)) <= HALF_ULP
    if P == n - 1:
        assert (c == 0).all()
    elif n == 200:
        assert (c[0] > 0).all()                                     # a random cubic is not piecewise linear


@pytest.mark.parametrize("batch,n,pu,pv", [(1, 2, 1, 1), (3, 4, 2, 1), (3, 4, 3, 3), (3, 25, 8, 2)])
def test_pieces_3d(dev, batch, n, pu, pv):
    v = engine.finger_mesh_3d(designs(batch, 42, 11 * n + pu).to(dev), n)
    pieces, chord = engine.finger_pieces_3d(v, pu, pv)
    assert pieces.shape == (batch, 2, 2 * pu * pv, 6, 3) and chord.shape == (batch, 2)
    vh = v.cpu().numpy()
    want = np.array([[fmo.pieces_3d(vh[b, f], n, pu, pv) for f in range(2)] for b in range(batch)])
    assert np.array_equal(pieces.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    pfaces = engine.finger_mesh_faces(13)
    check_pieces(pieces, pfaces, engine.finger_mesh_stats(pieces, pfaces), VOL3)
    c = chord.cpu().numpy()
    for b in range(batch):
        for f in range(2):
            assert abs(c[b, f] - fmo.chord_3d(vh[b, f], n, pu, pv)) <= HALF_ULP
    if pu == n - 1 and pv == n - 1:
        assert (c == 0).all()
    elif n == 25:
        assert (c[0] > 0).all()
    with pytest.raises(ValueError, match="knot cells"):
        engine.finger_pieces_3d(v, n, 1)


def _listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("mode", ["point", "point_3d"])
def test_save_grippers_end_to_end(dev, tmp_path, mode):
    three_d = mode == "point_3d"
    L, P, kind, n = (42, 32, 3, 25) if three_d else (14, 16, 2, 200)
    s = designs(3, L, 5).to(dev)
    root = str(tmp_path / "model")
    dirs = save_grippers(s, root, first_idx=5, mode=mode)
    assert dirs == [os.path.join(root, "grippers", str(i)) for i in (5, 6, 7)]
    per = ["fingerl.obj", "fingerr.obj", "mesh.json"] + [f"finger{side}{k:03d}.obj" for side in "lr" for k in range(P)]
    want = sorted([f"gripper_{i}.xml" for i in (5, 6, 7)] + [os.path.join("grippers", str(i), f) for i in (5, 6, 7) for f in per])
    assert _listing(root) == want
    verts = (engine.finger_mesh_3d(s) if three_d else engine.finger_mesh_2d(s)).cpu().numpy()
    faces = engine.finger_mesh_faces(kind, n)
    for b, d in enumerate(dirs):
        for f, side in enumerate("lr"):
            rv, rt = engine.read_obj(os.path.join(d, f"finger{side}.obj"))
            assert np.array_equal(rv.astype(np.float32).view(np.uint32), verts[b, f].view(np.uint32)) and np.array_equal(rt, faces)
        info = json.load(open(os.path.join(d, "mesh.json")))
        assert info["fingerl"]["pieces"] == P and info["fingerr"]["chord_err"] >= 0 and info["fingerl"]["volume"] > 0
        x = ET.parse(os.path.join(root, f"gripper_{5 + b}.xml")).getroot()
        meshes = [m.get("file") for m in x.iter("mesh")]
        assert all(os.path.exists(os.path.join(root, m)) for m in meshes)
        for side in "lr":
            on_disk = len(glob.glob(os.path.join(d, f"finger{side}0*.obj")))             # how the reference counts them
            assert on_disk == P == len([m for m in meshes if os.path.basename(m).startswith(f"finger{side}0")])
            assert len([g for g in x.iter("geom") if g.get("class") == "collision" and g.get("mesh").startswith(f"finger{side}")]) == on_disk
    # a second call leaves what is there alone
    before = {f: os.stat(os.path.join(root, f)).st_mtime_ns for f in want}
    assert save_grippers(s, root, first_idx=5, mode=mode) == dirs
    assert before == {f: os.stat(os.path.join(root, f)).st_mtime_ns for f in _listing(root)}
    # the project's own reader and sampler consume the export
    mesh = engine.read_obj(os.path.join(dirs[0], "fingerl.obj"))
    mv, mt, off = engine.concat_meshes([mesh])
    pts = engine.sample_mesh_points(mv, mt, off, [1], 64).cpu().numpy()[0]
    assert (pts >= mesh[0].min(0) - 1e-12).all() and (pts <= mesh[0].max(0) + 1e-12).all() and np.ptp(pts, axis=0).min() > 0
    # a degenerate finger is refused by index, before anything is written
    with pytest.raises(ValueError, match="gripper 41: fingerl is degenerate"):
        save_grippers(s, str(tmp_path / "bad"), first_idx=41, mode=mode, area_eps=1.0)
    assert not os.path.exists(tmp_path / "bad")


def test_reference_named_functions(dev, tmp_path):
    """generate_finger_shape / save_gripper / generate_3d_finger_mesh / save_3d_gripper: the reference's names, arguments and returns."""
    rs = np.random.RandomState(3)
    x, yl, yr = np.linspace(-0.12, 0.12, 7), rs.uniform(-0.045, 0.015, 7), rs.uniform(-0.045, 0.015, 7)
    mesh, x_new, y_new = finger_sampler.generate_finger_shape(x, yl, 0.03, 0.02, num_points=50)
    assert mesh.vertices.shape == (200, 3) and mesh.faces.shape == (2 * (4 * 49 + 2), 3) and mesh.is_watertight
    assert abs(mesh.volume - VOL2) <= 1e-5 * VOL2 and mesh.area > 0
    _, allpts = finger_sampler.generate_gripper(x, yl, yr, 50)
    assert np.array_equal(np.stack([x_new, y_new], -1), allpts[:50])
    ctrl, pts = finger_sampler.save_gripper(x, yl, yr, 0.03, 0.02, 50, str(tmp_path / "g2"))
    assert ctrl.shape == (14, 2) and np.array_equal(pts, allpts)
    assert sorted(os.listdir(tmp_path / "g2")) == ["fingerl.obj", "fingerr.obj"]
    rv, rt = engine.read_obj(str(tmp_path / "g2" / "fingerl.obj"))
    assert np.array_equal(rv.astype(np.float32), mesh.vertices.astype(np.float32)) and np.array_equal(rt, mesh.faces)
    with pytest.raises(NotImplementedError):
        finger_sampler.generate_finger_shape(x * 0.5, yl, 0.03, 0.02)
    y3l, y3r = rs.uniform(-0.1, 0.0, 21), rs.uniform(-0.1, 0.0, 21)
    cp = finger_3d.generate_3d_ctrlpts(y3l, y3r)
    mesh3, surf = finger_3d.generate_3d_finger_mesh(cp[:21].tolist(), sample_size=10, width=0.1)
    assert mesh3.vertices.shape == (200, 3) and surf.shape == (100, 3) and mesh3.is_watertight and abs(mesh3.volume - VOL3) <= 1e-5 * VOL3
    assert np.array_equal(surf, finger_3d.generate_3d_finger_vertices(cp[:21], sample_size=10))
    ctrl3, v3 = finger_3d.save_3d_gripper(y3l, y3r, width=0.1, sample_size=10, save_gripper_dir=str(tmp_path / "g3"))
    assert ctrl3.shape == (42, 3) and v3.shape == (200, 3) and np.array_equal(v3[:100], surf)
    assert sorted(os.listdir(tmp_path / "g3")) == ["fingerl.obj", "fingerr.obj"]


def test_save_meshes_flag(dev, tmp_path):
    """One tiny guided run through Diffusion.guided_sample: with save_meshes the gripper directories appear next to the .npy files and
    are recorded; without it the run writes exactly the files it wrote before, and the .npy files are the same bytes either way."""
    from dynamics.parser import parse
    from tests import test_gpu_api as api
    assert parse(["--save_meshes"]).save_meshes and not parse([]).save_meshes
    B, G, P, L, nv = 4, 10, 2, 14, 100
    objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(2)])
    d, _ = api._diffusion('point', dev, B, G, P, L, objs)
    noise = synth.synth_noise(0, B, L).to(dev)
    tag = "shift_up_orirange=-1.000_1.000"
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    d.guided_sample(0, B, noise, off, opt_obj='shift_up')
    plain = sorted(os.path.join("vis_guided", tag, f"{i}{suffix}.npy") for i in range(2) for suffix in ("", "_geometry"))
    assert _listing(off) == plain and d.last_gripper_dirs == {}
    d.save_meshes = True
    out = d.guided_sample(0, B, noise, on, opt_obj='shift_up')
    dirs = d.last_gripper_dirs[tag]
    assert len(dirs) == 2 and all(len(x) == B for x in dirs)
    for i, per_object in enumerate(dirs):
        assert per_object == [os.path.join(on, "vis_guided", tag, str(i), "grippers", str(b)) for b in range(B)]
        for b, g in enumerate(per_object):
            assert os.path.isdir(g) and os.path.exists(os.path.join(on, "vis_guided", tag, str(i), f"gripper_{b}.xml"))
            rv, _ = engine.read_obj(os.path.join(g, "fingerr.obj"))
            want = engine.finger_mesh_2d(out[i, b:b + 1])[0, 1].cpu().numpy()
            assert np.array_equal(rv.astype(np.float32), want)
    assert [f for f in _listing(on) if f.endswith(".npy")] == plain
    for f in plain:
        assert open(os.path.join(off, f), "rb").read() == open(os.path.join(on, f), "rb").read()
