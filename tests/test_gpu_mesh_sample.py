"""Object point clouds from OBJ meshes on the GPU (csrc/mesh.hip, dgdm_amd/dynamics/utils.py) against the float64 oracle of the sampling
contract (tests/test_mesh_obj.py, DESIGN.md "Object clouds from meshes"), and the two places the reference samples them: the test objects
of guided sampling (generator/train.py:100-109) and the objects of dynamics training (dynamics/dataloader.py:57-63)."""
import argparse
import os
import shlex
import zlib

import numpy as np
import pytest
import torch

from tests.test_mesh_obj import box_mesh, oracle_counts, oracle_sample

pytestmark = pytest.mark.gpu

LO, HI = np.array([-0.1, -0.1, 0.0]), np.array([0.1, 0.1, 0.12])       # the 3-D object box (generator/train.py:94-99)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def icosphere(level, seed):
    """A unit icosphere subdivided `level` times (20 * 4^level triangles), radius deformed smoothly."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = np.array(v, dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array(f, dtype=np.int64)
    for _ in range(level):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        e.sort(axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)
        v = np.concatenate([v, mid])
        a, b, c, ab, bc, ca = f[:, 0], f[:, 1], f[:, 2], m[0], m[1], m[2]
        f = np.concatenate([np.stack(x, axis=1) for x in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    rs = np.random.RandomState(seed)
    k = rs.uniform(1, 4, 3)
    r = 1 + 0.3 * np.sin(k[0] * v[:, 0]) * np.cos(k[1] * v[:, 1]) + 0.1 * np.sin(k[2] * v[:, 2])
    return v * r[:, None] * rs.uniform(0.5, 2.0, 3), f.astype(np.int32)


def object_mesh(i):
    """A small deformed icosphere inside the 3-D object box, metres."""
    v, f = icosphere(2, 100 + i)
    v = v / np.abs(v).max(axis=0) * np.array([0.05, 0.05, 0.05]) + np.array([0.0, 0.0, 0.06])
    return v, f


def write_obj(path, v, f):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("o object\n")
        fh.write("".join("v %.17g %.17g %.17g\n" % tuple(x) for x in v))
        fh.write("".join("f %d %d %d\n" % tuple(t + 1) for t in f))


def check_against_oracle(out, v, f, n, key, seed=0):
    """n_t as the oracle's except where cdf * N is within 1e-6 of a half-integer; those points lie on one of the two candidates."""
    pts, owner, cdfn = oracle_sample(v, f, n, key, seed)
    ambiguous = np.abs(cdfn - np.floor(cdfn) - 0.5) < 1e-6
    skip = np.zeros(n, dtype=bool)
    for t in np.nonzero(ambiguous)[0]:
        b = int(np.floor(cdfn[t] + 0.5))
        skip[max(b - 1, 0):min(b + 1, n)] = True
    scale = float(np.abs(v).max())
    err = np.abs(out - pts).max(axis=1)
    assert float(err[~skip].max(initial=0.0)) <= 1e-12 * scale, (float(err[~skip].max()), scale)
    # every point lies on its triangle (for the ambiguous boundary points: on one of the two triangles the count decides between)
    vv, ff = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)

    def bary(x, t):
        a, b, c = vv[ff[t, 0]], vv[ff[t, 1]], vv[ff[t, 2]]
        e1, e2, d = b - a, c - a, x - a
        g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        r1, r2 = (e1 * d).sum(1), (e2 * d).sum(1)
        det = g11 * g22 - g12 * g12
        bb, cc = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
        w = np.stack([1 - bb - cc, bb, cc], axis=1)
        return np.all((w >= -1e-12) & (w <= 1 + 1e-12), axis=1)

    on = bary(out, owner)
    if skip.any():
        alt = np.where(skip)[0]
        for nb in (owner[alt] - 1, owner[alt] + 1):
            nb = np.clip(nb, 0, len(ff) - 1)
            on[alt] |= bary(out[alt], nb)
    assert on.all(), np.nonzero(~on)[0][:10]
    return int(ambiguous.sum())


def test_against_oracle(dev):
    from dgdm_amd import engine
    tri = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]]), np.array([[0, 1, 2]], dtype=np.int32))
    bv, bf = box_mesh((-1.0, -0.5, 0.0), (1.0, 0.5, 0.25))
    # zero-area triangles mixed in: a repeated corner, three collinear corners (8 is the midpoint of 0-1)
    bv = np.concatenate([bv, [(bv[0] + bv[1]) / 2]])
    bf = np.insert(bf, [0, 3, 7, 12], [[0, 0, 1], [0, 8, 1], [2, 2, 2], [1, 8, 0]], axis=0).astype(np.int32)
    ico = icosphere(6, 0)                                # 81 920 triangles
    n_amb = {}
    for name, (v, f), n in (("triangle", tri, 1), ("triangle", tri, 1000), ("box", (bv, bf), 512), ("icosphere", ico, 512), ("icosphere", ico, 12345)):
        key = zlib.crc32(name.encode())
        vt, ft, off = engine.concat_meshes([(v, f)])
        out = engine.sample_mesh_points(vt, ft, off, [key], n).cpu().numpy()
        assert out.shape == (1, n, 3) and out.dtype == np.float64
        n_amb[(name, n)] = check_against_oracle(out[0], v, f, n, key)
    # zero-area triangles own no points: the box's device points lie on its twelve faces only
    _, _, _, counts = oracle_counts(bv, bf, 512)
    assert np.all(np.diff(np.concatenate([[0], counts]))[[0, 4, 9, 15]] == 0)
    print("triangles with cdf * N within 1e-6 of a half-integer:", n_amb)


def test_large_mesh_multi_chunk(dev):
    """About 2 M triangles (2 048 chunks of one mesh) and N = 2^20 points."""
    from dgdm_amd import engine
    k = 1001
    x, y = np.meshgrid(np.linspace(0, 1, k), np.linspace(0, 1, k), indexing="ij")
    z = 0.1 * np.sin(7 * x) * np.cos(5 * y) + 0.02 * np.sin(40 * x * y)
    v = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    i = (np.arange(k - 1)[:, None] * k + np.arange(k - 1)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + k, i + k + 1], 1), np.stack([i, i + k + 1, i + 1], 1)]).astype(np.int32)
    assert len(f) == 2_000_000
    n, key = 1 << 20, 99
    vt, ft, off = engine.concat_meshes([(v, f)])
    out = engine.sample_mesh_points(vt, ft, off, [key], n, seed=3).cpu().numpy()[0]
    amb = check_against_oracle(out, v, f, n, key, seed=3)
    print("2 M triangles, N = 2^20: ambiguous counts", amb)


def test_invariance_and_keys(dev):
    from dgdm_amd import engine
    A, B, C = icosphere(3, 1), icosphere(4, 2), box_mesh()
    kA, kB, kC = 11, 22, 33
    n = 777

    def run(ms, ks, seed=0):
        vt, ft, off = engine.concat_meshes(ms)
        return engine.sample_mesh_points(vt, ft, off, ks, n, seed=seed).cpu()

    abc = run([A, B, C], [kA, kB, kC])
    cab = run([C, A, B], [kC, kA, kB])
    alone = [run([m], [k])[0] for m, k in ((A, kA), (B, kB), (C, kC))]
    for j in range(3):
        assert torch.equal(abc[j], alone[j]) and torch.equal(cab[(j + 1) % 3], alone[j]), j
    assert torch.equal(run([A, B, C], [kA, kB, kC]), abc)                 # repeated call
    assert not torch.equal(run([A], [kA + 1])[0], alone[0])               # another key
    assert not torch.equal(run([A], [kA], seed=1)[0], alone[0])           # another seed


def test_errors_leave_the_stream_usable(dev):
    from dgdm_amd import _lib, engine
    good = box_mesh()
    flat = (np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]]), np.array([[0, 1, 2], [0, 0, 0]], dtype=np.int32))
    vt, ft, off = engine.concat_meshes([good, flat])
    with pytest.raises(_lib.DgdmError, match="mesh 1 has surface area 0") as e:
        engine.sample_mesh_points(vt, ft, off, [1, 2], 64)
    assert f"error {_lib.EINVAL}:" in str(e.value)
    bad = (good[0], np.array([[0, 1, 8]], dtype=np.int32))
    vt, ft, off = engine.concat_meshes([good, good, bad])
    with pytest.raises(_lib.DgdmError, match="mesh 2 has a triangle whose vertex index is outside"):
        engine.sample_mesh_points(vt, ft, off, [1, 2, 3], 64)
    vt, ft, off = engine.concat_meshes([good])
    out = engine.sample_mesh_points(vt, ft, off, [1], 64)
    torch.cuda.synchronize()
    check_against_oracle(out[0].cpu().numpy(), good[0], good[1], 64, 1)


def test_sample_pts_from_mesh(dev, tmp_path):
    from dynamics.utils import sample_pts_from_mesh
    v, f = object_mesh(0)
    path = str(tmp_path / "BABY_CAR" / "model.obj")
    write_obj(path, v, f)
    pts = sample_pts_from_mesh(path, 512)
    assert isinstance(pts, np.ndarray) and pts.shape == (512, 3) and pts.dtype == np.float64
    check_against_oracle(pts, v, f, 512, zlib.crc32(b"BABY_CAR"))
    assert np.array_equal(pts, sample_pts_from_mesh(path, 512))


def _unit(pts):
    return ((pts - LO) / (HI - LO) * 2.0 - 1.0).astype(np.float32)


def _write_sim_files(root, names, n_files, rs):
    """Data files in the simulator's format (as tests/test_gpu_train3d.py::test_training_driver_3d_end_to_end writes them)."""
    os.makedirs(root, exist_ok=True)
    for i in range(n_files):
        cells, y = 20, rs.uniform(-0.1, 0.0, 42)
        xg, zg = np.meshgrid(np.linspace(-0.12, 0.12, 7), np.linspace(0, 0.12, 3))
        ctrl = np.stack([np.tile(xg.T.reshape(-1), 2), y, np.tile(zg.T.reshape(-1), 2)], axis=1)
        th, pos = rs.uniform(0, 2 * np.pi, cells), rs.uniform(-0.03, 0.03, (cells, 3))
        d = {"ctrlpts": ctrl, "obj_theta": th, "obj_pos": pos, "object_name": names[i % len(names)],
             "delta_theta": 0.03 * np.sin(th) * (1 + 10 * y.mean()), "delta_pos": 0.05 * pos[:, :2] + 0.001 * np.cos(th)[:, None]}
        np.savez(os.path.join(root, f"s{i}.npz"), d)


def test_dataset_from_meshes(dev, tmp_path):
    from torch.utils.data import DataLoader
    from dynamics import dataloader as dl
    from dynamics.dataloader import DynamicsDataset
    names = ["obj0", "obj1"]
    objdir = tmp_path / "objects"
    meshes = {n: object_mesh(10 + k) for k, n in enumerate(names)}
    for n, (v, f) in meshes.items():
        write_obj(str(objdir / n / "model.obj"), v, f)
    _write_sim_files(str(tmp_path / "train"), names, 4, np.random.RandomState(0))
    _write_sim_files(str(tmp_path / "val"), names, 2, np.random.RandomState(1))
    kw = dict(object_max_num_vertices=512, fingers_3d=True, object_mesh_dir=str(objdir))
    ds = DynamicsDataset(str(tmp_path / "train"), **kw)
    for i in range(2):
        name = names[i % 2]
        pts, _, _ = oracle_sample(*meshes[name], 512, zlib.crc32(name.encode()))
        got = ds[i]["object_vertices"].numpy()
        assert got.shape == (512, 3) and got.dtype == np.float32
        assert np.abs(got - _unit(pts)).max() <= 2e-7                  # float32 of the normalised float64 cloud (one rounding)
    # the validation set reuses the clouds: no mesh is parsed again
    from dgdm_amd.dynamics import utils
    calls = []
    orig = utils.sample_object_clouds
    utils.sample_object_clouds = lambda *a, **k: calls.append(a) or orig(*a, **k)
    try:
        vs = DynamicsDataset(str(tmp_path / "val"), **kw)
    finally:
        utils.sample_object_clouds = orig
    assert not calls and torch.equal(vs[0]["object_vertices"], ds[0]["object_vertices"])
    assert len(dl._MESH_CLOUDS) >= 2
    # forked workers only read host arrays
    batches = list(DataLoader(ds, batch_size=2, shuffle=False, num_workers=2))
    assert len(batches) == 2 and torch.equal(batches[0]["object_vertices"][0], ds[0]["object_vertices"])
    # a points.npy next to the mesh still wins
    raw = np.random.RandomState(5).uniform(-0.05, 0.05, (600, 3)) + np.array([0, 0, 0.06])
    np.save(objdir / "obj0" / "points.npy", raw)
    ds2 = DynamicsDataset(str(tmp_path / "train"), **kw)
    assert np.abs(ds2[0]["object_vertices"].numpy() - _unit(raw[:512])).max() <= 2e-7


def _six_meshes(root):
    from dgdm_amd.generator.train import OBJECT_NAMES_3D
    meshes = {}
    for k, n in enumerate(OBJECT_NAMES_3D):
        meshes[n] = object_mesh(20 + k)
        write_obj(os.path.join(root, n, "model.obj"), *meshes[n])
    return meshes


def test_generator_objects(dev, tmp_path, capsys):
    from dgdm_amd.generator.train import OBJECT_NAMES_3D, _objects
    root = str(tmp_path / "objs")
    meshes = _six_meshes(root)
    args = argparse.Namespace(object_dir=root, object_max_num_vertices=512)
    objs, ids = _objects(args, True)
    assert ids == list(OBJECT_NAMES_3D) and objs.shape == (6, 512, 3) and objs.dtype == torch.float32
    for j, n in enumerate(OBJECT_NAMES_3D):
        pts, _, _ = oracle_sample(*meshes[n], 512, zlib.crc32(n.encode()))
        ref = ((torch.from_numpy(pts).float() - torch.tensor(LO).float()) / torch.tensor(HI - LO).float()) * 2.0 - 1.0
        assert float((objs[j] - ref).abs().max()) <= 1e-6, n
    assert "synthetic" not in capsys.readouterr().err
    # objects.npy keeps priority
    bank = np.random.RandomState(0).uniform(-0.05, 0.05, (3, 512, 3))
    np.save(os.path.join(root, "objects.npy"), bank)
    objs2, ids2 = _objects(args, True)
    assert ids2 == [0, 1, 2] and objs2.shape == (3, 512, 3)
    os.remove(os.path.join(root, "objects.npy"))
    # one mesh missing: synthetic objects, and the stderr line names the mesh
    os.remove(os.path.join(root, "BABY_CAR", "model.obj"))
    objs3, ids3 = _objects(args, True)
    err = capsys.readouterr().err
    assert ids3 == list(OBJECT_NAMES_3D) and "synthetic objects" in err and "BABY_CAR" in err and "3D_Dollhouse_Swing" not in err
    from dgdm_amd import synth
    assert torch.equal(objs3[0], synth.synth_object_3d(0, 512))


def test_guided_sampling_end_to_end_on_meshes(dev, tmp_path, capsys):
    from dgdm_amd.generator.train import train
    from dynamics.parser import parse
    root = tmp_path / "objs"
    _six_meshes(str(root))
    save = tmp_path / "out"
    argv = shlex.split(f"--mode=test --classifier_guidance --fingers_3d --num_fingers=4 --batch_size=2 --grid_size=3 --num_pos=2 --sub_bs=5 "
                       f"--object_max_num_vertices=512 --ctrlpts_dim=42 --num_train_timesteps=15 --num_inference_steps=5 --save_dir={save} "
                       f"--object_dir={root}")
    model, results = train(parse(argv))
    assert "synthetic objects" not in capsys.readouterr().err
    assert len(results) == 2 and results[0]["guided/rotate"].shape == (6, 2, 42, 1)
    assert os.path.exists(os.path.join(save, "vis_guided", "rotate_orirange=-1.000_1.000", "BABY_CAR.npy"))
