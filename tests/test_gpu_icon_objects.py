"""Icon objects as meshes, convex pieces and loadable model roots on the GPU (csrc/polygon.hip, dgdm_amd/assets/icon_process.py) against
the CPU oracle of the ring contract (tests/polygon_oracle.py): every synthetic icon's status, ring, triangles and pieces
index for index; the meshes closed, outward and of the exact volume; the pieces convex; and a model root in which every file the scene
names exists.

No test loads the output into MuJoCo (it is not a dependency): what is asserted is what a simulator needs from the files."""
import json
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

from tests import finger_mesh_oracle as fmo
from tests import polygon_oracle as po
from tests.test_gpu_icon_contours import icons         # make_icon's stacks: the generator is shared, not restated

pytestmark = pytest.mark.gpu

HEIGHT, POINTS, PIXEL = 0.02, 100, 0.1 / 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=[32, 64])
def stack(request, dev):
    """150 icons, seed 5: the images, their 100-point integer contours (device; held to the contour oracle by
    tests/test_gpu_icon_contours.py), the device decomposition as host arrays and the polygon oracle's results, computed once."""
    from dgdm_amd import engine
    imgs = icons(150, 5, request.param, request.param)
    pts = engine.icon_contours(torch.from_numpy(imgs), POINTS)
    dec = engine.polygon_decompose(pts)
    pieces = engine.canonical_pieces(dec["piece_count"], dec["piece_offsets"], dec["piece_index"])
    host = {k: v.cpu().numpy() for k, v in dec.items()}
    pts = pts.cpu().numpy()
    return imgs, pts, host, pieces, [po.polygon(p) for p in pts]


def test_icons_against_the_oracle(stack):
    imgs, pts, host, pieces, want = stack
    refused = 0
    for b, w in enumerate(want):
        M = w["count"]
        assert int(host["status"][b]) == w["status"] and int(host["count"][b]) == M and int(host["area2"][b]) == w["area2"], b
        assert host["ring"][b, :M].tolist() == w["ring"] and (host["ring"][b, M:] == -1).all(), b
        T = len(w["triangles"])
        assert [tuple(t) for t in host["triangles"][b, :T].tolist()] == w["triangles"] and (host["triangles"][b, T:] == -1).all(), b
        assert pieces[b] == w["pieces"], b
        if w["status"] == 0:
            assert T == M - 2 and sum(po.tri_area2(pts[b], t) for t in w["triangles"]) == abs(w["area2"])
        refused += w["status"] != 0
    counts = [len(p) for p, w in zip(pieces, want) if w["status"] == 0]
    print(f"{imgs.shape[1]} x {imgs.shape[2]}: {refused} of {len(want)} refused; pieces median {int(np.median(counts))} max {max(counts)}")
    assert refused <= 0.10 * len(want)                      # a condition: the comparison cannot pass by refusing everything


def test_meshes_are_closed_and_exact(stack):
    from dgdm_amd.assets import icon_process
    imgs, pts, host, pieces, want = stack
    worst = 0.0
    for b, w in enumerate(want):
        if w["status"] != 0:
            continue
        M = w["count"]
        (v, f), prisms = icon_process.icon_prisms(pts[b], host["ring"][b, :M], w["area2"], host["triangles"][b, :M - 2], pieces[b], HEIGHT)
        assert v.dtype == np.float32 and v.shape == (2 * M, 3) and f.shape == (4 * M - 4, 3)
        assert np.array_equal(v[:M, :2], (pts[b][w["ring"]] / 128 * 0.1 - 0.05).astype(np.float32)) and np.array_equal(v[:M, :2], v[M:, :2])
        assert (v[:M, 2] == 0).all() and (v[M:, 2] == np.float32(HEIGHT)).all()
        assert (f[:2 * M].max(axis=1) >= M).all() and (f[2 * M:3 * M - 2] >= M).all() and (f[3 * M - 2:] < M).all()   # sides, upper cap, lower cap
        assert fmo.is_closed(f), b
        vol = icon_process.signed_volume(v, f)
        exact = HEIGHT * abs(w["area2"]) / 2 * PIXEL ** 2
        worst = max(worst, abs(vol / exact - 1))
        assert vol > 0 and abs(vol - exact) <= 1e-5 * exact, (b, vol, exact)
        total = 0.0
        for (pv, pf), piece in zip(prisms, pieces[b]):
            k = len(pv) // 2
            assert 3 <= k <= len(piece) and pf.shape == (4 * k - 4, 3)
            assert fmo.is_closed(pf) and fmo.convexity_excess(pv, pf) <= 1e-9, (b, piece)
            total += icon_process.signed_volume(pv, pf)
        assert abs(total - vol) <= 1e-5 * vol, (b, total, vol)
    print(f"largest relative volume error {worst:.2e}")


@pytest.fixture(scope="module")
def eight(stack):
    """Eight icons of the stack with the first refused one among them, and the ids they are exported under."""
    imgs, pts, host, pieces, want = stack
    bad = [b for b, w in enumerate(want) if w["status"] != 0][:1]
    pick = bad + [b for b, w in enumerate(want) if w["status"] == 0][:8 - len(bad)]
    return pick, [1000 + b for b in pick], [1000 + b for b in bad]


def test_model_root_end_to_end(stack, eight, tmp_path):
    from dgdm_amd import engine
    from dgdm_amd.assets import icon_process, save_grippers, save_icon_objects
    from assets.finger_sampler import generate_scene_xml
    imgs, pts, host, pieces, want = stack
    pick, ids, refused = eight
    root = str(tmp_path / "root")
    assert refused, "the stacks hold refused icons (3 and 6 of 150)"
    with pytest.raises(ValueError, match=f"object {refused[0]} cannot be meshed \\(status 3\\)"):
        save_icon_objects(imgs[pick], root, ids, height=HEIGHT, num_points=POINTS)
    assert not os.path.exists(root)                                  # refused before anything is written
    assert save_icon_objects(imgs[pick], root, ids, height=HEIGHT, num_points=POINTS, skip_invalid=True) == refused
    design = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (2, 14, 1)).astype(np.float32)).cuda()
    save_grippers(design, root, first_idx=5)
    for b, idx in zip(pick, ids):
        d = os.path.join(root, "objects", str(idx))
        if idx in refused:
            assert not os.path.exists(d) and not os.path.exists(os.path.join(root, f"object_{idx}.xml"))
            continue
        w = want[b]
        M = w["count"]
        (v, f), prisms = icon_process.icon_prisms(pts[b], host["ring"][b, :M], w["area2"], host["triangles"][b, :M - 2], pieces[b], HEIGHT)
        names = ["object.obj"] + [f"object{k:03d}.obj" for k in range(len(prisms))]
        assert sorted(os.listdir(d)) == sorted(names + ["mesh.json"])
        for name, (mv, mf) in zip(names, [(v, f)] + prisms):
            rv, rf = engine.read_obj(os.path.join(d, name))
            assert np.array_equal(rv.astype(np.float32).view(np.uint32), mv.view(np.uint32)) and np.array_equal(rf, mf), (idx, name)
        info = json.load(open(os.path.join(d, "mesh.json")))
        assert info["M"] == M and info["area2"] == w["area2"] and info["pieces"] == len(prisms)
        assert info["volume"] == icon_process.signed_volume(v, f)
        # the scene over this object and gripper 5: every include exists, every mesh file the included models name exists
        scene = os.path.join(root, f"scene_{idx}_5.xml")
        generate_scene_xml(idx, 5, scene)
        includes = [e.get("file") for e in ET.parse(scene).getroot().iter("include")]
        assert includes == [f"object_{idx}.xml", "gripper_5.xml"]
        for inc in includes:
            meshes = [e.get("file") for e in ET.parse(os.path.join(root, inc)).getroot().iter("mesh")]
            assert len(meshes) >= 2 and all(os.path.isfile(os.path.join(root, m)) for m in meshes), (inc, meshes)
        assert len(list(ET.parse(os.path.join(root, includes[0])).getroot().iter("mesh"))) == 1 + len(prisms)
    # a second call leaves existing directories alone, as prepare_icon_object does
    keep = os.path.join(root, "objects", str(ids[-1]), "object.obj")
    os.remove(os.path.join(root, "objects", str(ids[1]), "object.obj"))
    before = os.stat(keep).st_mtime_ns
    assert save_icon_objects(imgs[pick], root, ids, height=HEIGHT, num_points=POINTS, skip_invalid=True) == refused
    assert os.stat(keep).st_mtime_ns == before and not os.path.exists(os.path.join(root, "objects", str(ids[1]), "object.obj"))


def test_reference_signatures(stack, eight, tmp_path):
    from assets.icon_process import extract_contours, generate_icon_mesh, save_icon_mesh
    from dgdm_amd import engine
    imgs, pts, host, pieces, want = stack
    pick, ids, refused = eight
    b = pick[1]
    mesh, contour = generate_icon_mesh(imgs[b], HEIGHT)
    assert np.array_equal(contour, extract_contours(imgs[b])) and contour.dtype == np.float64
    M = want[b]["count"]
    assert mesh.is_watertight and mesh.vertices.shape == (2 * M, 3) and mesh.faces.shape == (4 * M - 4, 3)
    exact = HEIGHT * abs(want[b]["area2"]) / 2 * PIXEL ** 2
    assert abs(mesh.volume - exact) <= 1e-5 * exact
    c2, path = save_icon_mesh(imgs[b], HEIGHT, POINTS, str(tmp_path / "one"))
    assert path == str(tmp_path / "one" / "object.obj") and np.array_equal(c2, contour)
    rv, rf = engine.read_obj(path)
    assert np.array_equal(rv.astype(np.float32), mesh.vertices.astype(np.float32)) and np.array_equal(rf, mesh.faces)
    with pytest.raises(ValueError, match="status 3"):
        generate_icon_mesh(imgs[pick[0]], HEIGHT)


def _listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_save_objects_flag(dev, tmp_path, capsys):
    """--save_objects as generator/train.py wires it, on an Icons-50-shaped file and one tiny guided run through Diffusion.guided_sample
    (as tests/test_gpu_finger_mesh.py::test_save_meshes_flag drives --save_meshes): with both flags every model root holds every file a
    scene over it names; without --save_objects the run writes the listing it writes today."""
    from dgdm_amd import synth
    from dgdm_amd.generator import train
    from dynamics.parser import parse
    from tests import test_gpu_api as api
    from tests.test_gpu_icon_contours import _icons50
    from assets.finger_sampler import generate_scene_xml
    f = str(tmp_path / "Icons-50.npy")
    _icons50(f, seed=7)
    args = parse(["--save_meshes", "--save_objects", f"--object_dir={f}", "--object_max_num_vertices=100"])
    assert args.save_objects and not parse(["--save_meshes"]).save_objects
    assert train._object_exporter(parse(["--save_objects"])) is None and "nothing to export" in capsys.readouterr().err
    B, G, P, L = 2, 10, 2, 14
    objs, ids = train._objects(args, False)
    d, _ = api._diffusion('point', dev, B, G, P, L, objs[:2])
    d.object_ids = ids[:2]
    noise = synth.synth_noise(0, B, L).to(dev)
    tag = "shift_up_orirange=-1.000_1.000"
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    d.save_meshes = True
    d.guided_sample(0, B, noise, off, opt_obj='shift_up')
    today = _listing(off)
    assert today and not any("object" in p for p in today)
    d.object_exporter = train._object_exporter(args)
    d.guided_sample(0, B, noise, on, opt_obj='shift_up')
    assert [p for p in _listing(on) if "object" not in os.path.basename(p) and os.sep + "objects" + os.sep not in p] == today
    for p in today:
        assert open(os.path.join(off, p), "rb").read() == open(os.path.join(on, p), "rb").read(), p
    from dgdm_amd import engine
    status = engine.polygon_triangulate(engine.icon_contours(torch.from_numpy(icons(len(ids), 7)), 100))[0].tolist()
    assert status[:2] == [0, 0]
    for i, idx in enumerate(ids[:2]):
        root = os.path.join(on, "vis_guided", tag, str(idx))
        if status[i] != 0:
            assert not os.path.exists(os.path.join(root, f"object_{idx}.xml"))
            continue
        scene = os.path.join(root, "scene.xml")
        generate_scene_xml(idx, 1, scene)
        for inc in [e.get("file") for e in ET.parse(scene).getroot().iter("include")]:
            meshes = [e.get("file") for e in ET.parse(os.path.join(root, inc)).getroot().iter("mesh")]
            assert meshes and all(os.path.isfile(os.path.join(root, m)) for m in meshes), (inc, meshes)
