"""CPU tests of the finger-mesh export (csrc/finger_mesh.hip host code, dgdm_amd/assets/gripper_xml.py): the triangle tables against the
numpy oracle, closedness and orientation consistency, the XML writers against the files recorded from the reference, the OBJ round trip
and the argument checks.  tests/test_gpu_finger_mesh.py holds the device side to the same oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from dgdm_amd import _lib, engine
from dgdm_amd.assets import finger_3d, finger_sampler
from tests import finger_mesh_oracle as fmo

TABLES = [(2, 2), (2, 3), (2, 200), (3, 2), (3, 3), (3, 25), (12, 0), (13, 0)]


@pytest.mark.parametrize("kind,n", TABLES)
def test_faces_match_the_oracle(kind, n):
    got, want = engine.finger_mesh_faces(kind, n), fmo.oracle_faces(kind, n)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    if kind == 2:
        assert len(got) == 2 * (4 * (n - 1) + 2) and got.max() == 4 * n - 1
    if kind == 3:
        assert len(got) == 4 * (n - 1) ** 2 + 8 * (n - 1) and got.max() == 2 * n * n - 1


@pytest.mark.parametrize("kind,n", TABLES)
def test_faces_are_closed_and_consistently_oriented(kind, n):
    """Every directed edge exactly once, its reverse exactly once."""
    f = engine.finger_mesh_faces(kind, n)
    assert fmo.is_closed(f)
    assert not fmo.is_closed(f[:-1])                                  # the check sees a hole ...
    g = f.copy()
    g[0] = g[0, ::-1]
    assert not fmo.is_closed(g)                                       # ... and one flipped triangle


def test_faces_are_outward_on_a_straight_finger():
    """Orientation rule of the header on the simplest solids: positive signed volume, the box's own."""
    n, w, h = 3, 0.03, 0.02
    x = np.linspace(-0.12, 0.12, n)
    ring = np.stack([x, np.zeros(n), np.zeros(n)], -1)
    v2 = np.concatenate([ring, ring + [0, w, 0], ring + [0, w, h], ring + [0, 0, h]])
    assert fmo.volume_area(v2, engine.finger_mesh_faces(2, n))[0] == pytest.approx(0.24 * w * h, rel=1e-12)
    xs, zs = np.meshgrid(x, np.linspace(0, 0.12, n), indexing="ij")
    sheet = np.stack([xs.reshape(-1), np.zeros(n * n), zs.reshape(-1)], -1)
    v3 = np.concatenate([sheet, sheet + [0, w, 0]])
    assert fmo.volume_area(v3, engine.finger_mesh_faces(3, n))[0] == pytest.approx(0.24 * 0.12 * w, rel=1e-12)
    assert fmo.convexity_excess(v2[[0, 3, 6, 9, 1, 4, 7, 10]], engine.finger_mesh_faces(12)) <= 1e-12
    assert fmo.convexity_excess(v3[[0, 3, 4, 9, 12, 13]], engine.finger_mesh_faces(13)) <= 1e-12


WRITERS = {
    "gripper_2d": finger_sampler.generate_xml,
    "gripper_2d_optimized": finger_sampler.generate_xml_optimized,
    "gripper_3d": finger_3d.generate_gripper_3d_xml,
}


@pytest.mark.parametrize("counts", [(0, 0), (3, 5), (16, 16)])
@pytest.mark.parametrize("name", sorted(WRITERS))
def test_gripper_xml_matches_the_reference_files(name, counts, golden_dir, tmp_path):
    """tag, attribute dict and child order of every element; (3, 5) tells left from right."""
    out = str(tmp_path / "g.xml")
    WRITERS[name](counts[0], counts[1], 7, out)
    assert fmo.xml_tree(out) == fmo.xml_tree(os.path.join(golden_dir, "gripper_xml", f"{name}_{counts[0]}_{counts[1]}.xml"))


@pytest.mark.parametrize("name,fn", [("scene_2d", finger_sampler.generate_scene_xml), ("scene_3d", finger_3d.generate_scene_3d_xml)])
def test_scene_xml_matches_the_reference_files(name, fn, golden_dir, tmp_path):
    out = str(tmp_path / "s.xml")
    fn(4, 7, out)
    assert fmo.xml_tree(out) == fmo.xml_tree(os.path.join(golden_dir, "gripper_xml", name + ".xml"))


def test_mesh_and_geom_elements():
    m = finger_sampler.create_mesh_elements(2, "fingerr", 11)
    assert [(e.tag, dict(e.attrib)) for e in m] == [("mesh", {"name": "fingerr000", "file": "grippers/11/fingerr000.obj"}),
                                                    ("mesh", {"name": "fingerr001", "file": "grippers/11/fingerr001.obj"})]
    g = finger_3d.create_geom_elements(1, "fingerl")
    assert [(e.tag, dict(e.attrib)) for e in g] == [("geom", {"mesh": "fingerl000", "type": "mesh", "class": "collision"})]


def test_obj_round_trip_is_bit_exact(tmp_path):
    tiny = np.float32(1e-45)                                           # the smallest subnormal
    assert tiny > 0 and tiny < np.finfo(np.float32).tiny
    v = np.array([[1 / 3, -0.12, tiny], [1e-9, 0.0, -1 / 3], [np.float32(0.1) + np.float32(0.03), 3.4e38, -tiny], [16777217.0, -1e-9, 0.02]],
                 dtype=np.float32)
    t = np.array([[0, 1, 2], [3, 2, 1], [0, 3, 1]], dtype=np.int32)
    path = str(tmp_path / "m.obj")
    engine.write_obj(path, v, t)
    rv, rt = engine.read_obj(path)
    assert rv.dtype == np.float64 and np.array_equal(rv.astype(np.float32).view(np.uint32), v.view(np.uint32))
    assert np.array_equal(rt, t)
    lines = open(path).read().splitlines()
    assert len(lines) == 7 and lines[4] == "f 1 2 3" and lines[0].startswith("v 0.333333343 -0.119999997 ")
    with pytest.raises(ValueError, match="refers to vertex 4"):
        engine.write_obj(path, v, np.array([[0, 1, 4]]))
    with pytest.raises(ValueError, match="cannot open"):
        engine.write_obj(str(tmp_path / "missing" / "m.obj"), v, t)


def _einval(rc, match):
    assert rc == _lib.EINVAL
    assert match in _lib.lib().dgdm_last_error().decode()


def test_argument_checks_return_einval_with_a_message():
    """Checked before anything touches a device: the pointers are never followed."""
    lib = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    nv, nt = C.c_int64(), C.c_int64()
    _einval(lib.dgdm_finger_mesh_counts(2, 1, C.byref(nv), C.byref(nt)), "resolution 1")
    _einval(lib.dgdm_finger_mesh_counts(3, 1, C.byref(nv), C.byref(nt)), "resolution 1")
    _einval(lib.dgdm_finger_mesh_counts(4, 5, C.byref(nv), C.byref(nt)), "kind 4")
    _einval(lib.dgdm_finger_mesh_vertices_2d(p, 1, 14, 1, 0.03, -0.015, 0.03, 0.02, p, None), "1 points")
    _einval(lib.dgdm_finger_mesh_vertices_2d(p, 1, 6, 200, 0.03, -0.015, 0.03, 0.02, p, None), "6 control values")
    _einval(lib.dgdm_finger_mesh_vertices_2d(p, 1, 14, 200, 0.03, -0.015, 0.0, 0.02, p, None), "width 0")
    _einval(lib.dgdm_finger_mesh_vertices_3d(p, 1, 42, 1, 0.05, -0.05, 0.1, p, None), "sample_size 1")
    _einval(lib.dgdm_finger_mesh_vertices_3d(p, 1, 6, 25, 0.05, -0.05, 0.1, p, None), "6 control values")
    _einval(lib.dgdm_finger_pieces_2d(p, 1, 5, 5, p, p, None), "5 pieces over 4 segments")
    _einval(lib.dgdm_finger_pieces_2d(p, 1, 1, 1, p, p, None), "1 points")
    _einval(lib.dgdm_finger_pieces_2d(p, 1, 2000, 1001, p, p, None), "at most 1000")
    _einval(lib.dgdm_finger_pieces_3d(p, 1, 4, 4, 1, p, p, None), "4 x 1 knot cells over 3 x 3")
    _einval(lib.dgdm_finger_pieces_3d(p, 1, 1, 1, 1, p, p, None), "sample_size 1")
    _einval(lib.dgdm_finger_pieces_3d(p, 1, 25, 24, 24, p, p, None), "at most 1000")
    _einval(lib.dgdm_finger_mesh_stats(p, p, 1, 2, 1, 0.0, p, None), "2 vertices")
    with pytest.raises(ValueError, match="resolution 1"):
        engine.finger_mesh_faces(2, 1)


def test_knots_cover_the_samples():
    for n, p in ((2, 1), (5, 2), (5, 4), (200, 16), (200, 199), (25, 8), (25, 2)):
        k = fmo.knots(n, p)
        assert k[0] == 0 and k[-1] == n - 1 and (np.diff(k) >= 1).all()
