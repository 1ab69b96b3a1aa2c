"""CPU tests of the OBJ reader behind dynamics/utils.py (csrc/mesh.hip, host code) and of the float64 oracle of the mesh sampling contract
(DESIGN.md "Object clouds from meshes"), which tests/test_gpu_mesh_sample.py holds the device sampler to."""
import ctypes as C

import numpy as np
import pytest

from dgdm_amd import _lib


# ---------------------------------------------------------------------------------------------------------------- the oracle
def oracle_areas(verts, tris):
    v = np.asarray(verts, dtype=np.float64)
    t = np.asarray(tris, dtype=np.int64)
    cr = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    return 0.5 * np.sqrt((cr * cr).sum(axis=1))


def oracle_counts(verts, tris, n):
    """(areas, A, cdf, n_t): A as a sequential sum, cdf as a sequential running sum of a / A, n_t = floor(cdf * N + 0.5)."""
    a = oracle_areas(verts, tris)
    A = float(np.cumsum(a)[-1])
    cdf = np.cumsum(a / A)
    return a, A, cdf, np.floor(cdf * n + 0.5).astype(np.int64)


def oracle_uniforms(seed, key, n):
    """r1, r2 of points 0 .. n-1: raw outputs 2p, 2p + 1 of numpy's Philox4x64-10 under key (seed, key), (u >> 11) * 2^-53."""
    raw = np.random.Philox(key=[seed, key]).random_raw(2 * n)
    u = (raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u[0::2], u[1::2]


def oracle_sample(verts, tris, n, key, seed=0):
    """(points (n, 3) float64, owner triangle of each point, cdf * N per triangle)."""
    v = np.asarray(verts, dtype=np.float64)
    t = np.asarray(tris, dtype=np.int64)
    _, _, cdf, counts = oracle_counts(v, t, n)
    owner = np.searchsorted(counts, np.arange(n), side='right')
    r1, r2 = oracle_uniforms(seed, key, n)
    s = np.sqrt(r1)
    a, b, c = 1.0 - s, s * (1.0 - r2), s * r2
    tt = t[owner]
    pts = a[:, None] * v[tt[:, 0]] + b[:, None] * v[tt[:, 1]] + c[:, None] * v[tt[:, 2]]
    return pts, owner, cdf * n


def box_mesh(lo=(0.0, 0.0, 0.0), hi=(1.0, 2.0, 3.0)):
    """The 8 corners and 12 outward triangles of an axis-aligned box."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = np.array([tri for q in quads for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int32)
    return v, t


def test_oracle_counts_on_a_box():
    v, t = box_mesh()
    a, A, cdf, n = oracle_counts(v, t, 100)
    # faces 1 x 2 (z), 1 x 2 (z), 1 x 3 (y), 1 x 3 (y), 2 x 3 (x), 2 x 3 (x): each split in two halves
    face = [2.0, 2.0, 3.0, 3.0, 6.0, 6.0]
    assert np.allclose(a, np.repeat(face, 2) / 2) and A == pytest.approx(22.0)
    want = np.floor(np.cumsum(np.repeat(face, 2) / 2 / 22.0) * 100 + 0.5)
    assert list(n) == list(want.astype(np.int64)) == [5, 9, 14, 18, 25, 32, 39, 45, 59, 73, 86, 100]
    assert n[-1] == 100 and np.all(np.diff(n) >= 0)
    pts, owner, _ = oracle_sample(v, t, 100, 7)
    assert pts.shape == (100, 3) and list(np.bincount(owner, minlength=12)) == list(np.diff(np.concatenate([[0], n])))


def test_oracle_philox_known_answer():
    # Random123's known answer for Philox4x64-10, key 0, counter 0; numpy's first block uses counter 1
    g = np.random.Philox(counter=[2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1], key=[0, 0])
    assert [hex(x) for x in g.random_raw(2)] == ["0x16554d9eca36314c", "0xdb20fe9d672d0fdc"]


# ---------------------------------------------------------------------------------------------------------------- the reader
@pytest.fixture(scope="module")
def lib():
    from dgdm_amd import build
    build.build()
    return _lib.lib()


def read(lib, path):
    from dgdm_amd import engine
    return engine.read_obj(str(path))


def write(tmp_path, text, name="m.obj", newline="\n"):
    p = tmp_path / name
    p.write_bytes(text.replace("\n", newline).encode())
    return p


def test_reader_triangles_quads_and_token_forms(lib, tmp_path):
    p = write(tmp_path, """# a comment
mtllib m.mtl
o thing
v 0 0 0
v 1 0 0 1.0
v 1 1 0 0.5 0.5 0.5
v 0 1 0
vt 0 0
vt 1 0
vn 0 0 1
g group
usemtl red
s 1
f 1 2 3
f 1/1 3/2 4/1
f 1//1 2//1 4//1
f 2/1/1 3/2/1 4/1/1

f -4 -3 -2 -1
l 1 2
""")
    v, t = read(lib, p)
    assert v.dtype == np.float64 and t.dtype == np.int32
    assert np.array_equal(v, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    assert t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3], [0, 1, 2], [0, 2, 3]]


def test_reader_polygon_fan_crlf_and_groups_in_file_order(lib, tmp_path):
    body = """o first
v 0 0 0
v 2 0 0
v 2 2 0
v 1 3 0
v 0 2 0
f 1 2 3 4 5
o second
g part
v 5 5 5
v 6 5 5
v 6 6 5
f -3 -2 -1 # a trailing comment
f 6 7 8
"""
    for nl in ("\n", "\r\n"):
        v, t = read(lib, write(tmp_path, body, newline=nl))
        assert v.shape == (8, 3) and v[5].tolist() == [5, 5, 5]
        assert t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4], [5, 6, 7], [5, 6, 7]]


def test_reader_forward_reference(lib, tmp_path):
    v, t = read(lib, write(tmp_path, "f 1 2 3\nv 0 0 0\nv 1 0 0\nv 0 1 0\n"))
    assert t.tolist() == [[0, 1, 2]] and v.shape == (3, 3)


@pytest.mark.parametrize("text, line, reason", [
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", 4, "index 0"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 4, "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\n\nf 1 2 -4\n", 5, "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", 4, "fewer than 3 vertices"),
    ("v 0 0 0\nv 1 zero 0\nv 0 1 0\nf 1 2 3\n", 2, "unparsable number"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x/1\n", 4, "unparsable number"),
    ("v 0 0 0\nv 1 0\n", 2, "fewer than 3 coordinates"),
    ("# nothing\nv 0 0 0\nv 1 0 0\nv 0 1 0\n", 4, "no faces"),
])
def test_reader_errors(lib, tmp_path, text, line, reason):
    p = write(tmp_path, text, name="bad.obj")
    h = C.c_void_p()
    rc = lib.dgdm_mesh_read_obj(str(p).encode(), C.byref(h))
    assert rc == _lib.EINVAL and not h.value
    msg = lib.dgdm_last_error().decode()
    assert msg.startswith(f"{p}:{line}: ") and reason in msg, msg
    with pytest.raises(_lib.DgdmError, match=f"{p}:{line}: "):
        read(lib, p)


def test_reader_missing_file(lib, tmp_path):
    with pytest.raises(_lib.DgdmError, match="cannot open"):
        read(lib, tmp_path / "none.obj")
