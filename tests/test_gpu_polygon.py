"""Triangulation and convex pieces of integer rings on the GPU (csrc/polygon.hip, engine.polygon_*) against the CPU oracle of the contract
(tests/polygon_oracle.py; include/dgdm_hip.h "integer rings"): statuses, rings, areas, triangles and canonical pieces,
index for index, on hand-made rings, at the sizes where a lane takes more than one candidate, and in any batch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import polygon_oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def padded(rings, n=None):
    """Rings of different lengths as one (batch, n, 2) int32 array: a ring is padded by repeating its last point (cleaned away)."""
    n = n or max(len(r) for r in rings)
    return np.array([list(r) + [r[-1]] * (n - len(r)) for r in rings], dtype=np.int32)


def run(points):
    """The device results of a (batch, n, 2) array as a list of dicts shaped like the oracle's."""
    from dgdm_amd import engine
    o = engine.polygon_decompose(torch.from_numpy(np.ascontiguousarray(points)))
    pieces = engine.canonical_pieces(o["piece_count"], o["piece_offsets"], o["piece_index"])
    h = {k: v.cpu().numpy() for k, v in o.items()}
    out = []
    for b in range(len(points)):
        M = int(h["count"][b])
        T = M - 2 if h["status"][b] == 0 else 0
        assert (h["ring"][b, M:] == -1).all() and (h["triangles"][b, T:] == -1).all()
        assert int(h["piece_count"][b]) == len(pieces[b]) and (h["piece_offsets"][b, len(pieces[b]) + 1 if pieces[b] else 0:] == -1).all()
        assert (h["piece_index"][b, sum(len(p) for p in pieces[b]):] == -1).all()
        out.append({"status": int(h["status"][b]), "count": M, "ring": h["ring"][b, :M].tolist(), "area2": int(h["area2"][b]),
                    "triangles": [tuple(t) for t in h["triangles"][b, :T].tolist()], "pieces": pieces[b]})
    return out


def check(rings, n=None):
    pts = padded(rings, n)
    got = run(pts)
    want = [po.polygon(p) for p in pts]
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, (b, {k: (g[k], w[k]) for k in g if g[k] != w[k]})
    return got, pts


def test_hand_made_rings(dev):
    names = sorted(po.VALID)
    got, _ = check([po.VALID[k] for k in names])
    r = dict(zip(names, got))
    assert all(v["status"] == 0 for v in got)
    assert r["triangle"]["triangles"] == [(2, 0, 1)] and r["triangle"]["pieces"] == [(0, 1, 2)]
    assert r["square_ccw"]["area2"] == 32 and r["square_cw"]["area2"] == -32
    assert r["square_ccw"]["pieces"] == [(0, 1, 2, 3)] and r["square_cw"]["pieces"] == [(0, 3, 2, 1)]
    assert r["square_doubled"]["ring"] == [0, 2, 4, 6] and r["square_doubled"]["count"] == 4
    assert r["dart"]["triangles"] == [(3, 0, 1), (3, 1, 2)] and len(r["dart"]["pieces"]) == 2
    assert r["rect_midpoints"]["pieces"] == [tuple(range(8))]                       # collinear points kept, every diagonal removed
    assert r["comb"]["count"] == 20 and len(r["comb"]["triangles"]) == 18


@pytest.mark.parametrize("name", sorted(po.VALID))
def test_each_ring_at_its_own_length(dev, name):
    """n = the ring's own length (3 for the triangle, 9 for the doubled square): no padding."""
    check([po.VALID[name]])


def test_refused_rings(dev):
    """All points equal (1), collinear points (2), a bow-tie and a spike A-B-A-C (3), a vertex on another edge (3).  The statuses apply
    in order, so the bow-tie is one with area and the spike sits on a rectangle; the bare four-point spike encloses nothing and is 2."""
    names = sorted(po.REFUSED)
    got, _ = check([po.REFUSED[k][0] for k in names])
    for k, g in zip(names, got):
        assert g["status"] == po.REFUSED[k][1] and g["triangles"] == [] and g["pieces"] == [], k
    assert dict(zip(names, got))["all_equal"]["count"] == 1


@pytest.mark.parametrize("n", [64, 65, 256])
def test_size_edges(dev, n):
    """64: one candidate a lane; 65: the second ballot holds one; 256: four.  A convex ring, a star (every other vertex reflex) and both
    given clockwise - the reversed working order takes the highest set bit of the last ballot."""
    rings = [po.round_ring(n), po.round_ring(n, 16000, 9000) if n % 2 == 0 else po.round_ring(n, 16000, 15000)]
    rings += [r[::-1] for r in rings]
    got, pts = check(rings)
    for g, p in zip(got, pts):
        assert g["status"] == 0 and g["count"] == n
        assert sum(po.tri_area2(p, t) for t in g["triangles"]) == abs(g["area2"])
    assert got[0]["pieces"] == [tuple(range(n))]


def test_batch_invariance(dev):
    """Valid and refused rings mixed: each ring alone, the batch and the batch reversed agree bit for bit."""
    from dgdm_amd import engine
    rings = [po.VALID[k] for k in sorted(po.VALID)] + [po.REFUSED[k][0] for k in sorted(po.REFUSED)] + [po.round_ring(70, 9000, 5000, 9000)]
    rings = [rings[i] for i in np.random.RandomState(0).permutation(len(rings))]
    pts = torch.from_numpy(padded(rings, 70))
    keys = ("status", "count", "ring", "area2", "triangles", "piece_count", "piece_offsets", "piece_index")
    batch = {k: v.cpu() for k, v in engine.polygon_decompose(pts).items()}
    back = {k: v.cpu() for k, v in engine.polygon_decompose(pts.flip(0)).items()}
    st = batch["status"].tolist()
    assert 0 in st and 1 in st and 2 in st and 3 in st
    for k in keys:
        assert torch.equal(back[k].flip(0), batch[k]), k
    for b in range(len(rings)):
        alone = engine.polygon_decompose(pts[b:b + 1])
        for k in keys:
            assert torch.equal(alone[k].cpu()[0], batch[k][b]), (b, k)
    s, c, r, a, t = engine.polygon_triangulate(pts)
    for k, v in zip(keys, (s, c, r, a, t)):
        assert torch.equal(v.cpu(), batch[k]), k
    assert engine.polygon_pieces(pts) == engine.canonical_pieces(batch["piece_count"], batch["piece_offsets"], batch["piece_index"])


def test_bad_arguments_are_einval(dev):
    from dgdm_amd import _lib, engine
    sq = np.array([po.SQUARE], dtype=np.int32)
    with pytest.raises(ValueError, match="2 points per ring"):
        engine.polygon_triangulate(sq[:, :2])
    with pytest.raises(ValueError, match="257 points per ring"):
        engine.polygon_pieces(np.zeros((1, 257, 2), dtype=np.int32))
    for bad in (32768, -1):
        p = sq.copy()
        p[0, 2, 1] = bad
        with pytest.raises(ValueError, match="coordinate outside"):
            engine.polygon_triangulate(p)
        with pytest.raises(ValueError, match="coordinate outside"):
            engine.polygon_pieces(np.concatenate([sq, p]))
    with pytest.raises(ValueError, match="coordinate outside"):
        engine.polygon_triangulate(sq.astype(np.int64) + 2 ** 32)
    with pytest.raises(ValueError, match="integer points"):
        engine.polygon_triangulate(sq.astype(np.float32))
    with pytest.raises(ValueError, match="shape"):
        engine.polygon_triangulate(sq[0])
    # the C entry points themselves: checked before anything is launched on the rings
    lib = _lib.lib()
    d = torch.from_numpy(sq).to(dev)
    out = torch.empty(64, dtype=torch.int64, device=dev)
    p, o = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
    assert lib.dgdm_polygon_triangulate(p, 1, 2, o, o, o, o, o, None) == _lib.EINVAL
    assert lib.dgdm_polygon_triangulate(p, 1, 257, o, o, o, o, o, None) == _lib.EINVAL
    assert lib.dgdm_polygon_triangulate(p, 0, 4, o, o, o, o, o, None) == _lib.EINVAL
    assert lib.dgdm_polygon_triangulate(p, 1, 4, o, None, o, o, o, None) == _lib.EINVAL
    assert lib.dgdm_polygon_convex_pieces(p, 1, 4, o, None, None, None, None, None, o, o, None) == _lib.EINVAL
    # and the stream is usable afterwards; count / ring / area2 / triangles are optional for the pieces
    st, pc = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    po_, pi = torch.empty(3, dtype=torch.int32, device=dev), torch.empty(6, dtype=torch.int32, device=dev)
    q = [C.c_void_p(t.data_ptr()) for t in (st, pc, po_, pi)]
    assert lib.dgdm_polygon_convex_pieces(p, 1, 4, q[0], None, None, None, None, q[1], q[2], q[3], None) == 0
    torch.cuda.synchronize()
    assert st.item() == 0 and pc.item() == 1 and po_.tolist() == [0, 4, -1] and pi.tolist() == [3, 0, 1, 2, -1, -1]         # from its lowest half-edge
