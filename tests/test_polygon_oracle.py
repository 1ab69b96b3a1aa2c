"""The CPU oracle of the ring contract (tests/polygon_oracle.py; include/dgdm_hip.h "integer rings") against the
invariants every triangulation and every convex decomposition of a simple ring has, on hand-made rings."""
from collections import Counter

import pytest

from tests import polygon_oracle as po

RINGS = dict(po.VALID, round_64=po.round_ring(64), round_65=po.round_ring(65), star_256=po.round_ring(256, 16000, 9000),
             star_256_cw=po.round_ring(256, 16000, 9000)[::-1])


@pytest.fixture(scope="module")
def results():
    return {k: po.polygon(v) for k, v in RINGS.items()}


def test_cleaning():
    assert po.clean(po.VALID["square_doubled"]) == [0, 2, 4, 6]
    assert po.clean([(1, 1), (1, 1), (2, 2), (1, 1), (1, 1)]) == [0, 2]
    assert po.clean([(5, 5)] * 4) == [0]
    assert po.clean(po.VALID["rect_midpoints"]) == list(range(8))                 # collinear points stay


@pytest.mark.parametrize("name", sorted(po.REFUSED))
def test_refused_rings(name):
    pts, status = po.REFUSED[name]
    r = po.polygon(pts)
    assert r["status"] == status and r["triangles"] == [] and r["pieces"] == []
    assert r["count"] == len(po.clean(pts))


def test_status_values():
    r = po.polygon(po.VALID["square_cw"])
    assert r["status"] == 0 and r["area2"] == -32 and po.polygon(po.VALID["square_ccw"])["area2"] == 32
    assert po.polygon(po.VALID["square_doubled"])["ring"] == [0, 2, 4, 6]
    assert po.polygon(po.VALID["dart"])["triangles"] == [(3, 0, 1), (3, 1, 2)]     # tip 0 first; of the last three, 1 is named as tip


@pytest.mark.parametrize("name", sorted(RINGS))
def test_triangulation_invariants(results, name):
    pts, r = RINGS[name], results[name]
    M, tris = r["count"], r["triangles"]
    assert r["status"] == 0 and len(tris) == M - 2
    areas = [po.tri_area2(pts, t) for t in tris]
    assert all(a > 0 for a in areas) and sum(areas) == abs(r["area2"])            # counter-clockwise in the working order, exactly
    # every input edge once as a directed triangle edge (in the working direction), every diagonal once in each direction
    ring = r["ring"] if r["area2"] > 0 else r["ring"][::-1]
    boundary = {(ring[k], ring[(k + 1) % M]) for k in range(M)}
    edges = Counter(e for t in tris for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])))
    assert all(c == 1 for c in edges.values())
    assert boundary <= set(edges)
    inner = set(edges) - boundary
    assert len(inner) == 2 * (M - 3) and all((b, a) in inner for a, b in inner)
    assert not any((b, a) in edges for a, b in boundary)


@pytest.mark.parametrize("name", sorted(RINGS))
def test_piece_invariants(results, name):
    pts, r = RINGS[name], results[name]
    pieces = r["pieces"]
    assert 1 <= len(pieces) <= r["count"] - 2
    assert all(po.piece_is_convex(pts, p) for p in pieces)
    assert sum(po.piece_area2(pts, p) for p in pieces) == abs(r["area2"])
    assert all(p[0] == min(p) for p in pieces) and pieces == sorted(pieces)
    assert set(v for p in pieces for v in p) == set(r["ring"])
    edges = Counter((p[k], p[(k + 1) % len(p)]) for p in pieces for k in range(len(p)))
    assert all(c == 1 for c in edges.values())


def test_known_pieces():
    assert po.polygon(po.VALID["square_ccw"])["pieces"] == [(0, 1, 2, 3)]
    assert po.polygon(po.VALID["square_cw"])["pieces"] == [(0, 3, 2, 1)]
    assert po.polygon(po.VALID["rect_midpoints"])["pieces"] == [tuple(range(8))]
    assert len(po.polygon(po.VALID["dart"])["pieces"]) == 2
    assert po.polygon(po.round_ring(64))["pieces"] == [tuple(range(64))]
    assert len(po.polygon(po.VALID["l_shape"])["pieces"]) == 2
