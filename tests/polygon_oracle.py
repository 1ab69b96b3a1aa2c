"""CPU oracle of the polygon contract (include/dgdm_hip.h "integer rings"): cleaning, status, ear clipping with the
fixed rule and the Hertel-Mehlhorn convex pieces of one closed ring of integer points, in plain Python and numpy int64 - no float
decides anything.  Test infrastructure only: tests/test_polygon_oracle.py checks its invariants on hand-made rings,
tests/test_gpu_polygon.py and tests/test_gpu_icon_objects.py hold csrc/polygon.hip to it index for index."""
import numpy as np

OK, TOO_FEW, NO_AREA, NOT_SIMPLE, NO_EAR = 0, 1, 2, 3, 4


def cross(a, b, c):
    """(b - a) x (c - a) of int64 arrays (..., 2) or int pairs."""
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])


def clean(points):
    """ring: the original indices kept - a point equal to the one kept before it is dropped, then trailing points equal to the first."""
    p = [(int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2).tolist()]
    ring = [0]
    for i in range(1, len(p)):
        if p[i] != p[ring[-1]]:
            ring.append(i)
    while len(ring) > 1 and p[ring[-1]] == p[ring[0]]:
        ring.pop()
    return ring


def area2(P):
    """The doubled signed area of the closed ring P (M, 2) int64, as a Python int."""
    Q = np.roll(P, -1, axis=0)
    return int((P[:, 0] * Q[:, 1] - Q[:, 0] * P[:, 1]).sum())


def _on_segment(a, b, c):
    """c, known to be collinear with a b, lies on the closed segment."""
    return ((np.minimum(a[..., 0], b[..., 0]) <= c[..., 0]) & (c[..., 0] <= np.maximum(a[..., 0], b[..., 0])) &
            (np.minimum(a[..., 1], b[..., 1]) <= c[..., 1]) & (c[..., 1] <= np.maximum(a[..., 1], b[..., 1])))


def segments_touch(a, b, c, d):
    """The closed segments a b and c d share a point (arrays of segments)."""
    d1, d2, d3, d4 = cross(c, d, a), cross(c, d, b), cross(a, b, c), cross(a, b, d)
    proper = (((d1 > 0) & (d2 < 0)) | ((d1 < 0) & (d2 > 0))) & (((d3 > 0) & (d4 < 0)) | ((d3 < 0) & (d4 > 0)))
    return (proper | ((d1 == 0) & _on_segment(c, d, a)) | ((d2 == 0) & _on_segment(c, d, b)) |
            ((d3 == 0) & _on_segment(a, b, c)) | ((d4 == 0) & _on_segment(a, b, d)))


def is_simple(P):
    """No two non-adjacent closed edges share a point and no two adjacent edges fold back on each other."""
    M = len(P)
    Q = np.roll(P, -1, axis=0)                                   # edge k: P[k] -> Q[k]
    R = np.roll(P, -2, axis=0)
    u, v = Q - P, R - Q
    fold = (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0] == 0) & (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] < 0)
    if fold.any():
        return False
    e, f = np.triu_indices(M, 2)
    keep = ~((e == 0) & (f == M - 1))
    e, f = e[keep], f[keep]
    return not segments_touch(P[e], Q[e], P[f], Q[f]).any()


def ear_clip(W, oid):
    """W (M, 2) int64 in the counter-clockwise working order, oid their original indices -> (triangles as working positions in clip
    order, or None when no ear is found)."""
    cur = list(range(len(W)))
    tris = []
    while len(cur) > 3:
        c = np.array(cur)
        A, B, C = W[np.roll(c, 1)], W[c], W[np.roll(c, -1)]
        convex = cross(A, B, C) > 0
        V = W[c][None, :, :]
        inside = (cross(A[:, None], B[:, None], V) >= 0) & (cross(B[:, None], C[:, None], V) >= 0) & (cross(C[:, None], A[:, None], V) >= 0)
        m = len(c)
        k = np.arange(m)
        own = (k[None, :] == k[:, None]) | (k[None, :] == (k[:, None] - 1) % m) | (k[None, :] == (k[:, None] + 1) % m)
        ear = convex & ~(inside & ~own).any(axis=1)
        if not ear.any():
            return None
        cand = np.nonzero(ear)[0]
        t = int(cand[np.argmin(oid[c[cand]])])
        tris.append((cur[t - 1], cur[t], cur[(t + 1) % m]))
        del cur[t]
    t = int(np.argmin(oid[np.array(cur)]))
    tris.append((cur[t - 1], cur[t], cur[(t + 1) % 3]))
    return tris


def hertel_mehlhorn(W, tris):
    """The faces left after removing, in reverse order of creation, every diagonal at whose two end points the boundary edges that
    become neighbours turn left or go straight.  tris: ear_clip's; triangle t < M - 3 created the diagonal between its first and last
    vertex.  Faces are lists of working positions, counter-clockwise, in order of their lowest half-edge."""
    T = len(tris)
    org = [v for t in tris for v in t]                           # half-edge 3 t + k leaves vertex k of triangle t
    nxt = [3 * (h // 3) + (h + 1) % 3 for h in range(3 * T)]
    prv = [3 * (h // 3) + (h + 2) % 3 for h in range(3 * T)]
    twin = {}
    where = {}                                                   # directed edge -> half-edge
    for h in range(3 * T):
        where[(org[h], org[nxt[h]])] = h
    for t in range(T - 1):
        h = 3 * t + 2                                            # l -> i of triangle t; i -> l lies in a later triangle
        twin[h] = where[(org[nxt[h]], org[h])]
    removed = [False] * (3 * T)

    def turn(a, b, c):
        return int(cross(W[a], W[b], W[c]))
    for t in range(T - 2, -1, -1):
        h = 3 * t + 2
        g = twin[h]
        at_i = turn(org[prv[g]], org[g], org[nxt[nxt[h]]])
        at_l = turn(org[prv[h]], org[h], org[nxt[nxt[g]]])
        if at_i >= 0 and at_l >= 0:
            a, b, c, d = prv[g], nxt[h], prv[h], nxt[g]
            nxt[a], prv[b], nxt[c], prv[d] = b, a, d, c
            removed[h] = removed[g] = True
    faces, seen = [], list(removed)
    for h in range(3 * T):
        if not seen[h]:
            face, e = [], h
            while not seen[e]:
                seen[e] = True
                face.append(org[e])
                e = nxt[e]
            faces.append(face)
    return faces


def canonical(pieces):
    """Each piece rotated to start at its smallest index, the pieces sorted."""
    out = []
    for p in pieces:
        k = p.index(min(p))
        out.append(tuple(p[k:] + p[:k]))
    return sorted(out)


def polygon(points):
    """One ring (n, 2) of integers -> dict(status, count, ring, area2, triangles, pieces): ring the original indices kept, triangles
    (M - 2) tuples of original indices in clip order, pieces canonical tuples of original indices.  status != 0: no triangles or pieces;
    area2 is 0 for status 1.  The first status that applies is reported."""
    pts = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    ring = clean(pts)
    M = len(ring)
    out = {"status": OK, "count": M, "ring": ring, "area2": 0, "triangles": [], "pieces": []}
    if M < 3:
        out["status"] = TOO_FEW
        return out
    P = pts[ring]
    a2 = out["area2"] = area2(P)
    if a2 == 0:
        out["status"] = NO_AREA
        return out
    if not is_simple(P):
        out["status"] = NOT_SIMPLE
        return out
    oid = np.array(ring, dtype=np.int64)
    if a2 < 0:
        P, oid = P[::-1], oid[::-1]
    tris = ear_clip(P, oid)
    if tris is None:
        out["status"] = NO_EAR
        return out
    out["triangles"] = [tuple(int(oid[v]) for v in t) for t in tris]
    out["pieces"] = canonical([[int(oid[v]) for v in f] for f in hertel_mehlhorn(P, tris)])
    return out


# ------------------------------------------------------------------------------------------------------------------ checks the tests share
def tri_area2(pts, tri):
    p = np.asarray(pts, dtype=np.int64)
    return int(cross(p[tri[0]], p[tri[1]], p[tri[2]]))


def piece_area2(pts, piece):
    return area2(np.asarray(pts, dtype=np.int64)[list(piece)])


def piece_is_convex(pts, piece):
    p = np.asarray(pts, dtype=np.int64)[list(piece)]
    return bool((cross(np.roll(p, 1, axis=0), p, np.roll(p, -1, axis=0)) >= 0).all())


# ------------------------------------------------------------------------------------------------------------------ hand-made rings
def comb(k):
    """k teeth of width 2 and height 6 on a base line, gaps of depth 4 between them: 4 k points, counter-clockwise, reflex at every gap."""
    pts = [(0, 0), (4 * k - 2, 0)]
    for i in reversed(range(k)):
        pts += [(4 * i + 2, 6), (4 * i, 6)]
        if i:
            pts += [(4 * i, 2), (4 * i - 2, 2)]
    return pts


def round_ring(n, r_even=16000, r_odd=16000, centre=16383):
    """n points around a circle (alternating radii: a star), rounded to integers up to 2^15."""
    a = 2 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, r_even, r_odd)
    return np.stack([np.rint(centre + r * np.cos(a)), np.rint(centre + r * np.sin(a))], -1).astype(np.int64).tolist()


SQUARE = [(0, 0), (4, 0), (4, 4), (0, 4)]
VALID = {
    "triangle": [(0, 0), (4, 0), (0, 3)],
    "square_ccw": SQUARE,
    "square_cw": SQUARE[::-1],
    "square_doubled": [p for q in SQUARE for p in (q, q)] + [SQUARE[0]],                   # n = 9, M = 4
    "dart": [(0, 0), (2, 1), (4, 0), (2, 4)],
    "dart_cw": [(2, 4), (4, 0), (2, 1), (0, 0)],
    "rect_midpoints": [(0, 0), (2, 0), (4, 0), (4, 1), (4, 2), (2, 2), (0, 2), (0, 1)],
    "comb": comb(5),
    "comb_cw": comb(5)[::-1],
    "l_shape": [(0, 0), (6, 0), (6, 2), (2, 2), (2, 6), (0, 6)],
    "big_coordinates": [(0, 0), (32767, 0), (32767, 32767), (16000, 100), (0, 32767)],
}
REFUSED = {
    "all_equal": ([(5, 5)] * 4, TOO_FEW),
    "two_points": ([(1, 1), (2, 2), (1, 1), (1, 1)], TOO_FEW),
    "collinear": ([(0, 0), (2, 0), (5, 0), (3, 0)], NO_AREA),
    "bare_spike": ([(0, 0), (3, 1), (0, 0), (1, 3)], NO_AREA),       # A-B-A-C alone encloses nothing: status 2 comes before 3
    "bow_tie": ([(0, 0), (4, 4), (4, 0), (0, 2)], NOT_SIMPLE),
    "spike": ([(0, 3), (4, 3), (4, 0), (4, 3), (4, 7), (0, 7)], NOT_SIMPLE),   # A-B-A-C on a rectangle: folds back at B
    "touching": ([(0, 0), (4, 0), (4, 4), (2, 0), (0, 4)], NOT_SIMPLE),        # a vertex on a non-adjacent edge
}
