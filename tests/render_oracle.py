"""CPU oracles of the mesh rasteriser (include/dgdm_hip.h "mesh rendering").  Pure numpy / Python.

(a) ``render_contract``: the contract, statement for statement - float32 operations as ``np.float32`` scalars (every operation
    rounded on its own), the integer predicates in Python ints.
(b) ``render_float64``: an independent rasteriser - float64 projection of the unsnapped vertices, the inside test decided exactly
    (float64 filter, ``fractions.Fraction`` when the filter cannot tell), float64 depth by the plane through the projected
    vertices, float64 shading in world coordinates.  It shares nothing with (a) but the camera matrices it is given.
Both return ``ids (n_views, H, W) int32, depth, rgb (n_views, H, W, 3) uint8, rejected (n_views,) int32`` ((a) float32 depth and the
snapped table as a fifth result; (b) float64 depth).
"""
from fractions import Fraction

import numpy as np

F = np.float32
SUB = 256
LIMIT = 1 << 20


# ------------------------------------------------------------------------------------------------------------------ (a) the contract
def project(m, p):
    """One vertex p (3,) float32 under the row-major matrix m (4, 4) float32 -> (X, Y, zs, ok)."""
    x, y, z = F(p[0]), F(p[1]), F(p[2])
    with np.errstate(all="ignore"):
        c = [((F(m[r][0]) * x + F(m[r][1]) * y) + F(m[r][2]) * z) + F(m[r][3]) for r in range(4)]
        px, py, zs = c[0] / c[3], c[1] / c[3], c[2] / c[3]
        fx, fy = np.rint(px * F(SUB)), np.rint(py * F(SUB))
    bad = (not c[3] > 0) or (not np.isfinite(c[3])) or (not abs(fx) < LIMIT) or (not abs(fy) < LIMIT) or (not np.isfinite(zs))
    if bad:
        return 0, 0, zs, 0
    return int(fx), int(fy), zs, 1


def edge(xa, ya, xb, yb, sx, sy):
    """(E, inside) of sample (sx, sy) for the edge a -> b, Python ints."""
    dx, dy = xb - xa, yb - ya
    E = dx * (sy - ya) - dy * (sx - xa)
    return E, E > 0 or (E == 0 and (dy < 0 or (dy == 0 and dx > 0)))


def orient(v0, v1, v2):
    """The snapped vertices (X, Y, ...) in drawing order, or None when the triangle has no area."""
    A = (v1[0] - v0[0]) * (v2[1] - v0[1]) - (v1[1] - v0[1]) * (v2[0] - v0[0])
    if A == 0:
        return None
    return (v0, v1, v2, A) if A > 0 else (v0, v2, v1, -A)


def pixel_range(lo, hi, n):
    """Pixels i in [0, n) whose sample 256 i + 128 lies in [lo, hi]."""
    a = max(0, -((128 - lo) // SUB))          # ceil((lo - 128) / 256)
    b = min(n - 1, (hi - 128) // SUB)
    return range(a, b + 1)


def cover_mask(tri, W, H):
    """(H, W) bool: the pixels a triangle of snapped vertices ((X0, Y0), (X1, Y1), (X2, Y2)) covers."""
    out = np.zeros((H, W), dtype=bool)
    o = orient(*[tuple(int(c) for c in v) for v in tri])
    if o is None:
        return out
    v0, v1, v2, _ = o
    for j in pixel_range(min(v0[1], v1[1], v2[1]), max(v0[1], v1[1], v2[1]), H):
        for i in pixel_range(min(v0[0], v1[0], v2[0]), max(v0[0], v1[0], v2[0]), W):
            sx, sy = SUB * i + 128, SUB * j + 128
            out[j, i] = edge(*v0[:2], *v1[:2], sx, sy)[1] and edge(*v1[:2], *v2[:2], sx, sy)[1] and edge(*v2[:2], *v0[:2], sx, sy)[1]
    return out


def shade(a, b, c, eye):
    """The flat shade of a triangle with model-space float32 vertices a, b, c (file order) seen from eye (model space)."""
    a, b, c, eye = ([F(v) for v in p] for p in (a, b, c, eye))
    with np.errstate(all="ignore"):
        e1 = [b[k] - a[k] for k in range(3)]
        e2 = [c[k] - a[k] for k in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        d = [eye[k] - ((a[k] + b[k]) + c[k]) / F(3) for k in range(3)]
        dot = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        q = np.sqrt(nn * dd)
        if not q > 0 or not np.isfinite(q):
            return F(0.3)
        return F(0.3) + F(0.7) * min(abs(dot) / q, F(1))


def _instances(inst_view):
    """Instance indices in view order, the caller's order within a view."""
    return sorted(range(len(inst_view)), key=lambda i: int(inst_view[i]))


def render_contract(verts, tris, offsets, inst_view, inst_mesh, inst_matrix, inst_id, n_views, W, H, inst_rgb=None, inst_eye=None):
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.asarray(tris).reshape(-1, 3)
    vo, to = offsets
    mats = np.asarray(inst_matrix, dtype=np.float32)
    ids = np.full((n_views, H, W), -1, dtype=np.int32)
    depth = np.full((n_views, H, W), np.inf, dtype=np.float32)
    rgb = np.full((n_views, H, W, 3), 255, dtype=np.uint8)
    rejected = np.zeros(n_views, dtype=np.int32)
    snapped = []
    for i in _instances(inst_view):
        view, m = int(inst_view[i]), int(inst_mesh[i])
        V = verts[int(vo[m]):int(vo[m + 1])]
        sn = [project(mats[i], p) for p in V]
        snapped += [(s[0], s[1], int(np.float32(s[2]).view(np.int32)), s[3]) for s in sn]
        for t in tris[int(to[m]):int(to[m + 1])]:
            a, b, c = (sn[int(k)] for k in t)
            if not (a[3] and b[3] and c[3]):
                rejected[view] += 1
                continue
            o = orient(a, b, c)
            if o is None:
                continue
            v0, v1, v2, A = o
            colour = None
            if inst_rgb is not None:
                s = shade(V[int(t[0])], V[int(t[1])], V[int(t[2])], inst_eye[i])
                colour = [int(min(max(np.rint((F(inst_rgb[i][k]) * s) * F(255)), 0), 255)) for k in range(3)]
            fA = F(A)
            for j in pixel_range(min(v0[1], v1[1], v2[1]), max(v0[1], v1[1], v2[1]), H):
                for x in pixel_range(min(v0[0], v1[0], v2[0]), max(v0[0], v1[0], v2[0]), W):
                    sx, sy = SUB * x + 128, SUB * j + 128
                    e01, in01 = edge(*v0[:2], *v1[:2], sx, sy)
                    e12, in12 = edge(*v1[:2], *v2[:2], sx, sy)
                    e20, in20 = edge(*v2[:2], *v0[:2], sx, sy)
                    if not (in01 and in12 and in20):
                        continue
                    b1, b2 = F(e20) / fA, F(e01) / fA
                    z = (v0[2] + b1 * (v1[2] - v0[2])) + b2 * (v2[2] - v0[2])
                    if z < depth[view, j, x]:
                        depth[view, j, x] = z
                        ids[view, j, x] = int(inst_id[i])
                        if colour is not None:
                            rgb[view, j, x] = colour
    return ids, depth, rgb, rejected, np.asarray(snapped, dtype=np.int32).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------------------------ (b) float64
def _side(ax, ay, bx, by, sx, sy):
    """Exact sign rule of the sample against the edge a -> b on float64 coordinates: filtered, exact rationals when in doubt."""
    dx, dy = bx - ax, by - ay
    t1, t2 = dx * (sy - ay), dy * (sx - ax)
    E = t1 - t2
    if abs(E) > 1e-12 * (abs(t1) + abs(t2)) + 1e-300:
        return E > 0
    ax, ay, bx, by, sx, sy = (Fraction(float(v)) for v in (ax, ay, bx, by, sx, sy))
    dx, dy = bx - ax, by - ay
    E = dx * (sy - ay) - dy * (sx - ax)
    return E > 0 or (E == 0 and (dy < 0 or (dy == 0 and dx > 0)))


def render_float64(verts, tris, offsets, inst_view, inst_mesh, inst_model, cams, eyes, inst_id, inst_rgb, n_views, W, H):
    """cams (n_views, 4, 4): world -> (pixel x, pixel y, depth, w); inst_model (n_inst, 4, 4): model -> world; eyes (n_views, 3) world."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    tris = np.asarray(tris).reshape(-1, 3)
    vo, to = offsets
    ids = np.full((n_views, H, W), -1, dtype=np.int32)
    depth = np.full((n_views, H, W), np.inf)
    rgb = np.full((n_views, H, W, 3), 255, dtype=np.uint8)
    rejected = np.zeros(n_views, dtype=np.int32)
    for i in _instances(inst_view):
        view, m = int(inst_view[i]), int(inst_mesh[i])
        model = np.asarray(inst_model[i], dtype=np.float64)
        V = verts[int(vo[m]):int(vo[m + 1])]
        world = (np.concatenate([V, np.ones((len(V), 1))], axis=1) @ model.T)
        clip = world @ np.asarray(cams[view], dtype=np.float64).T
        world = world[:, :3] / world[:, 3:4]
        for t in tris[int(to[m]):int(to[m + 1])]:
            c = clip[t]
            with np.errstate(all="ignore"):
                p = c[:, :3] / c[:, 3:4]
            if (c[:, 3] <= 0).any() or not np.isfinite(p).all() or (np.abs(np.rint(p[:, :2] * SUB)) >= LIMIT).any():
                rejected[view] += 1
                continue
            area = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0])
            if area == 0:
                continue
            if area < 0:
                p = p[[0, 2, 1]]
            w = world[t]
            n = np.cross(w[1] - w[0], w[2] - w[0])
            d = np.asarray(eyes[view], dtype=np.float64) - w.mean(axis=0)
            q = np.linalg.norm(n) * np.linalg.norm(d)
            s = 0.3 + 0.7 * min(abs(float(n @ d)) / q, 1.0) if q > 0 else 0.3
            colour = np.clip(np.rint(np.asarray(inst_rgb[i], dtype=np.float64) * s * 255.0), 0, 255).astype(np.uint8)
            # depth is affine over the screen: z = z0 + gx (x - x0) + gy (y - y0)
            M2 = np.array([[p[1, 0] - p[0, 0], p[1, 1] - p[0, 1]], [p[2, 0] - p[0, 0], p[2, 1] - p[0, 1]]])
            gx, gy = np.linalg.solve(M2, [p[1, 2] - p[0, 2], p[2, 2] - p[0, 2]])
            for j in range(max(0, int(np.floor(p[:, 1].min() - 0.5))), min(H - 1, int(np.ceil(p[:, 1].max() - 0.5))) + 1):
                for x in range(max(0, int(np.floor(p[:, 0].min() - 0.5))), min(W - 1, int(np.ceil(p[:, 0].max() - 0.5))) + 1):
                    sx, sy = x + 0.5, j + 0.5
                    if not (_side(p[0, 0], p[0, 1], p[1, 0], p[1, 1], sx, sy) and _side(p[1, 0], p[1, 1], p[2, 0], p[2, 1], sx, sy)
                            and _side(p[2, 0], p[2, 1], p[0, 0], p[0, 1], sx, sy)):
                        continue
                    z = p[0, 2] + gx * (sx - p[0, 0]) + gy * (sy - p[0, 1])
                    if z < depth[view, j, x]:
                        depth[view, j, x] = z
                        ids[view, j, x] = int(inst_id[i])
                        rgb[view, j, x] = colour
    return ids, depth, rgb, rejected
