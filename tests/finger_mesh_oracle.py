"""An independent numpy statement of the finger-mesh contract of include/dgdm_hip.h ("finger meshes"): the triangle tables, the knots and
collision pieces, chord_err, and the float64 checks (closedness, convexity, volume, area) the tests hold csrc/finger_mesh.hip to."""
import xml.etree.ElementTree as ET

import numpy as np


def split_quads(q):
    """(Q, 4) quads (a, b, c, d) -> (2 Q, 3) triangles (a, b, c), (a, c, d), quad by quad."""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 4)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def faces_2d(n):
    """Rings of n: curve z=0, curve+width z=0, curve+width z=height, curve z=height; the reference's quads left, right, front, back, top,
    bottom (assets/finger_sampler.py:24-31)."""
    i = np.arange(n - 1)
    left = np.stack([i, i + 1, i + 3 * n + 1, i + 3 * n], -1)
    right = np.stack([i + 2 * n, i + 2 * n + 1, i + n + 1, i + n], -1)
    front = np.array([[3 * n, 2 * n, n, 0]])
    back = np.array([[n - 1, 2 * n - 1, 3 * n - 1, 4 * n - 1]])
    top = np.stack([i + 2 * n, i + 3 * n, i + 3 * n + 1, i + 2 * n + 1], -1)
    bottom = np.stack([i + n, i + n + 1, i + 1, i], -1)
    return split_quads(np.concatenate([left, right, front, back, top, bottom])).astype(np.int32)


def faces_3d(n):
    N = n * n
    a, b = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    p00 = (a * n + b).reshape(-1)
    p01, p10, p11 = p00 + 1, p00 + n, p00 + n + 1
    sheet = np.stack([np.stack([p00, p10, p11], -1), np.stack([p00, p11, p01], -1)], 1).reshape(-1, 3)
    shifted = sheet[:, [0, 2, 1]] + N
    m = np.arange(n - 1)
    loop = np.concatenate([m, m * n + n - 1, (n - 1) * n + (n - 1 - m), (n - 1 - m) * n])
    nxt = np.roll(loop, -1)
    walls = np.stack([np.stack([loop, nxt, nxt + N], -1), np.stack([loop, nxt + N, loop + N], -1)], 1).reshape(-1, 3)
    return np.concatenate([sheet, shifted, walls]).astype(np.int32)


def faces_piece_2d():
    """A 2-D piece is the 2-point mesh with its vertices regrouped: ring r of point i sits at 4 i + r instead of 2 r + i."""
    f = faces_2d(2).astype(np.int64)
    return (4 * (f % 2) + f // 2).astype(np.int32)


def faces_piece_3d():
    """Sheet corners 0, 1, 2, shifted corners 3, 4, 5: the caps, then per cap edge (i, j) the wall quad (j, i, i + 3, j + 3)."""
    walls = split_quads([[j, i, i + 3, j + 3] for i, j in ((0, 1), (1, 2), (2, 0))])
    return np.concatenate([[[0, 1, 2], [3, 5, 4]], walls]).astype(np.int32)


def oracle_faces(kind, n=0):
    return {2: lambda: faces_2d(n), 3: lambda: faces_3d(n), 12: faces_piece_2d, 13: faces_piece_3d}[kind]()


def is_closed(faces):
    """Every directed edge occurs exactly once, and its reverse exactly once."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = sorted(map(tuple, e))
    return len(set(fwd)) == len(fwd) and fwd == sorted(map(tuple, e[:, ::-1]))


def knots(n, p):
    j = np.arange(p + 1)
    return (2 * j * (n - 1) + p) // (2 * p)


def volume_area(verts, faces):
    """(signed volume, area, smallest triangle area) in float64."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    vol = float((a * np.cross(b, c)).sum(axis=1).sum() / 6.0)
    ar = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1))
    return vol, float(ar.sum()), float(ar.min())


def convexity_excess(verts, faces):
    """How far (metres) any vertex lies OUTSIDE any face plane; <= 0 up to rounding for a convex, outward-oriented solid."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return float(((v[None, :, :] - a[:, None, :]) * nrm[:, None, :]).sum(-1).max())


def pieces_2d(verts, n, p):
    """verts (4 n, 3) -> (p, 8, 3)."""
    k = knots(n, p)
    rings = np.asarray(verts).reshape(4, n, 3)
    return np.concatenate([rings[:, k[:-1]].transpose(1, 0, 2), rings[:, k[1:]].transpose(1, 0, 2)], axis=1)


def chord_2d(verts, n, p):
    v = np.asarray(verts, dtype=np.float64)[:n]
    k = knots(n, p)
    err = 0.0
    for i0, i1 in zip(k[:-1], k[1:]):
        for i in range(i0 + 1, i1):
            t = (v[i, 0] - v[i0, 0]) / (v[i1, 0] - v[i0, 0])
            err = max(err, abs(v[i, 1] - (v[i0, 1] + (v[i1, 1] - v[i0, 1]) * t)))
    return err


def pieces_3d(verts, n, pu, pv):
    """verts (2 n^2, 3) -> (2 pu pv, 6, 3)."""
    v = np.asarray(verts).reshape(2, n, n, 3)
    ku, kv = knots(n, pu), knots(n, pv)
    out = []
    for j in range(pu):
        for l in range(pv):
            q00, q10, q11, q01 = (ku[j], kv[l]), (ku[j + 1], kv[l]), (ku[j + 1], kv[l + 1]), (ku[j], kv[l + 1])
            for tri in ((q00, q10, q11), (q00, q11, q01)):
                out.append([v[s][q] for s in (0, 1) for q in tri])
    return np.array(out)


def chord_3d(verts, n, pu, pv):
    v = np.asarray(verts, dtype=np.float64).reshape(2, n, n, 3)[0]
    ku, kv = knots(n, pu), knots(n, pv)
    err = 0.0
    for j in range(pu):
        for l in range(pv):
            a0, a1, b0, b1 = ku[j], ku[j + 1], kv[l], kv[l + 1]
            y00, y10, y11, y01 = v[a0, b0, 1], v[a1, b0, 1], v[a1, b1, 1], v[a0, b1, 1]
            for a in range(a0, a1 + 1):
                for b in range(b0, b1 + 1):
                    s = (v[a, b, 0] - v[a0, b0, 0]) / (v[a1, b0, 0] - v[a0, b0, 0])
                    t = (v[a, b, 2] - v[a0, b0, 2]) / (v[a0, b1, 2] - v[a0, b0, 2])
                    yl = y00 + s * (y10 - y00) + t * (y11 - y10) if s >= t else y00 + t * (y01 - y00) + s * (y11 - y01)
                    err = max(err, abs(v[a, b, 1] - yl))
    return err


def xml_tree(path):
    """(tag, attribute dict, [children]) of a file, recursively: what two model files must share."""
    def walk(e):
        return (e.tag, dict(e.attrib), [walk(c) for c in e])
    return walk(ET.parse(path).getroot())
