"""CPU restatement (numpy float64) of the sliced squeeze in include/dgdm_hip.h ("squeeze simulator, 3-D fingers"): the slicing of a
triangle mesh on the planes z = gz[j] and the touch tables of the segment soup between two jaw faces sampled on (gx, gz).  Every
product, sum and quotient below is one IEEE float64 operation in the order the header gives, so the device's segments and tables must
equal these bit for bit.  Everything after S is the 2-D contract and is taken from tests/squeeze_oracle.py unchanged."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from tests.squeeze_oracle import INF, kth_successor, map_outputs, pose_y, rotation_table, settled, snap, successors  # noqa: F401


def slice_mesh(verts, tris, gz) -> Tuple[np.ndarray, np.ndarray]:
    """(segments [n][4] = (A_x, A_y, B_x, B_y), offsets [mv + 1]) of one mesh: per level, the crossing triangles in index order."""
    V = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    segs, offsets = [], [0]
    for z in np.asarray(gz, dtype=np.float64):
        up = V[F, 2] >= z                                              # [nt][3]
        nup = up.sum(axis=1)
        rows = np.nonzero((nup != 0) & (nup != 3))[0]
        pts = np.zeros((len(rows), 2, 2))
        filled = np.zeros(len(rows), dtype=np.int64)
        for e in range(3):                                             # edges v0 v1, v1 v2, v2 v0
            e1 = (e + 1) % 3
            diff = up[rows, e] != up[rows, e1]
            d = np.where(up[rows, e], F[rows, e1], F[rows, e])       # the down end
            w = np.where(up[rows, e], F[rows, e], F[rows, e1])       # the up end
            D, W = V[d], V[w]
            with np.errstate(all="ignore"):
                r = (z - D[:, 2]) / (W[:, 2] - D[:, 2])
                p = np.stack([D[:, 0] + r * (W[:, 0] - D[:, 0]), D[:, 1] + r * (W[:, 1] - D[:, 1])], axis=1)
            k = np.nonzero(diff)[0]
            pts[k, filled[k]] = p[k]
            filled[k] += 1
        assert (filled == 2).all()
        segs.append(pts.reshape(-1, 4))
        offsets.append(offsets[-1] + len(rows))
    return np.concatenate(segs) if segs else np.zeros((0, 4)), np.asarray(offsets, dtype=np.int32)


def slice_meshes(meshes: Sequence, gz) -> Tuple[np.ndarray, np.ndarray]:
    """The one list of all meshes and offsets [O][mv + 1] into it."""
    segs, offs, base = [], [], 0
    for v, f in meshes:
        s, o = slice_mesh(v, f, gz)
        segs.append(s)
        offs.append(o + base)
        base += len(s)
    return np.concatenate(segs), np.stack(offs).astype(np.int32)


def touch_tables_3d(lower, upper, gx, segments, offsets, rot, x_cells: int, x_half: float, rows: int = 16):
    """(touch_l, touch_r, S), each [theta][x_cells], of one pair.  lower / upper [mv][mu]: the two jaw faces at travel 0; segments / offsets
    [mv + 1]: one object's (offsets into `segments`)."""
    L, U = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    gx = np.asarray(gx, dtype=np.float64)
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 4)
    rot = np.asarray(rot, dtype=np.float64)
    mv, mu = L.shape
    X, T = int(x_cells), len(rot)
    dx = 2.0 * float(x_half) / float(X - 1)
    xg = -float(x_half) + np.arange(X, dtype=np.float64) * dx
    tl, tr = np.full((T, X), INF), np.full((T, X), INF)
    with np.errstate(all="ignore"):
        for a0 in range(0, T, rows):
            c, s = rot[a0:a0 + rows, 0:1], rot[a0:a0 + rows, 1:2]
            bl, br = np.full((len(c), X), INF), np.full((len(c), X), INF)
            for j in range(mv):
                sj = seg[offsets[j]:offsets[j + 1]]
                if len(sj) == 0:
                    continue
                Lj, Uj = L[j], U[j]
                ends = []
                for k in (0, 2):                                           # P from A, Q from B
                    ax, ay = sj[None, :, k], sj[None, :, k + 1]
                    rx = c * ax - s * ay
                    ry = s * ax + c * ay
                    px = rx[:, None, :] + xg[None, :, None]                 # [rows][X][n]
                    ends.append((px, np.broadcast_to(ry[:, None, :], px.shape)))
                for px, py in ends:                                        # set A: both end points against the interpolated profiles
                    inr = (px >= gx[0]) & (px <= gx[-1])
                    i = np.clip(np.searchsorted(gx, px, side="right") - 1, 0, mu - 2)
                    f = (px - gx[i]) / (gx[i + 1] - gx[i])
                    lp = Lj[i] + f * (Lj[i + 1] - Lj[i])
                    up = Uj[i] + f * (Uj[i + 1] - Uj[i])
                    bl = np.minimum(bl, np.where(inr, py - lp, INF).min(axis=-1))
                    br = np.minimum(br, np.where(inr, up - py, INF).min(axis=-1))
                (px, py), (qx, qy) = ends                                  # set B: the abscissae under the segment
                slope = (qy - py) / (qx - px)
                lo, hi = np.minimum(px, qx), np.maximum(px, qx)
                for i in range(mu):
                    act = (px != qx) & (lo <= gx[i]) & (gx[i] <= hi)
                    if not act.any():
                        continue
                    ye = py + (gx[i] - px) * slope
                    bl = np.minimum(bl, np.where(act, ye - Lj[i], INF).min(axis=-1))
                    br = np.minimum(br, np.where(act, Uj[i] - ye, INF).min(axis=-1))
            tl[a0:a0 + rows], tr[a0:a0 + rows] = bl, br
        S = (tl + tr) / 2.0
    return tl, tr, S


def squeeze_pair_3d(lower, upper, gx, segments, offsets, rot, starts, x_cells: int, x_half: float, window: int, closing_steps: int,
                    travel_max: float) -> Dict[str, np.ndarray]:
    """Everything dgdm_squeeze_map_3d returns for one pair."""
    tl, tr, S = touch_tables_3d(lower, upper, gx, segments, offsets, rot, x_cells, x_half)
    return map_outputs(tl, tr, S, successors(S, window, travel_max), starts, len(rot), x_cells, x_half, closing_steps, travel_max)


def squeeze_map_3d(surfaces, gx, segments, offsets, pairs: Sequence, rot, starts, **cfg) -> Dict[str, np.ndarray]:
    """squeeze_pair_3d of every (finger, object) of `pairs`, stacked on a leading pair axis.  surfaces [F][2][mv][mu], offsets [O][mv + 1]."""
    outs = [squeeze_pair_3d(surfaces[f][0], surfaces[f][1], gx, segments, offsets[o], rot, starts, **cfg) for f, o in pairs]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}
