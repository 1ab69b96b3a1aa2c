"""CPU restatement (numpy float64) of the sliced squeeze with Coulomb friction, written from the contract in include/dgdm_hip.h ("squeeze
simulator, 3-D fingers, with Coulomb friction"): the triangle normals of the slicer, the two contacts of every cell in the contract's
visiting order with their 3-D points and normals, the 3-D antipodal jam test, and the map in which a jammed cell is a fixed point.  Every
product, sum, difference and quotient below is one IEEE float64 operation in the order the header gives, so the device's tables must
equal these bit for bit and its integers exactly.  The slicing, the rotation table and everything after the jam table are
tests/squeeze3d_oracle.py's and tests/squeeze_friction_oracle.py's, unchanged."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from tests import squeeze3d_oracle as so3
from tests import squeeze_friction_oracle as fo
from tests import squeeze_oracle as so

INF = np.inf


def slice_normals(verts, tris, gz) -> np.ndarray:
    """normals [n][3] of one mesh in slice_mesh's segment order: N = (V1 - V0) x (V2 - V0) of every crossing triangle, per level."""
    V = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    out = []
    for z in np.asarray(gz, dtype=np.float64):
        nup = (V[F, 2] >= z).sum(axis=1)
        rows = np.nonzero((nup != 0) & (nup != 3))[0]
        e = V[F[rows, 1]] - V[F[rows, 0]]
        g = V[F[rows, 2]] - V[F[rows, 0]]
        out.append(np.stack([e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1], e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2], e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]],
                            axis=1))
    return np.concatenate(out) if out else np.zeros((0, 3))


def slice_meshes(meshes: Sequence, gz) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(segments [n][4], offsets [O][mv + 1], normals [n][3]) of all meshes: squeeze3d_oracle.slice_meshes and the normals in its order."""
    seg, off = so3.slice_meshes(meshes, gz)
    nrm = np.concatenate([slice_normals(v, f, gz) for v, f in meshes])
    assert len(nrm) == len(seg)
    return seg, off, nrm


def contact_tables_3d(lower, upper, gx, gz, segments, normals, offsets, rot, x_cells: int, x_half: float) -> Dict[str, np.ndarray]:
    """One (finger, object) pair: touch_l, touch_r, S [theta][x_cells]; contact [theta][x_cells][2] int32, the code s (mu + 2) + k of the
    lower and of the upper contact (-1: none); c_l, n_l, c_u, n_u [theta][x_cells][3], the contacts' points and unnormalised normals (NaN
    where there is none).  offsets [mv + 1]: the object's, into segments / normals.  The candidates are walked one after the other -
    segment by segment, P, Q, then the abscissae ascending; numpy runs over the cells only."""
    L, U = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    gx, gz = np.asarray(gx, dtype=np.float64), np.asarray(gz, dtype=np.float64)
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 4)
    nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    rot = np.asarray(rot, dtype=np.float64)
    mv, mu = L.shape
    X, T = int(x_cells), len(rot)
    dx = 2.0 * float(x_half) / float(X - 1)
    xg = -float(x_half) + np.arange(X, dtype=np.float64) * dx
    c, s = rot[:, 0:1], rot[:, 1:2]
    g = [np.full((T, X), INF), np.full((T, X), INF)]                       # the running least gap: lower, upper
    code = [np.full((T, X), -1, dtype=np.int64), np.full((T, X), -1, dtype=np.int64)]
    pt = [np.full((T, X, 3), np.nan), np.full((T, X, 3), np.nan)]
    nr = [np.full((T, X, 3), np.nan), np.full((T, X, 3), np.nan)]

    def offer(side, ok, gap, k, point, normal):
        """A candidate of `side` where `ok`: it replaces the contact where its gap is strictly less than the running least gap."""
        win = ok & (gap < g[side])
        code[side] = np.where(win, k, code[side])
        pt[side] = np.where(win[..., None], np.stack(np.broadcast_arrays(*point), axis=-1), pt[side])
        nr[side] = np.where(win[..., None], np.stack(np.broadcast_arrays(*normal), axis=-1), nr[side])
        g[side] = np.where(ok, np.fmin(g[side], gap), g[side])

    s0 = int(offsets[0])
    with np.errstate(all="ignore"):
        for j in range(mv):
            Lj, Uj = L[j], U[j]
            jm, jp = max(j - 1, 0), min(j + 1, mv - 1)
            hz = gz[jp] - gz[jm] if mv > 1 else 1.0
            z = np.full((T, X), gz[j])
            for t in range(int(offsets[j]), int(offsets[j + 1])):
                kc = (t - s0) * (mu + 2)
                ax, ay, bx, by = seg[t]
                px = (c * ax - s * ay) + xg[None, :]                      # [T][X]
                py = np.broadcast_to(s * ax + c * ay, px.shape)
                qx = (c * bx - s * by) + xg[None, :]
                qy = np.broadcast_to(s * bx + c * by, px.shape)
                for k, (ex, ey) in enumerate(((px, py), (qx, qy))):        # set A: P, then Q, on the jaws' patch i, i + 1 of level j
                    inr = (ex >= gx[0]) & (ex <= gx[-1])
                    i = np.clip(np.searchsorted(gx, ex, side="right") - 1, 0, mu - 2)
                    hx = gx[i + 1] - gx[i]
                    f = (ex - gx[i]) / hx
                    dL, dU = Lj[i + 1] - Lj[i], Uj[i + 1] - Uj[i]
                    lp = Lj[i] + f * dL
                    up = Uj[i] + f * dU
                    if mv > 1:
                        lm, lq = L[jm][i] + f * (L[jm][i + 1] - L[jm][i]), L[jp][i] + f * (L[jp][i + 1] - L[jp][i])
                        um, uq = U[jm][i] + f * (U[jm][i + 1] - U[jm][i]), U[jp][i] + f * (U[jp][i + 1] - U[jp][i])
                        nlz, nuz = -(lq - lm) * hx, (uq - um) * hx
                    else:
                        nlz = nuz = np.zeros(ex.shape)
                    offer(0, inr, ey - lp, kc + k, (ex, ey, z), (-dL * hz, hx * hz, nlz))
                    offer(1, inr, up - ey, kc + k, (ex, ey, z), (dU * hz, -(hx * hz), nuz))
                slope = (qy - py) / (qx - px)                              # set B: the abscissae under the segment, the triangle's normal
                lo, hi = np.minimum(px, qx), np.maximum(px, qx)
                N = nrm[t]
                rx = np.broadcast_to(c * N[0] - s * N[1], px.shape)
                ry = np.broadcast_to(s * N[0] + c * N[1], px.shape)
                rz = np.full(px.shape, N[2])
                fl, fu = ry < 0.0, ry > 0.0                                # lower: n_y > 0; upper: n_y < 0
                n_l = (np.where(fl, -rx, rx), np.where(fl, -ry, ry), np.where(fl, -rz, rz))
                n_u = (np.where(fu, -rx, rx), np.where(fu, -ry, ry), np.where(fu, -rz, rz))
                for i in range(mu):
                    act = (px != qx) & (lo <= gx[i]) & (gx[i] <= hi)
                    if not act.any():
                        continue
                    ye = py + (gx[i] - px) * slope
                    xi = np.full(px.shape, gx[i])
                    offer(0, act, ye - Lj[i], kc + 2 + i, (xi, ye, z), n_l)
                    offer(1, act, Uj[i] - ye, kc + 2 + i, (xi, ye, z), n_u)
        S = (g[0] + g[1]) / 2.0
    return {"touch_l": g[0], "touch_r": g[1], "S": S, "contact": np.stack(code, axis=-1).astype(np.int32), "c_l": pt[0], "n_l": nr[0],
            "c_u": pt[1], "n_u": nr[1]}


def jam_table_3d(tab: Dict[str, np.ndarray], mu: float, travel_max: float) -> np.ndarray:
    """jam [theta][x_cells] int32 (0 / 1) of contact_tables_3d's output: the header's test, term by term (mu: the friction coefficient)."""
    cl, nl, cu, nu = tab["c_l"], tab["n_l"], tab["c_u"], tab["n_u"]
    mu = float(mu)
    with np.errstate(all="ignore"):
        d = [cu[..., k] - cl[..., k] for k in range(3)]

        def terms(n):
            a = n[..., 0] * d[0] + n[..., 1] * d[1] + n[..., 2] * d[2]
            wx = n[..., 1] * d[2] - n[..., 2] * d[1]
            wy = n[..., 2] * d[0] - n[..., 0] * d[2]
            wz = n[..., 0] * d[1] - n[..., 1] * d[0]
            return a, wx * wx + wy * wy + wz * wz

        a_l, q_l = terms(nl)
        a_u, q_u = terms(nu)
        a_u = -a_u
        both = (tab["contact"][..., 0] >= 0) & (tab["contact"][..., 1] >= 0)
        jam = both & (mu > 0.0) & (tab["S"] < float(travel_max)) & (a_l > 0.0) & (a_u > 0.0) & (q_l <= (mu * a_l) * (mu * a_l)) & \
            (q_u <= (mu * a_u) * (mu * a_u))
    return jam.astype(np.int32)


def squeeze_pair_3d(lower, upper, gx, gz, segments, normals, offsets, rot, starts, x_cells: int, x_half: float, window: int, closing_steps: int,
                    travel_max: float, mu: float = 0.0, tables: Dict[str, np.ndarray] = None) -> Dict[str, np.ndarray]:
    """Everything dgdm_squeeze_map_3d_friction returns for one pair: the three tables, succ, jam, contact, and per start cells, y and flags
    (8: the start cell is jammed, 16: the settled cell is).  mu: the friction coefficient.  tables: contact_tables_3d of the same inputs,
    when the caller already holds them (they do not depend on mu)."""
    tab = tables if tables is not None else contact_tables_3d(lower, upper, gx, gz, segments, normals, offsets, rot, x_cells, x_half)
    S = tab["S"]
    jam = jam_table_3d(tab, mu, travel_max)
    out = so.map_outputs(tab["touch_l"], tab["touch_r"], S, fo.successors(S, jam, window, travel_max), starts, len(rot), x_cells, x_half,
                         closing_steps, travel_max, jam=jam)
    out["contact"] = tab["contact"]
    return out


def squeeze_map_3d(surfaces, gx, gz, segments, normals, offsets, pairs: Sequence, rot, starts, **cfg) -> Dict[str, np.ndarray]:
    """squeeze_pair_3d of every (finger, object) of `pairs`, stacked on a leading pair axis.  surfaces [F][2][mv][mu], offsets [O][mv + 1]."""
    outs = [squeeze_pair_3d(surfaces[f][0], surfaces[f][1], gx, gz, segments, normals, offsets[o], rot, starts, **cfg) for f, o in pairs]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}
