"""CPU restatement (numpy float64) of the squeeze simulator with Coulomb friction, written from the contract in include/dgdm_hip.h
("squeeze simulator with Coulomb friction"): the frictionless tables of tests/squeeze_oracle.py, the two contacts of every cell in the
contract's visiting order, the antipodal jam test, and the map in which a jammed cell is a fixed point.  Every product, sum, difference
and quotient below is one IEEE float64 operation in the order the header gives, so the device's tables must equal these bit for bit and
its integers exactly."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from tests import squeeze_oracle as so

INF = np.inf


def contact_tables(lower, upper, verts, rot, x_cells: int, x_half: float, half_len: float) -> Dict[str, np.ndarray]:
    """One (finger, object) pair: touch_l, touch_r, S [theta][x_cells]; contact [theta][x_cells][2] int32, the code of the lower and of the
    upper contact (i for set A, nv + i m + j for set B, -1 for none); c_l, n_l, c_u, n_u [theta][x_cells][2], the contacts' points and
    unnormalised normals (NaN where there is none).  The candidates are walked one after the other, i = 0 .. nv - 1: vertex i (set A), then
    the samples j ascending under the edge (i, i + 1) (set B); numpy runs over the cells only."""
    L, U = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    v = np.asarray(verts, dtype=np.float64)
    rot = np.asarray(rot, dtype=np.float64)
    m, nv, X, hl, T = len(L), len(v), int(x_cells), float(half_len), len(rot)
    h = 2.0 * hl / float(m - 1)
    dx = 2.0 * float(x_half) / float(X - 1)
    xg = -float(x_half) + np.arange(X, dtype=np.float64) * dx
    c, s = rot[:, 0:1], rot[:, 1:2]
    rx = c * v[None, :, 0] - s * v[None, :, 1]                             # [T][nv]
    ry = s * v[None, :, 0] + c * v[None, :, 1]
    g = [np.full((T, X), INF), np.full((T, X), INF)]                       # the running least gap: lower, upper
    code = [np.full((T, X), -1, dtype=np.int64), np.full((T, X), -1, dtype=np.int64)]
    pt = [np.full((T, X, 2), np.nan), np.full((T, X, 2), np.nan)]
    nr = [np.full((T, X, 2), np.nan), np.full((T, X, 2), np.nan)]

    def offer(side, ok, gap, k, cx, cy, nx, ny):
        """A candidate of `side` where `ok`: it replaces the contact where its gap is strictly less than the running least gap."""
        win = ok & (gap < g[side])
        code[side] = np.where(win, k, code[side])
        pt[side] = np.where(win[..., None], np.stack(np.broadcast_arrays(cx, cy), axis=-1), pt[side])
        nr[side] = np.where(win[..., None], np.stack(np.broadcast_arrays(nx, ny), axis=-1), nr[side])
        g[side] = np.where(ok, np.fmin(g[side], gap), g[side])

    with np.errstate(all="ignore"):
        for i in range(nv):
            i1 = (i + 1) % nv
            px = rx[:, i:i + 1] + xg[None, :]                              # [T][X]
            py = np.broadcast_to(ry[:, i:i + 1], px.shape)
            qx = rx[:, i1:i1 + 1] + xg[None, :]
            qy = np.broadcast_to(ry[:, i1:i1 + 1], px.shape)
            t, tq = (px + hl) / h, (qx + hl) / h
            # set A: vertex i on the finger segment j, j + 1
            inr = (px >= -hl) & (px <= hl)
            jf = np.where(inr, np.minimum(np.floor(t), float(m - 2)), 0.0)
            j = jf.astype(np.int64)
            f = t - jf
            dL, dU = L[j + 1] - L[j], U[j + 1] - U[j]
            lp = L[j] + f * dL
            up = U[j] + f * dU
            offer(0, inr, py - lp, i, px, py, -dL, np.full(px.shape, h))
            offer(1, inr, up - py, i, px, py, dU, np.full(px.shape, -h))
            # set B: the finger samples under the edge (i, i + 1), j ascending
            j0 = np.maximum(np.ceil(np.minimum(t, tq)), 0.0)
            j1 = np.minimum(np.floor(np.maximum(t, tq)), float(m - 1))
            ok = (px != qx) & (j0 <= j1)
            ex, ey = qx - px, qy - py
            slope = ey / ex
            pos = ex > 0.0
            nlx, nly = np.where(pos, -ey, ey), np.where(pos, ex, -ex)
            nux, nuy = np.where(pos, ey, -ey), np.where(pos, -ex, ex)
            j0i = np.where(ok, j0, 0.0).astype(np.int64)
            j1i = np.where(ok, j1, -1.0).astype(np.int64)
            d = 0
            while True:
                jj = j0i + d
                act = ok & (jj <= j1i)
                if not act.any():
                    break
                jc = np.where(act, jj, 0)
                uj = -hl + jc.astype(np.float64) * h
                ye = py + (uj - px) * slope
                k = nv + i * m + jc
                offer(0, act, ye - L[jc], k, uj, ye, nlx, nly)
                offer(1, act, U[jc] - ye, k, uj, ye, nux, nuy)
                d += 1
        S = (g[0] + g[1]) / 2.0
    return {"touch_l": g[0], "touch_r": g[1], "S": S, "contact": np.stack(code, axis=-1).astype(np.int32), "c_l": pt[0], "n_l": nr[0],
            "c_u": pt[1], "n_u": nr[1]}


def jam_table(tab: Dict[str, np.ndarray], mu: float, travel_max: float) -> np.ndarray:
    """jam [theta][x_cells] int32 (0 / 1) of contact_tables' output: the header's test, term by term."""
    cl, nl, cu, nu = tab["c_l"], tab["n_l"], tab["c_u"], tab["n_u"]
    mu = float(mu)
    with np.errstate(all="ignore"):
        dx = cu[..., 0] - cl[..., 0]
        dy = cu[..., 1] - cl[..., 1]
        dot_l = nl[..., 0] * dx + nl[..., 1] * dy
        crs_l = nl[..., 0] * dy - nl[..., 1] * dx
        dot_u = -(nu[..., 0] * dx + nu[..., 1] * dy)
        crs_u = nu[..., 0] * dy - nu[..., 1] * dx
        both = (tab["contact"][..., 0] >= 0) & (tab["contact"][..., 1] >= 0)
        jam = both & (mu > 0.0) & (tab["S"] < float(travel_max)) & (dot_l > 0.0) & (dot_u > 0.0) & (np.abs(crs_l) <= mu * dot_l) & \
            (np.abs(crs_u) <= mu * dot_u)
    return jam.astype(np.int32)


def successors(S, jam, window: int, travel_max: float) -> np.ndarray:
    """The frictionless successors, except that a jammed cell is its own (every cell's successor is found on its own)."""
    succ = so.successors(S, window, travel_max)
    own = np.arange(len(succ), dtype=np.int32)
    return np.where(np.asarray(jam).reshape(-1) != 0, own, succ).astype(np.int32)


def squeeze_pair(lower, upper, verts, rot, starts, x_cells: int, x_half: float, window: int, closing_steps: int, travel_max: float,
                 half_len: float = 0.12, mu: float = 0.0, tables: Dict[str, np.ndarray] = None) -> Dict[str, np.ndarray]:
    """Everything dgdm_squeeze_map_friction returns for one pair: the three tables, succ, jam, contact, and per start cells (start, closed,
    settled), y (closed, settled) and flags (1 / 2 / 4 as without friction, 8 the start cell is jammed, 16 the settled cell is).
    tables: contact_tables of the same inputs, when the caller already holds them (they do not depend on mu)."""
    tab = tables if tables is not None else contact_tables(lower, upper, verts, rot, x_cells, x_half, half_len)
    S = tab["S"]
    jam = jam_table(tab, mu, travel_max)
    out = so.map_outputs(tab["touch_l"], tab["touch_r"], S, successors(S, jam, window, travel_max), starts, len(rot), x_cells, x_half,
                         closing_steps, travel_max, jam=jam)
    out["contact"] = tab["contact"]
    return out


def squeeze_map(surfaces, objects, pairs: Sequence, rot, starts, **cfg) -> Dict[str, np.ndarray]:
    """squeeze_pair of every (finger, object) of `pairs`, stacked on a leading pair axis.  surfaces [F][2][m], objects [O][nv][2]."""
    outs = [squeeze_pair(surfaces[f][0], surfaces[f][1], objects[o], rot, starts, **cfg) for f, o in pairs]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}
