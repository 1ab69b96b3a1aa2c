"""CPU restatement (numpy float64) of the squeeze simulator's contract in include/dgdm_hip.h ("squeeze simulator"): a frictionless,
quasi-static parallel-jaw squeeze of a polygon by two finger surfaces on a (theta, x) grid.  Every product, sum and quotient below is
one IEEE float64 operation in the order the header gives, so the device's tables must equal these bit for bit."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

INF = np.inf
TWO_PI = 6.283185307179586           # the float64 nearest 2 pi, the constant of the header

DEFAULTS = dict(theta=720, x_cells=241, x_half=0.06, window=2, closing_steps=6, travel_max=0.1, half_len=0.12)


def rotation_table(theta: int) -> np.ndarray:
    """rot [theta][2] = (cos, sin) of 2 pi a / theta, as the caller of dgdm_squeeze_map makes it."""
    ang = 2.0 * np.pi * np.arange(int(theta), dtype=np.float64) / float(theta)
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1))


def touch_tables(lower, upper, verts, rot, x_cells: int, x_half: float, half_len: float, rows: int = 16):
    """(touch_l, touch_r, S), each [theta][x_cells], of one (finger, object) pair.  lower / upper [m]: the two surfaces at jaw travel 0;
    verts [nv][2]."""
    L, U = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    v = np.asarray(verts, dtype=np.float64)
    rot = np.asarray(rot, dtype=np.float64)
    m, X, hl = len(L), int(x_cells), float(half_len)
    h = 2.0 * hl / float(m - 1)
    dx = 2.0 * float(x_half) / float(X - 1)
    xg = -float(x_half) + np.arange(X, dtype=np.float64) * dx
    u = -hl + np.arange(m, dtype=np.float64) * h
    T = len(rot)
    tl, tr = np.full((T, X), INF), np.full((T, X), INF)
    vx, vy = v[None, :, 0], v[None, :, 1]
    with np.errstate(all="ignore"):
        for a0 in range(0, T, rows):
            c, s = rot[a0:a0 + rows, 0:1], rot[a0:a0 + rows, 1:2]
            rx = c * vx - s * vy
            ry = s * vx + c * vy
            px = rx[:, None, :] + xg[None, :, None]                     # [rows][X][nv]
            py = np.broadcast_to(ry[:, None, :], px.shape)
            # set A: object vertices against the interpolated surfaces
            inr = (px >= -hl) & (px <= hl)
            t = (px + hl) / h
            jf = np.where(inr, np.minimum(np.floor(t), float(m - 2)), 0.0)
            j = jf.astype(np.int64)
            f = t - jf
            lp = L[j] + f * (L[j + 1] - L[j])
            up = U[j] + f * (U[j + 1] - U[j])
            bl = np.where(inr, py - lp, INF).min(axis=-1)
            br = np.where(inr, up - py, INF).min(axis=-1)
            # set B: finger samples against the object's edges
            qx, qy = np.roll(px, -1, axis=-1), np.roll(py, -1, axis=-1)
            j0 = np.maximum(np.ceil((np.minimum(px, qx) + hl) / h), 0.0)
            j1 = np.minimum(np.floor((np.maximum(px, qx) + hl) / h), float(m - 1))
            ok = (px != qx) & (j0 <= j1)
            slope = (qy - py) / (qx - px)
            j0i = np.where(ok, j0, 0.0).astype(np.int64)
            j1i = np.where(ok, j1, -1.0).astype(np.int64)
            d = 0
            while True:
                jj = j0i + d
                act = ok & (jj <= j1i)
                if not act.any():
                    break
                jc = np.where(act, jj, 0)
                ye = py + (u[jc] - px) * slope
                bl = np.minimum(bl, np.where(act, ye - L[jc], INF).min(axis=-1))
                br = np.minimum(br, np.where(act, U[jc] - ye, INF).min(axis=-1))
                d += 1
            tl[a0:a0 + rows], tr[a0:a0 + rows] = bl, br
        S = (tl + tr) / 2.0
    return tl, tr, S


def candidates(window: int):
    """The (da, db) of a successor search in visiting order: ascending (|db|, |da|, da, db)."""
    R = int(window)
    out = [(da, db) for da in range(-R, R + 1) for db in range(-R, R + 1) if (da, db) != (0, 0)]
    return sorted(out, key=lambda c: (abs(c[1]), abs(c[0]), c[0], c[1]))


def successors(S, window: int, travel_max: float) -> np.ndarray:
    """succ [theta * x_cells] int32: the cell each cell moves to (itself: a fixed point)."""
    S = np.asarray(S, dtype=np.float64)
    T, X = S.shape
    cell = np.arange(T * X, dtype=np.int64).reshape(T, X)
    best, succ = S.copy(), cell.copy()
    free = ~(S >= float(travel_max))
    b = np.arange(X)[None, :]
    for da, db in candidates(window):
        ok = free & (b + db >= 0) & (b + db < X)
        bb = np.clip(b + db, 0, X - 1)
        aa = (np.arange(T)[:, None] + da) % T
        cand = S[aa, bb]
        up = ok & (cand > best)
        best = np.where(up, cand, best)
        succ = np.where(up, cell[aa, bb], succ)
    return succ.reshape(-1).astype(np.int32)


def kth_successor(succ, k: int) -> np.ndarray:
    cur = np.arange(len(succ), dtype=np.int64)
    for _ in range(min(int(k), len(succ))):
        nxt = succ[cur]
        if np.array_equal(nxt, cur):
            break
        cur = nxt
    return cur.astype(np.int32)


def settled(succ) -> np.ndarray:
    return kth_successor(succ, len(succ))


def snap(starts, theta: int, x_cells: int, x_half: float) -> np.ndarray:
    """The cell a * x_cells + b nearest each start (theta0, x0, .): theta modulo 2 pi, x clamped, halves up."""
    st = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    T, X = int(theta), int(x_cells)
    with np.errstate(all="ignore"):
        dth = TWO_PI / float(T)
        q = np.floor(st[:, 0] / dth + 0.5)
        v = q - float(T) * np.floor(q / float(T))
        a = np.where((v >= 0.0) & (v < float(T)), v, 0.0).astype(np.int64)
        dx = 2.0 * float(x_half) / float(X - 1)
        w = np.floor((st[:, 1] + float(x_half)) / dx + 0.5)
        w = np.where(w >= 0.0, w, 0.0)                     # a NaN lands on cell 0
        b = np.where(w <= float(X - 1), w, float(X - 1)).astype(np.int64)
    return a * X + b


def pose_y(cells, y0, tl, tr, S, travel_max: float) -> np.ndarray:
    tl, tr, S = (np.asarray(t).reshape(-1)[cells] for t in (tl, tr, S))
    tm = float(travel_max)
    with np.errstate(all="ignore"):
        lo, hi = tm - tl, tr - tm
        y = np.asarray(y0, dtype=np.float64).copy()
        y = np.where(y < lo, lo, y)
        y = np.where(y > hi, hi, y)
        return np.where(S < tm, (tr - tl) / 2.0, y)


def squeeze_pair(lower, upper, verts, rot, starts, x_cells: int, x_half: float, window: int, closing_steps: int, travel_max: float,
                 half_len: float = 0.12) -> Dict[str, np.ndarray]:
    """Everything dgdm_squeeze_map returns for one pair: the three tables, succ, and per start cells (start, closed, settled), y
    (closed, settled) and flags."""
    tl, tr, S = touch_tables(lower, upper, verts, rot, x_cells, x_half, half_len)
    return map_outputs(tl, tr, S, successors(S, window, travel_max), starts, len(rot), x_cells, x_half, closing_steps, travel_max)


def map_outputs(tl, tr, S, succ, starts, T: int, x_cells: int, x_half: float, closing_steps: int, travel_max: float,
                jam=None) -> Dict[str, np.ndarray]:
    """From one pair's tables and successors to a map entry's outputs, the same for all three entries: the tables, succ, and per start
    cells (start, closed, settled), y (closed, settled) and flags 1 / 2 / 4.  jam [theta][x_cells] (friction; succ then holds its
    override): also returned, and flags carries 8 (the start cell is jammed) and 16 (the settled cell is)."""
    kth, fix = kth_successor(succ, closing_steps), settled(succ)
    st = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    c0 = snap(st, T, x_cells, x_half)
    ck, cf = kth[c0].astype(np.int64), fix[c0].astype(np.int64)
    Sf = S.reshape(-1)
    flags = (Sf[c0] >= travel_max) * 1 + (Sf[cf] >= travel_max) * 2 + ((cf % x_cells == 0) | (cf % x_cells == x_cells - 1)) * 4
    y = np.stack([pose_y(ck, st[:, 2], tl, tr, S, travel_max), pose_y(cf, st[:, 2], tl, tr, S, travel_max)], axis=1)
    out = {"touch_l": tl, "touch_r": tr, "S": S, "succ": succ, "cells": np.stack([c0, ck, cf], axis=1).astype(np.int32), "y": y}
    if jam is not None:
        jf = np.asarray(jam).reshape(-1)
        flags = flags + (jf[c0] != 0) * 8 + (jf[cf] != 0) * 16
        out["jam"] = jam
    out["flags"] = flags.astype(np.int32)
    return out


def squeeze_map(surfaces, objects, pairs: Sequence, rot, starts, **cfg) -> Dict[str, np.ndarray]:
    """squeeze_pair of every (finger, object) of `pairs`, stacked on a leading pair axis.  surfaces [F][2][m], objects [O][nv][2]."""
    outs = [squeeze_pair(surfaces[f][0], surfaces[f][1], objects[o], rot, starts, **cfg) for f, o in pairs]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def cell_pose(cells, theta: int, x_cells: int, x_half: float):
    """(theta in radians, x in metres) of cell indices."""
    c = np.asarray(cells, dtype=np.int64)
    dx = 2.0 * float(x_half) / float(x_cells - 1)
    return 2.0 * np.pi * (c // x_cells) / float(theta), -float(x_half) + (c % x_cells) * dx
