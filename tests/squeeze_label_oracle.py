"""Condition rows from the squeeze simulator, restated in numpy float64: the recipe of include/dgdm_hip.h "squeeze-simulator labels"
(dgdm_squeeze_label) line for line.  The maps the rows are made of are tests/squeeze_oracle.py's (squeeze_map / map_outputs) or, with
friction, tests/squeeze_friction_oracle.py's; the 64-lane stride and the xor butterfly are tests/resample_squeeze_oracle.py's wave_sum.

Pairs are finger-major: pair f * M + k is (finger f, objects[k]).  The first n_tally starts are tallied after one closing, the rest
are followed until they settle.  For a tally start:
  a = cell // X, b = cell % X of the start and the closed cell;  da = a_closed - a_start;  2 da > T: da -= T;  2 da < -T: da += T
  e0 = da * (6.283185307179586 / T);  e1 = (b_closed - b_start) * (2 x_half / (X - 1));  e2 = y_closed - y0
  class of e_j: 2 if e_j > thr_j, else 0 if e_j < -thr_j, else 1;  d_j = e_j / std_j
  per pair: class counts, and wave_sum of d0, |d0|, d1, d2
For a settle start, (a_s, b_s) the settled cell:
  (cos, sin) = rot[a_s];  px = (-x_half + b_s dx) / pos_norm;  py = y_settled / pos_norm;  r = sqrt(px px + py py)
  out = flag 4 or |px| > 1 or |py| > 1
  per pair: c = wave_sum(cos) / G, s = wave_sum(sin) / G, rho = sqrt(c c + s s), offset = wave_sum(r) / G, left = count(out) / G;
  a non-finite y_settled makes rho, c, s, offset NaN
A block ('mean': all M pairs of the finger, M' = M; 'per_object': one pair, M' = 1), pairs k ascending, n' = M' n_tally:
  0-5 float32(K / n');  6-9 float32((0.0 + s_k0 + s_k1 + ...) / n');  10-14 float32((0.0 + v_k0 + v_k1 + ...) / M')."""
import numpy as np

from tests import resample_squeeze_oracle as rso

TALLY_COLS, SETTLED_COLS = 10, 5


def pair_partials(cells, y, flags, starts, n_tally: int, rot, theta_cells: int, x_cells: int, x_half: float, threshold, score_std, pos_norm: float):
    """cells [P][N][3], y [P][N][2], flags [P][N] of a map over starts [N][3] -> per pair: cls [P][6] int64, sums [P][4], flag [P][3]
    int64, settle [P][5] (rho, c, s, offset, left; None without settle starts)."""
    c = np.asarray(cells, dtype=np.int64)
    y, fl = np.asarray(y, dtype=np.float64), np.asarray(flags, dtype=np.int64)
    st = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    rot = np.asarray(rot, dtype=np.float64)
    T, X, nt = int(theta_cells), int(x_cells), int(n_tally)
    thr, std = np.asarray(threshold, dtype=np.float64).reshape(3), np.asarray(score_std, dtype=np.float64).reshape(3)
    dth = rso.TWO_PI / float(T)
    dx = 2.0 * float(x_half) / float(X - 1)
    c0, ck = c[:, :nt, 0], c[:, :nt, 1]
    da = ck // X - c0 // X
    da = np.where(2 * da > T, da - T, da)
    da = np.where(2 * da < -T, da + T, da)
    with np.errstate(all="ignore"):
        e = [da.astype(np.float64) * dth, (ck % X - c0 % X).astype(np.float64) * dx, y[:, :nt, 0] - st[None, :nt, 2]]
        cls = np.zeros((c.shape[0], 6), dtype=np.int64)
        for j in range(3):
            hi = e[j] > thr[j]
            cls[:, 2 * j] = (~hi & (e[j] < -thr[j])).sum(axis=1)
            cls[:, 2 * j + 1] = hi.sum(axis=1)
        d0 = e[0] / std[0]
        sums = np.stack([rso.wave_sum(d0), rso.wave_sum(np.abs(d0)), rso.wave_sum(e[1] / std[1]), rso.wave_sum(e[2] / std[2])], axis=1)
    flag = np.stack([((fl[:, :nt] & b) != 0).sum(axis=1) for b in (1, 2, 4)], axis=1)
    G = c.shape[1] - nt
    if G == 0:
        return cls, sums, flag, None
    cf, ys = c[:, nt:, 2], y[:, nt:, 1]
    a_s, b_s = cf // X, cf % X
    with np.errstate(all="ignore"):
        xs = -float(x_half) + b_s.astype(np.float64) * dx
        px, py = xs / float(pos_norm), ys / float(pos_norm)
        r = np.sqrt(px * px + py * py)
        out = ((fl[:, nt:] & 4) != 0) | (np.abs(px) > 1.0) | (np.abs(py) > 1.0)
        cc, ss = rso.wave_sum(rot[a_s, 0]) / float(G), rso.wave_sum(rot[a_s, 1]) / float(G)
        rho = np.sqrt(cc * cc + ss * ss)
        off = rso.wave_sum(r) / float(G)
        left = out.sum(axis=1).astype(np.float64) / float(G)
    bad = ~np.isfinite(ys).all(axis=1)
    settle = np.stack([np.where(bad, np.nan, rho), np.where(bad, np.nan, cc), np.where(bad, np.nan, ss), np.where(bad, np.nan, off), left], axis=1)
    return cls, sums, flag, settle


def label_rows(cells, y, flags, starts, n_tally: int, n_objects: int, rot, theta_cells: int, x_cells: int, x_half: float, threshold, score_std,
               pos_norm: float, layout: str = "mean"):
    """-> (rows [F][gc] float32, counts [F][3] int32): gc = 10 (+5 with settle starts) for 'mean', M times that for 'per_object' (the
    blocks back to back)."""
    cls, sums, flag, settle = pair_partials(cells, y, flags, starts, n_tally, rot, theta_cells, x_cells, x_half, threshold, score_std, pos_norm)
    M = int(n_objects)
    F = cls.shape[0] // M
    assert F * M == cls.shape[0] and layout in ("mean", "per_object")
    cols = TALLY_COLS + (SETTLED_COLS if settle is not None else 0)
    blocks, per = (M, 1) if layout == "per_object" else (1, M)
    nn = float(per * int(n_tally))
    rows = np.zeros((F, blocks * cols), dtype=np.float32)
    with np.errstate(all="ignore"):
        for f in range(F):
            for blk in range(blocks):
                ks = [f * M + k for k in range(blk * per, (blk + 1) * per)]
                dst = rows[f, blk * cols:(blk + 1) * cols]
                K = cls[ks].sum(axis=0)
                dst[:6] = (K.astype(np.float64) / nn).astype(np.float32)
                for j in range(4):
                    s = 0.0
                    for k in ks:
                        s = s + sums[k, j]
                    dst[6 + j] = np.float32(s / nn)
                if settle is not None:
                    for j in range(5):
                        v = 0.0
                        for k in ks:
                            v = v + settle[k, j]
                        dst[TALLY_COLS + j] = np.float32(v / float(per))
    counts = flag.reshape(F, M, 3).sum(axis=1).astype(np.int32)
    return rows, counts
