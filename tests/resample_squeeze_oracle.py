"""Resampling fingers by the squeeze simulator's objective, restated in numpy: the two recipes of include/dgdm_hip.h (dgdm_ddim_pred_x0,
dgdm_squeeze_objective_values) line for line, and the start grid of dgdm_amd/resample.py (SqueezePotential).  The squeeze map the values
are made from is tests/squeeze_oracle.py's.

pred_x0:  x0 = fmin(fmax((x - sb * eps) / sa, -1), 1), every operation a float32 one rounded on its own (numpy float32 arrays do not
fuse); fmax / fmin return the other operand when one is a NaN, as fmaxf / fminf do.

values:   for pair p (finger p % B of group p // B) and start n, float64, every product, sum and quotient rounded on its own:
  a = cell // X, b = cell % X of the start and the closed cell;  da = a_closed - a_start;  2 da > T: da -= T;  2 da < -T: da += T
  d0 = (da * (6.283185307179586 / T)) / std0;  d1 = ((b_closed - b_start) * (2 x_half / (X - 1))) / std1;  d2 = (y_closed - y0) / std2
  t = ((l0 d0 + q0 (d0 d0)) + (l1 d1 + q1 (d1 d1))) + (l2 d2 + q2 (d2 d2)) [+ rowcoef[group][n * B + b] * d0]
  V[p]: 64 lanes, lane l adds n = l, l + 64, ... in ascending order from 0.0; then v += v[lane ^ s] for s = 32, 16, .., 1; lane 0."""
import numpy as np

TWO_PI = 6.283185307179586
POS_NORM = 0.03           # metres per unit of the dynamics model's position input


def pred_x0(x, eps, sqrt_abar, sqrt_1m_abar) -> np.ndarray:
    x, eps = np.asarray(x, dtype=np.float32), np.asarray(eps, dtype=np.float32)
    sa, sb = np.float32(sqrt_abar), np.float32(sqrt_1m_abar)
    with np.errstate(all="ignore"):
        prod = (sb * eps).astype(np.float32)
        diff = (x - prod).astype(np.float32)
        quot = (diff / sa).astype(np.float32)
        return np.fmin(np.fmax(quot, np.float32(-1.0)), np.float32(1.0)).astype(np.float32)


def deltas(cells, y, starts, theta_cells: int, x_cells: int, x_half: float, std):
    """(d0, d1, d2), each [n_pairs][n_starts] float64, of a squeeze map's cells [P][N][3] and y [P][N][2] over starts [N][3]."""
    c = np.asarray(cells, dtype=np.int64)
    y, st = np.asarray(y, dtype=np.float64), np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    T, X = int(theta_cells), int(x_cells)
    a0, b0, a1, b1 = c[..., 0] // X, c[..., 0] % X, c[..., 1] // X, c[..., 1] % X
    da = a1 - a0
    da = np.where(2 * da > T, da - T, da)
    da = np.where(2 * da < -T, da + T, da)
    dth = TWO_PI / float(T)
    dx = (2.0 * float(x_half)) / float(X - 1)
    with np.errstate(all="ignore"):
        d0 = (da.astype(np.float64) * dth) / float(std[0])
        d1 = ((b1 - b0).astype(np.float64) * dx) / float(std[1])
        d2 = (y[..., 0] - st[None, :, 2]) / float(std[2])
    return d0, d1, d2


def wave_sum(t) -> np.ndarray:
    """[P][N] -> [P]: the lane-strided sums and the xor butterfly of a 64-lane wave, literally."""
    t = np.asarray(t, dtype=np.float64)
    lanes = np.zeros((t.shape[0], 64))
    with np.errstate(all="ignore"):
        for n in range(t.shape[1]):                     # lane n % 64 takes its terms in ascending n
            lanes[:, n % 64] = lanes[:, n % 64] + t[:, n]
        idx = np.arange(64)
        for s in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ s]
    return lanes[:, 0].copy()


def objective_values(cells, y, starts, batch: int, objectives, rowcoef, std, theta_cells: int, x_cells: int, x_half: float) -> np.ndarray:
    """objectives: one per group, anything with .lin, .quad (three float32 each) and .use_rowcoef (0 or 1); rowcoef [groups][N * B]
    float32 or None -> V [n_pairs] float64."""
    d0, d1, d2 = deltas(cells, y, starts, theta_cells, x_cells, x_half, std)
    P, N = d0.shape
    B = int(batch)
    assert P % B == 0 and len(objectives) == P // B
    t = np.zeros((P, N))
    with np.errstate(all="ignore"):
        for p in range(P):
            o = objectives[p // B]
            assert int(o.use_rowcoef) in (0, 1)
            l, q = [float(np.float32(v)) for v in o.lin], [float(np.float32(v)) for v in o.quad]
            tp = ((l[0] * d0[p] + q[0] * (d0[p] * d0[p])) + (l[1] * d1[p] + q[1] * (d1[p] * d1[p]))) + (l[2] * d2[p] + q[2] * (d2[p] * d2[p]))
            if int(o.use_rowcoef) == 1:
                rc = np.asarray(rowcoef, dtype=np.float32).reshape(P // B, N * B)[p // B, np.arange(N) * B + p % B].astype(np.float64)
                tp = tp + rc * d0[p]
            t[p] = tp
    return wave_sum(t)


def start_grid(grid_size: int, num_pos: int, ori_range) -> np.ndarray:
    """The cells of cond_fn's pose grid (generator/diffusion.py:478) as squeeze starts [G P^2][3] = (theta0 rad, x0 m, y0 m), cell
    n = (io * P + ix) * P + iy: theta0 = (linspace(ori_lo, ori_hi, G)[io] + 1) * pi, x0 = POS_NORM * linspace(-1, 1, P)[ix], y0 likewise."""
    G, P = int(grid_size), int(num_pos)
    ori, pos = np.linspace(float(ori_range[0]), float(ori_range[1]), G), np.linspace(-1.0, 1.0, P)
    out = np.empty((G * P * P, 3))
    for io in range(G):
        for ix in range(P):
            for iy in range(P):
                out[(io * P + ix) * P + iy] = ((ori[io] + 1.0) * np.pi, POS_NORM * pos[ix], POS_NORM * pos[iy])
    return out
