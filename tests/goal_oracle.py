"""Restatements for the goal-pose tests: the goal field in numpy, and cond_fn with a per-row field objective under torch.autograd."""
import os

import numpy as np
import torch

from oracle import dgdm_oracle as orc

GOLDEN_3D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "goal_mixed3d.npz")


def goal_field(s: orc.Setup, B: int, ori_range, goals, specs) -> np.ndarray:
    """include/dgdm_hip.h dgdm_guidance_goal_field in numpy: goals (n, B, 3) float32, specs [(weight (3,), ori_window, pos_window,
    profile 0 | 1), ...] -> (n, R, 3) float32.  Which pose a row has is the oracle's (orc._pose_grid: row r = cell * B + b), so the row order
    is checked with the values; the pose's value is the handle's own grid entry nearest to the oracle's (linspace_f32 below)."""
    ori, pos = orc._pose_grid(s, B, ori_range)
    go, gp = linspace_f32(ori_range[0], ori_range[1], s.grid_size), linspace_f32(-1.0, 1.0, s.num_pos)
    nearest = lambda v, grid: grid[np.abs(v.numpy().astype(np.float64).reshape(-1, 1) - grid.astype(np.float64)[None]).argmin(axis=1)]      # noqa: E731
    ori, pos = nearest(ori, go), np.stack([nearest(pos[:, 0], gp), nearest(pos[:, 1], gp)], axis=1)
    R = len(ori)
    b = np.arange(R) % B
    goals = np.asarray(goals, dtype=np.float32)
    out = np.empty((len(specs), R, 3), dtype=np.float32)
    for i, (weight, ori_window, pos_window, profile) in enumerate(specs):
        g = goals[i][b].astype(np.float64)                                               # (R, 3)
        u = np.stack([g[:, 0] - ori.astype(np.float64), g[:, 1] - pos[:, 0].astype(np.float64), g[:, 2] - pos[:, 1].astype(np.float64)], axis=1)
        u[:, 0] = np.where(u[:, 0] > 1.0, u[:, 0] - 2.0, np.where(u[:, 0] < -1.0, u[:, 0] + 2.0, u[:, 0]))
        h = np.array([np.float32(ori_window), np.float32(pos_window), np.float32(pos_window)], dtype=np.float64)
        if profile == 0:
            sgn = np.where((np.abs(u) > 0) & (np.abs(u) <= h), np.sign(u), 0.0)
        else:
            sgn = np.clip(u / h, -1.0, 1.0)
        out[i] = (np.asarray(weight, dtype=np.float32).astype(np.float64) * sgn).astype(np.float32)
    return out


def linspace_f32(start, end, steps) -> np.ndarray:
    """The handle's own float32 grid (csrc/guidance_api.hip linspace_f32: symmetric evaluation around the midpoint, every operation
    rounded to float32).  torch.linspace's vectorised CPU kernel fuses the multiply-add and differs from it in the last bit at some
    entries, which matters to a goal that lies ON a grid value - so the field is restated on these values, not on torch's."""
    start, end = np.float32(start), np.float32(end)
    if steps == 1:
        return np.array([start], dtype=np.float32)
    step = np.float32((end - start) / np.float32(steps - 1))
    half = steps // 2
    return np.array([start + step * np.float32(i) if i < half else end - step * np.float32(steps - i - 1) for i in range(steps)], dtype=np.float32)


def cond_fn_rows(s: orc.Setup, x, t, object_vertices, objective, ori_range=(-1.0, 1.0), starts=None):
    """d/dx of sum over sub-batches [i, j) of objective(logits[i:j], i, j), logits = orc.dyn{2,3}d_forward on orc._pose_grid's rows
    (torch.autograd).  3-D: `starts` = one classifier call's draws in cond_fn's layout (per sub-batch sa1's then sa2's); a row's
    embedding depends on its own two draws only, so the rows are evaluated in ONE forward call fed the per-row draws through
    orc.StartLog (cond_fn's 13 calls of 11 rows each cost 13 Python FPS loops), and the objective is still summed sub-batch by
    sub-batch, which is what 'convergence' depends on."""
    T = s.sched.num_train_timesteps
    with torch.enable_grad():
        x = x.detach().requires_grad_(True)
        B = x.shape[0]
        cells = s.grid_size * s.num_pos ** 2
        R = B * cells
        ori, pos = orc._pose_grid(s, B, ori_range)
        tt = t.repeat(cells).float() / T
        if s.mode == 'point':
            pts = x.repeat(cells, 1, 1).reshape(R, -1)
            logits = orc.dyn2d_forward(s.dyn, pts, ori, pos, tt, object_vertices.reshape(1, -1).expand(R, -1))
            return torch.autograd.grad(objective(logits, 0, R), x)[0]
        sub = s.sub_batch_size
        st = torch.as_tensor(np.asarray(starts, dtype=np.int64))
        s1, s2, o = [], [], 0
        for i in range(0, R, sub):
            n = min(sub, R - i)
            s1.append(st[o:o + n]); s2.append(st[o + n:o + 2 * n])
            o += 2 * n
        log = orc.StartLog([torch.cat(s1), torch.cat(s2)])
        logits = orc.dyn3d_forward(s.dyn, orc._pts3d(s, x).repeat(cells, 1, 1), ori, pos, tt, object_vertices.t().unsqueeze(0).expand(R, -1, -1), log)
        total = sum(objective(logits[i:min(i + sub, R)], i, min(i + sub, R)) for i in range(0, R, sub))
        return torch.autograd.grad(total, x)[0]


def cond_fn_named(s: orc.Setup, x, t, opt_obj, object_vertices, ori_range=(-1.0, 1.0), centers=None, starts=None):
    """orc.cond_fn's gradient for a reference objective name through cond_fn_rows (orc.deltas_to_objective per sub-batch)."""
    kw = dict(centers=centers, grid_size=s.grid_size, num_pos=s.num_pos)
    return cond_fn_rows(s, x, t, object_vertices, lambda l, i, j: orc.deltas_to_objective(l, opt_obj, **kw).sum(), ori_range, starts)


def cond_fn_field(s: orc.Setup, x, t, object_vertices, field, lin=(0.0, 0.0, 0.0), quad=(0.0, 0.0, 0.0), ori_range=(-1.0, 1.0), starts=None):
    """The row-field objective: sum_r [ sum_j field[r][j] * delta[r][j] + lin . delta[r] + quad . delta[r]^2 ]."""
    field = torch.as_tensor(field, dtype=torch.float32)
    lin, quad = torch.tensor(lin, dtype=torch.float32), torch.tensor(quad, dtype=torch.float32)
    return cond_fn_rows(s, x, t, object_vertices, lambda l, i, j: (l * field[i:j]).sum() + (l * lin).sum() + (l ** 2 * quad).sum(), ori_range, starts)


# ------------------------------------------------------------------------------------------------ the 3-D mixed launch
def mixed3d_case():
    """Inputs of tests/test_gpu_goal.py::test_mixed_launch_3d_against_autograd: the set-up of test_dyn3d_cond_fn_oracle_fps_paths (seed 44,
    objects 31 and 32 with exact duplicate points, sub = 11, N = 512) at B = 3, G = 5, P = 3 (45 cells = two tiles per finger, R = 135 rows,
    not a multiple of sub), four chains: a named objective, 'convergence', a random field, a random field + lin + quad."""
    from dgdm_amd import sampler, synth
    from tests import util
    B, G, P, L, T, sub = 3, 5, 3, 42, 15, 11
    dup = synth.synth_object_3d(32).clone()
    dup[9] = dup[400]
    dup[10] = dup[400]
    R = B * G * P * P
    torch.manual_seed(3)
    st = sampler.StartStream(512, sub)
    return dict(B=B, G=G, P=P, L=L, T=T, sub=sub, R=R, t=3, sd=util.dyn3d_sd(44), objs=torch.stack([synth.synth_object_3d(31), dup]),
                x=torch.stack([synth.synth_noise(60 + i, B, L) for i in range(4)]).clamp(-1, 1), starts=np.concatenate([st.call(R) for _ in range(4)]),
                centers=torch.tensor([1, 4, 2]), lin=(0.25, -0.5, 0.125), quad=(0.5, 0.0, -0.25),
                chains=[(0, 'rotate'), (1, 'convergence'), (1, 'field'), (0, 'field+')],
                field=torch.randn((4, R, 3), generator=torch.Generator().manual_seed(10)))


def mixed3d_reference(c) -> torch.Tensor:
    """The four chains' gradients (4, B, L, 1) by torch.autograd over the oracle (cond_fn_rows).  540 PointNet++ evaluations on the CPU:
    half a minute, which is why the test reads them from tests/golden/goal_mixed3d.npz (`python -m tests.goal_oracle` writes it)."""
    from tests import util
    s = util.setup('point_3d', None, c["sd"], c["T"], 5, c["L"], c["G"], c["P"], c["sub"])
    t = torch.full((c["B"],), c["t"], dtype=torch.int64)
    out = []
    for k, (oi, o) in enumerate(c["chains"]):
        st = c["starts"][k * 2 * c["R"]:(k + 1) * 2 * c["R"]]
        if o.startswith('field'):
            out.append(cond_fn_field(s, c["x"][k], t, c["objs"][oi], c["field"][k], *((c["lin"], c["quad"]) if o == 'field+' else ()), starts=st))
        else:
            out.append(cond_fn_named(s, c["x"][k], t, o, c["objs"][oi], (-1.0, 1.0), c["centers"] if o == 'convergence' else None, st))
    return torch.stack(out)


if __name__ == "__main__":
    case = mixed3d_case()
    np.savez_compressed(GOLDEN_3D, grads=mixed3d_reference(case).numpy(), starts=case["starts"], x=case["x"].numpy(), field=case["field"].numpy())
    print("wrote", GOLDEN_3D)
