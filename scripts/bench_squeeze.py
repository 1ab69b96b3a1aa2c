"""Times the squeeze simulator (engine.squeeze_tables: csrc/squeeze.hip) at the dataset shape - theta_cells = 720, x_cells = 241, 100-vertex
contours, 200 surface samples, the 9000 start poses of sim/sim_2d.py, 64 pairs (8 designs x 8 objects) - with device events around the
call: one warm-up, the median of --reps runs, pairs per second.  The table kernel's float64 operation count is tallied on the host from
the candidate counts of the contract (+, -, x, / count 1 each; min, floor, ceil and comparisons count 0) on every --count-stride-th
orientation and set against the vector float64 peak (78.6 TFLOP/s, AMD's figure for the MI355X, which counts an FMA as 2 - this file is
built without FMA contraction, so half of it is the most plain operations can reach).
  --oracle            also time the numpy oracle (tests/squeeze_oracle.py) on one pair on this host: the only baseline there is
  --windows 1,2,3,5   also print the mean settled S over all cells for these windows, design 0 on object 0 scaled by 1.5 (DESIGN.md 4.1d's table)
  --friction MU       also time the call with Coulomb friction (dgdm_squeeze_map_friction) and report ms_friction, the share of jammed cells
                      and of starts that settle jammed; the operation count above is the frictionless kernel's
  --friction-only     with --friction: time only the friction call (for a kernel trace of its own)
  --tables-only       no starts (for a kernel trace: `rocprofv3 --kernel-trace --stats -- python scripts/bench_squeeze.py --reps 1`)
One JSON line."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib, engine, synth
from dgdm_amd.sim import sim_2d, squeeze

PEAK_F64_VECTOR = 78.6e12


def inputs(n_fingers=8, n_objects=8):
    samples = np.stack([np.concatenate(sim_2d.gripper_design(g)[1:]) for g in range(n_fingers)]).astype(np.float32)
    contours = np.stack([(synth.synth_object_2d(i, 100).double().numpy()) * squeeze.OBJECT_HALF_BOX_2D for i in range(n_objects)])
    return samples, contours


def count_ops(contours, pairs, cfg, m, stride):
    """Float64 operations of table_kernel for these pairs, from the contract's candidate counts on every stride-th orientation."""
    T, X, hl = cfg["theta_cells"], cfg["x_cells"], cfg["finger_half_len"]
    h, dx = 2.0 * hl / (m - 1), 2.0 * cfg["x_half"] / (X - 1)
    xg = -cfg["x_half"] + np.arange(X) * dx
    rot = engine.squeeze_rotation_table(T)[::stride]
    per_object = []
    for v in contours:
        rx = rot[:, 0:1] * v[None, :, 0] - rot[:, 1:2] * v[None, :, 1]
        px = rx[:, None, :] + xg[None, :, None]
        qx = np.roll(px, -1, axis=-1)
        n_a = np.count_nonzero((px >= -hl) & (px <= hl))
        j0 = np.maximum(np.ceil((np.minimum(px, qx) + hl) / h), 0.0)
        j1 = np.minimum(np.floor((np.maximum(px, qx) + hl) / h), m - 1.0)
        ok = (px != qx) & (j0 <= j1)
        n_e, n_b = np.count_nonzero(ok), float(np.where(ok, j1 - j0 + 1.0, 0.0).sum())
        # as the kernel evaluates it: per (cell, vertex) 1 (x + x_b) + 2 (t, shared by set A and the edges' ranges); set A 9; an edge's slope
        # 3; a finger sample 7; per cell 2 (x_b) + 2 (S)
        ops = px.size * 3 + n_a * 9 + n_e * 3 + n_b * 7 + px.shape[0] * X * 4
        per_object.append((ops * (T / len(rot)), n_a / (len(rot) * X), n_b / (len(rot) * X)))
    ops = sum(per_object[o][0] for _, o in pairs) + len(pairs) * T * 6 * contours.shape[1]       # the rotation of each vertex, once per workgroup
    return ops, float(np.mean([p[1] for p in per_object])), float(np.mean([p[2] for p in per_object]))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--count-stride", type=int, default=16)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--oracle-only", action="store_true", help="no GPU: time the numpy oracle on one pair")
    ap.add_argument("--windows", type=str, default="")
    ap.add_argument("--tables-only", action="store_true")
    ap.add_argument("--friction", type=float, default=None)
    ap.add_argument("--friction-only", action="store_true")
    a = ap.parse_args()
    cfg = dict(engine.SQUEEZE_DEFAULTS)
    samples, contours = inputs()
    pairs = squeeze.all_pairs(len(samples), len(contours))[:a.pairs]
    starts = sim_2d.pose_grid()
    out = {"theta_cells": cfg["theta_cells"], "x_cells": cfg["x_cells"], "vertices": 100, "surface_samples": 200, "starts": len(starts), "pairs": len(pairs)}
    if not a.oracle_only:
        _lib.device_init(0)
        sf = squeeze.finger_surfaces(samples, 200, 1.0, 0.0)
        ob = torch.as_tensor(contours).cuda()
        st = None if a.tables_only else torch.as_tensor(starts).cuda()
        rot = torch.as_tensor(engine.squeeze_rotation_table(cfg["theta_cells"])).cuda()
        run = lambda **kw: engine.squeeze_tables(sf, ob, pairs, st, rot=rot, **dict(cfg, **kw))      # noqa: E731
        if a.friction is not None:
            fric = lambda: run(friction=a.friction, jam=True)      # noqa: E731
            t = fric()
            fms = [event_ms(fric) for _ in range(a.reps)]
            out.update({"friction": a.friction, "ms_friction": float(np.median(fms)), "ms_friction_all": [round(v, 3) for v in fms],
                        "jammed_cell_share": float(t["jam"].double().mean())})
            if not a.tables_only:
                out["settled_jammed_share"] = float(((t["flags"] & 16) != 0).double().mean())
            if a.friction_only:
                print(json.dumps(out), flush=True)
                sys.exit(0)
        run()
        ms = [event_ms(run) for _ in range(a.reps)]
        med = float(np.median(ms))
        ops, n_a, n_b = count_ops(contours, pairs, cfg, 200, a.count_stride)
        out.update({"reps": a.reps, "ms": med, "ms_all": [round(v, 3) for v in ms], "pairs_per_s": len(pairs) / med * 1e3, "table_f64_ops": ops,
                    "set_a_candidates_per_cell": n_a, "set_b_candidates_per_cell": n_b,
                    "f64_ops_per_s_if_all_time_were_the_table_kernel": ops / med * 1e3, "share_of_vector_f64_peak": ops / med * 1e3 / PEAK_F64_VECTOR})
        if a.windows:
            res = {}
            for R in (int(v) for v in a.windows.split(",")):
                # object 0 scaled by 1.5 (9 to 15 cm across): at its own size it is narrower than 0.27 - 2 travel_max = 7 cm in places and loose there
                t = engine.squeeze_tables(sf, ob[:1] * 1.5, pairs[:1], None, rot=rot, tables=True, **dict(cfg, window=R))
                S, fix = t["S"].reshape(-1), t["succ"].reshape(-1).long()
                for _ in range(18):                       # 2^18 >= 720 x 241 cells: every path has ended
                    fix = fix[fix]
                res[R] = float(S[fix].mean())
            out["mean_settled_S_by_window"] = res
    if a.oracle or a.oracle_only:
        from tests import squeeze_oracle as so
        sfh = np.stack([np.zeros(200) - 0.12, np.zeros(200) + 0.15]) if a.oracle_only else sf[0].cpu().numpy()
        t0 = time.perf_counter()
        so.squeeze_pair(sfh[0], sfh[1], contours[0], so.rotation_table(cfg["theta_cells"]), starts, cfg["x_cells"], cfg["x_half"], cfg["window"],
                        cfg["closing_steps"], cfg["travel_max"], cfg["finger_half_len"])
        sec = time.perf_counter() - t0
        out.update({"oracle_pairs_per_s": 1.0 / sec, "oracle_threads": 1, "oracle_host_cpus": os.cpu_count()})
    print(json.dumps(out), flush=True)
