"""Times the sliced squeeze (engine.squeeze_slice + engine.squeeze_tables_3d: csrc/squeeze.hip) at the 3-D dataset shape - theta_cells = 720,
x_cells = 241, the 25 x 25 finger grid, the 9000 start poses of sim/sim_3d.py, lobed vases of about 5000 triangles, 16 pairs (8 designs x
2 objects) - with device events around the calls: one warm-up, the median of --reps runs, ms per pair.  The table kernel's float64
operation count is tallied on the host from the candidate counts of the contract (+, -, x, / count 1 each; min, comparisons and the
searches count 0) on every --count-stride-th orientation and set against the vector float64 peak (78.6 TFLOP/s, AMD's figure for the
MI355X, which counts an FMA as 2 - this file is built without FMA contraction, so half of it is the most plain operations can reach).
  --oracle / --oracle-only   time the numpy oracle (tests/squeeze3d_oracle.py) on one pair on this host: the only baseline there is
  --tables-only              no starts (for a kernel trace: `rocprofv3 --kernel-trace --stats -- python scripts/bench_squeeze3d.py --reps 1`)
  --friction_3d MU           also time the call with Coulomb friction (dgdm_squeeze_map_3d_friction) and report ms_friction, the share of
                             jammed cells and of starts that settle jammed; --friction-only skips the frictionless call (for a kernel trace
                             of the friction call alone)
One JSON line."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib, engine
from dgdm_amd.sim import sim_2d, sim_3d, squeeze

PEAK_F64_VECTOR = 78.6e12


def vase(seed, rings=50, sectors=50, height=0.1):
    """A lobed surface of revolution standing on z = 0: rings x sectors x 2 triangles (no caps: they never cross a level)."""
    rs = np.random.RandomState(seed)
    z = np.linspace(0.0, height, rings + 1)
    a = 2.0 * np.pi * np.arange(sectors) / sectors
    r = 0.035 * (1.0 + 0.25 * np.cos(3 * a + rs.uniform(0, 6))[None, :] * np.cos(9.0 * z + rs.uniform(0, 6))[:, None]) * (1.0 + 0.3 * np.sin(25.0 * z + rs.uniform(0, 6)))[:, None]
    v = np.stack([r * np.cos(a), r * np.sin(a), np.broadcast_to(z[:, None], r.shape)], axis=-1).reshape(-1, 3)
    f = []
    for i in range(rings):
        for j in range(sectors):
            p, q, s, t = i * sectors + j, i * sectors + (j + 1) % sectors, (i + 1) * sectors + j, (i + 1) * sectors + (j + 1) % sectors
            f += [[p, q, t], [p, t, s]]
    return v, np.array(f, dtype=np.int32)


def count_ops(seg, off, gx, pairs, cfg, stride):
    """Float64 operations of table3d_kernel for these pairs, from the contract's candidate counts on every stride-th orientation."""
    T, X = cfg["theta_cells"], cfg["x_cells"]
    xg = -cfg["x_half"] + np.arange(X) * (2.0 * cfg["x_half"] / (X - 1))
    rot = engine.squeeze_rotation_table(T)[::stride]
    per_object = []
    for o in range(len(off)):
        s = seg[off[o, 0]:off[o, -1]]
        n_a = n_e = n_b = 0.0
        for c, sn in rot:
            px = (c * s[:, 0] - sn * s[:, 1])[None, :] + xg[:, None]
            qx = (c * s[:, 2] - sn * s[:, 3])[None, :] + xg[:, None]
            n_a += np.count_nonzero((px >= gx[0]) & (px <= gx[-1])) + np.count_nonzero((qx >= gx[0]) & (qx <= gx[-1]))
            lo, hi = np.minimum(px, qx), np.maximum(px, qx)
            cnt = np.where(px != qx, np.searchsorted(gx, hi, side="right") - np.searchsorted(gx, lo, side="left"), 0)
            n_e += np.count_nonzero(cnt > 0)
            n_b += float(cnt.sum())
        # as the kernel evaluates it: per (cell, segment) 2 (x + x_b of both ends); an end point in range 11; a slope 3; an abscissa 5
        ops = len(rot) * X * len(s) * 2 + n_a * 11 + n_e * 3 + n_b * 5 + len(rot) * X * 4
        per_object.append((ops * (T / len(rot)), n_a / (len(rot) * X), n_b / (len(rot) * X), len(s)))
    ops = sum(per_object[o][0] for _, o in pairs) + sum(T * 12 * per_object[o][3] for _, o in pairs)      # the rotation of each segment, once per workgroup
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
    ap.add_argument("--fingers", type=int, default=8)
    ap.add_argument("--objects", type=int, default=2)
    ap.add_argument("--count-stride", type=int, default=48)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--oracle-only", action="store_true", help="no GPU: time the numpy oracle on one pair")
    ap.add_argument("--tables-only", action="store_true")
    ap.add_argument("--friction_3d", type=float, default=None)
    ap.add_argument("--friction-only", action="store_true")
    a = ap.parse_args()
    cfg = {k: v for k, v in engine.SQUEEZE_DEFAULTS.items() if k != "finger_half_len"}
    meshes = [vase(i) for i in range(a.objects)]
    samples = np.stack([np.concatenate(sim_3d.gripper_design(g)) for g in range(a.fingers)]).astype(np.float32)
    pairs = squeeze.all_pairs(a.fingers, a.objects)
    starts = sim_2d.pose_grid()
    out = {"theta_cells": cfg["theta_cells"], "x_cells": cfg["x_cells"], "triangles": [len(f) for _, f in meshes], "grid": [25, 25], "starts": len(starts),
           "pairs": len(pairs)}
    if not a.oracle_only:
        _lib.device_init(0)
        gx, gz, sf = squeeze.finger_surfaces_3d(samples, 25, scale=1.0, offset=0.0)
        engine.squeeze_slice(meshes, gz)
        slice_ms = [event_ms(lambda: engine.squeeze_slice(meshes, gz)) for _ in range(a.reps)]
        sl = engine.squeeze_slice(meshes, gz)
        st = None if a.tables_only else torch.as_tensor(starts).cuda()
        rot = torch.as_tensor(engine.squeeze_rotation_table(cfg["theta_cells"])).cuda()
        run = lambda: engine.squeeze_tables_3d(sf, gx, sl["segments"], sl["offsets"], pairs, st, rot=rot, **cfg)      # noqa: E731
        if a.friction_3d is not None:
            sn = engine.squeeze_slice(meshes, gz, normals=True)
            fric = lambda **kw: engine.squeeze_tables_3d(sf, gx, sn["segments"], sn["offsets"], pairs, st, rot=rot, friction_3d=a.friction_3d, gz=gz,      # noqa: E731
                                                         normals=sn["normals"], **kw, **cfg)
            fric()
            fms = [event_ms(fric) for _ in range(a.reps)]
            if not a.friction_only:
                res = fric(jam=True)
                out.update({"jammed_cells": float(res["jam"].float().mean())})
                if st is not None:
                    out.update({"starts_settled_jammed": float((res["flags"] & 16).ne(0).float().mean())})
            out.update({"friction_3d": a.friction_3d, "ms_friction": float(np.median(fms)), "ms_friction_all": [round(v, 3) for v in fms]})
        if a.friction_only:
            print(json.dumps(out), flush=True)
            sys.exit(0)
        run()
        ms = [event_ms(run) for _ in range(a.reps)]
        med = float(np.median(ms))
        ops, n_a, n_b = count_ops(sl["segments"].cpu().numpy(), sl["offsets"], gx, pairs, cfg, a.count_stride)
        out.update({"reps": a.reps, "segments": np.diff(sl["offsets"][:, [0, -1]], axis=1).reshape(-1).tolist(), "slice_ms": float(np.median(slice_ms)),
                    "ms": med, "ms_all": [round(v, 3) for v in ms], "ms_per_pair": med / len(pairs), "pairs_per_s": len(pairs) / med * 1e3,
                    "table_f64_ops": ops, "set_a_candidates_per_cell": n_a, "set_b_candidates_per_cell": n_b,
                    "f64_ops_per_s_if_all_time_were_the_table_kernel": ops / med * 1e3, "share_of_vector_f64_peak": ops / med * 1e3 / PEAK_F64_VECTOR})
    if a.oracle or a.oracle_only:
        from tests import squeeze3d_oracle as so3
        gzh = 0.12 * np.arange(25) / 24
        gxh = np.linspace(-0.12, 0.12, 25) if a.oracle_only else gx
        sfh = np.stack([np.zeros((25, 25)) - 0.18, np.zeros((25, 25)) + 0.18]) if a.oracle_only else sf[0].cpu().numpy()
        t0 = time.perf_counter()
        seg, off = so3.slice_mesh(*meshes[0], gzh if a.oracle_only else gz)
        so3.squeeze_pair_3d(sfh[0], sfh[1], gxh, seg, off, so3.rotation_table(cfg["theta_cells"]), starts, cfg["x_cells"], cfg["x_half"], cfg["window"],
                            cfg["closing_steps"], cfg["travel_max"])
        sec = time.perf_counter() - t0
        out.update({"oracle_pairs_per_s": 1.0 / sec, "oracle_threads": 1, "oracle_host_cpus": os.cpu_count()})
    print(json.dumps(out), flush=True)
