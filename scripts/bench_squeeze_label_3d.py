"""Times the 3-D labelling entry (engine.squeeze_label_3d -> dgdm_squeeze_label_3d: table3d_fingers_kernel, then every chunk's tables
reduced to condition rows on the device) at the 3-D dataset shape: bench_squeeze3d.py's two lobed vases of 5000 triangles, the 25 x 25
finger grid, theta_cells = 720, x_cells = 241, window 2, 6 steps, on the configs[2] pose grid (G = 45, P = 5: 1125 tally starts, 45 settle
starts).  Three lines on the same fingers x objects, same process, one warm-up each, the repeats alternating so that drift of a shared
machine lands on all three, device events around each run, medians and the spread between repeats of the same code ((max - min) /
median; a difference below the spreads is not a difference):
  label    the new entry;
  route    what the library offered before it: engine.squeeze_tables_3d in chunks, the per-start outputs copied to the host and tallied
           in numpy (bench_squeeze_label.py's host_rows, with the 3-D threshold and std);
  tables   dgdm_squeeze_map_3d with no starts on the same pairs: table3d_kernel's cost per pair plus the successor and pointer-doubling
           launches both entries share - the yardstick for the finger-shared kernel.
python scripts/bench_squeeze_label_3d.py [--reps N] [--fingers N] [--label-only]; one JSON line.  --label-only times the entry alone
(for `rocprofv3 --kernel-trace --stats`)."""
import argparse, ctypes as C, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib, engine, resample
from dgdm_amd.dynamics.dataloader import SCORE_STD, SCORE_THRESHOLD
from dgdm_amd.sim import sim_3d, squeeze
import bench_squeeze_label as b2
from bench_squeeze3d import vase

G, P, M = 45, 5, 2
b2.M = M
b2.THR, b2.STD = [float(v) for v in SCORE_THRESHOLD[0]], [float(v) for v in SCORE_STD[0]]      # host_rows reads its module's


def run(n_fingers, reps, label_only=False):
    dev = torch.device("cuda:0")
    meshes = [vase(i) for i in range(M)]
    samples = np.stack([np.concatenate(sim_3d.gripper_design(g)) for g in range(n_fingers)]).astype(np.float32)
    gx, gz, sf = squeeze.finger_surfaces_3d(samples, 25, scale=1.0, offset=0.0)
    sl = engine.squeeze_slice(meshes, gz)
    starts_h = np.concatenate([resample.start_grid(G, P, (-1.0, 1.0)), squeeze.start_orientations(G, (-1.0, 1.0))])
    nt = G * P * P
    cfg = engine.squeeze_config()
    T, X = cfg.theta_cells, cfg.x_cells
    rot_h = engine.squeeze_rotation_table(T)
    starts, rot = torch.from_numpy(starts_h).to(dev), torch.from_numpy(rot_h).to(dev)
    objects = list(range(M))
    pairs = [(f, o) for f in range(n_fingers) for o in objects]
    per_finger = int(_lib.lib().dgdm_squeeze_label_3d_workspace_bytes(C.byref(cfg), 1, M, 25, 25, M))
    chunk = max(1, min(n_fingers, engine.SQUEEZE_WORKSPACE_BYTES // per_finger))          # the fingers the entry takes per chunk of its default workspace
    label = lambda: engine.squeeze_label_3d(sf, gx, sl["segments"], sl["offsets"], objects, starts, nt, b2.THR, b2.STD, rot=rot)[0]      # noqa: E731
    tables = lambda: engine.squeeze_tables_3d(sf, gx, sl["segments"], sl["offsets"], pairs, None, rot=rot)      # noqa: E731

    def route():
        rows = np.empty((n_fingers, 15), dtype=np.float32)
        for f0 in range(0, n_fingers, chunk):
            f1 = min(n_fingers, f0 + chunk)
            pr = [(f, o) for f in range(f1 - f0) for o in objects]
            out = engine.squeeze_tables_3d(sf[f0:f1], gx, sl["segments"], sl["offsets"], pr, starts, rot=rot)
            rows[f0:f1] = b2.host_rows(out, starts_h, nt, T, X, cfg.x_half, rot_h)
        return rows
    base = {"fingers": n_fingers, "objects": M, "pairs": len(pairs), "triangles": [len(f) for _, f in meshes], "grid": [25, 25],
            "segments": np.diff(sl["offsets"][:, [0, -1]], axis=1).reshape(-1).tolist(), "tally_starts": nt, "settle_starts": G, "table": [T, X],
            "fingers_per_chunk": chunk, "reps": reps}
    med = lambda v: float(np.median(v))               # noqa: E731
    spread = lambda v: float((max(v) - min(v)) / np.median(v))                  # noqa: E731
    if label_only:
        label()
        t = [b2.event_ms(label)[0] for _ in range(reps)]
        print(json.dumps(dict(base, label_ms=med(t), label_spread=spread(t), label_ms_per_pair=med(t) / len(pairs))), flush=True)
        return
    a, b = label().cpu().numpy(), route()
    tables()
    t = {"label": [], "route": [], "tables": []}
    for _ in range(reps):
        for name, fn in (("label", label), ("route", route), ("tables", tables)):
            t[name].append(b2.event_ms(fn)[0])
    out = dict(base, max_abs_diff_vs_route=float(np.abs(a.astype(np.float64) - b).max()))
    for name, v in t.items():
        out.update({f"{name}_ms": med(v), f"{name}_spread": spread(v), f"{name}_ms_per_pair": med(v) / len(pairs)})
    out["label_over_tables"] = out["label_ms"] / out["tables_ms"]
    out["label_over_route"] = out["label_ms"] / out["route_ms"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fingers", type=int, default=64)
    ap.add_argument("--label-only", action="store_true", help="time engine.squeeze_label_3d alone (for a kernel trace)")
    a = ap.parse_args()
    _lib.device_init(0)
    run(a.fingers, a.reps, a.label_only)
