"""Times one evaluation of the 3-D squeeze potential (engine.squeeze_values_3d -> dgdm_squeeze_values_3d: table3d_fingers_kernel over
groups of a chain's fingers, then every chunk's tables reduced to objective values on the device) at the configs[2] chain shape: 32
chains x 32 fingers, G = 45, P = 5 (1125 starts), bench_squeeze3d.py's two lobed vases of 5000 triangles (chain k on vase k % 2), the
25 x 25 finger grid, window 2, 6 steps; one JSON line per table size: 720 x 241 (the squeeze defaults) and 360 x 121 (the table of the 2-D
README example).  Two lines on the same inputs, same process, one warm-up each, the repeats alternating so that drift of a shared
machine lands on both, device events around each run, medians and the spread between repeats of the same code ((max - min) / median; a
difference below the sum of the two spreads is not a difference):
  values   the new entry;
  route    what the library offered before it: engine.squeeze_tables_3d on the same pairs (table3d_kernel, one workgroup per (pair,
           theta), cells and y stored per start), then engine.squeeze_objective_values.
python scripts/bench_resample_squeeze_3d.py [--reps N] [--chains N] [--fingers N] [--guided-step-ms MS] [--values-only]; --guided-step-ms:
bench.py's milliseconds per guided step, to state an evaluation's cost in steps; --values-only times the entry alone (for
`rocprofv3 --kernel-trace --stats`)."""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib, engine, resample
from dgdm_amd.dynamics.dataloader import SCORE_STD
from dgdm_amd.sim import sim_3d, squeeze
import bench_squeeze_label as b2
from bench_squeeze3d import vase

G, P, M = 45, 5, 2
STD = [float(v) for v in SCORE_STD[0]]
NAMES = ['rotate', 'clockwise_up', 'shift_left', 'counterclockwise_down']


def run(n_chains, batch, cells, reps, step_ms=None, values_only=False):
    dev = torch.device("cuda:0")
    meshes = [vase(i) for i in range(M)]
    n_fingers = n_chains * batch
    samples = np.stack([np.concatenate(sim_3d.gripper_design(g)) for g in range(n_fingers)]).astype(np.float32)
    gx, gz, sf = squeeze.finger_surfaces_3d(samples, 25, scale=1.0, offset=0.0)
    sl = engine.squeeze_slice(meshes, gz)
    T, X = cells
    cfg = dict(theta_cells=T, x_cells=X)
    starts = torch.from_numpy(resample.start_grid(G, P, (-1.0, 1.0))).to(dev)
    rot = torch.from_numpy(engine.squeeze_rotation_table(T)).to(dev)
    objectives = [engine.make_objective(NAMES[k % len(NAMES)], k % M) for k in range(n_chains)]
    group_first = [k * batch for k in range(n_chains)]
    pairs = [(k * batch + b, k % M) for k in range(n_chains) for b in range(batch)]
    values = lambda: engine.squeeze_values_3d(sf, gx, sl["segments"], sl["offsets"], group_first, batch, objectives, starts, None, STD, rot=rot, **cfg)      # noqa: E731

    def route():
        m = engine.squeeze_tables_3d(sf, gx, sl["segments"], sl["offsets"], pairs, starts, rot=rot, **cfg)
        return engine.squeeze_objective_values(m["cells"], m["y"], starts, batch, objectives, None, STD, **cfg)
    base = {"chains": n_chains, "fingers_per_chain": batch, "pairs": len(pairs), "triangles": [len(f) for _, f in meshes], "grid": [25, 25],
            "segments": np.diff(sl["offsets"][:, [0, -1]], axis=1).reshape(-1).tolist(), "starts": G * P * P, "table": [T, X], "reps": reps}
    med = lambda v: float(np.median(v))               # noqa: E731
    spread = lambda v: float((max(v) - min(v)) / np.median(v))                  # noqa: E731
    a = values()
    if values_only:
        t = [b2.event_ms(values)[0] for _ in range(reps)]
        print(json.dumps(dict(base, values_ms=med(t), values_spread=spread(t), values_ms_per_pair=med(t) / len(pairs))), flush=True)
        return
    b = route()
    t = {"values": [], "route": []}
    for _ in range(reps):
        for name, fn in (("values", values), ("route", route)):
            t[name].append(b2.event_ms(fn)[0])
    out = dict(base, bit_identical_to_route=bool(torch.equal(a.view(torch.int64), b.view(torch.int64))))
    for name, v in t.items():
        out.update({f"{name}_ms": med(v), f"{name}_spread": spread(v), f"{name}_ms_per_pair": med(v) / len(pairs)})
    out["route_minus_values_ms"] = out["route_ms"] - out["values_ms"]
    out["spreads_ms"] = out["values_spread"] * out["values_ms"] + out["route_spread"] * out["route_ms"]
    out["values_is_faster"] = bool(out["route_minus_values_ms"] > out["spreads_ms"])      # the difference exceeds the sum of the two spreads
    if step_ms:
        out.update(guided_step_ms=float(step_ms), values_in_guided_steps=out["values_ms"] / float(step_ms))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--fingers", type=int, default=32)
    ap.add_argument("--guided-step-ms", type=float, default=None, help="bench.py's milliseconds per guided step")
    ap.add_argument("--values-only", action="store_true", help="time engine.squeeze_values_3d alone (for a kernel trace)")
    a = ap.parse_args()
    _lib.device_init(0)
    for cells in ((720, 241), (360, 121)):
        run(a.chains, a.fingers, cells, a.reps, a.guided_step_ms, a.values_only)
