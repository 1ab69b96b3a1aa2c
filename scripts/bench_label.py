"""Times the labelling pass (Guidance.label: one call over all batches, csrc/label.hip reductions) against the path a user had before it:
a Python loop of Guidance.score per padded batch plus torch reductions to the same ten columns.  Fingers labelled per second at user
sizes - 2-D: N = 4096 fingers on the configs[1] grid (B = 64, G = 360, P = 5, 4 objects); 3-D: N = 1024 on the configs[2] grid (B = 32,
G = 45, P = 5, sub_bs = 512, 6 objects).  Same process, same handle, warmed up; the two alternate, wall time between device
synchronisations (the loop's cost is partly host round trips, which device events would not see); medians over the repeats, and the
spread between repeats of the same code ((max - min) / median) printed beside them: a difference below that spread is not a difference.
python scripts/bench_label.py [--reps N] [--only 2d|3d]; one JSON line per workload.  --runner-only leaves the loop out: under
`rocprofv3 --kernel-trace --stats` the kernel table is then the runner's alone (the trunk's share of the time quoted in DESIGN.md 5)."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib, engine, sampler, synth

SHAPES = {"2d": dict(kind=2, fingers=4096, objects=4, B=64, G=360, P=5, L=14, N=100, sub=0, thr=[0.531, 0.769, 0.638]),
          "3d": dict(kind=3, fingers=1024, objects=6, B=32, G=45, P=5, L=42, N=512, sub=512, thr=[0.641, 0.625, 0.385])}


def loop_rows(gd, x, M, thr, starts, cells):
    """The parent path: per padded batch one Guidance.score and the ten columns by torch reductions (float64 on the device)."""
    N, B = x.shape[0], gd.cfg.batch
    out = torch.empty((N, 10), dtype=torch.float32, device=x.device)
    objs = list(range(M))
    for k in range(-(-N // B)):
        idx = torch.arange(k * B, (k + 1) * B, device=x.device).clamp(max=N - 1)
        counts, sums = gd.score(x[idx][None].expand(M, B, x.shape[1]).contiguous(), objs, thr, 0, None if starts is None else starts[k].reshape(-1))
        c = counts.to(torch.int64).sum(dim=0)                                   # (B, 3, 3, 3)
        k6 = torch.stack([c[:, 0].sum((1, 2)), c[:, 2].sum((1, 2)), c[:, :, 0].sum((1, 2)), c[:, :, 2].sum((1, 2)), c[:, :, :, 0].sum((1, 2)),
                          c[:, :, :, 2].sum((1, 2))], dim=1).double()
        rows = torch.cat([k6, sums.double().sum(dim=0)], dim=1) / float(M * cells)
        n = min(B, N - k * B)
        out[k * B:k * B + n] = rows[:n].float()
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(name, reps, runner_only=False):
    s = SHAPES[name]
    dev = torch.device("cuda:0")
    kind, M, B, L, N = s["kind"], s["objects"], s["B"], s["L"], s["fingers"]
    sd = synth.synth_state_dict(synth.dyn2d_spec(L, 2 * s["N"]) if kind == 2 else synth.dyn3d_spec(L), 22 if kind == 2 else 33)
    dyn = engine.Dynamics(kind, sd, L, 2 * s["N"] if kind == 2 else 0)
    objs = torch.stack([(synth.synth_object_2d(i, s["N"]) if kind == 2 else synth.synth_object_3d(i)) for i in range(M)]).to(dev)
    x = synth.synth_noise(7, N, L).reshape(N, L).clamp(-1, 1).to(dev)
    gd = engine.Guidance(dyn, B, s["G"], s["P"], (-1.0, 1.0), M, 15, s["N"], s["sub"], max_objects=M)
    gd.debug_fps_path(5)                              # 3-D: the embedding tables at set_objects, the steady state of both paths
    gd.set_objects(objs, wait=True)
    nb, cells = -(-N // B), s["G"] * s["P"] ** 2
    starts = sampler.TorchRng(seed=1).fps_starts(s["N"], s["sub"], gd.rows, n_calls=nb * M).reshape(nb, M, -1) if kind == 3 else None
    runner = lambda: gd.label(x, list(range(M)), s["thr"], 0, starts)           # noqa: E731
    loop = lambda: loop_rows(gd, x, M, s["thr"], starts, cells)                 # noqa: E731
    if runner_only:
        runner()
        t = [wall_ms(runner) for _ in range(reps)]
        print(json.dumps({"workload": name, "fingers": N, "objects": M, "batches": nb, "reps": reps, "runner_ms": float(np.median(t))}), flush=True)
        return None
    a, b = runner(), loop()
    torch.cuda.synchronize()
    agree = float((a.double() - b.double()).abs().max())                        # the loop's torch sums are not the contract's order: close, not equal
    t_r, t_l = [], []
    for _ in range(reps):                             # alternate so that drift of a shared machine lands on both
        t_r.append(wall_ms(runner)); t_l.append(wall_ms(loop))
    med = lambda v: float(np.median(v))               # noqa: E731
    spread = lambda v: float((max(v) - min(v)) / np.median(v))                  # noqa: E731
    out = {"workload": name, "fingers": N, "objects": M, "batch": B, "batches": nb, "rows_per_chain": B * cells, "reps": reps,
           "runner_ms": med(t_r), "loop_ms": med(t_l), "runner_fingers_per_s": N / med(t_r) * 1e3, "loop_fingers_per_s": N / med(t_l) * 1e3,
           "runner_spread": spread(t_r), "loop_spread": spread(t_l), "runner_over_loop": med(t_r) / med(t_l), "max_abs_diff_vs_loop": agree}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=list(SHAPES), default=None)
    ap.add_argument("--runner-only", action="store_true", help="time Guidance.label alone (for a kernel trace)")
    a = ap.parse_args()
    _lib.device_init(0)
    for n in ([a.only] if a.only else list(SHAPES)):
        run(n, a.reps, a.runner_only)
