"""Times Guidance.score against Guidance.grad on one handle per workload: ms per call at the BASELINE configs[1] shape (2-D: 4 chains x
B = 64 fingers, G = 360, P = 5) and the configs[2] shape (3-D: 32 chains x B = 32, G = 45, P = 5, sub_bs = 512, N = 512), in 'f32' (the
forward-only f16x3 trunk) and 'f32_mfma' (the float32 MFMA chain's forward-only form).  Same process, same handle, warmed up, median of
repeated timed calls between device events.  A call = the whole entry point (front end, 3-D start upload + embedding lookup, trunk,
tally / gradient tail), as a user pays for it.  python scripts/bench_score.py [--reps N] [--only 2d|3d]; prints one JSON line per
workload.  (Under `rocprofv3 --kernel-trace --stats` for the kernel breakdown quoted in DESIGN.md 5.)"""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib, engine, sampler, synth

SHAPES = {"2d": dict(kind=2, chains=4, B=64, G=360, P=5, L=14, N=100, sub=0, thr=[0.531, 0.769, 0.638]),
          "3d": dict(kind=3, chains=32, B=32, G=45, P=5, L=42, N=512, sub=512, thr=[0.641, 0.625, 0.385])}


def median_ms(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def run(name, reps):
    s = SHAPES[name]
    dev = torch.device("cuda:0")
    kind, nc, B, L = s["kind"], s["chains"], s["B"], s["L"]
    sd = synth.synth_state_dict(synth.dyn2d_spec(L, 2 * s["N"]) if kind == 2 else synth.dyn3d_spec(L), 22 if kind == 2 else 33)
    dyn = engine.Dynamics(kind, sd, L, 2 * s["N"] if kind == 2 else 0)
    objs = torch.stack([(synth.synth_object_2d(i, s["N"]) if kind == 2 else synth.synth_object_3d(i)) for i in range(nc)]).to(dev)
    x = torch.stack([synth.synth_noise(c, B, L).reshape(B, L) for c in range(nc)]).clamp(-1, 1).to(dev)
    objectives = [engine.make_objective('rotate' if c % 2 else 'shift_left', c) for c in range(nc)]
    out = {"workload": name, "chains": nc, "fingers": B, "rows_per_chain": B * s["G"] * s["P"] ** 2, "reps": reps}
    for mode in ("f32", "f32_mfma"):
        gd = engine.Guidance(dyn, B, s["G"], s["P"], (-1.0, 1.0), nc, 15, s["N"], s["sub"], max_objects=nc, contraction_dtype=mode)
        gd.debug_fps_path(5)                          # 3-D: the embedding tables at set_objects, the steady state of both calls
        gd.set_objects(objs, wait=True)
        starts = sampler.TorchRng(seed=1).fps_starts(s["N"], s["sub"], gd.rows, n_calls=nc).reshape(-1) if kind == 3 else None
        score = lambda: gd.score(x, list(range(nc)), s["thr"], 0, starts)              # noqa: E731
        grad = lambda: gd.grad(x, 0, objectives, None, starts)                         # noqa: E731
        for _ in range(3):
            score(); grad()
        torch.cuda.synchronize()
        # alternate the two in blocks so that drift of the shared machine lands on both
        t_s, t_g = [], []
        for _ in range(3):
            t_s.append(median_ms(score, reps)); t_g.append(median_ms(grad, reps))
        out[f"score_ms_{mode}"], out[f"grad_ms_{mode}"] = float(np.median(t_s)), float(np.median(t_g))
        out[f"score_over_grad_{mode}"] = out[f"score_ms_{mode}"] / out[f"grad_ms_{mode}"]
        del gd
    out["score_f32_over_score_f32_mfma"] = out["score_ms_f32"] / out["score_ms_f32_mfma"]
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=list(SHAPES), default=None)
    a = ap.parse_args()
    _lib.device_init(0)
    for n in ([a.only] if a.only else list(SHAPES)):
        run(n, a.reps)
