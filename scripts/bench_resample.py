"""What an evaluation of `resample` costs: the BASELINE configs[2] grid (3-D: 32 chains x B = 32 fingers, G = 45, P = 5, sub_bs = 512,
N = 512, T = 15 / S = 5) through the walk (sampler.run_chains(stepwise=True)), eta = 0.5 - ms per denoise step without `resample` and with
Resample(every=1) (S - 1 evaluations in S steps: a forward-only trunk call, the values and the resampling step each), in ONE process on
one device, the two alternated; and the share of the two new calls (objective_values; chain_resample = weight / resample + gather) in that
step, timed alone on the run's own shapes between device events - launch gaps included; the kernels' own time comes from a separate run
under `rocprofv3 --kernel-trace --stats` (objective_values_kernel, resample_kernel, gather_kernel).  Synthetic weights and objects: a
cost, not an outcome.  python scripts/bench_resample.py [--reps N]; prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib, engine, sampler, synth
from dgdm_amd.resample import Resample
from dgdm_amd.scheduler import DDIMScheduler

SHAPE = dict(chains=32, B=32, G=45, P=5, L=42, N=512, sub=512, T=15, S=5)


def main(reps):
    s, dev = SHAPE, torch.device("cuda:0")
    nc, B, L, S = s["chains"], s["B"], s["L"], s["S"]
    net = engine.Unet1d(synth.synth_state_dict(synth.unet_spec(), 11))
    dyn = engine.Dynamics(3, synth.synth_state_dict(synth.dyn3d_spec(L), 33), L)
    gd = engine.Guidance(dyn, B, s["G"], s["P"], (-1.0, 1.0), nc, s["T"], s["N"], s["sub"], max_objects=nc)
    gd.debug_fps_path(5)                                  # the embedding tables at set_objects: the steady state of every call
    gd.set_objects(torch.stack([synth.synth_object_3d(i) for i in range(nc)]).to(dev), wait=True)
    sched = DDIMScheduler(num_train_timesteps=s["T"])
    sched.set_timesteps(S)
    x0 = synth.synth_noise(0, B, L).reshape(B, L).to(dev)
    chains = [(c, 'rotate' if c % 2 else 'shift_left') for c in range(nc)]
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    rs = Resample(1, 1.0, 0.5)
    n_eval = len(rs.evaluations(S))
    _, steps, pot = sampler.draw_chain_starts(gd, chains, S, sampler.pair_stream(s["N"], s["sub"], 1, 0), n_potential=n_eval)
    scales = [sampler.chain_scale('point_3d', o) for _, o in chains]
    log = []

    def run(resample):
        del log[:]
        t0 = time.perf_counter()
        out = sampler.run_chains(net, gd, sched, x0, nc, 1, objectives, None, steps, sched.timesteps, scales, stepwise=True, eta=0.5, noise_seed=3,
                                 resample=resample, resample_log=log, resample_starts=pot if resample is not None else None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / S, out

    for _ in range(2):
        run(None); run(rs)
    plain, with_rs = [], []
    for _ in range(reps):                                 # alternated, so that drift of a shared machine lands on both
        plain.append(run(None)[0]); with_rs.append(run(rs)[0])
    resamples = int(sum(int(d.sum()) for _, _, d, _ in log))
    # the three new kernels alone, on the shapes of the run
    x = run(None)[1]
    logits = gd.score(x, [oi for oi, _ in chains], (1.0, 1.0, 1.0), 3, pot[0].reshape(-1), want_logits=True)[2]
    keys = list(range(nc))

    def new_kernels():
        v = gd.objective_values(logits, objectives, None)
        engine.chain_resample(x, v, 1, rs.beta / (gd.rows // B), 2.0, 3, keys, 0, torch.zeros_like(v), torch.zeros_like(v))

    for _ in range(3):
        new_kernels()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for a, b in ev:
        a.record(); new_kernels(); b.record()
    torch.cuda.synchronize()
    k_ms = float(np.median([a.elapsed_time(b) for a, b in ev]))
    p, w = float(np.median(plain)), float(np.median(with_rs))
    print(json.dumps({"workload": "3d configs[2] grid through the walk", "chains": nc, "fingers": B, "rows_per_chain": gd.rows, "steps": S, "eta": 0.5,
                      "evaluations_per_run": n_eval, "resamples_last_run": resamples, "reps": reps, "ms_per_step_plain": p, "ms_per_step_resample_every_1": w,
                      "ms_per_evaluation": (w - p) * S / n_eval, "new_calls_ms_per_evaluation": k_ms,
                      "new_calls_share_of_step": k_ms * n_eval / S / w, "device": torch.cuda.get_device_name(0),
                      "date": time.strftime("%Y-%m-%d")}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    _lib.device_init(0)
    main(a.reps)
