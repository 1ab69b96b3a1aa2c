"""Times one evaluation of the squeeze simulator's potential for resampling (sampler.run_chains with
Resample(potential='squeeze')) - the eps-net call on the step's output, dgdm_ddim_pred_x0, the squeeze map over cond_fn's grid cells
(G = 45, P = 5: 1125 starts per pair, the configs[2] grid) and dgdm_squeeze_objective_values - with device events around each: one
warm-up, the median of --reps runs.  Shapes: (chains, fingers) = (4, 64) and (32, 32); tables: the squeeze defaults (720 x 241) and
360 x 121.  Synthetic eps-net weights, synthetic 100-vertex contours, random designs: the timings do not depend on the values.
`whole` is the sequence as run_chains issues it (SqueezePotential.values included); the parts are timed alone, so they need not add up
to it.  One JSON line per (shape, table).  Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_resample_squeeze.py --reps 1`
for the kernels."""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib, engine, synth
from dgdm_amd.dynamics.dataloader import SCORE_STD
from dgdm_amd.resample import SqueezePotential
from dgdm_amd.scheduler import DDIMScheduler
from dgdm_amd.sim import squeeze

G, P, ORI, L = 45, 5, (-1.0, 1.0), 14
NAMES = ['rotate', 'shift_up', 'clockwise_left', 'rotate_clockwise']


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps):
    fn()
    return float(np.median([event_ms(fn) for _ in range(reps)]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", type=str, default="4x64,32x32")
    ap.add_argument("--tables", type=str, default="720x241,360x121")
    a = ap.parse_args()
    _lib.device_init(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    net = engine.Unet1d(synth.synth_state_dict(synth.unet_spec(), 11))
    sched = DDIMScheduler(num_train_timesteps=100)
    sched.set_timesteps(5)
    t = int(sched.timesteps[1])
    contours = np.stack([synth.synth_object_2d(i, 100).double().numpy() * squeeze.OBJECT_HALF_BOX_2D for i in range(8)])
    std = tuple(float(v) for v in SCORE_STD[1])
    for shape in a.shapes.split(","):
        nc, B = (int(v) for v in shape.split("x"))
        x = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (nc, B, L)).astype(np.float32)).to(dev)
        ts = torch.full((nc * B,), t, dtype=torch.int32, device=dev)
        objectives = [engine.make_objective(NAMES[k % len(NAMES)], k % len(contours)) for k in range(nc)]
        for table in a.tables.split(","):
            T, X = (int(v) for v in table.split("x"))
            cfg = dict(theta_cells=T, x_cells=X)
            pot = SqueezePotential(contours, **cfg)
            eps_net = lambda: net.forward_cfg(x.reshape(nc * B, L, 1), ts, None, 1.0)                                   # noqa: E731
            eps = eps_net().reshape(nc, B, L).contiguous()
            pred = lambda: engine.ddim_pred_x0(x, eps, sched.coefficients(t)[:2])                                       # noqa: E731
            clean = pred()
            whole = lambda: pot.values(engine.ddim_pred_x0(x, eps_net().reshape(nc, B, L).contiguous(), sched.coefficients(t)[:2]), objectives,      # noqa: E731
                                       None, 1, G, P, ORI)
            whole()                                                   # the potential's bank, rotation table and starts are on the device now
            starts = pot.starts(G, P, ORI)
            pairs = np.stack([np.arange(nc * B, dtype=np.int32), np.repeat(np.array([int(o.object) for o in objectives], dtype=np.int32), B)], axis=1)
            smap = lambda: engine.squeeze_tables(squeeze.finger_surfaces(clean.reshape(nc * B, L)), pot._bank, pairs, starts, rot=pot._rot, **cfg)      # noqa: E731
            m = smap()
            vals = lambda: engine.squeeze_objective_values(m["cells"], m["y"], starts, B, objectives, None, std, **cfg)  # noqa: E731
            out = {"chains": nc, "fingers": B, "pairs": nc * B, "starts": G * P * P, "theta_cells": T, "x_cells": X, "reps": a.reps,
                   "whole_ms": median_ms(whole, a.reps), "eps_net_ms": median_ms(eps_net, a.reps), "pred_x0_ms": median_ms(pred, a.reps),
                   "squeeze_map_ms": median_ms(smap, a.reps), "objective_values_ms": median_ms(vals, a.reps)}
            out["pairs_per_s"] = nc * B / out["squeeze_map_ms"] * 1e3
            print(json.dumps(out), flush=True)
