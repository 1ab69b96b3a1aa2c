"""Cases and oracle side of tests/test_gpu_grad_shapes.py: the guidance gradient and its forward half across the sizes the handle accepts
(include/dgdm_hip.h, "accepted domain" of dgdm_dynamics_create / dgdm_guidance_create).  Nothing here touches the GPU: the GPU test, the
generator of the 3-D fixture (tests/golden/make_golden_grad_shapes.py) and the CPU tests that pin seeds and fixture share it.

Inputs.  Weights synth.synth_state_dict(spec, sd_seed); object i of a case synth.synth_object_2d / _3d(objs[i]); chain c's fingers
synth.synth_noise(xseeds[c], B, L).clamp(-1, 1).  The seeds are fixed: each x seed is the first one, counting up from the case's base, at
which the float64 oracle's smallest relative ReLU margin over the chain's rows and layers (orc.TRUNK_MARGIN) is at least MARGIN - so that
no float32 evaluation, the HIP kernels' and the oracle's own alike, resolves a ReLU the other way than float64 does
(`python -m tests.golden.make_golden_grad_shapes --search` reruns that search).

Objectives of a chain: a reference name (linear ones, 'rotate' = quadratic, 'convergence' with per-finger centres) or 'field' (a random
row field + lin + quad, engine.make_objective(None, oi, row_field=True, ...); float64 reference tests/goal_oracle.cond_fn_field)."""
import numpy as np
import torch

from dgdm_amd import synth
from oracle import dgdm_oracle as orc
from tests import goal_oracle, util

MARGIN = 5e-7
N3D = 512
NAMED4 = ('shift_left', 'rotate', 'clockwise_up', 'rotate_counterclockwise')
FIELD_LIN, FIELD_QUAD = (0.25, -0.5, 1.0), (0.5, 0.0, -0.25)
GOLDEN_3D = "g16_grad_shapes.npz"


def _case(dim, name, B, G, P, L, nc, objs, chain_obj, chain_goal, xseeds, sd_seed, nv=0, sub=0, T=15, t=6, ori=(-1.0, 1.0), bf16=False,
          distinct=None):
    """distinct: the chains that differ (a 256-chain launch repeats them: chain c has the inputs of chain c % distinct)."""
    d = dict(dim=dim, name=name, B=B, G=G, P=P, L=L, nc=nc, objs=objs, chain_obj=chain_obj, chain_goal=chain_goal, xseeds=xseeds,
             sd_seed=sd_seed, nv=nv, sub=sub, T=T, t=t, ori=ori, bf16=bf16, distinct=distinct or nc)
    d["C"] = G * P * P
    d["R"] = B * d["C"]
    assert len(chain_obj) == len(chain_goal) == len(xseeds) == d["distinct"] and max(chain_obj) < len(objs)
    return d


#                 name       B   G  P    L  nc  objects           object / objective / x seed of each chain
CASES_2D = [
    _case(2, "one_row",      1,  1, 1,   1,   1, [0],              [0], ['field'], [1000], 301, nv=1, t=0, bf16=True),
    _case(2, "c20_last_t",   3,  5, 2,   2,   2, [1, 2],           [0, 1], ['convergence', 'shift_left'], [1101, 1106], 302, nv=1, t=14, ori=(-0.5, 0.25)),
    _case(2, "one_tile",     1, 32, 1,  14,   1, [3],              [0], ['rotate'], [1201], 303, nv=100, bf16=True),
    _case(2, "tile_plus_1",  2, 33, 1,  17,   3, [4, 5, 6],        [0, 1, 2], ['clockwise_up', 'field', 'convergence'], [1301, 1302, 1304], 304, nv=33),
    _case(2, "L65_7fingers", 7,  3, 3,  65,   1, [7],              [0], ['counterclockwise_left'], [1400], 305, nv=5, ori=(0.0, 0.0), bf16=True),
    _case(2, "L256",         2, 11, 3, 256,   2, [8, 9],           [0, 1], ['field', 'rotate'], [1501, 1503], 306, nv=7),
    _case(2, "K256_T1000",   5,  7, 3, 100,   3, list(range(10, 19)), [0, 4, 8], ['shift_up', 'convergence', 'rotate'], [1607, 1618, 1602], 307, nv=128,
          T=1000, t=999),
    _case(2, "fold15",       3, 13, 6,  14,   3, [19, 20],         [0, 1, 0], ['convergence', 'field', 'shift_right'], [(1730, 1771, 1814), (1810, 1837, 1840), (1912, 1916, 1931)], 308, nv=100, bf16=True),
    _case(2, "chains256",    1,  3, 1,  14, 256, list(range(21, 30)), [c % 9 for c in range(36)], [NAMED4[c % 4] for c in range(36)],
          list(range(2000, 2033)) + [2036, 2034, 2035], 309, nv=10, distinct=36),
]

#                 name       B   G  P    L  nc  objects (object 2: every centre crowded; 1: none)
CASES_3D = [
    _case(3, "one_row",      1,  1, 1,   2,   1, [31],             [0], ['rotate_counterclockwise'], [2000], 401, sub=1, t=0, bf16=True),
    _case(3, "sub7_tail4",   3,  5, 2,   6,   2, [31, 32],         [0, 1], ['shift_left', 'rotate'], [2101, 2102], 402, sub=7, t=14),
    _case(3, "sub_gt_R",     1, 33, 1,  42,   1, [33],             [0], ['clockwise_up'], [2200], 403, sub=512, t=3, bf16=True),
    _case(3, "L256_split",   2,  9, 2, 256,   2, [1, 2],           [0, 1], ['rotate', 'counterclockwise_left'], [2300, 2303], 404, sub=64, t=3),
    _case(3, "chains256",    1,  1, 1,  14, 256, [31, 32],         [0, 1, 0, 1], list(NAMED4), [2400, 2401, 2402, 2403], 405, sub=1, t=3, distinct=4),
]
SMALLEST_3D = ("one_row", "chains256")          # regenerated and pinned to the fixture by tests/test_oracle_golden.py


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


def f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def state_dict(case):
    spec = synth.dyn2d_spec(case["L"], 2 * case["nv"]) if case["dim"] == 2 else synth.dyn3d_spec(case["L"])
    return synth.synth_state_dict(spec, case["sd_seed"])


def objects(case):
    return torch.stack([synth.synth_object_2d(i, case["nv"]) if case["dim"] == 2 else synth.synth_object_3d(i, N3D) for i in case["objs"]])


def fingers(case, seed):
    """A chain's fingers (B, L, 1): one seed for all of them, or a tuple with a seed per finger."""
    if isinstance(seed, tuple):
        return torch.cat([synth.synth_noise(s, 1, case["L"]) for s in seed]).clamp(-1, 1)
    return synth.synth_noise(seed, case["B"], case["L"]).clamp(-1, 1)


def x_all(case):
    """(distinct, B, L, 1) float32."""
    return torch.stack([fingers(case, s) for s in case["xseeds"]])


def centers(case, c):
    """'convergence' centres of chain c: one orientation cell per finger."""
    return torch.from_numpy(np.random.RandomState(7000 + 10 * case["sd_seed"] + c).randint(0, case["G"], case["B"]))


def field(case, c):
    """The row field of chain c, (R, 3) float32."""
    return torch.from_numpy(np.random.RandomState(8000 + 10 * case["sd_seed"] + c).standard_normal((case["R"], 3)).astype(np.float32))


def start_lens(case):
    R, sub = case["R"], case["sub"]
    return [n for r0 in range(0, R, sub) for n in (min(sub, R - r0),) * 2]


def starts(case, c):
    """FPS start draws of chain c's rows in cond_fn's layout: per sub-batch the sa1 draws in [0, 512), then the sa2 draws in [0, 128)."""
    rs = np.random.RandomState(9000 + 10 * case["sd_seed"] + c)
    return np.concatenate([rs.randint(0, N3D if i % 2 == 0 else 128, n) for i, n in enumerate(start_lens(case))]).astype(np.int64)


def _setup(case, sd):
    return util.setup('point' if case["dim"] == 2 else 'point_3d', None, sd, case["T"], 5, case["L"], case["G"], case["P"], case["sub"] or 1024)


def _log(case, st):
    return orc.StartLog(util.unpack_starts(st, start_lens(case))) if case["dim"] == 3 else None


def _cast(v, dtype):
    return v.to(dtype) if dtype == torch.float64 else v


def oracle_grad(case, sd, c, x, obj, dtype=torch.float32, st=None):
    """Chain c's gradient (B, L) by the oracle in `dtype` (sd already in that dtype), under whatever orc.contraction is in force."""
    s, goal = _setup(case, sd), case["chain_goal"][c]
    t = torch.full((case["B"],), case["t"], dtype=torch.int64)
    x, obj = _cast(x, dtype), _cast(obj, dtype)
    if goal == 'field':
        g = goal_oracle.cond_fn_field(s, x, t, obj, field(case, c), FIELD_LIN, FIELD_QUAD, case["ori"], st)
    else:
        g = orc.cond_fn(s, x, t, goal, obj, case["ori"], centers(case, c) if goal == 'convergence' else None, _log(case, st))
    return g.reshape(case["B"], case["L"])


def oracle_logits(case, sd, x, obj, dtype=torch.float32, st=None, want_margin=False):
    """The R rows' logits (R, 3), row = cell * B + finger, sub-batch by sub-batch as cond_fn calls the model; with want_margin also the
    smallest relative ReLU margin over the rows and layers of each finger, (B,) float64."""
    s = _setup(case, sd)
    B, C, R = case["B"], case["C"], case["R"]
    x, obj = _cast(x, dtype), _cast(obj, dtype)
    ori, pos = orc._pose_grid(s, B, case["ori"])
    tt = torch.full((B,), case["t"], dtype=torch.int64).repeat(C).float() / case["T"]
    orc.TRUNK_MARGIN = [] if want_margin else None
    try:
        with torch.no_grad():
            if case["dim"] == 2:
                out = orc.dyn2d_forward(sd, x.repeat(C, 1, 1).reshape(R, -1), ori, pos, tt, obj.reshape(1, -1).expand(R, -1))
            else:
                pts, cloud, log, sub = orc._pts3d(s, x).repeat(C, 1, 1), obj.t().unsqueeze(0), _log(case, st), case["sub"]
                out = torch.cat([orc.dyn3d_forward(sd, pts[i:i + sub], ori[i:i + sub], pos[i:i + sub], tt[i:i + sub],
                                                   cloud.expand(min(sub, R - i), -1, -1), log) for i in range(0, R, sub)])
        margin = torch.cat(orc.TRUNK_MARGIN).reshape(C, B).min(dim=0).values if want_margin else None
    finally:
        orc.TRUNK_MARGIN = None
    return (out, margin) if want_margin else out


def reference(case, bf16=None):
    """Every distinct chain of a case by the oracle: dict of stacked arrays
         g64, g32[, g16]  gradients (distinct, B, L) in float64 / float32 / under orc.contraction('bf16')
         l64, l32         logits (distinct, R, 3)
         margin           (distinct,) smallest relative ReLU margin of the float64 evaluation
         starts           3-D: (distinct, 2 R) int64."""
    bf16 = case["bf16"] if bf16 is None else bf16
    sd = state_dict(case)
    sd64, objs, xs = f64(sd), objects(case), x_all(case)
    out = {k: [] for k in ("g64", "g32", "l64", "l32", "margin")}
    if bf16:
        out["g16"] = []
    if case["dim"] == 3:
        out["starts"] = []
    for c in range(case["distinct"]):
        x, obj = xs[c], objs[case["chain_obj"][c]]
        st = starts(case, c) if case["dim"] == 3 else None
        l64, m = oracle_logits(case, sd64, x, obj, torch.float64, st, want_margin=True)
        out["l64"].append(l64)
        out["margin"].append(m.min())
        out["l32"].append(oracle_logits(case, sd, x, obj, torch.float32, st).double())
        out["g64"].append(oracle_grad(case, sd64, c, x, obj, torch.float64, st))
        out["g32"].append(oracle_grad(case, sd, c, x, obj, torch.float32, st).double())
        if bf16:
            with orc.contraction('bf16'):
                out["g16"].append(oracle_grad(case, sd, c, x, obj, torch.float32, st).double())
        if st is not None:
            out["starts"].append(torch.from_numpy(st))
    return {k: torch.stack(v) for k, v in out.items()}


def search_xseeds(case, tries=4000, width=64):
    """The hard-coded x seeds: per chain the first seed, counting up from the listed one, whose float64 margin is at least MARGIN.  A chain
    listed with a seed per finger (a row's margin depends on its own finger alone, and with more than a thousand rows per chain no
    single seed passes for all fingers at once): per finger the first such seed, `width` candidates evaluated per oracle call."""
    sd64, objs, found, used = f64(state_dict(case)), objects(case), [], set()
    for c in range(case["distinct"]):
        st, obj, first = starts(case, c) if case["dim"] == 3 else None, objs[case["chain_obj"][c]], case["xseeds"][c]
        if isinstance(first, tuple):
            wide = dict(case, B=width, R=width * case["C"])
            good, base = [], first[0]
            while len(good) < case["B"] and base < first[0] + tries:
                cand = tuple(range(base, base + width))
                _, m = oracle_logits(wide, sd64, fingers(wide, cand), obj, torch.float64, st, want_margin=True)
                good += [s for s, ok in zip(cand, (m >= MARGIN).tolist()) if ok and s not in used]
                base += width
            if len(good) < case["B"]:
                raise RuntimeError(f"{case['name']}: no seeds with margin >= {MARGIN} for chain {c}")
            found.append(tuple(good[:case["B"]]))
            used.update(found[-1])
            continue
        for seed in range(first, first + tries):
            if seed in used:
                continue
            _, m = oracle_logits(case, sd64, fingers(case, seed), obj, torch.float64, st, want_margin=True)
            if float(m.min()) >= MARGIN:
                found.append(seed)
                used.add(seed)
                break
        else:
            raise RuntimeError(f"{case['name']}: no seed with margin >= {MARGIN} for chain {c}")
    return found
