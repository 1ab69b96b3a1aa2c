"""Forward-only scoring (engine.Guidance.score: csrc/trunk_f16l.hip forward-only form, csrc/score.hip tally) against the float64 CPU
oracle, and the predicted-simulator path end to end.

Yardstick: oracle/dgdm_oracle.py in float64 on the same rows, the same FPS starts, t = 0.  Tolerance of the logits: not fixed in
advance - the rows API of the parent code path (Dynamics.forward2d / forward3d, the float32 MFMA chain) is run on the same rows and its
maximum absolute error against the float64 oracle, e_ref, is measured live; the new path must stay within 2 x e_ref (the two arithmetics
are the same grade: 1.9e-7 against 2.0e-7 rms per 256-term contraction, csrc/trunk_f16l.hip; a maximum over the rows fluctuates).
delta = 2 x e_ref then decides which rows are 'undecided' for the class counts (a reference logit within delta of a threshold).

Thresholds and seeds were picked on the CPU with the oracle alone (float64 logits of the cases below): THR sits near the middle of the
logits' spread so that all three classes occur, and the share of rows within 1e-4 of a threshold - a hundred times the delta
expected - was 0 of 678 rows (2-D, both grids) and 0 of 316 (3-D, both grids); the cap the tests assert on the live delta is 1 %."""
import functools
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import engine, sampler, synth
from dgdm_amd._lib import DgdmError
from oracle import dgdm_oracle as orc
from tests import util

pytestmark = pytest.mark.gpu

T = 15
# (kind, B, G, P, chains): C = G P^2 cells per finger - 81 / 63 are not multiples of the 32-row tile (the last tile holds padding rows), 32 is
CASES = {"2d_pad": (2, 3, 9, 3, 2), "2d_full": (2, 3, 8, 2, 2), "3d_pad": (3, 2, 7, 3, 2), "3d_full": (3, 2, 8, 2, 1)}
THR = {2: [0.4, 0.7, 1.0], 3: [1.2, 0.3, 1.4]}          # threshold / std, the model's normalised units
SUB = 50
NV = 100


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def inputs(name):
    kind, B, G, P, nc = CASES[name]
    L = 14 if kind == 2 else 42
    sd = util.dyn2d_sd(22, NV) if kind == 2 else util.dyn3d_sd(33)
    objs = torch.stack([synth.synth_object_2d(i, NV) if kind == 2 else synth.synth_object_3d(50 + i) for i in range(2)])
    x = torch.stack([synth.synth_noise(80 + c, B, L).reshape(B, L) for c in range(nc)]).clamp(-1, 1)
    R = B * G * P * P
    starts = None
    if kind == 3:
        starts = sampler.TorchRng(seed=1234).fps_starts(512, SUB, R, n_calls=nc).reshape(-1)
    return kind, B, G, P, nc, L, sd, objs, x, R, starts


def sub_batches(R):
    return [(r0, min(SUB, R - r0)) for r0 in range(0, R, SUB)]


def row_starts(starts, c, R):
    """(sa1, sa2) per row of chain c from the [sub-batch: sa1 x n, sa2 x n] layout."""
    flat = starts[c * 2 * R:(c + 1) * 2 * R]
    s1 = np.concatenate([flat[2 * r0:2 * r0 + n] for r0, n in sub_batches(R)])
    s2 = np.concatenate([flat[2 * r0 + n:2 * r0 + 2 * n] for r0, n in sub_batches(R)])
    return s1, s2


def rows_of(name, c):
    """The classifier inputs of chain c's rows in cond_fn's order (generator/diffusion.py:478-491), float32."""
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    s = util.setup('point' if kind == 2 else 'point_3d', None, sd, T, 5, L, G, P, SUB)
    ori, pos = orc._pose_grid(s, B, (-1.0, 1.0))
    cells = G * P * P
    tt = torch.zeros(R)
    if kind == 2:
        return x[c].repeat(cells, 1), ori, pos, tt, objs[c % 2].reshape(1, -1).expand(R, -1).contiguous()
    return orc._pts3d(s, x[c].reshape(B, L, 1)).repeat(cells, 1, 1), ori, pos, tt, objs[c % 2].t().unsqueeze(0).expand(R, -1, -1).contiguous()


@functools.lru_cache(maxsize=None)
def oracle64(name):
    """float64 logits (chains, R, 3) of the case."""
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    sd64 = {k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()}
    out = []
    with torch.no_grad():
        for c in range(nc):
            a = [v.double() for v in rows_of(name, c)]
            if kind == 2:
                out.append(orc.dyn2d_forward(sd64, *a))
                continue
            log = orc.StartLog(util.unpack_starts(starts[c * 2 * R:(c + 1) * 2 * R], [n for _, n in sub_batches(R) for _ in range(2)]))
            out.append(torch.cat([orc.dyn3d_forward(sd64, *[v[r0:r0 + n] for v in a], log) for r0, n in sub_batches(R)]))
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def e_ref(name):
    """Maximum absolute error of the parent commit's rows API (float32 MFMA chain) on the same rows against the float64 oracle."""
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    dyn = engine.Dynamics(kind, sd, L, 2 * NV if kind == 2 else 0)
    dev = torch.device("cuda:0")
    err = 0.0
    for c in range(nc):
        a = [v.to(dev) for v in rows_of(name, c)]
        if kind == 2:
            got = dyn.forward2d(*a)
        else:
            s1, s2 = row_starts(starts, c, R)
            got = dyn.forward3d(*a, torch.from_numpy(s1), torch.from_numpy(s2))
        err = max(err, float((got.cpu().double() - oracle64(name)[c]).abs().max()))
    return err


@functools.lru_cache(maxsize=None)
def scored(name, mode):
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    dev = torch.device("cuda:0")
    dyn = engine.Dynamics(kind, sd, L, 2 * NV if kind == 2 else 0)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), nc, T, NV if kind == 2 else 512, SUB if kind == 3 else 0, max_objects=2, contraction_dtype=mode)
    gd.set_objects(objs.to(dev))
    oc = [c % 2 for c in range(nc)]
    counts, sums, logits = gd.score(x.to(dev), oc, THR[kind], timestep=0, starts=starts, want_logits=True)
    return gd, counts.cpu(), sums.cpu(), logits.cpu()


def ref_tally(name, delta):
    """Per (chain, finger): reference histogram and sums from the float64 logits, and the number of undecided rows."""
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    l = oracle64(name).reshape(nc, G * P * P, B, 3).transpose(1, 2)              # (chain, finger, cell, 3)
    thr = torch.tensor(THR[kind], dtype=torch.float32).double()
    cls = torch.where(l > thr, 2, torch.where(l < -thr, 0, 1))
    bins = (cls[..., 0] * 3 + cls[..., 1]) * 3 + cls[..., 2]
    counts = torch.stack([torch.stack([torch.bincount(bins[c, b], minlength=27) for b in range(B)]) for c in range(nc)]).reshape(nc, B, 3, 3, 3)
    sums = torch.stack([l[..., 0].sum(-1), l[..., 0].abs().sum(-1), l[..., 1].sum(-1), l[..., 2].sum(-1)], dim=-1)
    undecided = (((l - thr).abs() <= delta) | ((l + thr).abs() <= delta)).any(-1)
    return counts, sums, undecided.sum(-1), float(undecided.double().mean())


@pytest.mark.parametrize("mode", ["f32", "f32_mfma"])
@pytest.mark.parametrize("name", list(CASES))
def test_logits_counts_sums_vs_float64_oracle(dev, name, mode):
    """Tests 1-4 of the issue: logits within 2 x e_ref of the float64 oracle; every histogram bin within the finger's undecided rows,
    each histogram summing to C exactly; sums within C x delta; grids with and without padding rows in the last tile."""
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    C = G * P * P
    er = e_ref(name)
    gd, counts, sums, logits = scored(name, mode)
    err = float((logits.double() - oracle64(name)).abs().max())
    delta = 2.0 * er
    rc, rs, und, share = ref_tally(name, delta)
    print(f"[score] {name} {mode}: max |logit - f64| = {err:.3e}, e_ref (rows API, f32 MFMA chain) = {er:.3e}, bound 2 e_ref = {delta:.3e}, "
          f"undecided rows {share * 100:.3f} %, max |count - ref| = {int((counts - rc).abs().max())}, "
          f"max |sum - ref| = {float((sums.double() - rs).abs().max()):.3e} (bound {C * delta:.3e})")
    assert er > 0.0
    assert err <= delta, (err, er)
    assert share <= 0.01, share                                   # asserted on the reference: a bad seed fails loudly
    assert bool((counts.sum(dim=(2, 3, 4)) == C).all())
    assert bool(((counts - rc).abs() <= und[..., None, None, None]).all())
    assert bool(((sums.double() - rs).abs() <= C * delta).all())


@pytest.mark.parametrize("name", ["2d_pad", "3d_pad"])
def test_no_logit_outside_the_buffer(dev, name):
    """The padding rows of a finger's last tile are not written: a guard region behind [0, chains x R) keeps its fill value, and the
    rows inside are all written.  (C ABI called directly: the guard lives in the caller's buffer.)"""
    import ctypes as C
    from dgdm_amd._lib import check, dptr, lib, stream_ptr
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    gd, counts, sums, logits = scored(name, "f32")
    fill, guard = -12345.0, 4096
    buf = torch.full((nc * R * 3 + guard,), fill, dtype=torch.float32, device=dev)
    c2 = torch.empty((nc, B, 27), dtype=torch.int32, device=dev)
    s2 = torch.empty((nc, B, 4), dtype=torch.float32, device=dev)
    xd = x.to(dev).contiguous()
    oc = (C.c_int32 * nc)(*[c % 2 for c in range(nc)])
    thr = (C.c_float * 3)(*THR[kind])
    check(lib().dgdm_guidance_score(gd._h, dptr(xd), 0, oc, starts.ctypes.data if starts is not None else None, thr, nc, dptr(buf), dptr(c2), dptr(s2),
                                    stream_ptr()))
    out = buf.cpu()
    assert bool((out[nc * R * 3:] == fill).all())
    assert torch.equal(out[:nc * R * 3].reshape(nc, R, 3), logits) and torch.equal(c2.cpu().reshape(counts.shape), counts)


@pytest.mark.parametrize("name", ["2d_pad", "3d_pad"])
def test_determinism_and_modes_agree(dev, name):
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    gd, counts, sums, logits = scored(name, "f32")
    again = gd.score(x.to(dev), [c % 2 for c in range(nc)], THR[kind], timestep=0, starts=starts, want_logits=True)
    assert torch.equal(again[0].cpu(), counts) and torch.equal(again[1].cpu(), sums) and torch.equal(again[2].cpu(), logits)
    quiet = gd.score(x.to(dev), [c % 2 for c in range(nc)], THR[kind], timestep=0, starts=starts)           # logits in the handle's scratch
    assert len(quiet) == 2 and torch.equal(quiet[0].cpu(), counts) and torch.equal(quiet[1].cpu(), sums)
    _, counts_m, _, _ = scored(name, "f32_mfma")
    _, _, und, _ = ref_tally(name, 2.0 * e_ref(name))
    assert bool(((counts - counts_m).abs() <= und[..., None, None, None]).all())


def test_bf16_handle_is_refused(dev):
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs("2d_full")
    dyn = engine.Dynamics(2, sd, L, 2 * NV)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), nc, T, NV, 0, max_objects=2, contraction_dtype="bf16")
    gd.set_objects(objs.to(dev))
    with pytest.raises(DgdmError, match=r"error -1: .*bf16"):                   # DGDM_EINVAL
        gd.score(x.to(dev), [0, 1], THR[2])


@pytest.mark.parametrize("name", ["2d_pad", "3d_pad"])
def test_grad_is_untouched_by_score(dev, name):
    kind, B, G, P, nc, L, sd, objs, x, R, starts = inputs(name)
    gd, _, _, _ = scored(name, "f32")
    objectives = [engine.make_objective(o, c % 2) for c, o in zip(range(nc), ('rotate', 'counterclockwise_left'))]
    before = gd.grad(x.to(dev), 3, objectives, None, starts).cpu()
    state = torch.get_rng_state()
    gd.score(x.to(dev), [c % 2 for c in range(nc)], THR[kind], timestep=0, starts=starts)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(gd.grad(x.to(dev), 3, objectives, None, starts).cpu(), before)


@pytest.mark.parametrize("fingers_3d", [False, True])
def test_predicted_sim_end_to_end(dev, tmp_path, fingers_3d):
    """A reduced validation_step through the command-line entry point: with --predicted_sim the unguided / guided / multi-object tables
    are written (scores marked predicted) and nothing is skipped; without it the run writes the `skipped` line as before; the sampled
    designs are bit-identical either way and scoring leaves the global CPU generator where the sampling left it."""
    import json
    from dgdm_amd.generator.train import train
    from dynamics.parser import parse
    shape = ("--fingers_3d --object_max_num_vertices=512 --ctrlpts_dim=42 --sub_bs=40" if fingers_3d else "--object_max_num_vertices=100 --ctrlpts_dim=14")
    common = (f"--mode=test --classifier_guidance {shape} --num_fingers=2 --batch_size=2 --grid_size=3 --num_pos=3 "
              f"--num_train_timesteps=15 --num_inference_steps=2")
    runs, states = {}, {}
    for tag, extra in (("off", ""), ("on", " --predicted_sim")):
        torch.manual_seed(7)
        _, runs[tag] = train(parse(shlex.split(common + extra + f" --save_dir={tmp_path / tag}")))
        states[tag] = torch.get_rng_state()
    assert runs["on"][0].keys() == runs["off"][0].keys()
    for k, v in runs["off"][0].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, runs["on"][0][k]), k
    assert torch.equal(states["on"], states["off"])
    assert "simulator" in open(tmp_path / "off" / "tables" / "SKIPPED.txt").read() and len(os.listdir(tmp_path / "off" / "tables")) == 1
    tables = sorted(os.listdir(tmp_path / "on" / "tables"))
    assert "SKIPPED.txt" not in tables
    assert len([t for t in tables if t.startswith("val__unguided_sample__")]) == 12
    assert len([t for t in tables if t.startswith("val__guided_sample__allobj_")]) == 11
    assert len([t for t in tables if t.startswith("val__guided_sample__") and "allobj" not in t]) == 12
    for t in tables:
        tab = json.load(open(tmp_path / "on" / "tables" / t))
        oc = tab["columns"].index("objective")
        scores = [row[oc] for row in tab["data"] if isinstance(row[oc], dict) and row[oc].get("predicted")]
        assert tab["data"] and scores, t
    with pytest.raises(ValueError, match="even"):
        train(parse(shlex.split(common.replace("--num_pos=3", "--num_pos=2") + f" --predicted_sim --save_dir={tmp_path / 'even'}")))
