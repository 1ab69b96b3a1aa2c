"""Predicted roll-outs (engine.Guidance.rollout: csrc/rollout.hip around the per-row pose form of the forward-only f16x3 trunk) against
the float64 CPU oracle, and the predicted simulator with --predicted_rollout end to end.

Semantics under test (include/dgdm_hip.h, dgdm_guidance_rollout): state (ori, pos_x, pos_y) per row r = g * B + b in float64, start =
the sweep's poses; per interaction the state rounded to float32, the model at t = 0, then in double ori += l0 std0 / pi wrapped into
[-1, 1], pos += l std / 0.03, left = the first interaction after which |pos| > 1.

Yardsticks.  (1) One interaction at a time: oracle/dgdm_oracle.py in float64 on the device's own poses (rounded to float32), the same
FPS draws; tolerance not fixed in advance - the rows API of the parent code path (Dynamics.forward2d / forward3d, the float32 MFMA
chain) runs on the same rows, its maximum error against the same oracle, e_ref, is measured live and the new path must stay within
2 x e_ref (the two arithmetics are the same grade; a maximum over rows fluctuates).  The update is recomputed in numpy float64 and must
agree within 1e-14.  (2) Free-running: the float64 oracle iterated on the CPU (T64), the float32 oracle iterated the same way (T32: the
reference's own arithmetic, no HIP input) and the device; rows whose T64 orientation comes within 1e-3 of +-1 right after an update,
before wrapping, are excluded from then on (the embedding is discontinuous across the wrap: such a row may wrap on one side only), their
share asserted <= 10 %; on the rest max |device - T64| <= 4 x max |T32 - T64| per interaction (4, not 2: the deviation accumulates and
the per-step maxima sit on different rows).

Seeds were checked on the CPU with the oracle alone (T64 of the cases below): rows that leave |pos| <= 1 within K interactions 20 of
54, 64 of 128, 80 of 160 (2-D), none in 3-D; updates that wrap 13 / 11 / 13 and 4 / 2; excluded rows 3.7 % / 0 % / 0.6 % and 7.1 % / 0 %
- under the 10 % cap, so `left` and the wrap are both exercised without special inputs.  Measured values: DESIGN.md 4.1a."""
import functools
import json
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import engine, sampler, synth
from dgdm_amd._lib import DgdmError
from dgdm_amd.dynamics.dataloader import POS_NORM, SCORE_STD
from oracle import dgdm_oracle as orc
from tests import util

pytestmark = pytest.mark.gpu

T = 15
SUB = 50
NV = 100
P = 1           # positions of the handle's cond_fn grid (not part of a roll-out; grad / score on it serve the isolation test)
# (kind, B, G, chains, K): G = 9 / 7 one padded tile, 32 one full tile, 40 / 33 a full tile and a padded one
CASES = {"2d_pad": (2, 3, 9, 2, 6), "2d_full": (2, 2, 32, 2, 6), "2d_mixed": (2, 2, 40, 2, 6), "3d_pad": (3, 2, 7, 2, 3), "3d_mixed": (3, 2, 33, 1, 3)}
STD = {2: [float(v) for v in SCORE_STD[1]], 3: [float(v) for v in SCORE_STD[0]]}
THR = {2: [0.4, 0.7, 1.0], 3: [1.2, 0.3, 1.4]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def scale_of(kind):
    s = STD[kind]
    return np.array([s[0] / np.pi, s[1] / POS_NORM, s[2] / POS_NORM], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def inputs(name):
    kind, B, G, nc, K = CASES[name]
    L = 14 if kind == 2 else 42
    sd = util.dyn2d_sd(22, NV) if kind == 2 else util.dyn3d_sd(33)
    objs = torch.stack([synth.synth_object_2d(i, NV) if kind == 2 else synth.synth_object_3d(50 + i) for i in range(2)])
    x = torch.stack([synth.synth_noise(80 + c, B, L).reshape(B, L) for c in range(nc)]).clamp(-1, 1)
    Rs = B * G
    starts = None
    if kind == 3:
        starts = sampler.TorchRng(seed=1234).fps_starts(512, SUB, Rs, n_calls=K * nc).reshape(K, nc, 2 * Rs)
    return kind, B, G, nc, K, L, sd, objs, x, Rs, starts


def sub_batches(R):
    return [(r0, min(SUB, R - r0)) for r0 in range(0, R, SUB)]


def row_starts(flat, R):
    """(sa1, sa2) per row from one chain's [sub-batch: sa1 x n, sa2 x n] layout."""
    s1 = np.concatenate([flat[2 * r0:2 * r0 + n] for r0, n in sub_batches(R)])
    s2 = np.concatenate([flat[2 * r0 + n:2 * r0 + 2 * n] for r0, n in sub_batches(R)])
    return s1, s2


def sweep_orientations(G):
    """The orientation grid of the handle's sweep (csrc/guidance_api.hip linspace_f32), stated independently: linspace(-1, 1, G) in
    float32 evaluated symmetrically around the midpoint, every product and sum rounded on its own.  torch.linspace follows the same
    rule one value at a time; where it fills a whole vector register from one base value it may differ from this by one float32 ulp
    at some g - the start of a roll-out is the SWEEP's grid, so that interaction 0 is the sweep."""
    lo, hi = np.float32(-1.0), np.float32(1.0)
    if G == 1:
        return np.array([lo], dtype=np.float32)
    step = np.float32((hi - lo) / np.float32(G - 1))
    return np.array([lo + step * np.float32(i) if i < G // 2 else hi - step * np.float32(G - i - 1) for i in range(G)], dtype=np.float32)


def start_grid(name):
    """(n, B*G, 3) float64: ori = the sweep's orientation g (float32), pos = 0; row = g * B + b."""
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    ori = sweep_orientations(G).astype(np.float64)
    assert float(np.abs(ori - torch.linspace(-1.0, 1.0, G).double().numpy()).max()) <= 2.0 ** -23
    st = np.zeros((nc, Rs, 3))
    st[:, :, 0] = np.repeat(ori, B)[None]
    return st


def rows_of(name, c, pose):
    """The classifier inputs of chain c's rows at the poses `pose` (B*G, 3) rounded to float32, float32 tensors."""
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    p32 = torch.from_numpy(np.asarray(pose, dtype=np.float64)).float()
    ori, pos, tt = p32[:, 0:1].contiguous(), p32[:, 1:3].contiguous(), torch.zeros(Rs)
    if kind == 2:
        return x[c].repeat(G, 1), ori, pos, tt, objs[c % 2].reshape(1, -1).expand(Rs, -1).contiguous()
    s = util.setup('point_3d', None, sd, T, 5, L, G, P, SUB)
    return orc._pts3d(s, x[c].reshape(B, L, 1)).repeat(G, 1, 1), ori, pos, tt, objs[c % 2].t().unsqueeze(0).expand(Rs, -1, -1).contiguous()


@functools.lru_cache(maxsize=None)
def weights(name, double):
    sd = inputs(name)[6]
    return {k: v.double() if (double and v.dtype.is_floating_point) else v for k, v in sd.items()}


_EMB = {}


class _embedding_once:
    """Within the block orc.pointnet2_forward remembers its results under (key, call number): the object embedding depends on the
    cloud, the draws and the arithmetic - not on the pose - so the oracle runs of one (chain, interaction, arithmetic) share it.  (The
    calls of one block are all remembered or all new, so a StartLog that is not consumed is never read further.)"""

    def __init__(self, key):
        self.key, self.calls = key, 0

    def __enter__(self):
        self.real = orc.pointnet2_forward

        def once(*a, **kw):
            kk = self.key + (self.calls,)
            self.calls += 1
            if kk not in _EMB:
                _EMB[kk] = self.real(*a, **kw)
            return _EMB[kk]
        orc.pointnet2_forward = once

    def __exit__(self, *exc):
        orc.pointnet2_forward = self.real


def oracle_logits(name, c, k, pose, double=True):
    """Oracle logits (B*G, 3) of chain c at interaction k's draws on `pose` rounded to float32; float64 or float32 arithmetic."""
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    a = rows_of(name, c, pose)
    if double:
        a = [v.double() for v in a]
    w = weights(name, double)
    with torch.no_grad():
        if kind == 2:
            return orc.dyn2d_forward(w, *a).double().numpy()
        log = orc.StartLog(util.unpack_starts(starts[k, c], [n for _, n in sub_batches(Rs) for _ in range(2)]))
        with _embedding_once((name, c, k, double)):
            return torch.cat([orc.dyn3d_forward(w, *[v[r0:r0 + n] for v in a], log) for r0, n in sub_batches(Rs)]).double().numpy()


def update(pose, logits, scale):
    """One update of the contract in numpy float64 -> (new pose, orientation before wrapping)."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    new = np.array(pose, dtype=np.float64, copy=True)
    pre = new[..., 0] + l[..., 0] * scale[0]
    o = pre.copy()
    for _ in range(64):                        # while ori > 1: ori -= 2; while ori < -1: ori += 2 (finite values: a few passes)
        hi, lo = o > 1.0, o < -1.0
        if not (hi.any() or lo.any()):
            break
        o = np.where(hi, o - 2.0, np.where(lo, o + 2.0, o))
    new[..., 0] = o
    new[..., 1] = new[..., 1] + l[..., 1] * scale[1]
    new[..., 2] = new[..., 2] + l[..., 2] * scale[2]
    return new, pre


def circ(a, b):
    """|a - b| with the orientation (column 0) compared as a circular distance mod 2."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    d[..., 0] = np.minimum(d[..., 0] % 2.0, 2.0 - d[..., 0] % 2.0)
    return d


def left_of(traj):
    """left (n, R) from a trajectory (K + 1, n, R, 3): the first k after which |pos_x| > 1 or |pos_y| > 1, -1 if never."""
    out = np.full(traj.shape[1:3], -1, dtype=np.int32)
    for k in range(traj.shape[0] - 1):
        gone = (np.abs(traj[k + 1, :, :, 1]) > 1.0) | (np.abs(traj[k + 1, :, :, 2]) > 1.0)
        out = np.where((out < 0) & gone, k, out)
    return out.astype(np.int32)


@functools.lru_cache(maxsize=None)
def free_run(name, double):
    """The oracle iterated on the CPU by the contract: (trajectory (K + 1, n, R, 3), orientations before wrapping (K, n, R))."""
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    sc = scale_of(kind)
    traj, pres = [start_grid(name)], []
    for k in range(K):
        l = np.stack([oracle_logits(name, c, k, traj[-1][c], double) for c in range(nc)])
        new, pre = update(traj[-1], l, sc)
        traj.append(new)
        pres.append(pre)
    return np.stack(traj), np.stack(pres)


def make_handle(name, mode="f32"):
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    dyn = engine.Dynamics(kind, sd, L, 2 * NV if kind == 2 else 0)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), nc, T, NV if kind == 2 else 512, SUB if kind == 3 else 0, max_objects=2, contraction_dtype=mode)
    return gd


@functools.lru_cache(maxsize=None)
def rolled(name):
    """One roll-out with trajectories on a fresh handle -> (handle, final, first_logits, left, traj_pose, traj_logits) as numpy."""
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    dev = torch.device("cuda:0")
    gd = make_handle(name)
    gd.set_objects(objs.to(dev))
    out = gd.rollout(x.to(dev), [c % 2 for c in range(nc)], STD[kind], K, starts=starts, want_trajectory=True)
    return (gd,) + tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def e_ref_step(name):
    """Per interaction, on the device's own poses: (max error of the rows API of the parent path, max error of the roll-out's logits),
    both against the float64 oracle on the same rows."""
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    gd, final, first, left, tp, tl = rolled(name)
    dyn = engine.Dynamics(kind, sd, L, 2 * NV if kind == 2 else 0)
    dev = torch.device("cuda:0")
    out = []
    for k in range(K):
        er = en = 0.0
        for c in range(nc):
            ref = oracle_logits(name, c, k, tp[k, c], True)
            a = [v.to(dev) for v in rows_of(name, c, tp[k, c])]
            if kind == 2:
                got = dyn.forward2d(*a)
            else:
                s1, s2 = row_starts(starts[k, c], Rs)
                got = dyn.forward3d(*a, torch.from_numpy(s1), torch.from_numpy(s2))
            er = max(er, float(np.abs(got.cpu().double().numpy() - ref).max()))
            en = max(en, float(np.abs(tl[k, c].astype(np.float64) - ref).max()))
        out.append((er, en))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_one_interaction_at_a_time(dev, name):
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    gd, final, first, left, tp, tl = rolled(name)
    sc = scale_of(kind)
    assert np.array_equal(tp[0], start_grid(name))                    # the sweep grid exactly
    assert np.array_equal(final, tp[K]) and np.array_equal(first, tl[0])
    assert np.isfinite(tp).all() and np.isfinite(tl).all()
    wraps = 0
    for k in range(K):
        new, pre = update(tp[k], tl[k], sc)
        wraps += int((np.abs(pre) > 1.0).sum())
        d = float(circ(tp[k + 1], new).max())
        assert d <= 1e-14, (k, d)
        assert float(np.abs(tp[k + 1][..., 0]).max()) <= 1.0
    assert np.array_equal(left, left_of(tp))
    print(f"[rollout] {name}: {int((left >= 0).sum())} of {left.size} rows leave |pos| <= 1 within {K} interactions, {wraps} wraps")
    errs = e_ref_step(name)
    for k, (er, en) in enumerate(errs):
        print(f"[rollout] {name} interaction {k}: max |logit - f64| = {en:.3e}, e_ref (rows API, f32 MFMA chain) = {er:.3e}, bound 2 e_ref = {2 * er:.3e}")
    for k, (er, en) in enumerate(errs):
        assert er > 0.0
        assert en <= 2.0 * er, (k, en, er)
    # one interaction alone: the same bits as the first of K (3-D: the same first-call draws)
    one = gd.rollout(x.to(dev), [c % 2 for c in range(nc)], STD[kind], 1, starts=None if starts is None else starts[:1], want_trajectory=True)
    assert np.array_equal(one[4].cpu().numpy()[0], tl[0]) and np.array_equal(one[1].cpu().numpy(), tl[0])
    assert np.array_equal(one[0].cpu().numpy(), tp[1])


@pytest.mark.parametrize("name", list(CASES))
def test_start_poses_carry_the_sweep_table(dev, name):
    """Interaction 0's pose term of every (chain, finger) tile = the orientation sweep's table tile, bit for bit, padding rows included."""
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    gd = rolled(name)[0]
    gd.rollout(x.to(dev), [c % 2 for c in range(nc)], STD[kind], 1, starts=None if starts is None else starts[:1])
    tiles, sweep = gd.debug_rollout_table(nc)
    assert tiles.shape[:3] == (nc, B, (G + 31) // 32) and tiles.shape[3] == (256 if kind == 2 else 512) * 32
    assert torch.equal(tiles.view(torch.int32), sweep.view(torch.int32)[None, None].expand_as(tiles))


@pytest.mark.parametrize("name", list(CASES))
def test_free_running(dev, name):
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    gd, final, first, left, tp, tl = rolled(name)
    t64, pre64 = free_run(name, True)
    t32, _ = free_run(name, False)
    near = np.abs(np.abs(pre64) - 1.0) < 1e-3                          # (K, n, R): right after update k, before wrapping
    excluded = np.cumsum(near, axis=0) > 0                            # from that interaction on
    share = float(excluded[-1].mean())
    print(f"[rollout] {name}: excluded rows (T64 orientation within 1e-3 of +-1 after an update) {share * 100:.1f} %")
    assert share <= 0.10, share
    for k in range(K):
        keep = ~excluded[k]
        d_dev = float(circ(tp[k + 1], t64[k + 1])[keep].max())
        d_32 = float(circ(t32[k + 1], t64[k + 1])[keep].max())
        print(f"[rollout] {name} after interaction {k + 1}: max |device - T64| = {d_dev:.3e}, max |T32 - T64| = {d_32:.3e}, bound 4 x = {4 * d_32:.3e}")
    for k in range(K):
        keep = ~excluded[k]
        d_dev = float(circ(tp[k + 1], t64[k + 1])[keep].max())
        d_32 = float(circ(t32[k + 1], t64[k + 1])[keep].max())
        assert d_dev <= 4.0 * d_32, (k, d_dev, d_32)


@pytest.mark.parametrize("name", ["2d_pad", "3d_pad"])
def test_nothing_outside_the_buffers(dev, name):
    """C ABI called directly: every output in a filled buffer with a guard region behind it - the guard keeps its fill, every valid
    element is written - and a run without trajectories returns the same bits."""
    import ctypes as C
    from dgdm_amd._lib import check, dptr, lib, stream_ptr
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    gd, final, first, left, tp, tl = rolled(name)
    guard = 4096
    n = nc * Rs
    xd = x.to(dev).contiguous()
    oc = (C.c_int32 * nc)(*[c % 2 for c in range(nc)])
    sc = (C.c_double * 3)(*scale_of(kind))
    sp = starts.ctypes.data if starts is not None else None

    def bufs(traj):
        f64, f32, i32 = -12345.0, -12345.0, -777
        b = dict(final=torch.full((n * 3 + guard,), f64, dtype=torch.float64, device=dev), first=torch.full((n * 3 + guard,), f32, dtype=torch.float32, device=dev),
                 left=torch.full((n + guard,), i32, dtype=torch.int32, device=dev))
        if traj:
            b["tp"] = torch.full(((K + 1) * n * 3 + guard,), f64, dtype=torch.float64, device=dev)
            b["tl"] = torch.full((K * n * 3 + guard,), f32, dtype=torch.float32, device=dev)
        return b

    res = {}
    for traj in (True, False):
        b = bufs(traj)
        check(lib().dgdm_guidance_rollout(gd._h, dptr(xd), oc, sp, sc, K, nc, dptr(b["final"]), dptr(b["first"]), dptr(b["left"]), dptr(b.get("tp")),
                                          dptr(b.get("tl")), stream_ptr()))
        res[traj] = {k: v.cpu() for k, v in b.items()}
        for k, v in res[traj].items():
            fill = -777 if k == "left" else -12345.0
            assert bool((v[-guard:] == fill).all()), k
    a = res[True]
    assert np.array_equal(a["final"][:n * 3].numpy().reshape(nc, Rs, 3), final) and np.array_equal(a["first"][:n * 3].numpy().reshape(nc, Rs, 3), first)
    assert np.array_equal(a["left"][:n].numpy().reshape(nc, Rs), left)
    assert np.array_equal(a["tp"][:-guard].numpy().reshape(K + 1, nc, Rs, 3), tp) and np.array_equal(a["tl"][:-guard].numpy().reshape(K, nc, Rs, 3), tl)
    assert bool((a["left"][:n] != -777).all()) and bool((a["tp"][:-guard] != -12345.0).all()) and bool((a["tl"][:-guard] != -12345.0).all())
    for k in ("final", "first", "left"):
        assert torch.equal(res[False][k], a[k]), k


@pytest.mark.parametrize("name", ["2d_pad", "3d_pad"])
def test_determinism_and_isolation(dev, name):
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs(name)
    gd, final, first, left, tp, tl = rolled(name)
    oc = [c % 2 for c in range(nc)]
    xd = x.to(dev)
    R = B * G * P * P
    cs = sampler.TorchRng(seed=99).fps_starts(512, SUB, R, n_calls=nc).reshape(-1) if kind == 3 else None
    ss = sampler.TorchRng(seed=98).fps_starts(512, SUB, Rs, n_calls=nc).reshape(-1) if kind == 3 else None
    objectives = [engine.make_objective(o, c % 2) for c, o in zip(range(nc), ('rotate', 'counterclockwise_left'))]

    def others():
        g = gd.grad(xd, 3, objectives, None, cs).cpu()
        c, s, l = gd.score(xd, oc, THR[kind], timestep=0, starts=cs, want_logits=True)
        return g, c.cpu(), s.cpu(), l.cpu(), gd.sweep(xd, oc, ss).cpu()

    before = others()
    state = torch.get_rng_state()
    again = gd.rollout(xd, oc, STD[kind], K, starts=starts, want_trajectory=True)
    assert torch.equal(torch.get_rng_state(), state)
    for got, want in zip(again, (final, first, left, tp, tl)):
        assert np.array_equal(got.cpu().numpy(), want)
    for got, want in zip(others(), before):
        assert torch.equal(got, want)


def test_sweep_and_rollout_agree_on_every_embedding_path(dev):
    """3-D: the orientation sweep and the roll-out give the same bits whichever way the rows' embeddings are made - the (chain, s1)-group
    gather kernel (modes 0 on a fresh handle and 3), the per-row table kernel (2), per-row FPS (1), and the per-object embedding tables
    (5: the index kernel over Rs * K rows, call k reading xidx + k * Rs).  Shapes of 3d_pad: K = 3 calls (the per-call row offset), 2
    chains (the chain stride), G = 7 (padding rows); the second object is the duplicate-point cloud of test_xobj_kernels_agree."""
    kind, B, G, nc, K, L, sd, _, x, Rs, starts = inputs("3d_pad")
    dup = synth.synth_object_3d(32).clone()
    dup[9] = dup[400]
    dup[10] = dup[400]
    objs = torch.stack([synth.synth_object_3d(50), dup]).to(dev)
    oc = [c % 2 for c in range(nc)]
    xd = x.to(dev)
    gd = make_handle("3d_pad")
    gd.set_objects(objs)

    def record():
        return [gd.sweep(xd, oc, starts[0]).cpu()] + [t.cpu() for t in gd.rollout(xd, oc, STD[kind], K, starts=starts, want_trajectory=True)]

    res = {}
    for mode in (0, 3, 2, 1):
        gd.debug_fps_path(mode)
        res[mode] = record()
    gd.debug_fps_path(5)                         # the next set_objects builds the embedding tables right away
    gd.set_objects(objs)
    res[5] = record()
    other = gd.sweep(xd, oc, starts[1]).cpu()
    gd.debug_fps_path(0)
    for mode in (3, 2, 1, 5):
        for i, (got, want) in enumerate(zip(res[mode], res[0])):
            assert torch.equal(got, want), (mode, i)
    assert float(res[0][0].abs().max()) > 0 and float(res[0][5].abs().max()) > 0
    assert not torch.equal(other, res[5][0])     # the draws are read


def test_refusals(dev):
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs("2d_pad")
    xd = x.to(dev)
    gd = make_handle("2d_pad")
    with pytest.raises(DgdmError, match=r"error -1: .*set_objects"):
        gd.rollout(xd, [0, 1], STD[2], K)
    gd.set_objects(objs.to(dev))
    with pytest.raises(DgdmError, match=r"error -1: .*interactions"):
        gd.rollout(xd, [0, 1], STD[2], 0)
    for mode in ("bf16", "f32_mfma"):           # f32_mfma is refused too (include/dgdm_hip.h): that trunk has no per-row pose form
        gd.set_contraction_dtype(mode)
        with pytest.raises(DgdmError, match=r"error -1: .*(bf16|MFMA)"):
            gd.rollout(xd, [0, 1], STD[2], K)
    gd.set_contraction_dtype("f32_f16x3")
    assert np.array_equal(gd.rollout(xd, [0, 1], STD[2], K)[0].cpu().numpy(), rolled("2d_pad")[1])
    kind, B, G, nc, K, L, sd, objs, x, Rs, starts = inputs("3d_pad")
    g3 = rolled("3d_pad")[0]
    with pytest.raises((DgdmError, AssertionError)):
        g3.rollout(x.to(dev), [0, 1], STD[3], K, starts=None)


@pytest.mark.parametrize("fingers_3d", [False, True])
def test_predicted_rollout_end_to_end(dev, tmp_path, fingers_3d):
    """The reduced validation_step of test_predicted_sim_end_to_end with --predicted_sim --predicted_rollout=3: tables written, every
    predicted metric marked with the interaction count, a settled rotation that differs from the one-step rotation somewhere, integer
    convergence ranges, and the sampled designs and the global CPU generator exactly as without the flag."""
    from dgdm_amd.dynamics import predicted
    from dgdm_amd.generator.train import train
    from dynamics.parser import parse
    shape = ("--fingers_3d --object_max_num_vertices=512 --ctrlpts_dim=42 --sub_bs=40" if fingers_3d else "--object_max_num_vertices=100 --ctrlpts_dim=14")
    common = (f"--mode=test --classifier_guidance {shape} --num_fingers=2 --batch_size=2 --grid_size=3 --num_pos=3 "
              f"--num_train_timesteps=15 --num_inference_steps=2")
    seen = []
    real = predicted.PredictedSimulator.__call__

    def spy(self, *a, **kw):
        out = real(self, *a, **kw)
        seen.extend(out[1])
        return out

    runs, states = {}, {}
    predicted.PredictedSimulator.__call__ = spy
    try:
        for tag, extra in (("one", " --predicted_sim"), ("rolled", " --predicted_sim --predicted_rollout=3")):
            torch.manual_seed(7)
            seen.clear()
            _, runs[tag] = train(parse(shlex.split(common + extra + f" --save_dir={tmp_path / tag}")))
            states[tag] = torch.get_rng_state()
            if tag == "rolled":
                assert seen and all(m.get("predicted") and m["rollout_interactions"] == 3 and isinstance(m["rollout_left_range"], int) for m in seen)
            else:
                assert seen and all("rollout_interactions" not in m for m in seen)
    finally:
        predicted.PredictedSimulator.__call__ = real
    assert runs["rolled"][0].keys() == runs["one"][0].keys()
    for k, v in runs["one"][0].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, runs["rolled"][0][k]), k
    assert torch.equal(states["rolled"], states["one"])
    tables = sorted(os.listdir(tmp_path / "rolled" / "tables"))
    assert tables == sorted(os.listdir(tmp_path / "one" / "tables")) and "SKIPPED.txt" not in tables
    differs, conv = False, 0
    for t in tables:
        tab = json.load(open(tmp_path / "rolled" / "tables" / t))
        oc = tab["columns"].index("objective")
        scores = [row[oc] for row in tab["data"] if isinstance(row[oc], dict) and row[oc].get("predicted")]
        assert tab["data"] and scores, t
        for s in scores:
            if "final_delta_theta" in s and "delta_theta" in s:
                differs = differs or s["final_delta_theta"] != s["delta_theta"]
            for deg in (3, 5, 10):
                if f"max_convergence_range_{deg}deg" in s:
                    conv += 1
                    assert isinstance(s[f"max_convergence_range_{deg}deg"], int), (t, s)
    assert differs and conv > 0
    with pytest.raises(ValueError, match="--predicted_sim"):
        train(parse(shlex.split(common + f" --predicted_rollout=3 --save_dir={tmp_path / 'bad'}")))
