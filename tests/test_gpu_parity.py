"""GPU parity tests: the HIP path (through the C-ABI of libdgdm_hip.so) against
(a) the golden vectors captured from the reference and (b) the CPU oracle on seeded inputs.

Tolerances (float32 path; north_star asks for finger-profile L2 error < 1e-4):
  * forward passes / gradients: relative L2 <= 2e-5 (summation order and folded BatchNorm differ from torch's)
  * final samples of a chain:   absolute L2 per finger <= 1e-4
"""
import os

import numpy as np
import pytest
import torch

from dgdm_amd import engine, sampler, synth
from dgdm_amd.scheduler import DDIMScheduler
from oracle import dgdm_oracle as orc
from tests import util
from tests.golden.make_golden_names import OBJ16

pytestmark = pytest.mark.gpu
REL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def sched(T, S):
    s = DDIMScheduler(num_train_timesteps=int(T))
    s.set_timesteps(int(S))
    return s


def finger_l2(a, b):
    a = torch.as_tensor(a, dtype=torch.float64).reshape(-1, a.shape[-2] * a.shape[-1])
    b = torch.as_tensor(b, dtype=torch.float64).reshape(a.shape)
    return float((a - b).norm(dim=1).max())


# ------------------------------------------------------------------------------------------------ a7 / a13
def test_unet_golden(dev):
    g = util.load("g2_unet.npz")
    net = engine.Unet1d(util.unet_sd(g["seed"]))
    for L in (14, 42):
        x = torch.from_numpy(g[f"x_L{L}"]).to(dev)
        for t in (0, 3, 12, 999):
            y = net.forward(x, torch.full((4,), t, device=dev))
            assert util.rel_l2(y.cpu(), g[f"y_L{L}_t{t}"]) < REL, (L, t)


def test_unet_mixed_timesteps_and_batch(dev):
    sd = util.unet_sd(5)
    net = engine.Unet1d(sd)
    x = torch.randn(37, 42, 1, generator=torch.Generator().manual_seed(1))
    t = torch.randint(0, 1000, (37,), generator=torch.Generator().manual_seed(2))
    y = net.forward(x.to(dev), t.to(dev))
    assert util.rel_l2(y.cpu(), orc.unet1d_forward(sd, x, t)) < REL


@pytest.mark.parametrize("L", [14, 42, 44])
def test_unet_arithmetic_modes_vs_float64(dev, L):
    """The eps-net's three float32-grade statements against the oracle evaluated in float64 (generator/diffusion_utils.py:238-285): the
    default (three f16 MFMA products on exactly scaled two-way splits, csrc/unet.hip conv_mfma_f16x3) and the float32 MFMA chain both
    within 1e-6 - the default no farther than the chain + 1e-7 - and within 2e-6 of each other; bf16 mode at its own level (1e-2).
    L = 44: the split form's LDS slabs do not fit beside one sample's activations there, the library runs the chain (same numbers)."""
    sd = util.unet_sd(7)
    sd64 = {k: v.double() for k, v in sd.items()}
    x = torch.randn(64, L, 1, generator=torch.Generator().manual_seed(3))
    t = torch.randint(0, 15, (64,), generator=torch.Generator().manual_seed(1))
    ref = orc.unet1d_forward(sd64, x.double(), t)
    out = {m: engine.Unet1d(sd, contraction_dtype=m).forward(x.to(dev), t.to(dev)).cpu().double() for m in ("f32", "f32_mfma", "bf16")}
    err = {m: float((o - ref).norm() / ref.norm()) for m, o in out.items()}
    assert err["f32_mfma"] < 1e-6 and err["f32"] < 1e-6 and err["f32"] <= err["f32_mfma"] + 1e-7, err
    assert float((out["f32"] - out["f32_mfma"]).norm() / ref.norm()) < 2e-6
    assert 1e-4 < err["bf16"] < 2e-2, err
    if L == 44:
        assert torch.equal(out["f32"], out["f32_mfma"])


def test_ddim_step_and_unguided_chain(dev):
    sd = util.unet_sd(11)
    net = engine.Unet1d(sd)
    # (1000, 1000, 4, 14) is BASELINE configs[0] itself: 2-D unconditional sampling, B = 4, L = 14, T = S = 1000 (dynamics/parser.py:29,31
    # defaults; generator/diffusion.py:249-256), teacher-forced along the oracle's trajectory through all 1000 steps
    for T, S, B, L in ((15, 5, 3, 14), (1000, 100, 2, 42), (1000, 1000, 4, 14)):
        s = sched(T, S)
        so = orc.DDIM(T)
        so.set_timesteps(S)
        assert torch.equal(s.timesteps, so.timesteps) and torch.equal(s.alphas_cumprod, so.alphas_cumprod)
        x = synth.synth_noise(3, B, L)
        e = synth.synth_noise(4, B, L)
        for t in (int(s.timesteps[0]), int(s.timesteps[-1])):
            got = s.step(e.to(dev), t, x.to(dev)).prev_sample.cpu()
            assert util.rel_l2(got, so.step(e, t, x)) < 1e-6
        tn = min(S, T - 1)
        n = s.add_noise(x.to(dev), e.to(dev), torch.full((B,), tn, dtype=torch.int64)).cpu()
        assert util.rel_l2(n, so.add_noise(x, e, torch.full((B,), tn, dtype=torch.int64))) < 1e-6
        # Random-init nets make long chains chaotic: on the CPU oracle itself a 1e-7 relative change of the start noise moves
        # the end of the 100-step chain by 5e-3 (finger L2) but the 5-step chain by 5e-6.  So the shipped 5-step chain is
        # compared end to end, and long chains step by step along the oracle's trajectory (teacher forcing).
        if S <= 10:
            out = sampler.unguided_sample(net, s, x.to(dev)).cpu()
            ref = orc.unguided_sample(util.setup('point', sd, None, T, S, L, 1, 1), x)
            assert finger_l2(out, ref) < 1e-4
        xo = x.clone()
        for t in so.timesteps:
            ts = torch.full((B,), int(t), dtype=torch.int64)
            nxt = so.step(orc.unet1d_forward(sd, xo, ts), t, xo)
            got = s.step(net.forward(xo.to(dev), ts.to(dev)), int(t), xo.to(dev)).prev_sample.cpu()
            assert finger_l2(got, nxt) < 2e-5, int(t)
            xo = nxt
        if S == 1000:       # and the library's own loop over the 1000 steps, free-running: finite, inside the scheduler's clip range
            out = sampler.unguided_sample(net, s, x.to(dev)).cpu()
            assert out.shape == (B, L, 1) and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------ a8 / a4 (2-D)
def test_dyn2d_forward_golden(dev):
    g = util.load("g3_dyn2d.npz")
    nv = int(g["dims"][6])
    dyn = engine.Dynamics(2, util.dyn2d_sd(g["seed"], nv), 14, 2 * nv)
    f = lambda k: torch.from_numpy(g[k]).to(dev)
    y = dyn.forward2d(f("fwd_xc"), f("fwd_xo"), f("fwd_xp"), f("fwd_t"), f("fwd_obj"))
    assert util.rel_l2(y.cpu(), g["fwd_logits"]) < REL


def _guid2d(dyn, B, G, P, rng, T, nv, objs, dev, max_chains=4):
    gd = engine.Guidance(dyn, B, G, P, rng, max_chains, T, nv, 0, max_objects=max(1, len(objs)))
    gd.set_objects(torch.stack(list(objs)).to(dev))
    return gd


def test_dyn2d_cond_fn_golden(dev):
    g = util.load("g3_dyn2d.npz")
    B, G, P, L, T, S, nv = [int(v) for v in g["dims"]]
    dyn = engine.Dynamics(2, util.dyn2d_sd(g["seed"], nv), 14, 2 * nv)
    x = torch.from_numpy(g["x"]).to(dev).reshape(1, B, L)
    obj = torch.from_numpy(g["obj"])
    centers = torch.from_numpy(g["centers"])
    for name, rng in (("full", (-1.0, 1.0)), ("half", (-0.5, 0.25))):
        gd = _guid2d(dyn, B, G, P, rng, T, nv, [obj], dev)
        rc = torch.from_numpy(gd.rowcoef(centers)).to(dev).reshape(1, -1)
        for o in OBJ16:
            gr = gd.grad(x, 9, [engine.make_objective(o, 0)], rc if o == 'convergence' else None)
            assert util.rel_l2(gr.cpu().reshape(B, L, 1), g[f"grad_{o}_{name}"]) < REL, (o, name)


def test_dyn2d_cond_fn_oracle_multichain(dev):
    """Several chains with different objects/objectives in one launch; ragged last cell tile (C = 7*9 = 63)."""
    nv, B, G, P, L, T = 100, 5, 7, 3, 14, 15
    sd = util.dyn2d_sd(77, nv)
    dyn = engine.Dynamics(2, sd, L, 2 * nv)
    objs = [synth.synth_object_2d(i, nv) for i in range(3)]
    gd = _guid2d(dyn, B, G, P, (-1.0, 1.0), T, nv, objs, dev, max_chains=6)
    s = util.setup('point', None, sd, T, 5, L, G, P)
    chains = [(0, 'rotate'), (1, 'shift_left'), (2, 'clockwise_up'), (1, 'rotate'), (0, 'convergence'), (2, 'rotate_counterclockwise')]
    xs = torch.stack([synth.synth_noise(50 + i, B, L).clamp(-1, 1) for i in range(len(chains))])
    centers = torch.tensor([2, 0, 6, 3, 1])
    rc = np.zeros((len(chains), gd.rows), np.float32)
    rc[4] = gd.rowcoef(centers)
    gr = gd.grad(xs.reshape(len(chains), B, L).to(dev), 6, [engine.make_objective(o, oi) for oi, o in chains], torch.from_numpy(rc).to(dev)).cpu()
    ties = 0
    for c, (oi, o) in enumerate(chains):
        ref = orc.cond_fn(s, xs[c], torch.full((B,), 6, dtype=torch.int64), o, objs[oi], (-1.0, 1.0), centers if o == 'convergence' else None)
        # rounding level - except that ONE ReLU whose pre-activation is within rounding of zero may fall on the other side than in torch's
        # arithmetic and move ONE finger's gradient by ~1e-4 of the chain's (tests/test_gpu_fullgrid.py); a wrong kernel moves them all
        err = util.finger_err(gr[c].reshape(B, L, 1), ref).sort().values
        norm = float(ref.double().norm())
        if float(err.norm()) / norm < REL:
            continue
        ties += 1
        assert float(err[:-1].norm()) / norm < REL and float(err[-1]) / norm < 1e-3, (c, o, err / norm)
    assert ties <= 1, ties


# ------------------------------------------------------------------------------------------------ a9-a12 (3-D)
def test_pointnet_golden(dev):
    g = util.load("g4_pointnet.npz")
    dyn = engine.Dynamics(3, util.dyn3d_sd(g["seed"]), 42)
    clouds = torch.from_numpy(g["clouds"]).permute(0, 2, 1).contiguous().to(dev)
    st = util.unpack_starts(g["starts"], g["start_lens"])
    emb = dyn.pointnet2(clouds, st[0], st[1])
    assert util.rel_l2(emb.cpu(), g["emb"]) < REL


def test_pointnet_heavy_object_vs_oracle(dev):
    """An object whose EVERY centre is crowded (506 of 512: the clouds that carry the table build), 160 variants of it:
    the launches sized by device data run their stride loops (l2c: eight centres per workgroup; sa3's table: 80 k rows on a bounded
    grid) - embeddings against the oracle's PointNet++ on the same FPS starts."""
    sd = util.dyn3d_sd(44)
    dyn = engine.Dynamics(3, sd, 42)
    rows = 160
    cloud = synth.synth_object_3d(2)
    xyz = cloud.t().contiguous()[None].repeat(rows, 1, 1)
    s1 = torch.arange(rows, dtype=torch.int64) * 3
    s2 = torch.from_numpy(np.random.RandomState(3).randint(0, 512, rows).astype(np.int64))
    emb = dyn.pointnet2(xyz.to(dev), s1, s2)
    want = orc.pointnet2_forward(sd, xyz, orc.StartLog([s1, s2]), prefix="object_encoder.")
    assert util.rel_l2(emb.cpu(), want) < REL, util.rel_l2(emb.cpu(), want)
    assert float((emb.cpu() - want).abs().max()) < 1e-4 * float(want.abs().max())


def test_guidance_grad_bit_reproducible(dev):
    """The same 3-D (full grid, 36 000 rows) and 2-D guidance gradient three times over, each from a fresh Guidance handle: bit-identical.
    (A hand-scheduled kernel with inline assembly between MFMAs can lose that without failing a tolerance: round 5's first mix-fma
    split fed an MFMA straight from an asm statement the hazard recogniser does not see as a VALU write - DESIGN.md 4.1.)"""
    g = util.load("g9_3d_rotate.npz")
    B, G, P, L, T, S, N = [int(v) for v in g["dims"]]
    dyn = engine.Dynamics(3, synth.scale_output(util.dyn3d_sd(g["dyn3d_seed"]), float(g["gain"])), L)
    x = torch.from_numpy(g["trace_x"][0]).to(dev).reshape(1, B, L)
    outs = []
    for _ in range(3):
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 2, T, N, 512, max_objects=2)
        gd.set_objects(torch.from_numpy(g["objs"]).to(dev))
        st = sampler.StartStream(N, 512, util.unpack_starts(g["starts"].astype(np.int64), g["start_lens"]))
        outs.append(gd.grad(x, 12, [engine.make_objective("rotate", 0)], None, st.call(gd.rows)).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    nv = 100
    dyn2 = engine.Dynamics(2, util.dyn2d_sd(77, nv), 14, 2 * nv)
    x2 = synth.synth_noise(50, 5, 14).clamp(-1, 1).reshape(1, 5, 14).to(dev)
    outs = []
    for _ in range(3):
        gd2 = engine.Guidance(dyn2, 5, 360, 5, (-1.0, 1.0), 1, 15, nv, 0, max_objects=1)
        gd2.set_objects(synth.synth_object_2d(1, nv)[None].to(dev))
        outs.append(gd2.grad(x2, 6, [engine.make_objective("rotate", 0)], None).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_dyn3d_forward_golden(dev):
    g = util.load("g5_dyn3d.npz")
    dyn = engine.Dynamics(3, util.dyn3d_sd(g["seed"]), 42)
    f = lambda k: torch.from_numpy(g[k]).to(dev)
    st = util.unpack_starts(g["fwd_starts"], g["fwd_start_lens"])
    y = dyn.forward3d(f("fwd_xc"), f("fwd_xo"), f("fwd_xp"), f("fwd_t"), f("fwd_clouds").permute(0, 2, 1).contiguous(), st[0], st[1])
    assert util.rel_l2(y.cpu(), g["fwd_logits"]) < REL


def test_dyn3d_cond_fn_golden(dev):
    g = util.load("g5_dyn3d.npz")
    B, G, P, L, T, S = [int(v) for v in g["dims"]]
    dyn = engine.Dynamics(3, util.dyn3d_sd(g["seed"]), 42)
    x = torch.from_numpy(g["x"]).to(dev).reshape(1, B, L)
    obj = torch.from_numpy(g["obj"])
    for sub in (7, 512):
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 2, T, 512, sub, max_objects=1)
        gd.set_objects(obj[None].to(dev))
        rc = torch.from_numpy(gd.rowcoef(torch.tensor([1, 0]))).to(dev).reshape(1, -1)
        for o in ('rotate', 'clockwise_left', 'convergence'):
            starts = g[f"starts_{o}_sub{sub}"].astype(np.int64)
            gr = gd.grad(x, 6, [engine.make_objective(o, 0)], rc if o == 'convergence' else None, starts)
            assert util.rel_l2(gr.cpu().reshape(B, L, 1), g[f"grad_{o}_sub{sub}"]) < REL, (o, sub)


# ------------------------------------------------------------------------------------------------ a1-a3, a6: chains
def _teacher_forced(net, gd, s, mode, g, key, chains, final, step_starts, dev, n_grad=1, scale=None, multi_obj=None, rowcoef=None, errs=None, rel=None, grads=None):
    """Replays the reference's recorded trajectory (tests/golden: trace*_x/_eps/_grad): at every step the HIP eps-net, cond_fn
    and scheduler step see exactly the inputs the reference saw.  This is the precise check; free-running chains at these
    tiny R (24-72 rows) can be thrown off by a single ReLU sign flip (see DESIGN_HISTORY.md §7)."""
    xs, es, gs = g[key + "_x"], g[key + "_eps"], g[key + "_grad"]
    # gradient tolerance: REL, or what a full-grid fixture calibrated against float64 - one value or one per recorded cond_fn call
    rel = REL if rel is None else rel
    rel_of = (lambda i: rel[i]) if isinstance(rel, (list, tuple, np.ndarray)) else (lambda i: rel)
    S = xs.shape[0]
    B, L = xs.shape[1], xs.shape[2]
    oi, o = chains[0]
    for si, t in enumerate(s.timesteps):
        t = int(t)
        x = torch.from_numpy(xs[si]).to(dev)
        eps = net.forward(x, torch.full((B,), t, device=dev))
        assert util.rel_l2(eps.cpu(), es[si]) < REL, (key, si)
        if multi_obj is None:
            st = step_starts[si].reshape(-1) if step_starts is not None else None
            gr = gd.grad(x.reshape(1, B, L), t, [engine.make_objective(o, oi)], rowcoef, st)
            if errs is not None:
                errs.append(util.rel_l2(gr.cpu().reshape(B, L, 1), gs[si]))
            if grads is not None:
                grads.append(gr.cpu().reshape(B, L, 1))
            assert util.rel_l2(gr.cpu().reshape(B, L, 1), gs[si]) < rel_of(si), (key, si)
            g_ref = torch.from_numpy(gs[si]).to(dev).reshape(1, -1)
        else:
            n = len(multi_obj)
            st = step_starts[si].reshape(-1) if step_starts is not None else None
            gr = gd.grad(x.reshape(1, B, L).expand(n, -1, -1).contiguous(), t, [engine.make_objective(o, k) for k in multi_obj], None, st)
            for k in range(n):
                if errs is not None:
                    errs.append(util.rel_l2(gr[k].cpu().reshape(B, L, 1), gs[si * n + k]))
                if grads is not None:
                    grads.append(gr[k].cpu().reshape(B, L, 1))
                assert util.rel_l2(gr[k].cpu().reshape(B, L, 1), gs[si * n + k]) < rel_of(si * n + k), (key, si, k)
            g_ref = torch.from_numpy(gs[si * n:(si + 1) * n]).to(dev).reshape(n, -1)
        nxt = engine.ddim_guided_step(x, torch.from_numpy(es[si]).to(dev), g_ref, g_ref.shape[0], s.coefficients(t), scale).cpu()
        want = xs[si + 1] if si + 1 < S else final
        # x_t reaches ~15 on the small golden chains: 1e-5 is a few float32 ulps over 14-42 entries (scaled up where |x| is larger)
        assert finger_l2(nxt, want) < 1e-5 * max(1.0, float(np.abs(want).max()) / 15.0), (key, si)


def test_chains_golden_2d(dev):
    g = util.load("g6_chains.npz")
    B, G, P, L, T, S, nv = [int(v) for v in g["dims2d"]]
    net = engine.Unet1d(util.unet_sd(g["unet_seed"]))
    dyn = engine.Dynamics(2, util.dyn2d_sd(g["dyn2d_seed"], nv), L, 2 * nv)
    objs = torch.from_numpy(g["objs2d"])
    gd = _guid2d(dyn, B, G, P, (-1.0, 1.0), T, nv, list(objs), dev, max_chains=8)
    s = sched(T, S)
    noise = synth.synth_noise(0, B, L).to(dev)
    ug = sampler.unguided_sample(net, s, noise)
    assert finger_l2(ug.cpu(), g["unguided2d"]) < 1e-4
    names = ('rotate', 'shift_left', 'counterclockwise_up', 'convergence')
    chains = [(oi, o) for o in names for oi in range(2)]
    out = sampler.guided_chains(net, gd, s, 'point', noise, chains, unguided=ug).cpu()
    centers = sampler.convergence_centers(gd, 'point', ug, [0, 1])
    for c, (oi, o) in enumerate(chains):
        # 'convergence' runs with classifier_scale 10 (generator/diffusion.py:31): on random-init weights that chain is chaotic
        # (a last-bit change of eps moves the end point by O(1)), so only its step-by-step replay is checked
        if o != 'convergence':
            assert finger_l2(out[c], g[f"guided2d_{o}_obj{oi}"]) < 1e-4, (o, oi)
        rc = torch.from_numpy(gd.rowcoef(centers[oi])).to(dev).reshape(1, -1) if o == 'convergence' else None
        _teacher_forced(net, gd, s, 'point', g, f"trace2d_{o}_obj{oi}", [(oi, o)], g[f"guided2d_{o}_obj{oi}"], None, dev,
                        scale=sampler.classifier_scale('point', o), rowcoef=rc)
    m = sampler.guided_multi_object(net, gd, s, 'point', noise, [0, 1], 'rotate_clockwise').cpu()
    assert finger_l2(m, g["multi2d_rotate_clockwise"]) < 1e-4
    _teacher_forced(net, gd, s, 'point', g, "tracemulti2d", [(0, 'rotate_clockwise')], g["multi2d_rotate_clockwise"], None, dev,
                    scale=sampler.SCALE_2D, multi_obj=[0, 1])


def test_chains_golden_3d(dev):
    g = util.load("g6_chains.npz")
    B, G, P, L, T, S = [int(v) for v in g["dims3d"]]
    net = engine.Unet1d(util.unet_sd(g["unet_seed"]))
    dyn = engine.Dynamics(3, util.dyn3d_sd(g["dyn3d_seed"]), L)
    objs = torch.from_numpy(g["objs3d"])
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 2, T, 512, 5, max_objects=2)
    gd.set_objects(objs.to(dev))
    s = sched(T, S)
    noise = synth.synth_noise(0, B, L).to(dev)
    ug = sampler.unguided_sample(net, s, noise)
    assert finger_l2(ug.cpu(), g["unguided3d"]) < 1e-4
    # These golden chains use the He-init dynamics weights as they are: the guidance term is ~10^3 x eps and the chain is a
    # chaotic map (tests/test_gpu_fullgrid.py: the reference parts from ITSELF by 0.2 .. 6 on such chains; here a change of the
    # eps-net's float32 summation order alone moved one end point by 8e-2).  A free-running comparison says nothing there, so
    # the chains only have to run and stay inside the clamp; the step-by-step replay below is the check, and the free-running
    # comparison is made on the calibrated full-grid fixtures (test_gpu_fullgrid.py).
    forced = lambda k: sampler.StartStream(512, 5, util.unpack_starts(g[k + "_starts"], g[k + "_start_lens"]))      # noqa: E731
    sane = lambda t: bool(torch.isfinite(t).all()) and float(t.abs().max()) <= 1.0 + 1e-6                            # noqa: E731
    out = sampler.guided_chains(net, gd, s, 'point_3d', noise, [(0, 'rotate')], unguided=ug, starts=forced("guided3d_rotate")).cpu()
    assert sane(out)
    _, step = sampler.draw_chain_starts(gd, [(0, 'rotate')], S, forced("guided3d_rotate"))
    _teacher_forced(net, gd, s, 'point_3d', g, "trace3d_rotate", [(0, 'rotate')], g["guided3d_rotate"], step, dev, scale=sampler.SCALE_3D)
    out = sampler.guided_chains(net, gd, s, 'point_3d', noise, [(0, 'convergence')], unguided=ug, starts=forced("guided3d_convergence")).cpu()
    assert sane(out)
    st = forced("multi3d_shift_up")
    m = sampler.guided_multi_object(net, gd, s, 'point_3d', noise, [0, 1], 'shift_up', starts=st).cpu()
    assert sane(m)
    st = forced("multi3d_shift_up")
    step = np.stack([np.stack([st.call(gd.rows), st.call(gd.rows)]) for _ in range(S)])       # step-major, object after object
    _teacher_forced(net, gd, s, 'point_3d', g, "tracemulti3d", [(0, 'shift_up')], g["multi3d_shift_up"], step, dev,
                    scale=sampler.SCALE_3D, multi_obj=[0, 1])


def test_convergence_centers_golden(dev):
    g = util.load("g7_convergence.npz")
    B, G, P, nv = [int(v) for v in g["cc2d_dims"]]
    dyn = engine.Dynamics(2, util.dyn2d_sd(g["dyn2d_seed"], nv), 14, 2 * nv)
    gd = _guid2d(dyn, B, G, P, (-1.0, 1.0), 15, nv, [torch.from_numpy(g["cc2d_obj"])], dev)
    c = sampler.convergence_centers(gd, 'point', torch.from_numpy(g["cc2d_unguided"]).to(dev), [0])
    assert np.array_equal(c[0].numpy(), g["cc2d_centers"])
    B, G, P = [int(v) for v in g["cc3d_dims"]]
    dyn = engine.Dynamics(3, util.dyn3d_sd(g["dyn3d_seed"]), 42)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 1, 15, 512, 4, max_objects=1)
    gd.set_objects(torch.from_numpy(g["cc3d_obj"])[None].to(dev))
    st = sampler.StartStream(512, 4, util.unpack_starts(g["cc3d_starts"], g["cc3d_start_lens"]))
    c = sampler.convergence_centers(gd, 'point_3d', torch.from_numpy(g["cc3d_unguided"]).to(dev), [0], st.call(B * G))
    assert np.array_equal(c[0].numpy(), g["cc3d_centers"])


# ------------------------------------------------------------------------------------------------ larger shapes vs the oracle
def test_dyn3d_cond_fn_oracle_fps_paths(dev):
    """3-D cond_fn on a cloud without / with exact duplicate points: table path == per-row FPS path == oracle."""
    B, G, P, L, T, sub = 3, 4, 2, 42, 15, 11
    sd = util.dyn3d_sd(44)
    dyn = engine.Dynamics(3, sd, L)
    clean = synth.synth_object_3d(31)
    dup = synth.synth_object_3d(32).clone()
    dup[9] = dup[400]
    dup[10] = dup[400]
    objs = torch.stack([clean, dup])
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 2, T, 512, sub, max_objects=2)
    gd.set_objects(objs.to(dev))
    gd.debug_fps_path(False)
    x = torch.stack([synth.synth_noise(60, B, L), synth.synth_noise(61, B, L)]).clamp(-1, 1)
    torch.manual_seed(3)
    st = sampler.StartStream(512, sub)
    starts = np.concatenate([st.call(gd.rows), st.call(gd.rows)])
    objectives = [engine.make_objective('rotate', 0), engine.make_objective('counterclockwise_left', 1)]
    fast = gd.grad(x.reshape(2, B, L).to(dev), 3, objectives, None, starts).cpu()
    gd.debug_fps_path(True)
    slow = gd.grad(x.reshape(2, B, L).to(dev), 3, objectives, None, starts).cpu()
    gd.debug_fps_path(False)
    assert torch.equal(fast, slow)
    s = util.setup('point_3d', None, sd, T, 5, L, G, P, sub)
    for c, (oi, o) in enumerate(((0, 'rotate'), (1, 'counterclockwise_left'))):
        log = orc.StartLog(util.unpack_starts(starts[c * 2 * gd.rows:(c + 1) * 2 * gd.rows],
                                              [n for r0 in range(0, gd.rows, sub) for n in (min(sub, gd.rows - r0),) * 2]))
        ref = orc.cond_fn(s, x[c], torch.full((B,), 3, dtype=torch.int64), o, objs[oi], (-1.0, 1.0), None, log)
        assert util.rel_l2(fast[c].reshape(B, L, 1), ref) < REL, (c, o)


def test_xobj_kernels_agree(dev):
    """The four ways of getting a row's embedding - the per-object embedding table X[s1][q] (default: no per-step kernel at all), the
    (chain, s1)-group gather kernel (LDS slab; 1, 2 or 8 feature chunks depending on how many crowded centres the object has), the
    per-row table kernel, per-row FPS - give bit-identical gradients; float32 and
    bf16 table formats; objects with 0 / 146 / 506 crowded centres and one with exact duplicate points (tie-flagged start points)."""
    B, G, P, L, T, sub = 2, 12, 3, 42, 15, 64
    dyn = engine.Dynamics(3, util.dyn3d_sd(44), L)
    dup = synth.synth_object_3d(32).clone()
    dup[9] = dup[400]
    dup[10] = dup[400]
    objs = torch.stack([synth.synth_object_3d(1), synth.synth_object_3d(8), synth.synth_object_3d(2), dup])
    nc = objs.shape[0]
    x = torch.stack([synth.synth_noise(70 + i, B, L) for i in range(nc)]).clamp(-1, 1).reshape(nc, B, L).to(dev)
    objectives = [engine.make_objective(o, i) for i, o in enumerate(('rotate', 'shift_up', 'clockwise_left', 'rotate'))]
    for dtype in ("f32", "bf16"):
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), nc, T, 512, sub, max_objects=nc, contraction_dtype=dtype)
        gd.set_objects(objs.to(dev))
        torch.manual_seed(5)
        st = sampler.StartStream(512, sub)
        starts = np.concatenate([st.call(gd.rows) for _ in range(nc)])
        res = {}
        for mode in (0, 3, 2, 1):
            gd.debug_fps_path(mode)
            res[mode] = gd.grad(x, 3, objectives, None, starts).cpu()
        gd.debug_fps_path(5)                      # embedding tables X[s1][q] built by set_objects: no per-step gather kernel at all
        gd.set_objects(objs.to(dev))
        res[5] = gd.grad(x, 3, objectives, None, starts).cpu()
        gd.debug_fps_path(4)                      # tables rebuilt with l2_kernel's per-(variant, centre) gathers instead of l2c_kernel
        gd.set_objects(objs.to(dev))
        res[4] = gd.grad(x, 3, objectives, None, starts).cpu()
        gd.debug_fps_path(0)
        assert all(torch.equal(res[0], res[m]) for m in (3, 2, 1, 5, 4)), dtype
        # default policy: the embedding tables appear once the objects have served more than 5 calls; nothing changes numerically
        gd.set_objects(objs.to(dev))
        for k in range(8):
            assert torch.equal(gd.grad(x, 3, objectives, None, starts).cpu(), res[0]), (dtype, k)
        assert float(res[0].abs().max()) > 0


def test_native_loop_equals_step_by_step(dev):
    """dgdm_guided_chains_run (the whole denoise loop inside the library) against the same loop driven step by step from Python through
    dgdm_unet1d_forward / dgdm_dyn*_guidance_grad / dgdm_ddim_guided_step: bit-identical, 2-D and 3-D, per-object chains with mixed
    classifier scales ('convergence' among them), one multi-object chain, several multi-object chains per launch."""
    net = engine.Unet1d(util.unet_sd(11))
    for mode in ('point', 'point_3d'):
        if mode == 'point':
            nv, B, G, P, L, T, sub = 100, 3, 7, 3, 14, 15, 0
            dyn = engine.Dynamics(2, util.dyn2d_sd(22, nv), L, 2 * nv)
            objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(4)])
        else:
            nv, B, G, P, L, T, sub = 512, 2, 4, 2, 42, 15, 9
            dyn = engine.Dynamics(3, util.dyn3d_sd(33), L)
            objs = torch.stack([synth.synth_object_3d(i) for i in (1, 8, 2, 31)])
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 8, T, nv, sub, max_objects=4)
        gd.set_objects(objs.to(dev))
        s = sched(T, 5)
        noise = synth.synth_noise(0, B, L).to(dev)
        ug = sampler.unguided_sample(net, s, noise)
        chains = [(0, 'rotate'), (1, 'convergence'), (2, 'shift_up'), (3, 'clockwise_left'), (0, 'convergence')]
        torch.manual_seed(4)
        a = sampler.guided_chains(net, gd, s, mode, noise, chains, unguided=ug)
        torch.manual_seed(4)
        b = sampler.guided_chains(net, gd, s, mode, noise, chains, unguided=ug, trace=[])
        assert torch.equal(a, b), mode
        if mode == 'point_3d':
            # the library embeds all calls of a run in one gather launch unless their rows pass the packed-row limit (2^22 per chain): then in
            # groups of calls, each before its first step - forced here (test hook), same bits
            for cpe in ("2", "1"):
                os.environ["DGDM_EMBED_CALLS"] = cpe
                try:
                    torch.manual_seed(4)
                    c = sampler.guided_chains(net, gd, s, mode, noise, chains, unguided=ug)
                finally:
                    os.environ.pop("DGDM_EMBED_CALLS", None)
                assert torch.equal(a, c), (mode, cpe)
        torch.manual_seed(5)
        a = sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1, 2, 3], 'shift_left')
        torch.manual_seed(5)
        b = sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1, 2, 3], 'shift_left', on_step=lambda i, x: None)
        assert torch.equal(a, b), mode
        groups, objv = [[0, 1], [2, 3], [1, 3]], ['rotate', 'shift_down', 'counterclockwise_up']
        pre = None
        if mode == 'point_3d':
            pre = sampler.draw_ensemble_starts(gd, 3, 2, 5, [sampler.pair_stream(nv, sub, 7, k) for k in range(3)])
        a = sampler.guided_multi_object_groups(net, gd, s, mode, noise, groups, objv, predrawn=pre)
        b = sampler.guided_multi_object_groups(net, gd, s, mode, noise, groups, objv, predrawn=pre, python_loop=True)
        assert torch.equal(a, b), mode


def test_unet_batched_equals_per_sample(dev):
    """The eps-net's two execution forms of the default (f16x3) arithmetic - one workgroup per sample with the whole network in LDS, and, for
    large batches, layer-by-layer launches with four samples per workgroup and the activations in global memory (csrc/unet.hip, "batched
    form") - are the same arithmetic operation for operation: identical bits, for every batch size (ragged last workgroup included), both
    finger lengths, mixed timesteps, and when a smaller batch follows a larger one in the same workspace.  Also at the lengths where a sample's
    boundary falls elsewhere inside the batched form's 16-row position tiles (L = 2, 4, 16, 32, 34), and with a step embedding of 12."""
    sd = util.unet_sd(11)
    env = os.environ.get("DGDM_UNET_BATCHED_MIN")
    try:
        os.environ["DGDM_UNET_BATCHED_MIN"] = "0"
        per_sample = engine.Unet1d(sd)
        os.environ["DGDM_UNET_BATCHED_MIN"] = "1"
        batched = engine.Unet1d(sd)
        # a step embedding narrower than dot_kn's step of 8 (dsed = 12: padded rows in se1_wt / cond_wt, ub_cond_kernel's copy of the walk)
        sd12 = synth.synth_state_dict(synth.unet_spec(dsed=12), 12)
        os.environ["DGDM_UNET_BATCHED_MIN"] = "0"
        per_sample12 = engine.Unet1d(sd12, step_embed_dim=12)
        os.environ["DGDM_UNET_BATCHED_MIN"] = "1"
        batched12 = engine.Unet1d(sd12, step_embed_dim=12)
    finally:
        if env is None:
            os.environ.pop("DGDM_UNET_BATCHED_MIN", None)
        else:
            os.environ["DGDM_UNET_BATCHED_MIN"] = env
    g = torch.Generator().manual_seed(5)
    # L = 2, 4, 16, 32, 34: where a sample's boundary falls inside the 16-row position tiles moves with L (one-position second level, exactly
    # full tiles, a tile and two rows)
    for L in (2, 4, 16, 32, 34, 42, 14):
        assert batched.effective_form(37, L) == ("f32_f16x3", True) and per_sample.effective_form(37, L) == ("f32_f16x3", False)
        for B in ((1024, 37, 5, 4, 3, 1, 130) if L in (42, 14) else (37, 5, 4, 3, 1)):
            x = torch.randn((B, L, 1), generator=g).to(dev)
            x[B // 2] *= 1e-3                                   # samples of very different magnitude in one workgroup (the scale is per sample)
            t = torch.randint(0, 15, (B,), generator=g).to(dev)
            a, b = per_sample.forward(x, t), batched.forward(x, t)
            assert bool(torch.isfinite(b).all())
            assert torch.equal(a, b), (L, B, float((a - b).abs().max()))
    ref = orc.unet1d_forward(sd, x.cpu(), t.cpu())
    assert util.rel_l2(b.cpu(), ref) < REL
    for L in (34, 14):
        assert batched12.effective_form(37, L) == ("f32_f16x3", True) and per_sample12.effective_form(37, L) == ("f32_f16x3", False)
        for B in (37, 5, 4, 3, 1):
            x = torch.randn((B, L, 1), generator=g).to(dev)
            x[B // 2] *= 1e-3
            t = torch.randint(0, 1000, (B,), generator=g).to(dev)
            a, b = per_sample12.forward(x, t), batched12.forward(x, t)
            assert bool(torch.isfinite(b).all())
            assert torch.equal(a, b), ("dsed 12", L, B, float((a - b).abs().max()))
    assert util.rel_l2(b.cpu(), orc.unet1d_forward(sd12, x.cpu(), t.cpu())) < REL
    # what runs is reported, not assumed (advisor, round 4): the split form falls back to the float32 chain where its slabs do not fit
    assert batched.effective_form(1024, 42) == ("f32_f16x3", True) and per_sample.effective_form(1024, 42) == ("f32_f16x3", False)
    assert batched.effective_form(4, 46) == ("f32_mfma", False)
    assert engine.Unet1d(sd, contraction_dtype="bf16").effective_form(1024, 42) == ("bf16", False)
    assert engine.Unet1d(sd).effective_form(767, 42)[1] is False and engine.Unet1d(sd).effective_form(768, 42)[1] is True


def test_xobj_rows_large_groups(dev):
    """xobj_rows_kernel takes a (chain, s1) group in passes of 1024 rows: clouds of 128 points give 128 groups per chain, i.e. ~1400 rows per
    group for the five calls of a configs[2]-sized chain (B = 32, G = 45, P = 5) - two passes, runs cut at the pass boundary - against the
    per-row table kernel (test hook mode 2): bit-identical end points, 3 chains, objects with and without crowded centres, float32 and
    bf16 table formats."""
    B, G, P, L, T, sub, N = 32, 45, 5, 42, 15, 512, 128
    dyn = engine.Dynamics(3, util.dyn3d_sd(45), L)
    objs = torch.stack([synth.synth_object_3d(s, N) for s in (1, 8, 2)])
    s = sched(T, 5)
    noise = synth.synth_noise(3, B, L).to(dev)
    chains = [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left')]
    for dtype in ("f32", "bf16"):
        net = engine.Unet1d(util.unet_sd(11), contraction_dtype=dtype)
        out = {}
        for mode in (0, 2):
            gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 3, T, N, sub, max_objects=3, contraction_dtype=dtype)
            gd.debug_fps_path(mode)
            gd.set_objects(objs.to(dev))
            torch.manual_seed(6)
            if mode == 0:
                out[mode] = sampler.guided_chains(net, gd, s, 'point_3d', noise, chains).cpu()      # one gather launch for the five calls: the large groups
            else:
                out[mode] = sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, trace=[]).cpu()      # step by step, per-row kernel
        assert torch.equal(out[0], out[2]), dtype
        assert bool(torch.isfinite(out[0]).all()) and float(out[0].abs().max()) > 0
