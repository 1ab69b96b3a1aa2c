"""Resampling fingers by predicted objective on the GPU: the keyed uniform against numpy's Philox, the objectives' values
against the float64 formula, the weight / effective-sample-size / systematic step against tests/resample_oracle.py on the committed
inputs of tests/resample_cases.py (whose margins tests/test_resample_host.py checks on the CPU), and run_chains(resample=...) against a
walk written here from engine primitives and the oracle's step.  Ancestors, did and the gathered samples are compared exactly.

Sizes: T = 15, S = 5; 2-D B = 8, L = 14, G = 4, P = 1; 3-D B = 4, L = 42, G = 4, P = 2, sub_bs = 9 (tests/test_gpu_step_noise.py's, with
more fingers; both handles accept these B)."""
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine, sampler, synth
from dgdm_amd import dist as ddist
from dgdm_amd.edit import Edit
from dgdm_amd.resample import Resample, summarise
from dgdm_amd.scheduler import DDIMScheduler
from tests import resample_cases as cases
from tests import resample_oracle as orc
from tests import util

pytestmark = pytest.mark.gpu
T, S = 15, 5
NAMES = ['convergence', 'rotate', 'rotate_clockwise', 'rotate_counterclockwise', 'shift_up', 'shift_down', 'shift_left', 'shift_right',
         'clockwise_up', 'clockwise_down', 'clockwise_left', 'clockwise_right', 'counterclockwise_up', 'counterclockwise_down',
         'counterclockwise_left', 'counterclockwise_right']
LINEAR = [n for n in NAMES if n not in ('convergence', 'rotate')]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def _sched():
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(S)
    return s


_RIGS = {}


def _rig(dev, mode):
    """(net, guidance handle over 4 objects, scheduler, noise (B, L, 1), GuidanceSpec of the handle), built once per module."""
    if mode not in _RIGS:
        net = engine.Unet1d(util.unet_sd(11))
        if mode == 'point':
            nv, B, G, P, L, sub = 100, 8, 4, 1, 14, 0
            dyn = engine.Dynamics(2, util.dyn2d_sd(22, nv), L, 2 * nv)
            objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(4)])
        else:
            nv, B, G, P, L, sub = 512, 4, 4, 2, 42, 9
            dyn = engine.Dynamics(3, util.dyn3d_sd(33), L)
            objs = torch.stack([synth.synth_object_3d(i) for i in (1, 8, 2, 31)])
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 20, T, nv, sub, max_objects=4)
        gd.set_objects(objs.to(dev))
        gd._objs = objs
        spec = ddist.GuidanceSpec(dyn, B, G, P, (-1.0, 1.0), T, nv, sub)
        _RIGS[mode] = (net, gd, _sched(), synth.synth_noise(0, B, L).to(dev), spec)
    return _RIGS[mode]


def _bits(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stream(seed=4):
    return sampler.pair_stream(512, 9, seed, 0)


# ------------------------------------------------------------------------------------------------ 1. the uniform
def test_uniform_matches_numpy(dev):
    seen = {}
    for step in (0, 3):
        u = engine.resample_uniform(cases.SEED, cases.KEYS, step).cpu().numpy()
        ref = np.array([orc.uniform(cases.SEED, k, step) for k in cases.KEYS])
        assert u.dtype == np.float64 and np.array_equal(u, ref), (step, u, ref)
        assert np.all((u >= 0.0) & (u < 1.0)) and len(set(u.tolist())) == 3
        seen[step] = u
        # not the words the step noise of the same (seed, key, step) starts from
        for c, k in enumerate(cases.KEYS):
            words = orc.step_noise_first_words(cases.SEED, k, step)
            assert all(u[c] != float(int(w) >> 11) * 2.0 ** -53 for w in words)
    assert not np.array_equal(seen[0], seen[3])
    one = engine.resample_uniform(cases.SEED, [5], 3).cpu().numpy()
    assert one[0] == seen[3][1]                                   # a chain's uniform does not depend on its place in the launch
    assert not np.array_equal(engine.resample_uniform(cases.SEED + 1, cases.KEYS, 0).cpu().numpy(), seen[0])


# ------------------------------------------------------------------------------------------------ 2. the values
def _starts_for(gd, mode, n_rows, seed=12):
    if mode != 'point_3d':
        return None
    return np.ascontiguousarray(sampler.draw_chain_starts(gd, [(0, 'rotate')] * n_rows, 1, _stream(seed))[1][0])


@pytest.mark.parametrize("mode", ['point', 'point_3d'])
def test_objective_values(dev, mode):
    """2-D: all 16 reference names and a goal chain in one launch; 3-D: 'convergence', 'rotate', three linear names and a goal chain."""
    net, gd, s, noise, _ = _rig(dev, mode)
    B, L = noise.shape[:2]
    G, P = gd.cfg.grid_size, gd.cfg.num_pos
    names = NAMES if mode == 'point' else ['convergence', 'rotate', 'shift_up', 'clockwise_left', 'counterclockwise_right']
    goal = sampler.Goal(ori=0.25, pos=(0.3, -0.2), weight=(1.0, 0.5, -0.25), profile='linear')
    chains = [(i % 4, n) for i, n in enumerate(names)] + [(1, goal)]
    nc = len(chains)
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.uniform(-1.0, 1.0, (nc, B, L)).astype(np.float32)).to(dev)
    rc = np.zeros((nc, gd.rows), dtype=np.float32)
    rc[0] = gd.rowcoef(torch.from_numpy(rs.randint(0, G, B)))                       # 'convergence' with real centres
    assert np.any(rc[0] != 0)
    rcd = torch.from_numpy(rc).to(dev)
    with sampler.keeps_row_field(gd):
        objectives, field = sampler.chain_objectives(gd, chains)
        gd.set_row_field(field)
        counts, sums, logits = gd.score(x, [c[0] for c in chains], (1.0, 1.0, 1.0), 3, _starts_for(gd, mode, nc), want_logits=True)
        v = gd.objective_values(logits, objectives, rcd)
        again = gd.objective_values(logits, objectives, rcd)
        assert torch.equal(v, again)                                                 # the same bits run to run
        gd.set_row_field(None)
        with pytest.raises(_lib.DgdmError):                                          # a row-field chain without a field: DGDM_EINVAL
            gd.objective_values(logits, objectives, rcd)
        with pytest.raises(_lib.DgdmError):                                          # 'convergence' without its coefficients
            gd.objective_values(logits, objectives, None)
        short = torch.zeros((nc - 1, gd.rows, 3), dtype=torch.float32, device=dev)
        gd.set_row_field(short)
        with pytest.raises(_lib.DgdmError):                                          # a field that does not reach the chain's index
            gd.objective_values(logits, objectives, rcd)
    assert v.shape == (nc, B) and v.dtype == torch.float64
    v, lg, sm, fld = v.cpu().numpy(), logits.cpu().numpy(), sums.cpu().numpy().astype(np.float64), field.cpu().numpy()
    worst = 0.0
    for i, (_, name) in enumerate(chains):
        o = objectives[i]
        ref, mag = orc.objective_values(lg[i], list(o.lin), list(o.quad), int(o.use_rowcoef), B, rc[i], fld[i])
        assert np.all(mag > 0) or name == 'convergence'
        err = np.abs(v[i] - ref)
        worst = max(worst, float(np.max(err / np.maximum(mag, 1e-300))))
        assert np.all(err <= 1e-12 * mag), (name, float(err.max()), float(mag.min()))
        if name in LINEAR:
            lin = np.array(list(o.lin), dtype=np.float64)
            assert set(np.abs(lin)) <= {0.0, 1.0} and np.all(np.array(list(o.quad)) == 0)
            from_sums = lin[0] * sm[i, :, 0] + lin[1] * sm[i, :, 2] + lin[2] * sm[i, :, 3]
            absd = np.abs(lg[i].astype(np.float64)).reshape(-1, B, 3).sum(axis=(0, 2))
            assert np.all(np.abs(v[i] - from_sums) <= 1e-5 * absd), (name, float(np.abs(v[i] - from_sums).max()))
    print(f"{mode}: {nc} chains, worst |V - oracle| / sum |terms| = {worst:.3e}")
    assert len({round(float(t), 9) for t in v[:, 0]}) > nc // 2                      # the chains' values are not one number


# ------------------------------------------------------------------------------------------------ 3. the step on synthetic values
def _run_calls(dev, x, calls, n_grad):
    """The device's result of every call (logw / vprev carried on the device), as the oracle's dicts."""
    nc, B, _ = x.shape
    xd = torch.from_numpy(x).to(dev)
    logw, vprev = (torch.zeros((nc, B), dtype=torch.float64, device=dev) for _ in range(2))
    out = []
    for c in calls:
        xo, anc, ess, did = engine.chain_resample(xd, torch.from_numpy(np.asarray(c["values"], dtype=np.float64)).to(dev), n_grad, c["beta"],
                                                  c["ess_frac"], cases.SEED, cases.KEYS, c["step"], logw, vprev)
        out.append(dict(x=xo.cpu().numpy(), ancestors=anc.cpu().numpy(), ess=ess.cpu().numpy(), did=did.cpu().numpy(),
                        logw=logw.cpu().numpy().copy(), vprev=vprev.cpu().numpy().copy()))
    assert np.array_equal(_bits(xd), _bits(x))                                       # the input is not touched
    return out


def _same(got, ref, what):
    assert np.array_equal(got["ancestors"], ref["ancestors"]), (what, got["ancestors"], ref["ancestors"])
    assert got["ancestors"].dtype == np.int32 and np.array_equal(got["did"], ref["did"]), (what, got["did"], ref["did"])
    assert np.array_equal(_bits(got["x"]), _bits(ref["x"])), what
    assert np.all(np.abs(got["ess"] - ref["ess"]) <= 1e-12 * np.abs(ref["ess"])), (what, got["ess"], ref["ess"])
    for k in ("logw", "vprev"):
        a, b = got[k], ref[k]
        assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.array_equal(a[~np.isfinite(b)], b[~np.isfinite(b)]), (what, k)
        fin = np.isfinite(b)
        assert np.all(np.abs(a[fin] - b[fin]) <= 1e-12), (what, k, float(np.abs(a[fin] - b[fin]).max()))


@pytest.mark.parametrize("kind", cases.KINDS)
def test_resample_step(dev, kind):
    n = 0
    for B in cases.BS:
        for L in cases.LS:
            for n_grad in cases.NGRADS:
                x, calls = cases.case(kind, B, L, n_grad)
                ref = cases.expected(x, calls, n_grad)
                got = _run_calls(dev, x, calls, n_grad)
                for ci, (g, r) in enumerate(zip(got, ref)):
                    _same(g, r, (kind, B, L, n_grad, ci))
                    n += int(r["did"].sum())
    print(f"{kind}: {n} chain resamplings compared")


def test_resample_arguments(dev):
    x, calls = cases.case("dominant", 8, 14, 1)
    xd, v = torch.from_numpy(x).to(dev), torch.from_numpy(calls[0]["values"]).to(dev)
    z = lambda: torch.zeros((3, 8), dtype=torch.float64, device=dev)      # noqa: E731
    with pytest.raises(ValueError):
        engine.chain_resample(xd, v, 2, 0.25, 0.5, 7, cases.KEYS, 0, z(), z())       # values of one gradient for n_grad = 2
    with pytest.raises(ValueError):
        engine.chain_resample(xd, v, 1, 0.25, 0.5, 7, cases.KEYS[:2], 0, z(), z())
    with pytest.raises(ValueError):
        engine.chain_resample(xd, v.float(), 1, 0.25, 0.5, 7, cases.KEYS, 0, z(), z())
    with pytest.raises(ValueError):
        engine.chain_resample(xd, v, 1, 0.25, 0.5, 7, cases.KEYS, 0, z()[:2], z())
    lib, P = _lib.lib(), _lib.dptr
    kd, out, anc = engine.chain_keys_tensor(cases.KEYS, dev), torch.empty_like(xd), torch.empty((3, 8), dtype=torch.int32, device=dev)
    ess, did, lw, vp = torch.empty(3, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.int32, device=dev), z(), z()
    call = lambda xo, nc=3, B=8, L=14, ng=1, step=0: lib.dgdm_chain_resample(P(xd), P(v), nc, B, L, ng, 0.25, 0.5, 7, P(kd), step, P(lw), P(vp),      # noqa: E731
                                                                         xo, P(anc), P(ess), P(did), _lib.stream_ptr())
    assert call(P(out)) == _lib.OK
    for bad in (dict(B=0), dict(L=0), dict(ng=0), dict(nc=0), dict(step=-1)):
        assert call(P(out), **bad) == _lib.EINVAL, bad
    assert call(P(xd)) == _lib.EINVAL and call(None) == _lib.EINVAL                  # x_out must not be x


# ------------------------------------------------------------------------------------------------ 4. the greedy limit
def test_greedy_limit(dev):
    for B in cases.BS:
        for L in cases.LS:
            x, calls = cases.greedy_case(B, L)
            got = _run_calls(dev, x, calls, 1)[0]
            best = np.argmax(calls[0]["values"], axis=1)
            assert np.array_equal(got["ancestors"], np.repeat(best[:, None], B, axis=1)) and np.all(got["did"] == 1)
            assert np.array_equal(_bits(got["x"]), _bits(x[np.arange(3), best][:, None].repeat(B, axis=1)))
            assert np.allclose(got["ess"], 1.0, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ 5. chain level
CHAINS = {'point': [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left'), (3, 'rotate_clockwise')],
          'point_3d': [(0, 'rotate'), (1, 'shift_up'), (3, 'clockwise_left'), (2, 'shift_left')]}


def _predrawn(gd, mode, chains, n_pot, seed=4):
    return sampler.draw_chain_starts(gd, chains, S, _stream(seed), n_potential=n_pot) if mode == 'point_3d' else None


def _cut(pre, lo, hi):
    return None if pre is None else (pre[0][lo:hi],) + tuple(np.ascontiguousarray(a[:, lo:hi]) for a in pre[1:])


def _per_cell_values(gd, x, chains, t, starts):
    """(values per finger (nc, B) float64 on the device, the chains' objectives) of x at timestep t."""
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    logits = gd.score(x, [oi for oi, _ in chains], (1.0, 1.0, 1.0), t, starts, want_logits=True)[2]
    return gd.objective_values(logits, objectives, None), objectives


def _walk(dev, mode, chains, rs, seed, pre):
    """The walk of run_chains written from engine primitives, the resampling step being the oracle's on the device's values."""
    net, gd, s, noise, _ = _rig(dev, mode)
    B, L = noise.shape[:2]
    nc, cells = len(chains), gd.rows // B
    scales = [sampler.chain_scale(mode, o) for _, o in chains]
    assert len(set(scales)) == 1
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    x = noise.reshape(1, B, L).expand(nc, -1, -1).contiguous()
    logw, vprev = np.zeros((nc, B)), np.zeros((nc, B))
    log, e, margin = [], 0, np.inf
    for si, t in enumerate(s.timesteps):
        t = int(t)
        n = 1 if si == 0 else nc
        eps = net.forward_cfg(x[:n].reshape(n * B, L, 1), torch.full((n * B,), t, dtype=torch.int32, device=dev), None, 1.0)
        eps = eps.reshape(n, B, L).expand(nc, -1, -1).contiguous()
        g = gd.grad(x, t, objectives, None, None if pre is None else pre[1][si].reshape(-1))
        x = engine.ddim_guided_step(x, eps, g, 1, s.coefficients(t), scales[0], None, eta_coef=s.eta_coefficients(t, 0.5), seed=seed,
                                    chain_keys=list(range(nc)), step_index=si)
        if rs.evaluates(si, S):
            v, _ = _per_cell_values(gd, x, chains, int(s.timesteps[si + 1]), None if pre is None else pre[2][e].reshape(-1))
            u = [orc.uniform(seed, k, si) for k in range(nc)]
            r = orc.resample_step(x.cpu().numpy(), v.cpu().numpy(), 1, rs.beta / cells, rs.ess_frac, u, logw, vprev)
            logw, vprev = r["logw"], r["vprev"]
            idx = torch.from_numpy(r["ancestors"].astype(np.int64)).to(dev)
            x = torch.stack([x[k][idx[k]] for k in range(nc)])
            assert np.array_equal(_bits(x), _bits(r["x"]))
            log.append((si, r["ess"], r["did"], r["ancestors"]))
            margin = min(margin, float(r["margin"].min()))
            e += 1
    return x, log, margin


def _beta_from_first_evaluation(dev, mode, chains, pre, seed):
    """A beta that spreads the first evaluation's log weights over about 1.5: the weights then differ visibly without one finger
    taking everything.  Chosen from the values the plain walk reaches, before any resampling."""
    _, gd, s, _, _ = _rig(dev, mode)
    seen = []
    net, _, _, noise, _ = _rig(dev, mode)
    B, L = noise.shape[:2]
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    sampler.run_chains(net, gd, s, noise.reshape(B, L), len(chains), 1, objectives, None, None if pre is None else pre[1], s.timesteps[:1],
                       [sampler.chain_scale(mode, o) for _, o in chains], eta=0.5, noise_seed=seed, on_step=lambda si, x, eps: seen.append(x.clone()))
    v, _ = _per_cell_values(gd, seen[0], chains, int(s.timesteps[1]), None if pre is None else pre[2][0].reshape(-1))
    v = v.cpu().numpy() / (gd.rows // B)
    spread = float(np.median(v.max(axis=1) - v.min(axis=1)))
    assert spread > 0
    return float(f"{1.5 / spread:.3g}")


@pytest.mark.parametrize("mode", ['point', 'point_3d'])
def test_chains_equal_the_walk(dev, mode):
    net, gd, s, noise, spec = _rig(dev, mode)
    B, L = noise.shape[:2]
    chains, seed = CHAINS[mode], 5
    nc = len(chains)
    pre = _predrawn(gd, mode, chains, 4)
    beta = _beta_from_first_evaluation(dev, mode, chains, pre, seed)
    kw = dict(eta=0.5, noise_seed=seed)
    plain = sampler.guided_chains(net, gd, s, mode, noise, chains, predrawn=_cut(pre, 0, nc), **kw)
    for rs in (Resample(1, beta, 2.0), Resample(2, beta, 0.9)):
        n_pot = len(rs.evaluations(S))
        p = None if pre is None else (pre[0], pre[1], pre[2][:n_pot])
        log = []
        out = sampler.guided_chains(net, gd, s, mode, noise, chains, predrawn=p, resample=rs, resample_log=log, **kw)
        ref, ref_log, margin = _walk(dev, mode, chains, rs, seed, p)
        print(f"{mode} {rs}: smallest ancestor margin {margin:.3e}; resamples per chain {[r['resamples'] for r in summarise(log, nc, B)]}")
        assert margin > cases.MARGIN                                 # a condition on this test's inputs, as for the committed ones
        assert [e[0] for e in log] == [e[0] for e in ref_log] == rs.evaluations(S)
        for (_, ess, did, anc), (_, ress, rdid, ranc) in zip(log, ref_log):
            assert np.array_equal(anc.cpu().numpy(), ranc) and np.array_equal(did.cpu().numpy(), rdid)
            assert np.all(np.abs(ess.cpu().numpy() - ress) <= 1e-12 * ress)
        assert np.array_equal(_bits(out.reshape(nc, B, L)), _bits(ref))
        if rs.ess_frac > 1.0:
            assert all(int(d.sum()) == nc for _, _, d, _ in log) and not torch.equal(out, plain)
            # the potential of the final designs, with and without resampling: printed, not asserted (beta is untuned)
            st = None if pre is None else pre[2][0].reshape(-1)
            for tag, res in (("resampled", out), ("plain", plain)):
                v, _ = _per_cell_values(gd, res.reshape(nc, B, L), chains, 0, st)
                print(f"{mode} mean potential per cell of the final designs, {tag}: {(v.mean(dim=1) / (gd.rows // B)).cpu().numpy()}")
            # chains [0, nc) in one call == two calls with their keys
            halves = [sampler.guided_chains(net, gd, s, mode, noise, chains[lo:lo + 2], predrawn=_cut(p, lo, lo + 2), chain_keys=[lo, lo + 1],
                                            resample=rs, **kw) for lo in (0, 2)]
            assert torch.equal(torch.cat(halves), out)
            # the sharded sampler at world size 1, from the same start stream
            sh = ddist.guided_chains_sharded(net, spec, s, mode, noise, gd._objs, chains, starts=_stream() if mode == 'point_3d' else None,
                                             resample=rs, **kw)
            assert torch.equal(sh, out)
    # beta = 0 never resamples, every >= S never evaluates: both are the run without `resample`, bit for bit
    log = []
    p1 = None if pre is None else (pre[0], pre[1], pre[2][:4])
    zero = sampler.guided_chains(net, gd, s, mode, noise, chains, predrawn=p1, resample=Resample(1, 0.0), resample_log=log, **kw)
    assert torch.equal(zero, plain) and len(log) == 4 and all(int(d.sum()) == 0 for _, _, d, _ in log)
    assert all(np.allclose(e.cpu().numpy(), B, rtol=1e-12) for _, e, _, _ in log)
    log = []
    never = sampler.guided_chains(net, gd, s, mode, noise, chains, predrawn=_cut(pre, 0, nc), resample=Resample(S, 5.0, 2.0), resample_log=log, **kw)
    assert torch.equal(never, plain) and log == []
    # 3-D: the guidance draws of a resampled run are those of the run without
    if pre is not None:
        two = sampler.draw_chain_starts(gd, chains, S, _stream())
        assert np.array_equal(two[1], pre[1]) and all(a is None for a in two[0])


def test_multi_object_and_groups(dev):
    """The averaged-gradient samplers take the same argument: the walk (python_loop) and the default agree, n_grad = 2."""
    net, gd, s, noise, _ = _rig(dev, 'point')
    rs = Resample(2, 50.0, 2.0)
    kw = dict(eta=0.5, noise_seed=3, resample=rs)
    log = []
    m = sampler.guided_multi_object(net, gd, s, 'point', noise, [0, 1], 'shift_left', resample_log=log, **kw)
    assert len(log) == 2 and all(int(d.sum()) == 1 for _, _, d, _ in log)
    g = sampler.guided_multi_object_groups(net, gd, s, 'point', noise, [[0, 1], [2, 3]], ['shift_left', 'shift_left'], **kw)
    assert torch.equal(g[0], m) and torch.equal(g, sampler.guided_multi_object_groups(net, gd, s, 'point', noise, [[0, 1], [2, 3]],
                                                                                       ['shift_left', 'shift_left'], python_loop=True, **kw))


# ------------------------------------------------------------------------------------------------ 6. rejections
def test_rejections(dev):
    """Every refusal is raised before anything runs: the eps-net handed over is None, so a first launch would be an AttributeError."""
    _, gd, s, noise, spec = _rig(dev, 'point')
    B, L = noise.shape[:2]
    rs = Resample(1, 1.0)
    chains = [(0, 'rotate'), (1, 'shift_up')]
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    run = lambda **kw: sampler.run_chains(None, kw.pop("guid", gd), s, noise.reshape(B, L), 2, kw.pop("n_grad", 1), kw.pop("objectives", objectives),      # noqa: E731
                                          None, None, s.timesteps, kw.pop("scales", [0.001] * 2), resample=rs, **kw)
    with pytest.raises(ValueError, match="eta"):
        run()
    with pytest.raises(ValueError, match="eta"):
        run(eta=0.0)
    lo = torch.full((B, L), -1.0, device=dev)
    with pytest.raises(ValueError, match="bounds"):
        run(eta=0.5, bounds=(lo, -lo))
    with pytest.raises(ValueError, match="global_cond"):
        run(eta=0.5, global_cond=torch.zeros((B, 3), device=dev))
    with pytest.raises(ValueError, match="n_grad"):
        run(eta=0.5, n_grad=0, objectives=[])
    with pytest.raises(ValueError, match="n_grad"):
        run(eta=0.5, guid=None)
    with pytest.raises(ValueError, match="scales"):
        run(eta=0.5, n_grad=2, objectives=objectives * 2, scales=[0.001, 10.0])
    bf = engine.Guidance(gd.dyn, B, 4, 1, (-1.0, 1.0), 2, T, 100, 0, max_objects=4, contraction_dtype="bf16")
    with pytest.raises(ValueError, match="bf16"):
        run(eta=0.5, guid=bf)
    with pytest.raises(ValueError, match="Resample"):
        sampler.run_chains(None, gd, s, noise.reshape(B, L), 2, 1, objectives, None, None, s.timesteps, [0.001] * 2, eta=0.5, resample=(1, 1.0))
    # the samplers above run_chains refuse the same, before they prepare anything
    edit = Edit.from_physical(np.zeros((B, L), dtype=np.float32), pins=(0,), band_mm=2.0, steps=3, mode='point')
    for fn, args in ((sampler.guided_chains, (chains,)), (sampler.guided_multi_object, ([0, 1], 'rotate')),
                     (sampler.guided_multi_object_groups, ([[0, 1]], ['rotate']))):
        with pytest.raises(ValueError, match="eta"):
            fn(None, gd, s, 'point', noise, *args, resample=rs)
        with pytest.raises(ValueError, match="edit"):
            fn(None, gd, s, 'point', noise, *args, resample=rs, eta=0.5, edit=edit)
        with pytest.raises(ValueError, match="global_cond"):
            fn(None, gd, s, 'point', noise, *args, resample=rs, eta=0.5, global_cond=torch.zeros((B, 3), device=dev))
    with pytest.raises(ValueError, match="eta"):
        ddist.guided_chains_sharded(None, spec, s, 'point', noise, gd._objs, chains, resample=rs)
    with pytest.raises(ValueError, match="not supported"):
        ddist.guided_multi_object_sharded(None, spec, s, 'point', noise, gd._objs[:2], 'rotate', eta=0.5, resample=rs)


# ------------------------------------------------------------------------------------------------ 7. the entry point
def test_cli_resample(dev, monkeypatch):
    """generator/train.py --mode=test with the 2-D flags of test_cli_eta (tests/test_gpu_step_noise.py) and the three new flags.  beta:
    the oracle's greedy limit - with beta = 1e8 over the grid's 12 cells, two fingers whose values differ by more than 1e-5 leave one of
    them all the weight, ess = 1 < 0.9 * 2 - so a chain resamples at an evaluation unless its two fingers are tied that closely."""
    from dgdm_amd.generator import artefacts
    from dgdm_amd.generator.train import train
    from dgdm_amd.dynamics.parser import parse
    monkeypatch.setattr(artefacts, "plot_fingers", lambda path, *a, **k: path)
    x = np.zeros((1, 2, 1), dtype=np.float32)
    r = orc.resample_step(x, np.array([[0.0, 1e-5]]), 1, 1e8 / 12, 0.9, [0.3], np.zeros((1, 2)), np.zeros((1, 2)))
    assert r["did"][0] == 1 and r["ancestors"].tolist() == [[1, 1]] and r["ess"][0] < 1.0 + 1e-9
    common = ("--mode=test --classifier_guidance --num_fingers=2 --batch_size=2 --grid_size=3 --num_pos=2 --object_max_num_vertices=10 "
              "--ctrlpts_dim=14 --num_train_timesteps=15 --num_inference_steps=5 --eta 0.5 --noise_seed 3")
    _, plain = train(parse(shlex.split(common)))
    _, res = train(parse(shlex.split(common + " --resample_every 2 --resample_beta 1e8 --resample_ess 0.9")))
    assert "resample" not in plain[0] and len(res) == 1
    rep = res[0]["resample"]
    keys = [k for k in res[0] if k.startswith(("guided/", "multi/"))]
    assert len(keys) == 23 and sorted(rep) == sorted(keys)
    total = 0
    for k in keys:
        n = res[0][k].shape[0] if k.startswith("guided/") else 1
        assert len(rep[k]) == n, k
        for c in rep[k]:
            assert sorted(c) == ["distinct_min", "ess_min", "evaluations", "resamples"], c
            assert c["evaluations"] == 2 and 0 <= c["resamples"] <= 2 and 1 <= c["distinct_min"] <= 2 and 1.0 - 1e-9 <= c["ess_min"] <= 2.0 + 1e-9
            total += c["resamples"]
        assert bool(torch.isfinite(res[0][k]).all()) and float(res[0][k].abs().max()) <= 1.0, k
    print("resamples per sampler:", {k: [c["resamples"] for c in rep[k]] for k in keys})
    assert all(c["resamples"] >= 1 for c in rep["guided/shift_up"]) and total >= len(keys)
    assert any(not torch.equal(res[0][k], plain[0][k]) for k in keys)
    assert torch.equal(res[0]["unguided"], plain[0]["unguided"])
    with pytest.raises(ValueError, match="eta"):
        train(parse(shlex.split(common.replace(" --eta 0.5", "") + " --resample_every 2 --resample_beta 1.0")))
    with pytest.raises(ValueError, match="classifier_guidance"):
        train(parse(shlex.split(common.replace(" --classifier_guidance", "") + " --resample_every 2 --resample_beta 1.0")))
