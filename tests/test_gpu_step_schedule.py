"""The step schedule: the 3-D table build off the caller's stream with its readers joining it, the eps-net on a side
stream inside the denoise loop, and the float64 stages around the trunk with more loads in flight.

The schedule moves kernels between streams and changes none of them, so every comparison is bit for bit between a handle created
with DGDM_SERIAL_STEP=1 (everything on the caller's stream, in the order of the data dependencies) and one created without."""
import contextlib
import os

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine, sampler, synth
from dgdm_amd.scheduler import DDIMScheduler
from tests import util

pytestmark = pytest.mark.gpu
L, T, N = 42, 15, 512
CROWDED, UNCROWDED, THIRD = 2, 1, 9       # synth_object_3d indices: one with crowded centres, one without (asserted below)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dyn(dev):
    return engine.Dynamics(3, util.dyn3d_sd(44), L)


@pytest.fixture(scope="module")
def net(dev):
    return engine.Unet1d(util.unet_sd(11))


@pytest.fixture(scope="module")
def objs(dev, dyn):
    o = torch.stack([synth.synth_object_3d(i) for i in (CROWDED, UNCROWDED, THIRD)]).to(dev)
    ncr = [int((engine.debug_pointnet_indices(dyn, c)["crowded"] != 0).sum()) for c in o]
    assert ncr[0] > 0 and ncr[1] == 0, ncr
    return o


@contextlib.contextmanager
def _env(serial):
    old = os.environ.pop("DGDM_SERIAL_STEP", None)
    if serial:
        os.environ["DGDM_SERIAL_STEP"] = "1"
    try:
        yield
    finally:
        os.environ.pop("DGDM_SERIAL_STEP", None)
        if old is not None:
            os.environ["DGDM_SERIAL_STEP"] = old


def _guidance(serial, *args, **kw):
    with _env(serial):         # read when the handle is created
        return engine.Guidance(*args, **kw)


def _sched(S=3):
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(S)
    return s


def _chains(net, gd, dev, chains, seed=4, S=3, **kw):
    B = gd.cfg.batch
    noise = synth.synth_noise(0, B, L).to(dev)
    _, step = sampler.draw_chain_starts(gd, chains, S, sampler.StartStream(N, gd.cfg.sub_batch_size, seed=seed))
    return sampler.guided_chains(net, gd, _sched(S), 'point_3d', noise, chains, predrawn=([None] * len(chains), step), **kw)


SMALL = dict(B=2, G=3, P=2, sub=7)
CHAINS3 = [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left')]


def _small(serial, dyn, nc=3):
    return _guidance(serial, dyn, SMALL["B"], SMALL["G"], SMALL["P"], (-1.0, 1.0), nc, T, N, SMALL["sub"], max_objects=3)


@pytest.fixture(scope="module")
def serial_small(dev, dyn, net, objs):
    """The serial handle's results for the small case, computed once: chains on objs, chains on objs reversed."""
    gd = _small(True, dyn)
    assert gd.rows == 24
    gd.set_objects(objs)
    a = _chains(net, gd, dev, CHAINS3).cpu()
    gd.set_objects(objs.flip(0).contiguous())
    b = _chains(net, gd, dev, CHAINS3, seed=5).cpu()
    assert float(a.abs().max()) > 0 and not torch.equal(a, b)
    return a, b


def test_chains_3d(dev, dyn, net, objs, serial_small):
    gd = _small(False, dyn)
    gd.set_objects(objs)
    assert torch.equal(_chains(net, gd, dev, CHAINS3).cpu(), serial_small[0])


def test_chains_3d_batched_eps_net(dev, dyn, net, objs):
    """24 chains x 32 fingers: from step 1 on the eps-net sees 768 samples and runs in its batched form, on the side stream."""
    B, nc = 32, 24
    assert net.effective_form(nc * B, L) != net.effective_form(B, L)
    chains = [(c % 2, ('rotate', 'shift_up', 'shift_down')[c % 3]) for c in range(nc)]
    res = []
    for serial in (True, False):
        gd = _guidance(serial, dyn, B, 1, 1, (-1.0, 1.0), nc, T, N, 16, max_objects=2)
        gd.set_objects(objs[:2])
        res.append(_chains(net, gd, dev, chains).cpu())
    assert float(res[0].abs().max()) > 0
    assert torch.equal(res[0], res[1])


def test_back_to_back(dev, dyn, net, objs, serial_small):
    """set_objects(X), chains, set_objects(Y), chains with no host synchronisation in between: the second build must not overwrite
    tables the first chains still read."""
    gd = _small(False, dyn)
    gd.set_objects(objs)
    a = _chains(net, gd, dev, CHAINS3)
    gd.set_objects(objs.flip(0).contiguous())
    b = _chains(net, gd, dev, CHAINS3, seed=5)
    assert torch.equal(a.cpu(), serial_small[0])
    assert torch.equal(b.cpu(), serial_small[1])


def test_set_objects_twice_then_chains(dev, dyn, net, objs, serial_small):
    gd = _small(False, dyn)
    gd.set_objects(objs.flip(0).contiguous())
    gd.set_objects(objs)
    assert torch.equal(_chains(net, gd, dev, CHAINS3).cpu(), serial_small[0])


def test_non_default_caller_stream(dev, dyn, net, objs, serial_small):
    gd = _small(False, dyn)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gd.set_objects(objs)
        out = _chains(net, gd, dev, CHAINS3)
        st.synchronize()
    assert torch.equal(out.cpu(), serial_small[0])


def test_every_reader_joins(dev, dyn, objs):
    """Each reader of the tables as the FIRST call after set_objects."""
    B, nc = SMALL["B"], 3
    x = torch.stack([synth.synth_noise(70 + i, B, L) for i in range(nc)]).clamp(-1, 1).reshape(nc, B, L).to(dev)
    objectives = [engine.make_objective(o, oi) for oi, o in CHAINS3]
    oc = [0, 1, 2]
    res = []
    for serial in (True, False):
        gd = _small(serial, dyn)
        ss = sampler.StartStream(N, SMALL["sub"], seed=9)
        g_st = np.concatenate([ss.call(gd.rows) for _ in range(nc)])
        s_st = np.concatenate([ss.call(gd.sweep_rows) for _ in range(nc)])
        r_st = np.concatenate([ss.call(gd.sweep_rows) for _ in range(2 * nc)])
        readers = [lambda: (gd.grad(x, 3, objectives, None, g_st),),
                   lambda: gd.score(x, oc, (0.1, 0.1, 0.1), 3, g_st, want_logits=True),
                   lambda: (gd.sweep(x, oc, s_st),),
                   lambda: gd.rollout(x, oc, (0.3, 0.02, 0.02), 2, r_st)]
        out = []
        for fn in readers:
            gd.set_objects(objs)
            out.append([t.cpu() for t in fn()])
        res.append(out)
    for a, b in zip(*res):
        assert float(a[0].abs().max()) > 0
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_wait_then_host_read(dev, dyn, objs):
    """set_objects(wait=True) blocks until the tables exist; the host-side flags behind it are those of the serial build."""
    ok = []
    for serial in (True, False):
        gd = _small(serial, dyn)
        gd.set_objects(objs, wait=True)
        ok.append(gd.debug_fps_path(0))
    assert len(ok[0]) == 3 and ok[0] == ok[1]


def test_multi_object_classifier_free(dev, dyn, objs):
    """n_grad = 2 with a classifier-free mix on a small conditional eps-net: the side stream's doubled batch, condition rows and mix."""
    gc, B = 6, SMALL["B"]
    cnet = engine.Unet1d(synth.synth_state_dict(synth.unet_spec(global_cond_dim=gc), 11))
    cond = torch.from_numpy(np.random.RandomState(31).uniform(-1, 1, (B, gc)).astype(np.float32)).to(dev)
    noise = synth.synth_noise(0, B, L).to(dev)
    res = []
    for serial in (True, False):
        gd = _small(serial, dyn, nc=2)
        gd.set_objects(objs)
        res.append(sampler.guided_multi_object(cnet, gd, _sched(), 'point_3d', noise, [0, 1], 'shift_up',
                                               starts=sampler.StartStream(N, SMALL["sub"], seed=6), global_cond=cond, cfg_weight=0.5).cpu())
    assert float(res[0].abs().max()) > 0
    assert torch.equal(res[0], res[1])


def test_chains_2d(dev, net):
    B, G, P, nv, L2 = 2, 4, 2, 100, 14
    d2 = engine.Dynamics(2, util.dyn2d_sd(5, nv), L2, 2 * nv)
    o2 = torch.stack([synth.synth_object_2d(i, nv) for i in range(2)]).to(dev)
    noise = synth.synth_noise(0, B, L2).to(dev)
    chains = [(0, 'rotate'), (1, 'shift_left')]
    res = []
    for serial in (True, False):
        gd = _guidance(serial, d2, B, G, P, (-1.0, 1.0), 2, T, nv, 0, max_objects=2)
        gd.set_objects(o2)
        res.append(sampler.guided_chains(net, gd, _sched(), 'point', noise, chains).cpu())
    assert float(res[0].abs().max()) > 0
    assert torch.equal(res[0], res[1])


# ------------------------------------------------------------------------------------------------ the float64 stages
# Bound: a float64 fma chain of K terms is off by at most K * 2^-53 * sum |terms| (K <= 512: 5.7e-14 sum |terms|), numpy's dot by as
# much; for the uniform operands below sum |terms| is within a small multiple of the largest output, so 1e-12 of the largest output
# holds both with a margin of an order of magnitude.
def _rand(rs, *shape):
    return rs.uniform(-1, 1, shape)


@pytest.mark.parametrize("K,Nout,act", [(14, 256, 1), (42, 256, 1), (27, 512, 0), (256, 256, 0), (256, 512, 0)])
def test_linear64(dev, K, Nout, act):
    rs = np.random.RandomState(K + Nout)
    rows = 3
    x, wt, b = _rand(rs, rows, K), _rand(rs, K, Nout) / np.sqrt(K), _rand(rs, Nout)
    ref = x @ wt + b
    if act == 1:
        ref = np.maximum(ref, 0.0)
    xd, wd, bd = (torch.from_numpy(v).to(dev) for v in (x, wt, b))
    out = []
    for _ in range(2):
        y = torch.full((rows, Nout), 7.0, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().dgdm_debug_linear64(xd.data_ptr(), K, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), Nout, rows, K, Nout, act, _lib.stream_ptr()))
        out.append(y.cpu().numpy())
    err = np.abs(out[0] - ref).max() / np.abs(ref).max()
    print(f"linear64 K={K} N={Nout}: {err:.2e} of the largest output")
    assert err < 1e-12
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("W1", [256, 512])
@pytest.mark.parametrize("tiles", [1, 36])
@pytest.mark.parametrize("Lp", [14, 42])
def test_dyn_post64(dev, W1, tiles, Lp):
    """The output is float32: it must be the rounding of a float64 value within 1e-12 (of the largest output) of numpy's, i.e. off by
    at most half a float32 spacing plus that."""
    rs = np.random.RandomState(W1 + tiles + Lp)
    rows = 3
    partial = _rand(rs, rows, tiles, W1).astype(np.float32)
    w1c, g2w, g0w, V = _rand(rs, W1, 256) / 16, _rand(rs, 256, 256) / 16, _rand(rs, 256, Lp) / 16, _rand(rs, rows, 256)
    da = partial.astype(np.float64).sum(axis=1)
    ref = np.where(V > 0, (da @ w1c) @ g2w, 0.0) @ g0w
    dv = [torch.from_numpy(v).to(dev) for v in (partial, w1c, g2w, g0w, V)]
    out = []
    for _ in range(2):
        g = torch.full((rows, Lp), 7.0, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().dgdm_debug_dyn_post64(W1, dv[0].data_ptr(), tiles, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(),
                                                    g.data_ptr(), rows, Lp, _lib.stream_ptr()))
        out.append(g.cpu().numpy())
    slack = np.abs(out[0].astype(np.float64) - ref) - 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = slack.max() / np.abs(ref).max()
    print(f"dyn_post64 W1={W1} tiles={tiles} L={Lp}: {worst:.2e} of the largest output beyond the float32 rounding")
    assert worst < 1e-12
    assert np.array_equal(out[0], out[1])
