"""The gather of an object's rows starts when that object's tables are done: an early read-back of the tie flags and
crowded-centre counts, one completion event per object, one gather launch per object behind its event, the tie-flagged rows and the
trunk behind the joined build.

Nothing is computed differently, so every comparison is bit for bit against a handle created with DGDM_SERIAL_STEP=1.  Five objects
on three build streams, so the order in which the builds end matters; and before every compared build another set_objects has run
on the same handle (the same objects in reversed order), so that every object slot holds ANOTHER object's tables: a gather that
starts before its object is done reads the wrong bits."""
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
B, G, P, SUB, S = 2, 3, 2, 7, 3            # 24 rows per call
NOBJ = 5
OF_CHAIN = [4, 0, 0, 2, 3]                 # unlike the objects' order: two chains on object 0, object 1 unused
CHAINS = list(zip(OF_CHAIN, ('rotate', 'shift_up', 'clockwise_left', 'shift_down', 'rotate')))


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


def _mirrored(i):
    """Point-symmetric about the origin: different points at exactly equal distances, so most starts carry a tie flag; still uncrowded."""
    o = synth.synth_object_3d(i).clone()
    o[256:] = -o[:256]
    return o


def _ncr(dyn, cloud):
    return int((engine.debug_pointnet_indices(dyn, cloud)["crowded"] != 0).sum())


@pytest.fixture(scope="module")
def objs(dev, dyn):
    """crowded, uncrowded, a third, uncrowded with tie-flagged starts, a second crowded one"""
    second = next((i for i in (8, 3, 4, 5, 6, 7, 10, 11, 12) if _ncr(dyn, synth.synth_object_3d(i).to(dev)) > 0), None)
    assert second is not None, "no second crowded object among the candidates"
    o = torch.stack([synth.synth_object_3d(2), synth.synth_object_3d(1), synth.synth_object_3d(9), _mirrored(1), synth.synth_object_3d(second)]).to(dev)
    ncr = [_ncr(dyn, c) for c in o]
    assert ncr[0] > 0 and ncr[1] == 0 and ncr[3] == 0 and ncr[4] > 0, ncr
    return o


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.pop(k, None) for k in ("DGDM_SERIAL_STEP", "DGDM_EMBED_CALLS")}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _guidance(serial, dyn):
    with _env(**({"DGDM_SERIAL_STEP": serial} if serial else {})):         # read when the handle is created
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), len(CHAINS), T, N, SUB, max_objects=NOBJ)
    assert gd.rows == 24
    return gd


def _sched():
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(S)
    return s


def _chains(net, gd, dev, chains=CHAINS, seed=4):
    noise = synth.synth_noise(0, B, L).to(dev)
    _, step = sampler.draw_chain_starts(gd, chains, S, sampler.StartStream(N, SUB, seed=seed))
    return sampler.guided_chains(net, gd, _sched(), 'point_3d', noise, chains, predrawn=([None] * len(chains), step))


def _set(gd, objs):
    """The compared build, on slots that hold the tables of the reversed set."""
    gd.set_objects(objs.flip(0).contiguous())
    gd.set_objects(objs)


@pytest.fixture(scope="module")
def serial_ref(dev, dyn, net, objs):
    """The serial handle's results, computed once: the chains on objs, then on objs reversed."""
    gd = _guidance(1, dyn)
    _set(gd, objs)
    ok = gd.debug_fps_path(0)
    assert ok[1] and not ok[3], ok          # object 1 has no tie-flagged start, the mirrored one has
    a = _chains(net, gd, dev).cpu()
    gd.set_objects(objs.flip(0).contiguous())
    b = _chains(net, gd, dev, seed=5).cpu()
    assert float(a.abs().max()) > 0 and not torch.equal(a, b)
    return a, b


def test_chains_out_of_object_order(dev, dyn, net, objs, serial_ref):
    gd = _guidance(0, dyn)
    _set(gd, objs)
    assert torch.equal(_chains(net, gd, dev).cpu(), serial_ref[0])


def test_second_embed_meets_completed_events(dev, dyn, net, objs, serial_ref):
    gd = _guidance(0, dyn)
    _set(gd, objs)
    with _env(DGDM_EMBED_CALLS=2):           # read by every run: steps 0-1 and step 2 are embedded apart
        out = _chains(net, gd, dev)
    assert torch.equal(out.cpu(), serial_ref[0])


def test_back_to_back(dev, dyn, net, objs, serial_ref):
    """set_objects(X), chains, set_objects(Y), chains with no host synchronisation in between: the second build must not overwrite
    tables the first chains' gathers still read."""
    gd = _guidance(0, dyn)
    _set(gd, objs)
    a = _chains(net, gd, dev)
    gd.set_objects(objs.flip(0).contiguous())
    b = _chains(net, gd, dev, seed=5)
    assert torch.equal(a.cpu(), serial_ref[0])
    assert torch.equal(b.cpu(), serial_ref[1])


def test_serial_gather_switch(dev, dyn, net, objs, serial_ref):
    """DGDM_SERIAL_STEP=8: early read-back and events, one gather launch behind the joined build."""
    gd = _guidance(8, dyn)
    _set(gd, objs)
    assert torch.equal(_chains(net, gd, dev).cpu(), serial_ref[0])


def test_every_reader_first(dev, dyn, objs):
    """Each reader of the tables as the FIRST call after set_objects."""
    nc = len(CHAINS)
    x = torch.stack([synth.synth_noise(70 + i, B, L) for i in range(nc)]).clamp(-1, 1).reshape(nc, B, L).to(dev)
    objectives = [engine.make_objective(o, oi) for oi, o in CHAINS]
    res = []
    for serial in (1, 0):
        gd = _guidance(serial, dyn)
        ss = sampler.StartStream(N, SUB, seed=9)
        g_st = np.concatenate([ss.call(gd.rows) for _ in range(nc)])
        s_st = np.concatenate([ss.call(gd.sweep_rows) for _ in range(nc)])
        r_st = np.concatenate([ss.call(gd.sweep_rows) for _ in range(2 * nc)])
        readers = [lambda: (gd.grad(x, 3, objectives, None, g_st),),
                   lambda: gd.score(x, OF_CHAIN, (0.1, 0.1, 0.1), 3, g_st, want_logits=True),
                   lambda: (gd.sweep(x, OF_CHAIN, s_st),),
                   lambda: gd.rollout(x, OF_CHAIN, (0.3, 0.02, 0.02), 2, r_st)]
        out = []
        for fn in readers:
            _set(gd, objs)
            out.append([t.cpu() for t in fn()])
        res.append(out)
    for a, b in zip(*res):
        assert float(a[0].abs().max()) > 0
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_ensemble(dev, dyn, net, objs):
    """One chain with the mean of two objects' gradients (n_grad = 2): a crowded object behind the tie-flagged one."""
    noise = synth.synth_noise(0, B, L).to(dev)
    res = []
    for serial in (1, 0):
        gd = _guidance(serial, dyn)
        _set(gd, objs)
        res.append(sampler.guided_multi_object(net, gd, _sched(), 'point_3d', noise, [3, 0], 'shift_up',
                                               starts=sampler.StartStream(N, SUB, seed=6)).cpu())
    assert float(res[0].abs().max()) > 0
    assert torch.equal(res[0], res[1])


def test_m0_only_chains(dev, dyn, net, objs):
    """Every chain on the uncrowded object without tie flags: no gather launch, the index kernel alone runs ahead of the build's end."""
    chains = [(1, 'rotate'), (1, 'shift_up')]
    res = []
    for serial in (1, 0):
        gd = _guidance(serial, dyn)
        _set(gd, objs)
        res.append(_chains(net, gd, dev, chains, seed=7).cpu())
    assert float(res[0].abs().max()) > 0
    assert torch.equal(res[0], res[1])


def test_wait_then_host_read(dev, dyn, objs):
    """set_objects(wait=True) still means that the tables exist; the host-side flags behind it are those of the serial build."""
    ok = []
    for serial in (1, 0):
        gd = _guidance(serial, dyn)
        gd.set_objects(objs.flip(0).contiguous())
        gd.set_objects(objs, wait=True)
        ok.append(gd.debug_fps_path(0))
    assert len(ok[0]) == NOBJ and ok[0] == ok[1]
    assert ok[1][1] and not ok[1][3], ok[1]
