"""The conditional eps-net on the HIP path: ``global_cond`` through the forward kernels (per-sample and batched form), the trainer, the
chain runner with classifier-free guidance, ``Diffusion`` and the command line.

References: tests/golden/g15_unet_cond.npz (the reference's own ConditionalUnet1D with global_cond_dim > 0, make_golden_cond.py) and
tests/cond_oracle.py (pinned to that fixture by tests/test_cond_oracle.py) in float32 / float64."""
import math
import os

import numpy as np
import pytest
import torch

from dgdm_amd import engine, sampler, synth
from dgdm_amd.scheduler import DDIMScheduler
from tests import cond_oracle as co
from tests import util
from tests.util import sample_idx

pytestmark = pytest.mark.gpu
REL = 2e-5                      # tests/test_gpu_parity.py REL
FULL_GRADS = ("mid_modules.0.cond_encoder.1.weight", "down_modules.0.0.cond_encoder.1.weight")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def _sd(gc, seed=11):
    return synth.synth_state_dict(synth.unet_spec(global_cond_dim=gc), int(seed))


def _cond(seed, B, gc, zero_row=None):
    c = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (B, gc)).astype(np.float32))
    if zero_row is not None:
        c[zero_row] = 0.0
    return c


def _two_forms(sd):
    """(per-sample handle, batched handle) through the DGDM_UNET_BATCHED_MIN hook."""
    env = os.environ.get("DGDM_UNET_BATCHED_MIN")
    try:
        os.environ["DGDM_UNET_BATCHED_MIN"] = "0"
        per_sample = engine.Unet1d(sd)
        os.environ["DGDM_UNET_BATCHED_MIN"] = "1"
        batched = engine.Unet1d(sd)
    finally:
        if env is None:
            os.environ.pop("DGDM_UNET_BATCHED_MIN", None)
        else:
            os.environ["DGDM_UNET_BATCHED_MIN"] = env
    return per_sample, batched


def _coefs(T, ts):
    ac = DDIMScheduler(num_train_timesteps=T).alphas_cumprod[ts]
    return ac ** 0.5, (1 - ac) ** 0.5


# ------------------------------------------------------------------------------------------------ 1. golden forward
@pytest.mark.parametrize("gc", [1, 6, 16])
def test_cond_forward_golden(dev, gc):
    from dgdm_amd.generator.diffusion_utils import ConditionalUnet1D
    g = util.load("g15_unet_cond.npz")
    sd = _sd(gc, g["seed"])
    mod = ConditionalUnet1D(input_dim=1, global_cond_dim=gc, down_dims=[128, 256], diffusion_step_embed_dim=32)
    mod.load_state_dict(sd)
    mod = mod.to(dev)
    net = engine.Unet1d(sd)
    assert net.global_cond_dim == gc
    t = torch.from_numpy(g["fwd_t"]).to(dev)
    for L in (14, 42):
        x, c, ref = (torch.from_numpy(g[f"fwd_gc{gc}_L{L}_{k}"]) for k in ("x", "cond", "y"))
        y = mod.forward(x.to(dev), t, c.to(dev))
        e1, e2 = util.rel_l2(y.cpu(), ref), util.rel_l2(net.forward(x.to(dev), t, c.to(dev)).cpu(), ref)
        print(f"gc={gc} L={L}: module {e1:.2e}, engine {e2:.2e}")
        assert e1 < REL and e2 < REL, (L, e1, e2)
        # the condition reaches the output: the same call with the rows rolled by one is far from the fixture
        d = util.rel_l2(net.forward(x.to(dev), t, torch.roll(c, 1, 0).to(dev)).cpu(), ref)
        assert d > 1e-2, (L, d)


# ------------------------------------------------------------------------------------------------ 2. arithmetic modes against float64
@pytest.mark.parametrize("L", [14, 42, 44])
def test_cond_arithmetic_modes_vs_float64(dev, L):
    """The assertions of test_gpu_parity.py::test_unet_arithmetic_modes_vs_float64 with a condition (gc = 6)."""
    gc = 6
    sd = _sd(gc, 7)
    sd64 = {k: v.double() for k, v in sd.items()}
    x = torch.randn(64, L, 1, generator=torch.Generator().manual_seed(3))
    t = torch.randint(0, 15, (64,), generator=torch.Generator().manual_seed(1))
    c = _cond(9, 64, gc, zero_row=5)
    with torch.no_grad():
        ref = co.unet1d_forward_cond(sd64, x.double(), t, c.double())
    out = {m: engine.Unet1d(sd, contraction_dtype=m).forward(x.to(dev), t.to(dev), c.to(dev)).cpu().double() for m in ("f32", "f32_mfma", "bf16")}
    err = {m: float((o - ref).norm() / ref.norm()) for m, o in out.items()}
    print(f"L={L}: {err}")
    assert err["f32_mfma"] < 1e-6 and err["f32"] < 1e-6 and err["f32"] <= err["f32_mfma"] + 1e-7, err
    assert float((out["f32"] - out["f32_mfma"]).norm() / ref.norm()) < 2e-6
    assert 1e-4 < err["bf16"] < 2e-2, err


@pytest.mark.parametrize("gc", [6, 64, 256])
def test_cond_effective_form_and_wide_condition(dev, gc):
    """The split form is what runs at L = 14 and 42 up to gc = 64; gc = 256 runs what the handle reports and still meets the 1e-6."""
    sd = _sd(gc, 7)
    net = engine.Unet1d(sd)
    if gc <= 64:
        assert net.effective_form(4, 14) == ("f32_f16x3", False) and net.effective_form(4, 42) == ("f32_f16x3", False)
        return
    sd64 = {k: v.double() for k, v in sd.items()}
    for L in (14, 42):
        form = net.effective_form(8, L)
        assert form[0] in ("f32_f16x3", "f32_mfma")
        x = torch.randn(8, L, 1, generator=torch.Generator().manual_seed(L))
        t = torch.randint(0, 15, (8,), generator=torch.Generator().manual_seed(2))
        c = _cond(L, 8, gc)
        with torch.no_grad():
            ref = co.unet1d_forward_cond(sd64, x.double(), t, c.double())
        y = net.forward(x.to(dev), t.to(dev), c.to(dev)).cpu().double()
        e = float((y - ref).norm() / ref.norm())
        print(f"gc=256 L={L}: {form}, {e:.2e}")
        assert e < 1e-6, (L, form, e)


# ------------------------------------------------------------------------------------------------ 3. batched form == per-sample form
@pytest.mark.parametrize("gc", [1, 6])
def test_cond_batched_equals_per_sample(dev, gc):
    sd = _sd(gc)
    per_sample, batched = _two_forms(sd)
    g = torch.Generator().manual_seed(5 + gc)
    for L in (42, 14):
        assert batched.effective_form(130, L) == ("f32_f16x3", True) and per_sample.effective_form(130, L) == ("f32_f16x3", False)
        for B in (130, 37, 5, 4, 3, 1):
            x = torch.randn((B, L, 1), generator=g).to(dev)
            c = torch.rand((B, gc), generator=g).mul(2).sub(1).to(dev)
            # mixed timesteps
            t = torch.randint(0, 15, (B,), generator=g).to(dev)
            a, b = per_sample.forward(x, t, c), batched.forward(x, t, c)
            assert bool(torch.isfinite(b).all())
            assert torch.equal(a, b), (L, B, float((a - b).abs().max()))
            # ALL timesteps equal, all condition rows different: one shared FiLM row would hand every sample row 0's
            t = torch.full((B,), 7, dtype=torch.int64, device=dev)
            a, b = per_sample.forward(x, t, c), batched.forward(x, t, c)
            assert torch.equal(a, b), ("equal timesteps", L, B, float((a - b).abs().max()))
            for s in range(B):                                    # row s is the B = 1 evaluation of sample s
                one = per_sample.forward(x[s:s + 1], t[s:s + 1], c[s:s + 1])
                assert torch.equal(one[0], b[s]), ("row", L, B, s)
    with torch.no_grad():
        ref = co.unet1d_forward_cond(sd, x.cpu(), t.cpu(), c.cpu())
    assert util.rel_l2(b.cpu(), ref) < REL


# ------------------------------------------------------------------------------------------------ 4. degenerate and error paths
def test_cond_degenerate_and_error_paths(dev):
    from dgdm_amd import _lib
    lib = _lib.lib()
    x = synth.synth_noise(1, 5, 14).to(dev)
    t = torch.tensor([0, 3, 7, 12, 14], dtype=torch.int32, device=dev)
    # gc = 0: forward_cond(NULL) is forward
    net0 = engine.Unet1d(util.unet_sd(11))
    assert net0.global_cond_dim == 0
    a = net0.forward(x, t)
    b = torch.empty_like(x)
    _lib.check(lib.dgdm_unet1d_forward_cond(net0._h, x.data_ptr(), t.data_ptr(), None, b.data_ptr(), 5, 14, _lib.stream_ptr()))
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        net0.forward(x, t, torch.zeros(5, 3, device=dev))
    # gc > 0
    gc = 6
    sd = _sd(gc)
    net = engine.Unet1d(sd)
    c = _cond(4, 5, gc).to(dev)
    good = net.forward(x, t, c)
    with torch.no_grad():
        assert util.rel_l2(good.cpu(), co.unet1d_forward_cond(sd, x.cpu(), t.cpu().long(), c.cpu())) < REL
    out = torch.full_like(x, 7.0)
    assert lib.dgdm_unet1d_forward(net._h, x.data_ptr(), t.data_ptr(), out.data_ptr(), 5, 14, _lib.stream_ptr()) == _lib.EINVAL
    assert lib.dgdm_unet1d_forward_cond(net._h, x.data_ptr(), t.data_ptr(), None, out.data_ptr(), 5, 14, _lib.stream_ptr()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                   # nothing was launched
    assert torch.equal(net.forward(x, t, c), good)
    with pytest.raises(ValueError):
        net.forward(x, t)
    assert torch.equal(net.forward(x, t, c), good)
    with pytest.raises(ValueError):
        net.forward(x, t, torch.zeros(5, gc + 1, device=dev))
    with pytest.raises(ValueError):
        net.forward(x, t, torch.zeros(4, gc, device=dev))
    assert torch.equal(net.forward(x, t, c), good)
    # the eight cond encoders must agree
    bad = dict(sd)
    k = "mid_modules.1.cond_encoder.1.weight"
    bad[k] = torch.cat((sd[k], torch.zeros(sd[k].shape[0], 2)), dim=1)
    with pytest.raises(_lib.DgdmError, match="mid_modules.1.cond_encoder.1.weight"):
        engine.Unet1d(bad)
    with pytest.raises(_lib.DgdmError, match="cond_encoder"):
        engine.UnetTrainer(bad, 14)
    assert torch.equal(net.forward(x, t, c), good)


# ------------------------------------------------------------------------------------------------ 5. trainer golden
@pytest.mark.parametrize("tag", ["p2", "p3"])
def test_cond_trainer_golden(tag):
    """test_gpu_unet_train.py::test_unet_trainer_golden's bounds on the conditional fixture, plus the two full cond_encoder gradients:
    rel L2 < 2e-4 on the step columns and, separately, on the global columns (7 % of the step columns' norm)."""
    g = util.load("g15_unet_cond.npz")
    gc = int(g["train_gc"])
    B, L = [int(v) for v in g[f"{tag}_dims"]]
    T, lr0, E = int(g["num_train_timesteps"]), float(g["lr"]), int(g["num_epochs"])
    tr = engine.UnetTrainer(_sd(gc, g["seed"]), L)
    assert tr.global_cond_dim == gc
    x0, c = torch.from_numpy(g[f"{tag}_x0"]), torch.from_numpy(g[f"{tag}_cond"])
    for step in range(3):
        lr = lr0 if step < 2 else lr0 * (1 + math.cos(math.pi / E)) / 2
        assert abs(lr - float(g[f"{tag}_lr{step}"])) < 1e-12
        noise, ts = torch.from_numpy(g[f"{tag}_noise{step}"]), torch.from_numpy(g[f"{tag}_t{step}"])
        sa, sb = _coefs(T, ts)
        loss, _ = tr.step(x0, noise, sa, sb, ts, lr, global_cond=c)
        ref = float(g[f"{tag}_loss{step}"])
        print(f"{tag} step {step}: loss {loss:.7f} (reference {ref:.7f})")
        assert abs(loss - ref) < 2e-5 * abs(ref), (step, loss, ref)
        if step == 0:
            grads = tr.export(1)
            worst = 0.0
            for k, v in grads.items():
                f = v.double().flatten().numpy()
                refg, (s1, s2) = g[f"{tag}_grad/{k}"], g[f"{tag}_gradsum/{k}"]
                rms = math.sqrt(s2 / f.size)
                err = np.abs(f[sample_idx(k, f.size)] - refg).max() / rms
                worst = max(worst, err)
                assert err < 5e-5, (k, err)
                assert abs((f * f).sum() - s2) < 1e-4 * s2, (k, (f * f).sum(), s2)
            print(f"{tag}: worst sampled gradient entry error / tensor rms {worst:.2e}")
            for k in FULL_GRADS:
                full = g[f"{tag}_fullgrad/{k}"]
                es, eg = util.rel_l2(grads[k][:, :32], full[:, :32]), util.rel_l2(grads[k][:, 32:], full[:, 32:])
                print(f"{tag} {k}: step columns {es:.2e}, global columns {eg:.2e}")
                assert es < 2e-4, (k, es)
                assert eg < 2e-4, (k, eg)
    final = tr.export(0)
    flips = 0
    for k, v in final.items():
        f = v.double().flatten().numpy()
        d = np.abs(f[sample_idx(k, f.size)] - g[f"{tag}_final/{k}"])
        flips += int((d > 4e-6).sum())
        assert d.max() < 3 * 2 * lr0 + 1e-6, (k, d.max())
        s1, s2 = g[f"{tag}_finalsum/{k}"]
        assert abs((f * f).sum() - s2) < 1e-5 * s2 + 1e-12, (k, (f * f).sum(), s2)
    assert flips <= 2, flips


# ------------------------------------------------------------------------------------------------ 6. trainer against cond_oracle
@pytest.mark.parametrize("B,L,gc", [(1, 14, 6), (9, 42, 5)])
def test_cond_trainer_vs_oracle(B, L, gc):
    """Loss, noise prediction and every gradient tensor against cond_oracle's autograd (gc = 5: not a multiple of 4; B = 1); two runs
    give the same bits; export -> import resumes bit for bit; forward_backward on two halves, gradients summed, is one step."""
    T = 15
    sd = _sd(gc, 5)
    rs = np.random.RandomState(B * 100 + L)
    x0 = torch.from_numpy(rs.uniform(-1, 1, (B, L, 1)).astype(np.float32))
    noise = torch.from_numpy(rs.normal(size=(B, L, 1)).astype(np.float32))
    ts = torch.from_numpy(rs.randint(0, T, B))
    c = _cond(B + L, B, gc, zero_row=0 if B > 1 else None)
    sa, sb = _coefs(T, ts)
    lo, po, go = co.loss_and_grads(sd, T, x0, noise, ts, c)
    a, b = engine.UnetTrainer(sd, L), engine.UnetTrainer(sd, L)
    with pytest.raises(ValueError):
        a.step(x0, noise, sa, sb, ts, 1e-4)                           # a condition is required
    with pytest.raises(ValueError):
        a.step(x0, noise, sa, sb, ts, 1e-4, global_cond=torch.zeros(B, gc + 1))
    la, pa = a.step(x0, noise, sa, sb, ts, 1e-4, want_pred=True, global_cond=c)
    lb, _ = b.step(x0, noise, sa, sb, ts, 1e-4, global_cond=c)
    assert la == lb
    assert abs(la - lo) < 2e-5 * abs(lo), (la, lo)
    assert util.rel_l2(pa.cpu(), po) < REL
    ga, gb = a.export(1), b.export(1)
    assert all(torch.equal(ga[k], gb[k]) for k in ga)
    errs = sorted(((util.rel_l2(ga[k], go[k]), k) for k in ga), reverse=True)
    print(f"B={B} L={L} gc={gc}: loss {la:.6f} (oracle {lo:.6f}), worst gradient tensor rel L2 {errs[0][0]:.2e} ({errs[0][1]})")
    assert errs[0][0] < 2e-4, errs[:5]
    for k in FULL_GRADS:
        assert util.rel_l2(ga[k][:, 32:], go[k][:, 32:]) < 2e-4, k
    pa_, pb_ = a.export(0), b.export(0)
    assert all(torch.equal(pa_[k], pb_[k]) for k in pa_)
    # resume
    r = engine.UnetTrainer(pa_, L)
    r.load(2, a.export(2))
    r.load(3, a.export(3), adam_steps=a.steps())
    la, _ = a.step(x0, noise, sa, sb, ts, 5e-5, global_cond=c)
    lr_, _ = r.step(x0, noise, sa, sb, ts, 5e-5, global_cond=c)
    assert la == lr_
    pa_, pr_ = a.export(0), r.export(0)
    assert all(torch.equal(pa_[k], pr_[k]) for k in pa_)
    # data-parallel split (B >= 2): the halves' gradients add up to the whole batch's
    if B >= 2:
        h = B // 2
        whole, parts = engine.UnetTrainer(sd, L), engine.UnetTrainer(sd, L)
        lw, _ = whole.forward_backward(x0, noise, sa, sb, ts, global_cond=c)
        gw = whole.read_gradients()
        l1, _ = parts.forward_backward(x0[:h], noise[:h], sa[:h], sb[:h], ts[:h], total_samples=B, global_cond=c[:h])
        g1 = parts.read_gradients()
        l2, _ = parts.forward_backward(x0[h:], noise[h:], sa[h:], sb[h:], ts[h:], total_samples=B, global_cond=c[h:])
        g2 = parts.read_gradients()
        assert abs((l1 + l2) - lw) < 2e-5 * abs(lw)
        assert util.rel_l2((g1 + g2).cpu(), gw.cpu()) < 2e-4               # (only the order of the sums over the samples differs)
        parts.write_gradients(g1 + g2)
        parts.apply(1e-4)
        whole.apply(1e-4)
        pw, pp = whole.export(0), parts.export(0)
        assert max(float((pw[k] - pp[k]).abs().max()) for k in pw) < 2.5e-4      # <= 2 lr wherever a gradient's sign is rounding's


# ------------------------------------------------------------------------------------------------ 7. chain runner
def _compose(net, gd, s, noise, objectives, scales, cond, w, starts=None):
    """The step-by-step composition: forward with condition (+ the classifier-free mix in three separate float32 torch operations),
    Guidance.grad, ddim_guided_step.  cond (nc, B, gc); every chain's eps-net call covers all nc * B samples at every step."""
    nc, (B, L) = len(objectives), noise.shape[:2]
    x = noise.reshape(1, B, L).expand(nc, -1, -1).contiguous()
    crow = cond.reshape(nc * B, -1)
    for si, t in enumerate(s.timesteps):
        t = int(t)
        ts = torch.full((nc * B,), t, dtype=torch.int32, device=x.device)
        if w == 1.0:
            eps = net.forward(x.reshape(nc * B, L, 1), ts, crow)
        else:
            ec, eu = net.forward(x.reshape(nc * B, L, 1), ts, crow), net.forward(x.reshape(nc * B, L, 1), ts, torch.zeros_like(crow))
            d = ec - eu
            d = d * w
            eps = eu + d
        g = gd.grad(x, t, objectives, None, starts[si].reshape(-1) if starts is not None else None)
        coef = s.coefficients(t)
        x = torch.stack([engine.ddim_guided_step(x[c], eps.reshape(nc, B, L)[c], g[c], 1, coef, scales[c]) for c in range(nc)])
    return x.reshape(nc, B, L, 1)


def test_cond_chain_runner_2d(dev):
    g3 = util.load("g3_dyn2d.npz")
    B, G, P, L, T, _, nv = [int(v) for v in g3["dims"]]
    assert (B, G, P) == (2, 4, 2)
    gc, S = 6, 3
    net = engine.Unet1d(_sd(gc))
    dyn = engine.Dynamics(2, util.dyn2d_sd(g3["seed"], nv), L, 2 * nv)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 4, T, nv, 0, max_objects=2)
    gd.set_objects(torch.stack([synth.synth_object_2d(i, nv) for i in range(2)]).to(dev))
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(S)
    noise = synth.synth_noise(0, B, L).to(dev)
    chains = [(0, 'rotate'), (1, 'shift_left'), (0, 'counterclockwise_up')]
    nc = len(chains)
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    scales = [sampler.chain_scale('point', o) for _, o in chains]
    cond = torch.stack([_cond(20 + k, B, gc) for k in range(nc)]).to(dev)
    run = lambda **kw: sampler.guided_chains(net, gd, s, 'point', noise, chains, **kw)       # noqa: E731
    # (a) per-chain conditions: the library's loop is the composition, step 0 included
    a = run(global_cond=cond)
    ref = _compose(net, gd, s, noise, objectives, scales, cond, 1.0)
    assert torch.equal(a, ref), float((a - ref).abs().max())
    assert torch.equal(a, run(global_cond=cond, trace=[]))
    assert not torch.equal(a, run(global_cond=torch.roll(cond, 1, 0)))
    # (b) one shared block is three copies of it
    shared = run(global_cond=cond[1])
    assert torch.equal(shared, run(global_cond=cond[1:2].expand(nc, -1, -1).contiguous()))
    assert torch.equal(shared, run(global_cond=cond[1], trace=[]))
    # (c) classifier-free guidance
    assert torch.equal(run(global_cond=cond, cfg_weight=1.0), a)
    zero = run(global_cond=torch.zeros_like(cond))
    assert torch.equal(run(global_cond=cond, cfg_weight=0.0), zero)
    assert not torch.equal(zero, a)
    mixed = run(global_cond=cond, cfg_weight=2.5)
    ref = _compose(net, gd, s, noise, objectives, scales, cond, 2.5)
    e = util.rel_l2(mixed.cpu(), ref.cpu())
    print(f"cfg_weight 2.5 against the composition: rel L2 {e:.2e}")
    assert e < 1e-6
    assert torch.equal(mixed, run(global_cond=cond, cfg_weight=2.5, trace=[]))
    ms = run(global_cond=cond[1], cfg_weight=2.5)                    # shared block + mix: step 0 evaluates 2 B samples
    assert torch.equal(ms, run(global_cond=cond[1:2].expand(nc, -1, -1).contiguous(), cfg_weight=2.5))
    # shape errors are raised before anything runs
    with pytest.raises(ValueError):
        run()
    with pytest.raises(ValueError):
        run(global_cond=cond[:2])
    with pytest.raises(ValueError):
        run(global_cond=cond[..., :gc - 1].contiguous())
    # the C entry point: a chain stride that is neither 0 nor B * gc, or a missing condition, is DGDM_EINVAL before anything is launched
    import ctypes as C
    from dgdm_amd import _lib
    arr = (_lib.Objective * nc)(*objectives)
    tsa = (C.c_int32 * S)(*[int(t) for t in s.timesteps])
    cfa = (C.c_float * (4 * S))(*[float(v) for t in s.timesteps for v in s.coefficients(int(t))])
    sca = (C.c_float * nc)(*scales)
    x0, out = noise.reshape(B, L).contiguous(), torch.full((nc, B, L), 7.0, device=dev)
    call = lambda cptr, stride: _lib.lib().dgdm_guided_chains_run_cond(net._h, gd._h, x0.data_ptr(), nc, 1, arr, None, None, tsa, cfa, sca, S,      # noqa: E731
                                                                       out.data_ptr(), cptr, stride, 1.0, _lib.stream_ptr())
    assert call(cond.data_ptr(), B * gc + 1) == _lib.EINVAL and call(cond.data_ptr(), gc) == _lib.EINVAL and call(None, 0) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(cond.data_ptr(), B * gc) == _lib.OK and torch.equal(out.reshape(a.shape), a)
    # the unconditional mix call of the sampler: one forward of 2 B samples and the library's mix
    ug = sampler.unguided_sample(net, s, noise, global_cond=cond[0], cfg_weight=2.5)
    x = noise.clone()
    for t in s.timesteps:
        ts = torch.full((B,), int(t), dtype=torch.int32, device=dev)
        ec, eu = net.forward(x, ts, cond[0]), net.forward(x, ts, torch.zeros_like(cond[0]))
        x = engine.ddim_guided_step(x, engine.cfg_mix(ec, eu, 2.5), None, 0, s.coefficients(int(t)), 0.0)
    assert torch.equal(ug, x)


def test_cond_chain_runner_3d(dev):
    """One 3-D case (the small grid of test_gpu_table_sharing.py's run): the FPS start indices travel beside a per-chain condition."""
    L, T, N, B, G, P, sub, gc, S = 42, 15, 512, 2, 12, 3, 64, 6, 3
    net = engine.Unet1d(_sd(gc))
    dyn = engine.Dynamics(3, util.dyn3d_sd(44), L)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 2, T, N, sub, max_objects=2)
    objs = torch.stack([synth.synth_object_3d(i) for i in (1, 2)]).to(dev)
    gd.set_objects(objs)
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(S)
    noise = synth.synth_noise(0, B, L).to(dev)
    chains = [(0, 'rotate'), (1, 'shift_up')]
    cond = torch.stack([_cond(30 + k, B, gc) for k in range(2)]).to(dev)
    _, step = sampler.draw_chain_starts(gd, chains, S, sampler.StartStream(N, sub, seed=4))
    a = sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, predrawn=([None, None], step), global_cond=cond)
    gd.set_objects(objs)
    ref = _compose(net, gd, s, noise, [engine.make_objective(o, oi) for oi, o in chains], [sampler.chain_scale('point_3d', o) for _, o in chains],
                   cond, 1.0, starts=step)
    assert torch.equal(a, ref), float((a - ref).abs().max())


# ------------------------------------------------------------------------------------------------ 8. Diffusion and the command line
def test_cond_diffusion_api(dev):
    """training_step((x, c)) twice, validation_step((x, c)), a checkpoint round trip with equal eps afterwards, a width mismatch."""
    from dgdm_amd.generator.diffusion import Diffusion
    from dgdm_amd.generator.diffusion_utils import ConditionalUnet1D
    B, L, T, gc = 6, 14, 15, 5
    sd = _sd(gc, 21)

    def make(g=gc):
        net = ConditionalUnet1D(input_dim=1, global_cond_dim=g, down_dims=[128, 256], diffusion_step_embed_dim=32)
        if g == gc:
            net.load_state_dict(sd)
        d = Diffusion(noise_pred_net=net, noise_scheduler=DDIMScheduler(num_train_timesteps=T), num_inference_steps=5, mode='point', input_dim=1,
                      num_points=L, learning_rate=1e-4, ema_power=0.85).to(dev)
        d.configure_optimizers()
        return d
    d = make()
    d.cond_drop_prob, d.cfg_weight = 0.5, 2.0
    x0 = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (B, L, 1)).astype(np.float32))
    c = _cond(3, B, gc)
    with pytest.raises(ValueError):
        d.training_step(x0, 0)                                        # a conditional net needs (fingers, condition) batches
    with pytest.raises(ValueError):
        d.training_step((x0, c[:, :gc - 1]), 0)
    # the first step against cond_oracle on the same device-generator draws (drop-out included)
    torch.manual_seed(100)
    noise = torch.randn((B, L, 1), device=dev).cpu()
    ts = torch.randint(0, T, (B,), device=dev).long().cpu()
    drop = (torch.rand(B, device=dev) < 0.5).cpu()
    lo, _, _ = co.loss_and_grads(sd, T, x0, noise, ts, torch.where(drop[:, None], torch.zeros_like(c), c))
    losses = []
    for step in range(2):
        torch.manual_seed(100 + step)
        losses.append(float(d.training_step((x0, c), step)))
        d.on_train_batch_end(None, (x0, c), step)
    assert abs(losses[0] - lo) < 2e-5 * abs(lo), (losses[0], lo)
    assert "loss" in d.get_stats((x0, c))
    d.eval()
    out = d.validation_step((x0, c), 0)
    assert set(out["stats"]) == {"val/noise pred loss", "val/denoise loss", "val/accuracy"} and all(np.isfinite(v) for v in out["stats"].values())
    assert out["unguided"].shape == (B, L, 1) and bool(torch.isfinite(out["unguided"]).all())
    # the unguided sample is the sampler's with this condition and weight, and the condition matters
    noise0 = torch.from_numpy(np.random.RandomState(d.seed).randn(B, L, 1)).float().to(dev)
    assert torch.equal(out["unguided"], sampler.unguided_sample(d._net(), d.noise_scheduler, noise0, global_cond=c.to(dev), cfg_weight=2.0))
    assert not torch.equal(out["unguided"], d.validation_step((x0, torch.roll(c, 1, 0)), 0)["unguided"])
    # checkpoint round trip
    ck = d.checkpoint(epoch=1, global_step=2)
    assert ck["state_dict"]["ema_nets.noise_pred_net.mid_modules.0.cond_encoder.1.weight"].shape == (512, 32 + gc)
    assert ck["state_dict"]["ema_model"]["noise_pred_net.mid_modules.0.cond_encoder.1.weight"].shape == (512, 32 + gc)
    d2 = make()
    d2.load_checkpoint(ck)
    xs = torch.from_numpy(np.random.RandomState(0).randn(B, L, 1).astype(np.float32)).to(dev)
    t3 = torch.full((B,), 3, device=dev)
    assert torch.equal(d.noise_pred_net(xs, t3, c.to(dev)), d2.noise_pred_net(xs, t3, c.to(dev)))
    d.cond_drop_prob = d2.cond_drop_prob = 0.25
    torch.manual_seed(5)
    la = float(d.training_step((x0, c), 2))
    torch.manual_seed(5)
    lb = float(d2.training_step((x0, c), 2))
    assert la == lb
    pa, pb = d._trainer().export(0), d2._trainer().export(0)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    with pytest.raises(ValueError, match=str(32 + gc)):
        make(0).load_checkpoint(ck)
    with pytest.raises(ValueError, match=str(32 + gc)):
        make(gc + 1).load_checkpoint(ck)


def test_cond_diffusion_guided_sweep(dev):
    """validation_step((x, c)) with classifier guidance on a tiny 2-D grid: the batch's condition rows, shared by all chains, reach the
    multi-object chain and every per-object chain (each equals the sampler's call with that condition and weight)."""
    from dgdm_amd.dynamics.profile_forward_2d import ProfileForward2DModel
    from dgdm_amd.generator.diffusion import Diffusion
    from dgdm_amd.generator.diffusion_utils import ConditionalUnet1D
    B, G, P, L, T, nv, gc = 2, 4, 2, 14, 15, 10, 4
    net = ConditionalUnet1D(input_dim=1, global_cond_dim=gc, down_dims=[128, 256], diffusion_step_embed_dim=32)
    net.load_state_dict(_sd(gc))
    dyn = ProfileForward2DModel(output_ch=3, params_ch=L, object_ch=2 * nv)
    dyn.load_state_dict(util.dyn2d_sd(22, nv))
    objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(2)])
    d = Diffusion(noise_pred_net=net, noise_scheduler=DDIMScheduler(num_train_timesteps=T), num_inference_steps=3, mode='point', input_dim=1,
                  num_points=L, class_cond=True, classifier_model=dyn.to(dev).eval(), grid_size=G, num_pos=P, object_vertices=objs,
                  object_ids=[0, 1], seed=0).to(dev).eval()
    d.cfg_weight = 1.5
    x0 = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (B, L, 1)).astype(np.float32))
    c = _cond(8, B, gc).to(dev)
    out = d.validation_step((x0, c), 0)
    noise = torch.from_numpy(np.random.RandomState(0).randn(B, L, 1)).float().to(dev)
    gd = d._guidance_for(B, [-1.0, 1.0], objs, 2)
    ref = sampler.guided_chains(d._net(), gd, d.noise_scheduler, 'point', noise, [(0, 'rotate'), (1, 'rotate')], global_cond=c, cfg_weight=1.5)
    assert torch.equal(out["guided/rotate"], ref)
    ref = sampler.guided_multi_object(d._net(), gd, d.noise_scheduler, 'point', noise, [0, 1], 'shift_up', global_cond=c, cfg_weight=1.5)
    assert torch.equal(out["multi/shift_up"], ref)
    other = sampler.guided_chains(d._net(), gd, d.noise_scheduler, 'point', noise, [(0, 'rotate'), (1, 'rotate')], global_cond=torch.roll(c, 1, 0),
                                  cfg_weight=1.5)
    assert not torch.equal(out["guided/rotate"], other)
    with pytest.raises(ValueError):
        d.validation_step(x0, 0)


def test_cond_train_cli_end_to_end(tmp_path):
    """`python generator/train.py --mode=train ... --global_cond f.npy --cond_drop_prob 0.5` for two epochs, then `--mode=test ...
    --global_cond f.npy --cfg_weight 2` on the checkpoint it wrote (as test_gpu_unet_train.py::test_train_cli_end_to_end does)."""
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    n, gc = 160, 3
    f = tmp_path / "cond.npy"
    np.save(f, np.random.RandomState(0).uniform(-1, 1, (n, gc)).astype(np.float32))
    save = tmp_path / "out"
    base = [sys.executable, "generator/train.py", f"--num_fingers={n}", "--num_workers=0", "--num_train_timesteps=15", "--num_inference_steps=5",
            "--ema_power=0.85", "--ctrlpts_dim=14", f"--global_cond={f}"]
    r = subprocess.run(base + [f"--save_dir={save}", "--learning_rate=1e-3", "--lr_warmup_steps=0", "--val_step=2", "--batch_size=32", "--num_epochs=2",
                               "--cond_drop_prob=0.5"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if "train/loss=" in l]
    losses = [float(l.split("train/loss=")[1].split(",")[0]) for l in lines]
    assert len(losses) == 2 and losses[1] < losses[0], losses
    assert any("val/denoise loss" in l for l in lines)
    ck = torch.load(save / "checkpoints" / "last.ckpt", weights_only=False)
    assert ck["epoch"] == 2 and ck["state_dict"]["ema_nets.noise_pred_net.mid_modules.0.cond_encoder.1.weight"].shape == (512, 32 + gc)
    # sampling: its own finger set (8 fingers, two batches) with its own condition rows, on the checkpoint just written
    f2 = tmp_path / "cond_test.npy"
    np.save(f2, np.random.RandomState(1).uniform(-1, 1, (8, gc)).astype(np.float32))
    r = subprocess.run([sys.executable, "generator/train.py", "--mode=test", "--num_fingers=8", "--batch_size=4", "--ctrlpts_dim=14",
                        "--num_train_timesteps=15", "--num_inference_steps=5", f"--global_cond={f2}", "--cfg_weight=2",
                        f"--diffusion_checkpoint_path={save / 'checkpoints' / 'last.ckpt'}", f"--save_dir={tmp_path / 'smp'}"],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "diffusion checkpoint" not in r.stderr          # the trained checkpoint was read
    assert sum("val/denoise loss" in l for l in r.stdout.splitlines()) == 2
    assert (tmp_path / "smp" / "val_vis_noise" / "unguided" / "unguided.npy").exists()
