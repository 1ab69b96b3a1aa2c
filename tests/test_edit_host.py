"""Host side of editing designs (dgdm_amd/edit.py): flag parsing, unit conversion, validation, bounds, the start of an edit, and the
float32 restatement of the bounded step (tests/edit_oracle.py) the GPU tests compare the kernel with.  No GPU."""
import numpy as np
import pytest
import torch

from dgdm_amd import _lib, edit as ed
from dgdm_amd.scheduler import DDIMScheduler
from oracle import dgdm_oracle as orc
from tests import edit_oracle


def _sched(T=15, S=5):
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(S)
    return s


def _designs(B=3, L=14, seed=0):
    return np.random.RandomState(seed).uniform(-0.9, 0.9, (B, L)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. parsing
def test_pin_parsing():
    assert ed.parse_pins("0-6,10", 14) == (0, 1, 2, 3, 4, 5, 6, 10)
    assert ed.parse_pins("3", 14) == (3,)
    assert ed.parse_pins(" 2 , 5-7 ", 14) == (2, 5, 6, 7)
    assert ed.parse_pins("3,1-4,3,2", 14) == (1, 2, 3, 4)              # duplicates and overlaps: each index once, sorted
    assert ed.parse_pins("13", 14) == (13,)
    assert ed.parse_pins(None, 14) == () and ed.parse_pins("", 14) == ()
    for bad in ("14", "0-14", "-1", "5-3", "a", "1,,2", "1-2-3", "1.5"):
        with pytest.raises(ValueError):
            ed.parse_pins(bad, 14)


def test_flags_need_edit_from(tmp_path):
    from dgdm_amd.dynamics.parser import parse
    base = "--mode=test --classifier_guidance --batch_size=2 --num_inference_steps=5"
    assert ed.plan_from_args(parse(base.split())) is None
    for extra in ("--pin 0-6", "--edit_band_mm 2", "--edit_steps 3"):
        with pytest.raises(ValueError, match="edit_from"):
            ed.plan_from_args(parse((base + " " + extra).split()))
    f = str(tmp_path / "d.npy")
    np.save(f, _designs(5, 14)[..., None])                                    # (n, L, 1), n > batch_size
    plan = ed.plan_from_args(parse((base + f" --edit_from {f} --pin 0-6,10 --edit_band_mm 2 --edit_steps 3").split()))
    e1 = plan.batch(1, 2)
    assert np.array_equal(e1.designs, _designs(5, 14)[2:4]) and e1.pins == (0, 1, 2, 3, 4, 5, 6, 10) and e1.steps == 3 and e1.mode == 'point'
    assert e1.band == pytest.approx(2.0 / 30.0)
    with pytest.raises(ValueError):
        plan.batch(2, 2)                                                      # rows [4, 6) of 5
    for bad in ("--edit_steps 0", "--edit_steps 6", "--pin 14", "--batch_size=6", "--ctrlpts_dim=42"):
        with pytest.raises(ValueError):
            ed.plan_from_args(parse((base + f" --edit_from {f} " + bad).split()))
    np.save(f, np.full((2, 14), 1.5, dtype=np.float32))
    with pytest.raises(ValueError):
        ed.plan_from_args(parse((base + f" --edit_from {f}").split()))


# ------------------------------------------------------------------------------------------------ 2. band conversion
def test_band_conversion():
    assert ed.band_from_mm(1.0, 'point') == pytest.approx(1.0 / 30.0, rel=1e-12)
    assert ed.band_from_mm(1.0, 'point_3d') == pytest.approx(1.0 / 50.0, rel=1e-12)
    assert ed.Edit.from_physical(_designs(), band_mm=3.0, mode='point').band == pytest.approx(0.1, rel=1e-12)
    assert ed.Edit.from_physical(_designs(2, 42), band_mm=2.0, mode='point_3d').band == pytest.approx(0.04, rel=1e-12)
    assert ed.Edit.from_physical(_designs(), mode='point').band is None
    with pytest.raises(ValueError):
        ed.band_from_mm(1.0, 'mesh')


# ------------------------------------------------------------------------------------------------ 3. validation
def test_edit_validation():
    d = _designs()
    assert ed.Edit(d).shape == (3, 14) and ed.Edit(d[..., None]).shape == (3, 14) and ed.Edit(torch.from_numpy(d)).shape == (3, 14)
    assert ed.Edit(np.array([[1.0, -1.0]], dtype=np.float32)).shape == (1, 2)           # the range's ends are inside
    for bad in (d * 2.0, np.where(np.arange(14) == 3, np.float32(1.0000001), d), np.where(np.arange(14) == 5, np.nan, d),
                np.where(np.arange(14) == 5, np.inf, d), d[0], d[None, ..., None], d[..., None].repeat(2, -1), np.zeros((0, 14), np.float32)):
        with pytest.raises(ValueError):
            ed.Edit(bad)
    for pins in ((14,), (-1,), (0, 99)):
        with pytest.raises(ValueError):
            ed.Edit(d, pins=pins)
    for band in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ed.Edit(d, band=band)
    with pytest.raises(ValueError):
        ed.Edit(d, mode='mesh')
    s = _sched(15, 5)
    assert ed.Edit(d).n_steps(s) == 5 and ed.Edit(d, steps=1).n_steps(s) == 1 and ed.Edit(d, steps=5).n_steps(s) == 5
    with pytest.raises(ValueError):
        ed.Edit(d, steps=0)
    with pytest.raises(ValueError):
        ed.Edit(d, steps=-2)
    with pytest.raises(ValueError):
        ed.Edit(d, steps=6).n_steps(s)
    with pytest.raises(ValueError):
        ed.Edit(d, steps=6).start(s, torch.zeros(3, 14, 1))


# ------------------------------------------------------------------------------------------------ 4. bounds
def test_bounds():
    d = _designs(4, 14, seed=3)
    d[0, 0], d[0, 1], d[1, 2], d[1, 3] = 1.0, -1.0, 0.99, -0.97
    lo, hi = ed.Edit(d).bounds()
    assert lo.dtype == np.float32 and hi.dtype == np.float32 and lo.shape == (4, 14)
    assert np.all(lo == -1.0) and np.all(hi == 1.0)
    pins = (0, 1, 2, 9, 13)
    free = [i for i in range(14) if i not in pins]
    for band in (None, 0.05, 1.0 / 30.0, 0.0, 3.0):
        e = ed.Edit(d, pins=pins, band=band)
        lo, hi = e.bounds()
        assert lo.dtype == np.float32 and hi.dtype == np.float32
        assert np.all(lo <= d) and np.all(d <= hi) and np.all(lo >= -1.0) and np.all(hi <= 1.0)
        assert np.array_equal(lo[:, pins], d[:, pins]) and np.array_equal(hi[:, pins], d[:, pins])          # pins override the band
        if band is None:
            assert np.all(lo[:, free] == -1.0) and np.all(hi[:, free] == 1.0)
        else:
            u = np.float32(band)
            assert np.array_equal(lo[:, free], np.maximum(np.float32(-1.0), d[:, free] - u))
            assert np.array_equal(hi[:, free], np.minimum(np.float32(1.0), d[:, free] + u))
    lo, hi = ed.Edit(d, band=0.05).bounds()
    assert hi[0, 0] == 1.0 and lo[0, 1] == -1.0 and hi[1, 2] == 1.0 and lo[1, 3] == -1.0                    # clipped to the sampler's range
    assert lo[0, 0] == np.float32(1.0) - np.float32(0.05) and hi[0, 1] == np.float32(-1.0) + np.float32(0.05)
    lo2, _ = e.bounds()
    lo2[:] = 7.0
    assert np.all(e.bounds()[0] <= 1.0) and np.all(e.designs == d)                                          # bounds() hands out copies


def test_moved_mm():
    d = _designs(2, 14)
    e = ed.Edit(d, mode='point')
    out = d.copy()
    out[1, 4] += 0.1
    mx, rms = e.moved_mm(out[None, ..., None])
    assert mx.shape == (1, 2) and mx[0, 0] == 0.0 and mx[0, 1] == pytest.approx(3.0, rel=1e-5)              # 0.1 unit = 3 mm in 2-D
    assert rms[0, 1] == pytest.approx(3.0 / np.sqrt(14.0), rel=1e-5)
    assert ed.Edit(d, mode='point_3d').moved_mm(out)[0][1] == pytest.approx(5.0, rel=1e-5)


# ------------------------------------------------------------------------------------------------ 5. start
class _RecordingScheduler:
    """The two things Edit.start touches, add_noise recorded instead of run on a GPU."""

    def __init__(self, timesteps):
        self.timesteps, self.calls = torch.tensor(timesteps, dtype=torch.int64), []

    def add_noise(self, x0, noise, ts):
        self.calls.append((x0.clone(), noise.clone(), ts.clone()))
        return x0 * 2.0 + noise


def test_start():
    d = _designs(3, 14)
    noise = torch.from_numpy(np.random.RandomState(1).randn(3, 14, 1).astype(np.float32))
    real = _sched(15, 5)
    assert [int(t) for t in real.timesteps] == [12, 9, 6, 3, 0]
    for K in (None, 1, 2, 5):
        s = _RecordingScheduler([12, 9, 6, 3, 0])
        x, ts = ed.Edit(d, steps=K).start(s, noise)
        k = 5 if K is None else K
        assert [int(t) for t in ts] == [12, 9, 6, 3, 0][5 - k:]
        (x0, nz, t), = s.calls
        assert x0.shape == noise.shape and torch.equal(x0, torch.from_numpy(d)[..., None]) and torch.equal(nz, noise)
        assert t.shape == (3,) and bool((t == [12, 9, 6, 3, 0][5 - k]).all())
        assert torch.equal(x, torch.from_numpy(d)[..., None] * 2.0 + noise)
    with pytest.raises(ValueError):
        ed.Edit(d).start(_RecordingScheduler([12, 9, 6, 3, 0]), noise[:2])


# ------------------------------------------------------------------------------------------------ 6. the restatement
def _step_inputs(seed, shape=(3, 3, 14)):
    rs = np.random.RandomState(seed)
    x = (rs.randn(*shape) * 5.0).astype(np.float32)
    x.reshape(-1)[::7] = np.where(np.arange(x.size)[::7] % 2 == 0, 15.0, -15.0).astype(np.float32)           # |x| up to 15: the clamp is active
    return x, rs.randn(*shape).astype(np.float32)


def test_restatement_equals_the_oracle_step():
    o, s = orc.DDIM(15), _sched(15, 5)
    o.set_timesteps(5)
    free = (np.float32(-1.0).reshape(1), np.float32(1.0).reshape(1))
    clamped = 0
    for si, t in enumerate(s.timesteps):
        x, eps = _step_inputs(10 + si)
        ref = o.step(torch.from_numpy(eps), int(t), torch.from_numpy(x)).numpy()
        got = edit_oracle.bounded_step(x, eps, None, 0, s.coefficients(int(t)), 0.0, *free)
        assert got.dtype == np.float32 and got.shape == x.shape
        assert float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) <= 1e-6, int(t)
        sa, sb = s.coefficients(int(t))[:2]
        clamped += int((np.abs((x - sb * eps) / sa) > 1.0).sum())
        # a guided step: the oracle's step on eps - sqrt(1 - abar_t) * mean(grad) * scale (generator/diffusion.py:575, :640-645)
        g = np.random.RandomState(40 + si).randn(3, *x.shape).astype(np.float32)
        e2 = torch.from_numpy(eps) - torch.tensor(sb) * torch.from_numpy(g).mean(0) * 0.8
        ref = o.step(e2, int(t), torch.from_numpy(x)).numpy()
        got = edit_oracle.bounded_step(x, eps, g, 3, s.coefficients(int(t)), 0.8, *free)
        assert float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) <= 2e-6, int(t)         # (+ the mean's own rounding)
    assert clamped > 100


def test_restatement_pins_and_bounds():
    s = _sched(15, 5)
    d = _designs(3, 14, seed=5)
    e = ed.Edit(d, pins=(0, 1, 2, 3, 4, 5, 6, 10), band=0.05)
    lo, hi = e.bounds()
    x, eps = _step_inputs(21)
    last = s.coefficients(0)
    assert last[2] == 1.0 and last[3] == 0.0                                    # abar_prev = 1 after the last step
    out = edit_oracle.bounded_step(x, eps, None, 0, last, 0.0, lo, hi)          # period B * L under 3 chains
    assert np.array_equal(out[:, :, list(e.pins)], np.broadcast_to(d[:, list(e.pins)], (3, 3, 8)))           # the pins, exactly
    assert np.all(out >= lo[None]) and np.all(out <= hi[None])
    # an earlier step: the pinned entries are the consistent DDIM state sqrt(abar_prev) d + sqrt(1 - abar_prev) eps
    c = s.coefficients(6)
    out = edit_oracle.bounded_step(x, eps, None, 0, c, 0.0, lo, hi)
    want = np.float32(c[2]) * np.broadcast_to(d, x.shape) + np.float32(c[3]) * eps
    assert np.array_equal(out[:, :, list(e.pins)], want[:, :, list(e.pins)])


# ------------------------------------------------------------------------------------------------ 7. symbols
def test_symbols_declared():
    for name, n_args in (("dgdm_ddim_guided_step_bounded", 15), ("dgdm_guided_chains_run_bounded", 19)):
        assert name in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == n_args
