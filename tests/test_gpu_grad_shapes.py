"""The guidance gradient (dgdm_dyn{2,3}d_guidance_grad) and its forward half (dgdm_guidance_score with logits) against the oracle in float64
over the sizes dgdm_dynamics_create / dgdm_guidance_create accept (include/dgdm_hip.h, "accepted domain"), not only L = 14 / 42 at nv = 100.

2-D cases (tests/grad_shapes_cases.py CASES_2D; (b): also in bf16)
| name         | B | G  | P | L   | nv  | chains | objects | T    | t   | ori_range     | reaches                                                                  |
|--------------|---|----|---|-----|-----|--------|---------|------|-----|---------------|--------------------------------------------------------------------------|
| one_row      | 1 | 1  | 1 | 1   | 1   | 1      | 1       | 15   | 0   | (-1, 1)       | one row everywhere; linspace with one step; K = 1 and K = 2 (b)          |
| c20_last_t   | 3 | 5  | 2 | 2   | 1   | 2      | 2       | 15   | 14  | (-0.5, 0.25)  | C = 20 < 32; last timestep                                               |
| one_tile     | 1 | 32 | 1 | 14  | 100 | 1      | 1       | 15   | 6   | (-1, 1)       | exactly one full tile, ntiles = 1 (b)                                    |
| tile_plus_1  | 2 | 33 | 1 | 17  | 33  | 3      | 3       | 15   | 6   | (-1, 1)       | second tile holds one valid row; object_ch 66 = 64 + 2; ntiles 12        |
| L65_7fingers | 7 | 3  | 3 | 65  | 5   | 1      | 1       | 15   | 6   | (0, 0)        | L = 64 + 1; 7 fingers (no multiple of 4 or 8); equal orientations; ntiles 7 (b) |
| L256         | 2 | 11 | 3 | 256 | 7   | 2      | 2       | 15   | 6   | (-1, 1)       | largest L (t < L takes all 256 threads)                                  |
| K256_T1000   | 5 | 7  | 3 | 100 | 128 | 3      | 9       | 1000 | 999 | (-1, 1)       | object_ch 256 (four exact K chunks); objects 0, 4, 8 of 9; T = 1000      |
| fold15       | 3 | 13 | 6 | 14  | 100 | 3      | 2       | 15   | 6   | (-1, 1)       | C = 468 -> 15 tiles per finger (> the fold's 12-wide unroll); 135 tiles (b) |
| chains256    | 1 | 3  | 1 | 14  | 10  | 256    | 9       | 15   | 6   | (-1, 1)       | max_chains = n_chains = 256, ntiles 256                                  |

3-D cases (CASES_3D; N = 512)
| name        | B | G  | P | L   | sub | chains | reaches                                                                                   |
|-------------|---|----|---|-----|-----|--------|-------------------------------------------------------------------------------------------|
| one_row     | 1 | 1  | 1 | 2   | 1   | 1      | one row, smallest L (b)                                                                   |
| sub7_tail4  | 3 | 5  | 2 | 6   | 7   | 2      | R = 60 in slices of 7 with a tail of 4; C = 20; last timestep                             |
| sub_gt_R    | 1 | 33 | 1 | 42  | 512 | 1      | sub > R; one valid row in the second tile (b)                                             |
| L256_split  | 2 | 9  | 2 | 256 | 64  | 2      | largest L; R = 72 = 64 + 8; one tabled and one gathered chain: the split launch at L != 42 |
| chains256   | 1 | 1  | 1 | 14  | 1   | 256    | max_chains = 256 on the 3-D row planner; four distinct chains, each 64 times              |

Reference: the project's oracle evaluated in float64 (a .double() state dict and double inputs).  The oracle's own float32 run on the same
inputs is the yardstick: 2-D computed here, 3-D (40 ms per row in float64) read from tests/golden/g16_grad_shapes.npz, which
tests/golden/make_golden_grad_shapes.py writes from the oracle alone and tests/test_oracle_golden.py pins.

ReLU ties.  The gradient of a ReLU network jumps where a pre-activation lies within float32 rounding of zero; a test that tolerated that
would tolerate one wrong finger.  Every chain's inputs are therefore fixed seeds at which the float64 oracle's smallest relative ReLU
margin over all rows and layers is at least 5e-7 (asserted; the float32 oracle flipped a unit against float64 only at margins of 8.8e-8
and below, and was otherwise within 4e-6 of float64 - 1.2e-5 at the single 3-D row).  No case is skipped, and nothing here allows for a tie.

Asserted, f32 (f16x3) and f32_mfma, every case:
  * per chain      rel_l2(HIP, f64) <= max(2e-5, 2 rel_l2(oracle32, f64))                            (the rule of tests/test_gpu_fullgrid.py)
  * per finger     |HIP - f64| / |f64| of the finger's own rows of the gradient <= max(2e-5, 2 x the same for oracle32), for every
                   finger whose gradient is more than 1e-3 of the chain's: one wrong finger among many cannot hide in the chain's norm
  * logits         all R rows of every chain: max |HIP - f64| <= max(2e-5 max |f64|, 2 max |oracle32 - f64|)
  * counts         sum over the 27 classes == G P^2 per (chain, finger)
bf16 ((b) cases): finite, rel_l2(HIP, oracle32) <= max(5e-2 (2-D) / 8e-2 (3-D), 1.5 rel_l2(oracle under contraction('bf16'), oracle32))
(the constants of tests/test_gpu_bf16.py; the second term, measured on the oracle, covers small grids where one flip weighs more).
Every form: chain c of a multi-chain launch has the bits of chain c launched alone; a second call returns the same bits; chains with equal
inputs have equal bits.  The measured worst ratios are printed per case and form (pytest -s)."""
import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine, synth
from tests import grad_shapes_cases as gc
from tests import util

pytestmark = pytest.mark.gpu
F32_FORMS = ("f32", "f32_mfma")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden3d():
    return util.load(gc.GOLDEN_3D)


class Launch:
    """One case on the device: the handle's inputs for all chains of the launch (chain c = distinct chain c % distinct)."""

    def __init__(self, case, ref, dev, contraction_dtype="f32"):
        self.case, self.dev = case, dev
        nc, B, L, D = case["nc"], case["B"], case["L"], case["distinct"]
        self.of = [c % D for c in range(nc)]
        self.dyn = engine.Dynamics(case["dim"], gc.state_dict(case), L, 2 * case["nv"] if case["dim"] == 2 else 0)
        self.objs = gc.objects(case).to(dev)
        self.gd = self.handle(nc, contraction_dtype)
        self.x = gc.x_all(case).reshape(D, B, L)[self.of].contiguous().to(dev)
        self.oidx = [case["chain_obj"][k] for k in self.of]
        goals = [case["chain_goal"][k] for k in self.of]
        self.objectives = [engine.make_objective(None, oi, row_field=True, lin=gc.FIELD_LIN, quad=gc.FIELD_QUAD) if g == 'field'
                           else engine.make_objective(g, oi) for g, oi in zip(goals, self.oidx)]
        self.field = self.rowcoef = None
        if 'field' in goals:
            self.field = torch.stack([gc.field(case, k) if g == 'field' else torch.zeros(case["R"], 3) for k, g in zip(self.of, goals)]).to(dev)
        if 'convergence' in goals:
            self.rowcoef = torch.stack([torch.from_numpy(self.gd.rowcoef(gc.centers(case, k))) if g == 'convergence' else torch.zeros(case["R"])
                                        for k, g in zip(self.of, goals)]).to(dev)
        self.starts = ref["starts"].numpy()[self.of].reshape(-1) if case["dim"] == 3 else None

    def handle(self, max_chains, contraction_dtype="f32"):
        c = self.case
        gd = engine.Guidance(self.dyn, c["B"], c["G"], c["P"], c["ori"], max_chains, c["T"], c["nv"] if c["dim"] == 2 else gc.N3D, c["sub"],
                             max_objects=len(c["objs"]), contraction_dtype=contraction_dtype)
        gd.set_objects(self.objs)
        assert gd.rows == c["R"]
        return gd

    def grad(self, chains=None, gd=None):
        """The gradient of all chains, or of the listed ones as a launch of their own -> (n, B, L) on the host."""
        gd = gd or self.gd
        ch = list(range(self.case["nc"])) if chains is None else list(chains)
        gd.set_row_field(self.field[ch].contiguous() if self.field is not None else None)
        rc = self.rowcoef[ch].contiguous() if self.rowcoef is not None else None
        st = None if self.starts is None else np.ascontiguousarray(self.starts.reshape(self.case["nc"], -1)[ch]).reshape(-1)
        return gd.grad(self.x[ch].contiguous(), self.case["t"], [self.objectives[i] for i in ch], rc, st).cpu()

    def score(self):
        counts, _, logits = self.gd.score(self.x, self.oidx, (0.1, 0.1, 0.1), self.case["t"], self.starts, want_logits=True)
        return counts.cpu(), logits.cpu()


def check_f32(case, ref, got, counts, logits, form):
    """The float32-grade assertions of the module docstring; returns the worst measured figures."""
    D, B = case["distinct"], case["B"]
    worst = dict(chain=0.0, chain32=0.0, finger=0.0, finger32=0.0, logit=0.0, logit32=0.0)
    for c in range(D):
        g64, g32, hip = ref["g64"][c], ref["g32"][c], got[c].double()
        assert float(g64.norm()) > 0
        e, e32 = util.rel_l2(hip, g64), util.rel_l2(g32, g64)
        worst["chain"], worst["chain32"] = max(worst["chain"], e), max(worst["chain32"], e32)
        assert e <= max(2e-5, 2.0 * e32), (case["name"], form, "chain", c, e, e32)
        for b in range(B):
            if float(g64[b].norm()) <= 1e-3 * float(g64.norm()):
                continue
            f, f32 = util.rel_l2(hip[b], g64[b]), util.rel_l2(g32[b], g64[b])
            worst["finger"], worst["finger32"] = max(worst["finger"], f), max(worst["finger32"], f32)
            assert f <= max(2e-5, 2.0 * f32), (case["name"], form, "chain", c, "finger", b, f, f32)
        l64, l32, lh = ref["l64"][c], ref["l32"][c], logits[c].double()
        scale = float(l64.abs().max())
        d, d32 = float((lh - l64).abs().max()), float((l32 - l64).abs().max())
        worst["logit"], worst["logit32"] = max(worst["logit"], d / scale), max(worst["logit32"], d32 / scale)
        assert d <= max(2e-5 * scale, 2.0 * d32), (case["name"], form, "logits of chain", c, d, d32, scale)
    assert bool((counts.reshape(case["nc"], B, 27).sum(-1) == case["C"]).all()), (case["name"], form)
    return worst


def check_bf16(case, ref, got):
    floor = 5e-2 if case["dim"] == 2 else 8e-2
    worst = dict(hip=0.0, oracle=0.0)
    assert bool(torch.isfinite(got).all())
    for c in range(case["distinct"]):
        e, e16 = util.rel_l2(got[c], ref["g32"][c]), util.rel_l2(ref["g16"][c], ref["g32"][c])
        worst["hip"], worst["oracle"] = max(worst["hip"], e), max(worst["oracle"], e16)
        assert e <= max(floor, 1.5 * e16), (case["name"], "bf16", "chain", c, e, e16)
    return worst


def check_bits(case, run, got, form):
    """A second call; chains with equal inputs; chain c alone (every chain of a small launch, the last one of a 256-chain launch)."""
    nc, D = case["nc"], case["distinct"]
    assert torch.equal(got, run.grad()), (case["name"], form, "second call")
    for c in range(D, nc):
        assert torch.equal(got[c], got[c % D]), (case["name"], form, "replica", c)
    if nc > 1:
        for c in (range(nc) if nc <= 8 else (nc - 1,)):
            assert torch.equal(got[c], run.grad([c])[0]), (case["name"], form, "chain alone", c)


def run_case(case, ref, dev):
    assert float(ref["margin"].min()) >= gc.MARGIN, (case["name"], ref["margin"])
    run = Launch(case, ref, dev)
    for form in F32_FORMS:
        run.gd.set_contraction_dtype(form)
        got = run.grad()
        counts, logits = run.score()
        w = check_f32(case, ref, got, counts, logits, form)
        check_bits(case, run, got, form)
        print(f"grad shapes {case['dim']}-D {case['name']:12s} {form:8s} margin {float(ref['margin'].min()):.1e} | chain: HIP vs f64 {w['chain']:.2e} (oracle32 "
              f"{w['chain32']:.2e}) | finger: {w['finger']:.2e} ({w['finger32']:.2e}) | logits / max: {w['logit']:.2e} ({w['logit32']:.2e})")
    if case["nc"] > 8:                       # the last chain of the full launch on a handle that holds one chain
        run.gd.set_contraction_dtype("f32")
        assert torch.equal(run.grad()[-1], run.grad([case["nc"] - 1], gd=run.handle(1))[0]), (case["name"], "max_chains = 1")
    if case["bf16"]:
        if case["dim"] == 3:                 # a handle in bf16 mode when its tables are built (tests/test_gpu_bf16.py)
            run = Launch(case, ref, dev, contraction_dtype="bf16")
        run.gd.set_contraction_dtype("bf16")
        got = run.grad()
        w = check_bf16(case, ref, got)
        check_bits(case, run, got, "bf16")
        print(f"grad shapes {case['dim']}-D {case['name']:12s} bf16     | HIP vs oracle32 {w['hip']:.2e} (oracle bf16 vs oracle32 {w['oracle']:.2e})")
    return run


@pytest.mark.parametrize("name", [c["name"] for c in gc.CASES_2D])
def test_grad_shapes_2d(dev, name):
    case = gc.by_name(gc.CASES_2D, name)
    run_case(case, gc.reference(case), dev)


@pytest.mark.parametrize("name", [c["name"] for c in gc.CASES_3D])
def test_grad_shapes_3d(dev, golden3d, name):
    case = gc.by_name(gc.CASES_3D, name)
    keys = ["g64", "g32", "l64", "l32", "margin", "starts"] + (["g16"] if case["bf16"] else [])
    ref = {k: torch.from_numpy(golden3d[f"{name}/{k}"]) for k in keys}
    assert np.array_equal(golden3d[f"{name}/x"], gc.x_all(case).numpy()), "the fixture was made for other inputs"
    for c in range(case["distinct"]):
        assert np.array_equal(ref["starts"][c].numpy(), gc.starts(case, c))
    run = run_case(case, ref, dev)
    if name == "L256_split":                 # object 1: no crowded centre, its chain takes the layer-1 table; object 2: all crowded, gathered
        crowded = [int(engine.debug_pointnet_indices(run.dyn, synth.synth_object_3d(i).to(dev))["crowded"].sum()) for i in case["objs"]]
        assert crowded[0] == 0 and crowded[1] > 0, crowded
        assert run.gd.debug_fps_path(0)[0]


def test_rejections(dev):
    """Outside the accepted domain: DGDM_EINVAL with a message, and no handle."""
    einval = r"error -1: \S"
    sd2, sd3 = synth.synth_state_dict(synth.dyn2d_spec(14, 20), 1), synth.synth_state_dict(synth.dyn3d_spec(14), 1)
    for L in (0, 257):
        with pytest.raises(_lib.DgdmError, match=einval):
            engine.Dynamics(2, sd2, L, 20)
        with pytest.raises(_lib.DgdmError, match=einval):
            engine.Dynamics(3, sd3, L)
    d2, d3 = engine.Dynamics(2, sd2, 14, 20), engine.Dynamics(3, sd3, 14)

    def make(dyn, batch=2, grid=3, pos=2, max_chains=2, nop=None, sub=None):
        three = dyn.kind == 3
        return engine.Guidance(dyn, batch, grid, pos, (-1.0, 1.0), max_chains, 15, (512 if three else 10) if nop is None else nop,
                               (4 if three else 0) if sub is None else sub, max_objects=2)

    bad = [dict(max_chains=0), dict(max_chains=257), dict(batch=0), dict(grid=0), dict(pos=0)]
    for dyn, more in ((d2, [dict(nop=9), dict(nop=11)]), (d3, [dict(sub=0), dict(nop=0), dict(nop=1025)])):
        for kw in bad + more:
            with pytest.raises(_lib.DgdmError, match=einval):
                make(dyn, **kw)
    gd = make(d2)
    gd.set_objects(torch.stack([synth.synth_object_2d(i, 10) for i in range(2)]).to(dev))
    x = synth.synth_noise(0, 2, 14).clamp(-1, 1).reshape(1, 2, 14).to(dev)
    assert bool(torch.isfinite(gd.grad(x, 6, [engine.make_objective('rotate', 1)])).all())
    with pytest.raises(_lib.DgdmError, match=einval):          # n_chains > max_chains
        gd.grad(x.expand(3, -1, -1).contiguous(), 6, [engine.make_objective('rotate', 0)] * 3)
    with pytest.raises(_lib.DgdmError, match=einval):          # object index >= n_objects
        gd.grad(x, 6, [engine.make_objective('rotate', 2)])
