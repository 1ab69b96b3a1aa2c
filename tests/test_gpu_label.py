"""Condition rows from the dynamics model (engine.Guidance.label / label_settled: csrc/label.hip behind the runners of
csrc/guidance_api.hip; dgdm_amd/label.py; --mode=label, --cond_target).

Yardstick: the calls the labelling pass is built on, called the way a user had to before it existed - Guidance.score / Guidance.rollout
once per padded batch with the same start slices - and their results fed through tests/label_oracle.py (numpy).  Tally rows must equal
that bit for bit (integer counts and one IEEE division per value); settled columns 0-3 within 2^-23 * max(1, |oracle|): the float64 work
differs from numpy's by a few ulp of double over at most M*G + 3 operations, far below half a float32 ulp, so after the single rounding
the two differ by at most one float32 ulp; left_range is a count over G and is bit for bit.

Shapes: the smallest with a padded last 32-row tile (81 / 63 cells), a partial last batch and more than one object; models, objects and
thresholds are those of tests/test_gpu_score.py."""
import ctypes as C
import functools
import json
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import engine, sampler, synth
from dgdm_amd import label as lb
from dgdm_amd._lib import DgdmError, dptr, lib, stream_ptr
from tests import label_oracle as lo
from tests import util

pytestmark = pytest.mark.gpu

T = 15
NV = 100
SUB = 50
K = 3
# kind: (B, G, P, M, N): N = two batches and one finger (2-D), two batches and one finger (3-D)
CASES = {2: (3, 9, 3, 2, 7), 3: (2, 7, 3, 2, 5)}
THR = {2: [0.4, 0.7, 1.0], 3: [1.2, 0.3, 1.4]}                      # tests/test_gpu_score.py
STD = {2: [0.0565, 0.0026, 0.0047], 3: [0.0312, 0.0016, 0.0026]}    # the datasets' (rad, m, m)
LAYOUTS = ["mean", "per_object"]
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(kind, mode="f32"):
    """The handle, the fingers (N, L) on the device and the start draws of the case."""
    B, G, P, M, N = CASES[kind]
    L = 14 if kind == 2 else 42
    sd = util.dyn2d_sd(22, NV) if kind == 2 else util.dyn3d_sd(33)
    objs = torch.stack([synth.synth_object_2d(i, NV) if kind == 2 else synth.synth_object_3d(50 + i) for i in range(M)])
    dyn = engine.Dynamics(kind, sd, L, 2 * NV if kind == 2 else 0)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), M, T, NV if kind == 2 else 512, SUB if kind == 3 else 0, max_objects=M, contraction_dtype=mode)
    gd.set_objects(objs.cuda())
    x = synth.synth_noise(80, N, L).reshape(N, L).clamp(-1, 1).cuda()
    nb = -(-N // B)
    st_t = st_s = None
    if kind == 3:
        st_t = sampler.TorchRng(seed=1234).fps_starts(512, SUB, gd.rows, n_calls=nb * M).reshape(nb, M, -1)
        st_s = sampler.TorchRng(seed=4321).fps_starts(512, SUB, gd.sweep_rows, n_calls=nb * K * M).reshape(nb, K, M, -1)
    return gd, x, nb, st_t, st_s


def padded(x, k, B):
    """Batch k of the fingers, padded to B with copies of the last finger of the set."""
    idx = [min(i, x.shape[0] - 1) for i in range(k * B, (k + 1) * B)]
    return x[idx]


@functools.lru_cache(maxsize=None)
def yardstick(kind):
    """Per batch: what Guidance.score and Guidance.rollout return for the padded batch on every object, on the host."""
    B, G, P, M, N = CASES[kind]
    gd, x, nb, st_t, st_s = case(kind)
    out = []
    for k in range(nb):
        xb = padded(x, k, B)[None].expand(M, B, x.shape[1]).contiguous()
        counts, sums = gd.score(xb, list(range(M)), THR[kind], timestep=0, starts=None if st_t is None else st_t[k].reshape(-1))
        final, _, left = gd.rollout(xb, list(range(M)), STD[kind], K, starts=None if st_s is None else st_s[k].reshape(-1))
        out.append((counts.cpu().numpy(), sums.cpu().numpy(), final.cpu().numpy(), left.cpu().numpy()))
    return out


def oracle_rows(kind, layout, what):
    """(N, cols) or (N, M, cols) from the yardstick through the numpy oracle, the padding rows dropped."""
    B, G, P, M, N = CASES[kind]
    rows = []
    for counts, sums, final, left in yardstick(kind):
        rows.append(lo.tally_rows(counts, sums, G * P * P, layout) if what == "tally" else lo.settled_rows(final, left, B, layout))
    return np.concatenate(rows)[:N]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", [2, 3])
def test_tally_rows_bit_for_bit(dev, kind, layout):
    B, G, P, M, N = CASES[kind]
    gd, x, nb, st_t, st_s = case(kind)
    want = oracle_rows(kind, layout, "tally")
    # the inputs discriminate (asserted on the yardstick's tally, not on the code under test): at least 4 of the 6 fraction columns take
    # 3 or more distinct values over the fingers
    mean = oracle_rows(kind, "mean", "tally")
    distinct = [len(np.unique(mean[:, j])) for j in range(6)]
    print(f"[label] {kind}-D: distinct values per fraction column over {N} fingers: {distinct}")
    assert sum(d >= 3 for d in distinct) >= 4, distinct
    got = gd.label(x, list(range(M)), THR[kind], timestep=0, starts=st_t, layout=layout).cpu().numpy()
    assert got.shape == (N, 10 if layout == "mean" else M * 10)
    assert np.array_equal(bits(got), bits(want.reshape(N, -1)))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", [2, 3])
def test_settled_rows(dev, kind, layout):
    B, G, P, M, N = CASES[kind]
    gd, x, nb, st_t, st_s = case(kind)
    want = oracle_rows(kind, layout, "settled").reshape(-1, 5)
    got = gd.label_settled(x, list(range(M)), STD[kind], K, starts=st_s, layout=layout).cpu().numpy()
    assert got.shape == (N, 5 if layout == "mean" else M * 5)
    got = got.reshape(-1, 5)
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got[:, :4].astype(np.float64) - want[:, :4].astype(np.float64))
    bound = 2.0 ** -23 * np.maximum(1.0, np.abs(want[:, :4].astype(np.float64)))
    print(f"[label] {kind}-D {layout}: settled max |got - oracle| / bound = {float((err / bound).max()):.3f}, rho in "
          f"[{float(want[:, 0].min()):.4f}, {float(want[:, 0].max()):.4f}], left_range max {float(want[:, 4].max()):.3f}")
    assert np.array_equal(bits(got[:, 4]), bits(want[:, 4]))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("kind", [2, 3])
def test_placement_and_chunking(dev, kind):
    """Rows written into a wider sentinel-filled matrix at a column offset, per_object with both blocks interleaved 15 apart: floats
    outside the blocks keep the sentinel; one call over all batches equals one call per batch, bit for bit."""
    B, G, P, M, N = CASES[kind]
    gd, x, nb, st_t, st_s = case(kind)
    objs = list(range(M))
    off, tail = 3, 2
    for layout in LAYOUTS:
        nblk = 1 if layout == "mean" else M
        plain_t = gd.label(x, objs, THR[kind], starts=st_t, layout=layout).cpu().numpy().reshape(N, nblk, 10)
        plain_s = gd.label_settled(x, objs, STD[kind], K, starts=st_s, layout=layout).cpu().numpy().reshape(N, nblk, 5)
        wide = torch.full((N, off + 15 * nblk + tail), SENTINEL, dtype=torch.float32, device=dev)
        gd.label(x, objs, THR[kind], starts=st_t, layout=layout, out=wide, column_offset=off, object_stride=15)
        gd.label_settled(x, objs, STD[kind], K, starts=st_s, layout=layout, out=wide, column_offset=off + 10, object_stride=15)
        w = wide.cpu().numpy()
        assert (w[:, :off] == SENTINEL).all() and (w[:, off + 15 * nblk:] == SENTINEL).all()
        body = w[:, off:off + 15 * nblk].reshape(N, nblk, 15)
        assert np.array_equal(bits(body[:, :, :10]), bits(plain_t)) and np.array_equal(bits(body[:, :, 10:]), bits(plain_s))
        # tally alone into the same geometry: the settled slots between the blocks are not written
        wide.fill_(SENTINEL)
        gd.label(x, objs, THR[kind], starts=st_t, layout=layout, out=wide, column_offset=off, object_stride=15)
        body = wide.cpu().numpy()[:, off:off + 15 * nblk].reshape(N, nblk, 15)
        assert (body[:, :, 10:] == SENTINEL).all() and np.array_equal(bits(body[:, :, :10]), bits(plain_t))
        # batch by batch
        for k in range(nb):
            f0, f1 = k * B, min(N, (k + 1) * B)
            one_t = gd.label(x[f0:f1], objs, THR[kind], starts=None if st_t is None else st_t[k:k + 1], layout=layout).cpu().numpy()
            one_s = gd.label_settled(x[f0:f1], objs, STD[kind], K, starts=None if st_s is None else st_s[k:k + 1], layout=layout).cpu().numpy()
            assert np.array_equal(bits(one_t), bits(plain_t[f0:f1].reshape(f1 - f0, -1))), (layout, k)
            assert np.array_equal(bits(one_s), bits(plain_s[f0:f1].reshape(f1 - f0, -1))), (layout, k)


@pytest.mark.parametrize("kind", [2, 3])
def test_label_fingers_layout_and_chunks(dev, kind):
    """label.label_fingers: [tally | settled] per block, and the same rows whatever chunk_batches is (3-D draws batch after batch)."""
    B, G, P, M, N = CASES[kind]
    gd, x, nb, st_t, st_s = case(kind)
    objs = list(range(M))
    whole = lb.label_fingers(gd, x[:, :, None], objs, THR[kind], std=STD[kind], rollout=K, layout="per_object", seed=9)
    assert whole.shape == (N, M * 15) and whole.is_cuda
    for chunk in (1, 2):
        again = lb.label_fingers(gd, x, objs, THR[kind], std=STD[kind], rollout=K, layout="per_object", seed=9, chunk_batches=chunk)
        assert torch.equal(again, whole), chunk
    if kind == 2:           # no draws: the blocks are the plain calls'
        t = gd.label(x, objs, THR[kind], layout="per_object").reshape(N, M, 10)
        s = gd.label_settled(x, objs, STD[kind], K, layout="per_object").reshape(N, M, 5)
        assert torch.equal(whole.reshape(N, M, 15), torch.cat([t, s], dim=2))
    tally_only = lb.label_fingers(gd, x, objs, THR[kind], layout="mean", seed=9)
    assert tally_only.shape == (N, 10)
    with pytest.raises(ValueError, match="256"):
        lb.label_fingers(gd, x, objs * 13, THR[kind], layout="per_object")


@pytest.mark.parametrize("kind", [2, 3])
def test_grad_is_untouched_by_label(dev, kind):
    B, G, P, M, N = CASES[kind]
    gd, x, nb, st_t, st_s = case(kind)
    xb = padded(x, 0, B)[None].expand(M, B, x.shape[1]).contiguous()
    objectives = [engine.make_objective(o, c) for c, o in zip(range(M), ('rotate', 'counterclockwise_left'))]
    gs = None if st_t is None else st_t[0].reshape(-1)
    before = gd.grad(xb, 3, objectives, None, gs).cpu()
    state = torch.get_rng_state()
    gd.label(x, list(range(M)), THR[kind], starts=st_t)
    gd.label_settled(x, list(range(M)), STD[kind], K, starts=st_s)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(gd.grad(xb, 3, objectives, None, gs).cpu(), before)


def test_refusals(dev):
    B, G, P, M, N = CASES[2]
    gd, x, nb, _, _ = case(2)
    objs = [0, 1]
    with pytest.raises(DgdmError, match=r"error -1: .*n_objects 3 outside 1\.\.2"):
        gd.label(x, [0, 1, 0], THR[2])
    with pytest.raises(DgdmError, match=r"error -1: .*n_objects 0"):
        gd.label_settled(x, [], STD[2], K)
    with pytest.raises(DgdmError, match=r"error -1: .*object 2 of 2"):
        gd.label(x, [0, 2], THR[2])
    with pytest.raises(DgdmError, match=r"error -1: .*0 interactions"):
        gd.label_settled(x, objs, STD[2], 0)
    with pytest.raises(ValueError, match="layout"):
        gd.label(x, objs, THR[2], layout="median")
    bf = case(2, "bf16")[0]
    with pytest.raises(DgdmError, match=r"error -1: .*bf16"):
        bf.label(x, objs, THR[2])
    with pytest.raises(DgdmError, match=r"error -1: .*bf16"):
        bf.label_settled(x, objs, STD[2], K)
    mf = case(2, "f32_mfma")[0]
    assert mf.label(x, objs, THR[2]).shape == (N, 10)               # the tally takes the float32 MFMA trunk, as score does
    with pytest.raises(DgdmError, match=r"error -1: .*MFMA"):
        mf.label_settled(x, objs, STD[2], K)
    # the C ABI itself: an unknown layout, strides smaller than the columns, no fingers, a null pointer, 3-D without draws - the rows
    # matrix keeps its fill, nothing was launched into it
    rows = torch.full((N, 64), SENTINEL, dtype=torch.float32, device=dev)
    oc = (C.c_int32 * 2)(0, 1)
    thr = (C.c_float * 3)(*THR[2])
    sc = (C.c_double * 3)(0.01, 0.01, 0.01)

    def tally(n=N, layout=0, stride=64, ostride=15, fingers=x, g=gd, starts=None):
        return lib().dgdm_guidance_label(g._h, dptr(fingers), n, oc, 2, 0, thr, starts, layout, dptr(rows), stride, ostride, stream_ptr())

    def settled(layout=0, stride=64, ostride=15, k=K):
        return lib().dgdm_guidance_label_settled(gd._h, dptr(x), N, oc, 2, sc, k, None, layout, dptr(rows), stride, ostride, stream_ptr())
    assert tally() == 0
    rows.fill_(SENTINEL)
    assert tally(layout=2) == -1 and tally(layout=-1) == -1 and settled(layout=7) == -1
    assert tally(stride=9) == -1 and settled(stride=4) == -1
    assert tally(layout=1, ostride=9) == -1 and settled(layout=1, ostride=4) == -1
    assert tally(layout=1, stride=24, ostride=15) == -1 and tally(layout=1, stride=25, ostride=15) == 0     # (M - 1) * 15 + 10 = 25
    rows.fill_(SENTINEL)
    assert tally(n=0) == -1 and tally(fingers=None) == -1 and settled(k=-2) == -1
    g3, x3, _, _, _ = case(3)
    assert tally(g=g3, fingers=x3, n=x3.shape[0], starts=None) == -1
    assert b"start" in lib().dgdm_last_error()
    torch.cuda.synchronize()
    assert bool((rows == SENTINEL).all())


def test_label_cli_end_to_end_2d(dev, tmp_path):
    """--mode=label writes the three files; --mode=train takes the rows; --mode=test --cond_stats --cond_target samples under the target
    and reports what the unguided samples achieve, labelled by the stored recipe."""
    from dgdm_amd.dynamics.parser import parse
    from dgdm_amd.generator import train as gtrain
    from dgdm_amd.generator.dataloader import GripperDataset
    shape = "--object_max_num_vertices=100 --ctrlpts_dim=14 --num_fingers=8 --batch_size=4 --num_train_timesteps=15 --num_inference_steps=2 --num_workers=0"
    grid = "--classifier_guidance --grid_size=3 --num_pos=3"
    out = tmp_path / "rows.npy"
    stats, raw = gtrain.train(parse(shlex.split(f"--mode=label {shape} {grid} --label_out={out}")))
    rows = gtrain.load_global_cond(str(out), 8)
    raw_file = np.load(tmp_path / "rows_raw.npy")
    js = json.load(open(tmp_path / "rows.json"))
    assert rows.shape == (8, 10) and rows.dtype == np.float32 and raw_file.shape == (8, 10) and np.array_equal(raw_file, raw)
    assert js["predicted"] is True and js["columns"] == lb.TALLY_COLUMNS and js["G"] == 3 and js["P"] == 3 and len(js["object_ids"]) == 8
    assert np.array_equal(rows, stats.apply(raw_file))
    # the raw rows are label_fingers on the dataset's fingers
    args = parse(shlex.split(f"--mode=label {shape} {grid}"))
    classifier, objects, object_ids = gtrain._classifier(args, 14, dev)
    fingers = torch.from_numpy(np.stack(list(GripperDataset(gtrain.finger_control_points(8, False), 0.12, -0.12, 0.015, -0.045)._items)))
    thr, std = gtrain._threshold_std(False)
    gd = engine.Guidance(classifier.handle(), 4, 3, 3, (-1.0, 1.0), 8, 15, 100, 0, max_objects=8)
    gd.set_objects(objects.to(dev))
    direct = lb.label_fingers(gd, fingers, list(range(8)), thr, layout="mean", timestep=0)
    assert np.array_equal(bits(direct.cpu().numpy()), bits(raw_file))
    # one training epoch on (fingers, rows)
    model, _ = gtrain.train(parse(shlex.split(f"--mode=train {shape} --global_cond={out} --num_epochs=1 --val_step=100 --lr_warmup_steps=0")))
    assert len(model.train_log) == 1 and np.isfinite(model.train_log[0]["train/loss"]) and model.noise_pred_net.global_cond_dim == 10
    # sampling under a target
    save = tmp_path / "smp"
    torch.manual_seed(7)
    _, results = gtrain.train(parse(shlex.split(f"--mode=test {shape} {grid} --cond_stats={tmp_path / 'rows.json'} "
                                                f"--cond_target=frac_clockwise=0.9,shift_up=0.7 --cfg_weight=2 --save_dir={save}")))
    rep = results[0]["cond_target"]
    assert set(rep) >= {"columns", "requested", "achieved_mean", "achieved_std", "baseline_mean"}
    assert rep["columns"] == lb.TALLY_COLUMNS and rep["requested"] == {"frac_clockwise": 0.9, "frac_up": 0.7}
    assert np.array_equal(rep["baseline_mean"], np.asarray(js["mean"]))
    achieved = lb.label_fingers(gd, results[0]["unguided"], list(range(8)), thr, layout="mean", timestep=0).cpu().numpy().astype(np.float64)
    assert np.array_equal(rep["achieved_mean"], achieved.mean(axis=0)) and np.array_equal(rep["achieved_std"], achieved.std(axis=0))
    tab = json.load(open(save / "tables" / "val__cond_target__unguided_sample.json"))
    assert len(tab["data"]) == 10 and all(row[-1] == {"predicted": True} for row in tab["data"])
    assert tab["data"][0][:2] == ["frac_clockwise", 0.9] and tab["data"][1][1] is None
    assert "cond_target" not in results[1]                          # reported with the first batch's samples, as the tables are
    # without a dynamics model the step says so and goes on
    _, results = gtrain.train(parse(shlex.split(f"--mode=test {shape} --cond_stats={tmp_path / 'rows.json'} --cond_target=frac_up=0.7")))
    assert results[0]["cond_target"]["achieved_mean"] is None and results[0]["cond_target"]["requested"] == {"frac_up": 0.7}
    # another object count than the recipe's
    js["object_ids"] = js["object_ids"][:7]
    json.dump(js, open(tmp_path / "seven.json", "w"))
    with pytest.raises(ValueError, match="7 objects"):
        gtrain.train(parse(shlex.split(f"--mode=test {shape} {grid} --cond_stats={tmp_path / 'seven.json'} --cond_target=frac_up=0.7")))
