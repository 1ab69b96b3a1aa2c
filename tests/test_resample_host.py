"""Resampling fingers by predicted objective, host side: Resample's validation, the entry point's flag rules, properties of the oracle's
systematic step (tests/resample_oracle.py), and the condition on the committed inputs of the GPU tests (tests/resample_cases.py): every
ancestor decision has a margin above 1e-9, so an ulp of the device's exp cannot move one.  No GPU."""
import shlex

import numpy as np
import pytest

from dgdm_amd.dynamics.parser import parse
from dgdm_amd.resample import Resample, from_flags, resample_from_args
from tests import resample_cases as cases
from tests import resample_oracle as orc


def test_resample_validation():
    r = Resample(2, 0.5)
    assert (r.every, r.beta, r.ess_frac) == (2, 0.5, 0.5)
    assert Resample(1, 0.0, 3.0).ess_frac == 3.0                      # above 1: whenever evaluated
    for bad in (dict(every=0, beta=1.0), dict(every=-1, beta=1.0), dict(every=1.5, beta=1.0), dict(every=1, beta=-0.1),
                dict(every=1, beta=float("nan")), dict(every=1, beta=float("inf")), dict(every=1, beta=1.0, ess_frac=0.0),
                dict(every=1, beta=1.0, ess_frac=-1.0), dict(every=1, beta=1.0, ess_frac=float("nan"))):
        with pytest.raises(ValueError):
            Resample(**bad)
    # after every `every`-th step, never after the last
    assert Resample(1, 1.0).evaluations(5) == [0, 1, 2, 3]
    assert Resample(2, 1.0).evaluations(5) == [1, 3]
    assert Resample(5, 1.0).evaluations(5) == [] and Resample(7, 1.0).evaluations(5) == []
    assert Resample(2, 1.0).evaluations(4) == [1]


def test_flag_rules():
    assert from_flags(None, None, None, False, 0.0) is None
    r = from_flags(2, 0.5, None, True, 0.3)
    assert isinstance(r, Resample) and (r.every, r.beta, r.ess_frac) == (2, 0.5, 0.5)
    assert from_flags(2, 0.5, 1.5, True, 0.3).ess_frac == 1.5
    for every, beta, ess, guided, eta in ((2, 0.5, None, False, 0.3), (2, 0.5, None, True, 0.0), (2, None, None, True, 0.3),
                                          (None, 0.5, None, True, 0.3), (None, None, 0.5, True, 0.3), (0, 0.5, None, True, 0.3)):
        with pytest.raises(ValueError):
            from_flags(every, beta, ess, guided, eta)
    base = "--mode=test --num_fingers=2 --batch_size=2"
    ok = parse(shlex.split(base + " --classifier_guidance --eta 0.5 --resample_every 2 --resample_beta 0.7 --resample_ess 0.9"))
    r = resample_from_args(ok)
    assert (r.every, r.beta, r.ess_frac) == (2, 0.7, 0.9)
    assert resample_from_args(parse(shlex.split(base + " --classifier_guidance --eta 0.5"))) is None
    for flags in ("--eta 0.5 --resample_every 2 --resample_beta 0.7",                          # no --classifier_guidance
                  "--classifier_guidance --resample_every 2 --resample_beta 0.7",              # eta == 0
                  "--classifier_guidance --eta 0.5 --resample_every 2",                        # no beta
                  "--classifier_guidance --eta 0.5 --resample_ess 0.4",                        # the optional flag alone
                  "--classifier_guidance --eta 0.5 --resample_every 2 --resample_beta 0.7 --edit_from designs.npy",
                  "--classifier_guidance --eta 0.5 --resample_every 2 --resample_beta 0.7 --global_cond rows.npy"):
        with pytest.raises(ValueError):
            resample_from_args(parse(shlex.split(base + " " + flags)))
    with pytest.raises(ValueError):
        resample_from_args(parse(shlex.split("--mode=train --classifier_guidance --eta 0.5 --resample_every 2 --resample_beta 0.7")))


def test_uniform_is_keyed():
    u = [orc.uniform(7, k, s) for k in cases.KEYS for s in (0, 3)]
    assert all(0.0 <= v < 1.0 for v in u) and len(set(u)) == len(u)
    assert orc.uniform(7, 5, 3) == orc.uniform(7, 5, 3) != orc.uniform(8, 5, 3)
    # not the words the step noise of the same (seed, key, step) starts from
    for k in cases.KEYS:
        first = orc.step_noise_first_words(7, k, 3)
        assert all(orc.uniform(7, k, 3) != float(int(w) >> 11) * 2.0 ** -53 for w in first)


def _weights(B, rs):
    w = np.exp(rs.randn(B) * 2.0)
    return w / w.sum()


@pytest.mark.parametrize("B", [2, 8, 64])
def test_systematic_counts(B):
    """Each finger's number of copies lies within 1 of B w_b for every u, and its mean over 4096 independent u within five standard errors
    of B w_b: given u the count is floor(B w_b) + a Bernoulli variable of probability frac(B w_b)."""
    rs = np.random.RandomState(B)
    x = np.zeros((1, B, 1), dtype=np.float32)
    for _ in range(1 if B == 64 else 3):
        w = _weights(B, rs)
        values, zero = np.log(w)[None], np.zeros((1, B))
        us = rs.uniform(size=4096)
        counts = np.zeros((len(us), B))
        for i, u in enumerate(us):
            r = orc.resample_step(x, values, 1, 1.0, 2.0, [u], zero, zero)
            assert r["did"][0] == 1 and np.all(np.diff(r["ancestors"][0]) >= 0)
            counts[i] = np.bincount(r["ancestors"][0], minlength=B)
        target = B * w
        assert np.all(np.abs(counts - target[None]) < 1.0 + 1e-9)
        frac = target - np.floor(target)
        se = np.sqrt(frac * (1.0 - frac) / len(us))
        assert np.all(np.abs(counts.mean(axis=0) - target) <= 5.0 * se + 1e-12), float(np.max(np.abs(counts.mean(axis=0) - target) / (se + 1e-300)))


def test_oracle_step_by_hand():
    """Two fingers, weights 3/4 and 1/4: u < 1/2 copies finger 0 twice, u >= 1/2 keeps both; logw / vprev follow the recipe."""
    x = np.arange(4, dtype=np.float32).reshape(1, 2, 2)
    values, zero = np.log(np.array([[3.0, 1.0]])), np.zeros((1, 2))
    r = orc.resample_step(x, values, 1, 1.0, 2.0, [0.25], zero, zero)
    assert r["ancestors"].tolist() == [[0, 0]] and np.array_equal(r["x"][0], x[0, [0, 0]])
    assert np.allclose(r["ess"], 1.0 / (0.75 ** 2 + 0.25 ** 2)) and np.array_equal(r["logw"], zero)
    assert np.array_equal(r["vprev"], np.log(np.array([[3.0, 3.0]])))
    assert np.allclose(r["margin"], [[0.625, 0.125]])
    r = orc.resample_step(x, values, 1, 1.0, 2.0, [0.75], zero, zero)
    assert r["ancestors"].tolist() == [[0, 1]]
    keep = orc.resample_step(x, values, 1, 1.0, 0.5, [0.25], zero, zero)           # ess 1.6 >= 1: nothing moves, the weights are kept
    assert keep["did"][0] == 0 and keep["ancestors"].tolist() == [[0, 1]] and np.allclose(keep["logw"], values) and np.array_equal(keep["x"], x)
    again = orc.resample_step(x, values, 1, 1.0, 0.5, [0.25], keep["logw"], keep["vprev"])      # the same potentials again add nothing
    assert np.allclose(again["logw"], values) and np.allclose(again["ess"], keep["ess"])
    none = orc.resample_step(x, np.array([[np.nan, np.inf]]), 1, 1.0, 2.0, [0.25], values, zero)
    assert none["did"][0] == 0 and none["ess"][0] == 0.0 and np.array_equal(none["logw"], zero) and none["ancestors"].tolist() == [[0, 1]]


def test_committed_inputs_have_margin():
    """The condition on the GPU tests' inputs: wherever a chain resamples, min_b |cum_b - p_j| > 1e-9 for every ancestor, and the
    effective sample size stands further than 1e-9 B from its threshold - three ulps of exp(.) are ~1e-15 of either."""
    n = resampled = 0
    for kind, B, L, n_grad in cases.all_cases():
        x, calls = cases.case(kind, B, L, n_grad)
        for c, r in zip(calls, cases.expected(x, calls, n_grad)):
            n += 1
            resampled += int(r["did"].sum())
            m = r["margin"][r["did"] == 1]
            assert m.size == 0 or float(m.min()) > cases.MARGIN, (kind, B, L, n_grad, float(m.min()))
            live = r["ess"] > 0
            assert np.all(np.abs(r["ess"][live] - c["ess_frac"] * B) > cases.MARGIN * B), (kind, B, L, n_grad)
    for B in cases.BS:
        for L in cases.LS:
            x, calls = cases.greedy_case(B, L)
            r = cases.expected(x, calls, 1)[0]
            assert float(r["margin"].min()) > cases.MARGIN and np.all(r["did"] == 1)
            assert np.array_equal(r["ancestors"], np.repeat(np.argmax(calls[0]["values"], axis=1)[:, None], B, axis=1))
    assert n == len(cases.KINDS) * 16 + 16 and resampled > 100
    # what the kinds are there for
    ex = lambda kind, B=8, n_grad=1: cases.expected(*cases.case(kind, B, 14, n_grad), n_grad)      # noqa: E731
    assert np.all(ex("equal")[0]["did"] == 0) and np.allclose(ex("equal")[0]["ess"], 8.0)
    assert np.all(ex("dominant")[0]["did"] == 1) and np.all(ex("dominant")[0]["ancestors"] == 3)
    assert np.all(ex("all_non_finite")[0]["ess"] == 0.0) and np.all(ex("all_non_finite")[0]["did"] == 0)
    assert ex("ess_below")[0]["did"][0] == 1 and ex("ess_above")[0]["did"][0] == 0
    assert np.all(ex("nan_and_inf")[0]["did"] == 1) and 0 not in ex("nan_and_inf")[0]["ancestors"][0] and 7 not in ex("nan_and_inf")[0]["ancestors"][2]
    two = ex("two_calls")
    assert np.all(two[0]["did"] == 0) and np.any(two[0]["logw"] != 0.0) and np.all(two[1]["did"] == 1)


def test_in_place_gather_order():
    """The kernel permutes vprev in place by ancestors that never descend: slots with a_j >= j ascending, then slots with a_j < j
    descending.  The same two sweeps in numpy equal the gather from a copy."""
    rs = np.random.RandomState(3)
    for _ in range(2000):
        B = int(rs.randint(1, 20))
        anc = np.sort(rs.randint(0, B, size=B))
        v = rs.randn(B)
        w = v.copy()
        for j in range(B):
            if anc[j] >= j:
                w[j] = w[anc[j]]
        for j in range(B - 1, -1, -1):
            if anc[j] < j:
                w[j] = w[anc[j]]
        assert np.array_equal(w, v[anc]), (anc, v)


def test_tables_carry_the_resample_columns(tmp_path):
    """guided_table / multi_object_table with `resample` (dgdm_amd.resample.summarise entries): RESAMPLE_COLUMNS behind the usual columns -
    the object's chain in its rows, all chains in the average row - and without it the tables of old."""
    import json
    from dgdm_amd.dynamics import predicted as pr
    from dgdm_amd.generator import artefacts
    from dgdm_amd.generator.diffusion import Diffusion
    from tests.test_predicted_sim import STD, THR, hand_logits
    n_obj, n_grip = 2, 2
    model = Diffusion.__new__(Diffusion)
    metrics = [pr.build_metric(hand_logits(20 + i, 360), THR, STD) for i in range(n_obj * n_grip)]
    none = [None] * (n_obj * n_grip)
    sim = (list(none), metrics, list(none), list(none), list(none), list(none), [[] for _ in none], list(none))
    per_obj = [tuple(s[i * n_grip:(i + 1) * n_grip] for s in sim) for i in range(n_obj)]
    per_grip = [tuple([s[g], s[n_grip + g]] for s in sim) for g in range(n_grip)]
    chains = [dict(evaluations=2, resamples=1, ess_min=1.25, distinct_min=1), dict(evaluations=2, resamples=2, ess_min=1.5, distinct_min=2)]
    tables = {}
    for tag, kw_obj, kw_grip in (("with", dict(resample=chains), dict(resample=chains[:1])), ("without", {}, {})):
        log = artefacts.TableLog(str(tmp_path / tag))
        artefacts.guided_table(model, log, per_obj, 'rotate', [-1.0, 1.0], **kw_obj)
        artefacts.multi_object_table(model, log, per_grip, n_obj, 'clockwise_left', [-1.0, 1.0], **kw_grip)
        tables[tag] = [json.load(open(tmp_path / tag / "tables" / (key.replace("/", "__") + ".json"))) for key in log.keys]
    for t, plain in zip(tables["with"], tables["without"]):
        n = len(plain["columns"])
        assert t["columns"] == plain["columns"] + artefacts.RESAMPLE_COLUMNS and t["key"] == plain["key"]
        assert [row[:n] for row in t["data"]] == plain["data"] and all(len(row) == n + 3 for row in t["data"])
    guided, multi = tables["with"]
    assert guided["data"][0][-3:] == [3, 1.25, 1]                                   # the average row: all chains
    by_obj = {row[0]: row[-3:] for row in guided["data"][1:]}
    assert by_obj == {0: [1, 1.25, 1], 1: [2, 1.5, 2]}
    assert all(row[-3:] == [1, 1.25, 1] for row in multi["data"])
