"""The committed inputs of the resampling step's GPU tests (tests/test_gpu_resample.py), generated from fixed seeds, and what the oracle
(tests/resample_oracle.py) makes of them.  tests/test_resample_host.py checks on the CPU that every ancestor decision and every
effective-sample-size decision of these inputs has a margin far above what an ulp of the device's exp could move."""
import numpy as np

from tests import resample_oracle as orc

SEED, KEYS = 7, [0, 5, 2 ** 40 + 1]
NC = len(KEYS)
BS, LS, NGRADS = (1, 2, 8, 64), (14, 42), (1, 2)
KINDS = ("equal", "dominant", "nan_and_inf", "all_non_finite", "ess_below", "ess_above", "two_calls")
MARGIN = 1e-9


def _x(rs, B, L):
    x = (rs.randn(NC, B, L) * 2.0).astype(np.float32)
    x[0, 0, 0], x[NC - 1, B - 1, L - 1] = np.float32(-0.0), np.float32(np.nan)        # the gather copies bits, whatever they mean
    return x


def _values(rs, n_grad, B, spread):
    return rs.randn(n_grad * NC, B) * spread


def case(kind: str, B: int, L: int, n_grad: int):
    """-> (x (NC, B, L) float32, calls): calls is a list of dict(values, beta, ess_frac, step); logw / vprev start at zero and carry
    from call to call, x is the input of every call."""
    rs = np.random.RandomState(1000 * KINDS.index(kind) + 100 * BS.index(B) + 10 * LS.index(L) + n_grad)
    x = _x(rs, B, L)
    one = lambda values, beta=0.25, ess_frac=0.5, step=0: [dict(values=values, beta=beta, ess_frac=ess_frac, step=step)]      # noqa: E731
    if kind == "equal":
        return x, one(np.full((n_grad * NC, B), 1.75))
    if kind == "dominant":
        v = _values(rs, n_grad, B, 1.0)
        v[:, (B - 1) // 2] += 40.0
        return x, one(v, step=3)
    if kind == "nan_and_inf":
        v = _values(rs, n_grad, B, 3.0)
        v[0, 0] = np.nan
        v[n_grad * NC - 1, B - 1] = -np.inf
        return x, one(v, ess_frac=2.0, step=3)
    if kind == "all_non_finite":
        v = np.full((n_grad * NC, B), np.nan)
        v[:, ::2] = np.inf
        return x, one(v, ess_frac=2.0)
    if kind in ("ess_below", "ess_above"):
        v = _values(rs, n_grad, B, 3.0)
        z = np.zeros((NC, B))
        ess0 = orc.resample_step(x, v, n_grad, 0.25, 0.0, uniforms(0), z, z)["ess"][0]
        return x, one(v, ess_frac=float(ess0) / B * (1.0 + (1e-6 if kind == "ess_below" else -1e-6)))
    if kind == "two_calls":
        return x, one(_values(rs, n_grad, B, 2.0), ess_frac=1e-3) + one(_values(rs, n_grad, B, 3.0), ess_frac=2.0, step=3)
    raise KeyError(kind)


def uniforms(step: int) -> np.ndarray:
    return np.array([orc.uniform(SEED, k, step) for k in KEYS])


def expected(x, calls, n_grad):
    """The oracle's result of every call (logw / vprev carried), as a list."""
    B = x.shape[1]
    logw, vprev = np.zeros((NC, B)), np.zeros((NC, B))
    out = []
    for c in calls:
        r = orc.resample_step(x, c["values"], n_grad, c["beta"], c["ess_frac"], uniforms(c["step"]), logw, vprev)
        logw, vprev = r["logw"], r["vprev"]
        out.append(r)
    return out


def all_cases():
    for kind in KINDS:
        for B in BS:
            for L in LS:
                for n_grad in NGRADS:
                    yield kind, B, L, n_grad


def greedy_case(B: int, L: int):
    """beta = 1e6, ess_frac = 2, distinct values a unit apart: every ancestor is the argmax finger."""
    rs = np.random.RandomState(50 + B + L)
    x = _x(rs, B, L)
    v = np.stack([rs.permutation(B).astype(np.float64) for _ in range(NC)])
    return x, [dict(values=v, beta=1e6, ess_frac=2.0, step=0)]
