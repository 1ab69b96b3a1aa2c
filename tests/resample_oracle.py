"""Resampling fingers by predicted objective, restated in numpy float64: the recipe of include/dgdm_hip.h (dgdm_guidance_objective_values,
dgdm_chain_resample, dgdm_resample_uniform) line for line.  Every sum runs in ascending order, one term at a time - numpy's pairwise
np.sum is not used where the recipe fixes an order."""
import numpy as np


def uniform(seed: int, key: int, step_index: int) -> float:
    """u = (r >> 11) * 2^-53, r = raw output 0 of Philox(key=[seed, key], counter=[0, step_index, 1, 0])."""
    m = (1 << 64) - 1
    bg = np.random.Philox(key=np.array([int(seed) & m, int(key) & m], dtype=np.uint64), counter=np.array([0, int(step_index), 1, 0], dtype=np.uint64))
    return float(int(bg.random_raw(1)[0]) >> 11) * 2.0 ** -53


def step_noise_first_words(seed: int, key: int, step_index: int) -> np.ndarray:
    """The raw words the step noise of (seed, key, step_index) starts from: counter [0, step_index, 0, 0]."""
    m = (1 << 64) - 1
    bg = np.random.Philox(key=np.array([int(seed) & m, int(key) & m], dtype=np.uint64), counter=np.array([0, int(step_index), 0, 0], dtype=np.uint64))
    return bg.random_raw(4)


def objective_values(logits, lin, quad, use_rowcoef, batch: int, rowcoef=None, field=None):
    """One chain: logits (R, 3) float32, row r = cell * B + b -> (V (B,), sum |terms| (B,)), both float64."""
    d = np.asarray(logits, dtype=np.float32).astype(np.float64)
    R = d.shape[0]
    lin, quad = np.asarray(lin, dtype=np.float32).astype(np.float64), np.asarray(quad, dtype=np.float32).astype(np.float64)
    V, A = np.zeros(batch), np.zeros(batch)
    for r in range(R):
        b = r % batch
        terms = []
        for j in range(3):
            terms += [lin[j] * d[r, j], quad[j] * d[r, j] * d[r, j]]
        if use_rowcoef == 1:
            terms.append(float(np.float32(rowcoef[r])) * d[r, 0])
        if use_rowcoef == 2:
            terms += [float(np.float32(field[r, j])) * d[r, j] for j in range(3)]
        for t in terms:
            V[b] += t
            A[b] += abs(t)
    return V, A


def resample_step(x, values, n_grad: int, beta_per_cell: float, ess_frac: float, u, logw, vprev):
    """x (nc, B, L), values (n_grad * nc, B) object-major, u (nc,) the chains' uniforms, logw / vprev (nc, B) ->
    dict(x, ancestors, ess, did, logw, vprev, margin): the recipe's six steps per chain; margin (nc, B) = min_b |cum_b - p_j| of every
    ancestor decision (inf where the chain did not resample).  Inputs are not modified."""
    x = np.asarray(x)
    values = np.asarray(values, dtype=np.float64)
    nc, B = x.shape[0], x.shape[1]
    logw, vprev = np.array(logw, dtype=np.float64, copy=True), np.array(vprev, dtype=np.float64, copy=True)
    x_out = x.copy()
    anc = np.tile(np.arange(B, dtype=np.int32), (nc, 1))
    ess, did = np.zeros(nc), np.zeros(nc, dtype=np.int32)
    margin = np.full((nc, B), np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(nc):
            for b in range(B):
                s = 0.0
                for j in range(n_grad):
                    s = s + values[j * nc + k, b]
                v = beta_per_cell * (s / float(n_grad))
                if not np.isfinite(v):
                    logw[k, b] = -np.inf
                else:
                    logw[k, b] = logw[k, b] + (v - vprev[k, b])
                    vprev[k, b] = v
            m = -np.inf
            for b in range(B):
                if logw[k, b] > m:
                    m = logw[k, b]
            if m == -np.inf:
                logw[k] = 0.0
                continue
            w = np.exp(logw[k] - m)
            s = 0.0
            for b in range(B):
                s = s + w[b]
            w = w / s
            s2 = 0.0
            for b in range(B):
                s2 = s2 + w[b] * w[b]
            ess[k] = 1.0 / s2
            if not ess[k] < ess_frac * B:
                continue
            cum = np.zeros(B)
            c = 0.0
            for b in range(B):
                c = c + w[b] if b else w[0]
                cum[b] = c
            old = vprev[k].copy()
            for j in range(B):
                p = (float(u[k]) + j) / B
                a = min(int(np.count_nonzero(cum <= p)), B - 1)
                anc[k, j] = a
                margin[k, j] = float(np.min(np.abs(cum - p)))
                x_out[k, j] = x[k, a]
                vprev[k, j] = old[a]
            logw[k] = 0.0
            did[k] = 1
    return dict(x=x_out, ancestors=anc, ess=ess, did=did, logw=logw, vprev=vprev, margin=margin)
