"""Restatement for the stochastic-step tests (include/dgdm_hip.h, dgdm_ddim_guided_step_noisy): the raw Philox stream from numpy's own
generator, the Box-Muller recipe in float64 rounded once to float32, the noisy DDIM step in float32 numpy with one rounding per operation
in the kernel's order (csrc/smallnet.hip ddim_step_kernel<., true>), and the eta coefficients in float64."""
import numpy as np

MASK64 = (1 << 64) - 1


def raw_stream(seed: int, key: int, step_index: int, n: int) -> np.ndarray:
    """Raw outputs 0 .. n - 1 (uint64) of the stream keyed (seed, key) at step `step_index`."""
    bg = np.random.Philox(key=np.array([seed & MASK64, key & MASK64], dtype=np.uint64), counter=np.array([0, step_index, 0, 0], dtype=np.uint64))
    return bg.random_raw(n)


def normals(seed: int, key: int, step_index: int, per_chain: int) -> np.ndarray:
    """Elements 0 .. per_chain - 1 of one chain's step noise: (float32 values, the float64 values they were rounded from)."""
    r = raw_stream(seed, key, step_index, 2 * per_chain)
    r0, r1 = r[0::2], r[1::2]
    u1 = ((r0 >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = (r1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    return z.astype(np.float32), z


def step_noise(seed: int, keys, step_index: int, per_chain: int) -> np.ndarray:
    """(len(keys), per_chain) float32: what engine.step_noise returns."""
    return np.stack([normals(seed, k, step_index, per_chain)[0] for k in keys])


def noisy_step(x, eps, grad, n_grad, coef, scale, sigma, dirc, z, lo=None, hi=None) -> np.ndarray:
    """x, eps, z: float32 arrays of one shape (n entries); grad: None or (n_grad, *x.shape), whose mean guides the step; coef: the float32
    values sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_prev) (a fourth is ignored: dirc stands in its place); lo, hi: None ([-1, 1]) or
    float32 arrays whose entries repeat over x.  Returns x_next, float32, in the shape of x."""
    f = np.float32
    x, e, z = np.asarray(x, dtype=f), np.asarray(eps, dtype=f), np.asarray(z, dtype=f)
    n = x.size
    sa, sb, sap = (f(c) for c in coef[:3])
    sigma, dirc = f(sigma), f(dirc)
    if lo is None:
        lo, hi = np.full(n, -1.0, dtype=f), np.full(n, 1.0, dtype=f)
    else:
        lo, hi = np.asarray(lo, dtype=f).reshape(-1), np.asarray(hi, dtype=f).reshape(-1)
        assert lo.size == hi.size and lo.size > 0 and n % lo.size == 0
        lo, hi = np.tile(lo, n // lo.size), np.tile(hi, n // hi.size)
    xf, e, z = x.reshape(-1), e.reshape(-1), z.reshape(-1)
    if grad is not None:
        g = np.asarray(grad, dtype=f).reshape(int(n_grad) if n_grad > 1 else 1, n)
        acc = g[0]
        if n_grad > 1:                                  # grad = 0.0; grad += g_k; grad /= n
            acc = f(0.0) + g[0]
            for k in range(1, int(n_grad)):
                acc = acc + g[k]
            acc = acc / f(n_grad)
        e = e - (sb * acc) * f(scale)
    x0 = (xf - sb * e) / sa
    x0 = np.minimum(np.maximum(x0, lo), hi)
    out = (sap * x0 + dirc * e) + sigma * z
    assert out.dtype == f
    return out.reshape(x.shape)


def eta_coefficients64(abar_t: float, abar_prev: float, eta: float):
    """(sigma, dir) of the closed form in float64 from float64 copies of the table's two entries."""
    a_t, a_p = float(abar_t), float(abar_prev)
    variance = (1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p)
    sigma = float(eta) * variance ** 0.5
    return sigma, (1.0 - a_p - sigma ** 2) ** 0.5
