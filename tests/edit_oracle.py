"""Restatement for the edit tests: the bounded DDIM step (include/dgdm_hip.h dgdm_ddim_guided_step_bounded) in float32 numpy, one rounding
per operation and in the kernel's order (csrc/smallnet.hip ddim_step_kernel<true>)."""
import numpy as np


def bounded_step(x, eps, grad, n_grad, coef, scale, lo, hi) -> np.ndarray:
    """x, eps: float32 arrays of one shape (n entries); grad: None or (n_grad, *x.shape), whose mean guides the step; coef: the float32
    values sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_prev), sqrt(1 - abar_prev); lo, hi: float32 arrays whose entries repeat over x with
    period lo.size (which divides x.size).  Returns x_next, float32, in the shape of x."""
    f = np.float32
    x, e = np.asarray(x, dtype=f), np.asarray(eps, dtype=f)
    n = x.size
    sa, sb, sap, sbp = (f(c) for c in coef)
    lo, hi = np.asarray(lo, dtype=f).reshape(-1), np.asarray(hi, dtype=f).reshape(-1)
    assert lo.size == hi.size and lo.size > 0 and n % lo.size == 0
    lo, hi = np.tile(lo, n // lo.size), np.tile(hi, n // hi.size)
    xf, e = x.reshape(-1), e.reshape(-1)
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
    out = sap * x0 + sbp * e
    assert out.dtype == f
    return out.reshape(x.shape)
