"""Resampling the fingers of a chain by predicted objective during stochastic sampling.

The B fingers of a chain are treated as particles of the eta > 0 sampler: every `every` steps they are weighted by the quantity whose
gradient already guides the chain - the dynamics model's objective at (x_t, t), summed over the finger's grid cells -, and when the
weights have degenerated the promising fingers are copied over the poor ones (systematic resampling); the keyed step noise parts the
copies again.  The mechanism is this project's own: the reference has no counterpart, `beta` is untuned, and nothing here shows that it
improves an objective on real checkpoints.  The device recipe is in include/dgdm_hip.h (dgdm_chain_resample); the loop that applies it
is sampler.run_chains."""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence


class Resample:
    """every: evaluate after every `every`-th DDIM step (never after the last one).  beta: the inverse temperature of the weights,
    exp(beta * mean objective per grid cell), relative to the previous evaluation; 0 weighs all fingers alike and never resamples.
    ess_frac: resample when the effective sample size falls below ess_frac * B; above 1: whenever evaluated."""

    def __init__(self, every: int, beta: float, ess_frac: float = 0.5):
        if isinstance(every, bool) or int(every) != every or int(every) < 1:
            raise ValueError(f"Resample: every {every!r} is not a positive integer")
        beta, ess_frac = float(beta), float(ess_frac)
        if not (math.isfinite(beta) and beta >= 0.0):
            raise ValueError(f"Resample: beta {beta!r} is not a finite non-negative number")
        if not ess_frac > 0.0:
            raise ValueError(f"Resample: ess_frac {ess_frac!r} is not positive")
        self.every, self.beta, self.ess_frac = int(every), beta, ess_frac

    def __repr__(self) -> str:
        return f"Resample(every={self.every}, beta={self.beta}, ess_frac={self.ess_frac})"

    def evaluates(self, si: int, n_steps: int) -> bool:
        """Whether walk step `si` of `n_steps` is followed by an evaluation: every `every`-th step, never the last."""
        return (si + 1) % self.every == 0 and si < n_steps - 1

    def evaluations(self, n_steps: int) -> List[int]:
        return [si for si in range(n_steps) if self.evaluates(si, n_steps)]


def from_flags(every: Optional[int], beta: Optional[float], ess_frac: Optional[float], classifier_guidance: bool, eta: float) -> Optional[Resample]:
    """The Resample of --resample_every / --resample_beta / --resample_ess, or None when none of them is given.  ValueError: a flag
    without --resample_every and --resample_beta, or without --classifier_guidance and --eta > 0."""
    if every is None and beta is None and ess_frac is None:
        return None
    if every is None or beta is None:
        raise ValueError("--resample_every and --resample_beta go together (--resample_ess is optional)")
    if not classifier_guidance:
        raise ValueError("--resample_*: resampling weighs fingers by the dynamics model's objective and needs --classifier_guidance")
    if not float(eta) > 0.0:
        raise ValueError("--resample_*: copies of a finger only part again under stochastic steps; give --eta > 0")
    return Resample(every, beta) if ess_frac is None else Resample(every, beta, ess_frac)


def summarise(log: Sequence, n_chains: int, batch: int) -> List[Dict[str, Any]]:
    """Per chain, from the (si, ess, did, ancestors) entries run_chains hands its `resample_log`: evaluations, resamples, the minimum
    effective sample size and the minimum number of distinct ancestors over the evaluations (B when there were none)."""
    out = [dict(evaluations=0, resamples=0, ess_min=float(batch), distinct_min=int(batch)) for _ in range(n_chains)]
    for _, ess, did, anc in log:
        ess, did, anc = ess.cpu().numpy(), did.cpu().numpy(), anc.cpu().numpy()
        for k in range(n_chains):
            r = out[k]
            r["evaluations"] += 1
            r["resamples"] += int(did[k])
            r["ess_min"] = min(r["ess_min"], float(ess[k]))
            r["distinct_min"] = min(r["distinct_min"], len(set(anc[k].tolist())))
    return out


def resample_from_args(args) -> Optional[Resample]:
    """--resample_every / --resample_beta / --resample_ess of the generator's entry point, checked before anything is built."""
    r = from_flags(getattr(args, "resample_every", None), getattr(args, "resample_beta", None), getattr(args, "resample_ess", None),
                   bool(getattr(args, "classifier_guidance", False)), float(getattr(args, "eta", 0.0) or 0.0))
    if r is None:
        return None
    if getattr(args, "mode", "test") != "test":
        raise ValueError("--resample_*: resampling belongs to the sampling loops of --mode=test")
    if getattr(args, "edit_from", None) is not None:
        raise ValueError("--resample_* with --edit_from: a finger's bounds belong to its slot; resampled edits are not supported")
    if getattr(args, "global_cond", None) is not None or getattr(args, "cond_target", None) is not None:
        raise ValueError("--resample_* with --global_cond / --cond_target: a finger's condition row belongs to its slot; not supported")
    return r
