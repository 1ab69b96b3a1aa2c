"""Editing an existing design: per-point bounds and pins through the DDIM step.

Every chain of the reference starts from noise and may end anywhere in [-1, 1]^L.  An ``Edit`` says "improve THESE designs" instead:

* the chain starts from the designs, partially noised - ``add_noise(designs, noise, timesteps[S-K])`` - and runs the schedule's last K
  steps: the move the reference's first validation loop makes with its data (generator/diffusion.py:184-201);
* every step clips the predicted clean sample to per-entry bounds ``lo <= hi`` inside [-1, 1] instead of the scheduler's
  ``clip_sample=True`` range [-1, 1] (``dgdm_ddim_guided_step_bounded``).  ``lo == hi == d`` pins a control point: its predicted clean
  value is d at every step, its noisy state stays a consistent DDIM state the eps-net sees, and after the last step it is exactly d.
  ``lo = max(-1, d - u), hi = min(1, d + u)`` keeps a control point within u of the design.

The start from partially noised data is the reference's; the per-entry clip is this project's own and has no reference counterpart to
pin it to.  The default classifier scales are untuned for edits, and nothing here claims that an edit improves an objective on real
checkpoints.

Everything is validated here, on the host, before anything is uploaded.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

MODES = ('point', 'point_3d')
# metres per sampler unit: DGDM_DECODE_2D_SCALE / DGDM_DECODE_3D_SCALE of include/dgdm_hip.h (y = scale * p + offset)
DECODE_SCALE = {'point': 0.03, 'point_3d': 0.05}


def band_from_mm(mm: float, mode: str) -> float:
    """A half-width in millimetres -> sampler units: mm / 1000 / DGDM_DECODE_{2D,3D}_SCALE (1 mm = 1/30 unit in 2-D, 1/50 in 3-D)."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r} is neither 'point' nor 'point_3d'")
    return float(mm) / 1000.0 / DECODE_SCALE[mode]


def parse_pins(text: Optional[str], L: int) -> Tuple[int, ...]:
    """--pin 0-6,10: comma-separated indices and inclusive ranges into [0, L) -> the sorted distinct indices.  ValueError for anything else."""
    if text is None or not str(text).strip():
        return ()
    out: List[int] = []
    for part in str(text).split(","):
        a, sep, b = part.strip().partition("-")
        try:
            first = int(a)
            last = int(b) if sep else first
        except ValueError:
            raise ValueError(f"--pin {text!r}: '{part}' is neither an index nor a range FIRST-LAST")
        if last < first:
            raise ValueError(f"--pin {text!r}: range '{part}' runs backwards")
        out.extend(range(first, last + 1))
    return check_pins(out, L)


def check_pins(pins: Iterable[int], L: int) -> Tuple[int, ...]:
    out = sorted({int(p) for p in pins})
    if out and (out[0] < 0 or out[-1] >= L):
        raise ValueError(f"pins {[p for p in out if p < 0 or p >= L]} outside [0, {L})")
    return tuple(out)


class Edit:
    """designs: (B, L) or (B, L, 1) float32 in sampler units, finite and inside [-1, 1].  pins: indices into [0, L) held at the design's
    value (the first L/2 entries are the left finger, include/dgdm_hip.h "finger-geometry decode").  band: half-width in sampler units
    every unpinned entry stays within (None: only the scheduler's [-1, 1]).  steps = K: how many of the schedule's S steps the edit runs
    (None: all S); 1 <= K <= S is checked where the schedule is known (``n_steps``).  mode: 'point' / 'point_3d', the units of
    ``from_physical`` and ``moved_mm``."""

    def __init__(self, designs, pins: Sequence[int] = (), band: Optional[float] = None, steps: Optional[int] = None, mode: str = 'point'):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r} is neither 'point' nor 'point_3d'")
        d = np.asarray(designs.detach().cpu().numpy() if isinstance(designs, torch.Tensor) else designs)
        if d.ndim == 3 and d.shape[-1] == 1:
            d = d[..., 0]
        if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] < 1:
            raise ValueError(f"designs have shape {d.shape}, expected (B, L) or (B, L, 1)")
        if d.dtype.kind not in "fiu":
            raise ValueError(f"designs hold {d.dtype}, expected float32")
        d = np.ascontiguousarray(d, dtype=np.float32)
        if not np.isfinite(d).all():
            raise ValueError("designs hold non-finite values")
        if (np.abs(d) > 1.0).any():
            raise ValueError(f"designs leave the sampler's range [-1, 1] (max |value| {float(np.abs(d).max())})")
        if band is not None and not (np.isfinite(band) and float(band) >= 0.0):
            raise ValueError(f"band {band} is not a finite half-width >= 0")
        if steps is not None and int(steps) < 1:
            raise ValueError(f"steps = {steps}: an edit runs at least one step")
        self.designs = d
        self.pins = check_pins(pins, d.shape[1])
        self.band = None if band is None else float(band)
        self.steps = None if steps is None else int(steps)
        self.mode = mode
        self._dev = None

    @classmethod
    def from_physical(cls, designs, pins: Sequence[int] = (), band_mm: Optional[float] = None, steps: Optional[int] = None, mode: str = 'point') -> "Edit":
        """The band as a half-width in millimetres of finger geometry."""
        return cls(designs, pins, None if band_mm is None else band_from_mm(band_mm, mode), steps, mode)

    @property
    def shape(self) -> Tuple[int, int]:
        return self.designs.shape

    def n_steps(self, sched) -> int:
        """K for this schedule: ``steps`` or all S; ValueError unless 1 <= K <= S."""
        S = len(sched.timesteps)
        K = S if self.steps is None else self.steps
        if not 1 <= K <= S:
            raise ValueError(f"an edit of {K} steps does not fit a schedule of {S}")
        return K

    def bounds(self) -> Tuple[np.ndarray, np.ndarray]:
        """(lo, hi) float32 (B, L), every operation in float32: lo <= designs <= hi everywhere, pins override the band."""
        d = self.designs
        if self.band is None:
            lo, hi = np.full_like(d, -1.0), np.full_like(d, 1.0)
        else:
            u = np.float32(self.band)
            lo, hi = np.maximum(np.float32(-1.0), d - u), np.minimum(np.float32(1.0), d + u)
        if self.pins:
            lo[:, list(self.pins)] = d[:, list(self.pins)]
            hi[:, list(self.pins)] = d[:, list(self.pins)]
        return lo, hi

    def bounds_on(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """bounds() on the device, uploaded once per device."""
        if self._dev is None or self._dev[0] != torch.device(device):
            lo, hi = self.bounds()
            self._dev = (torch.device(device), torch.from_numpy(lo).to(device), torch.from_numpy(hi).to(device))
        return self._dev[1], self._dev[2]

    def designs_on(self, device) -> torch.Tensor:
        """(B, L, 1) on the device."""
        return torch.from_numpy(self.designs).to(device)[..., None]

    def start(self, sched, noise: torch.Tensor):
        """(x_start, timesteps[-K:]): x_start = sched.add_noise(designs, noise, timesteps[S-K]), in the shape of `noise`."""
        K = self.n_steps(sched)
        if tuple(noise.shape[:2]) != self.shape or noise.numel() != self.designs.size:
            raise ValueError(f"noise of shape {tuple(noise.shape)} does not match the designs' {self.shape}")
        ts = sched.timesteps[len(sched.timesteps) - K:]
        d = torch.from_numpy(self.designs).to(noise.device).reshape(noise.shape)
        x = sched.add_noise(d, noise, torch.full((self.shape[0],), int(ts[0]), dtype=torch.int64))
        return x, ts

    def moved_mm(self, out) -> Tuple[np.ndarray, np.ndarray]:
        """How far `out` (..., B, L[, 1]) lies from the designs, in millimetres of finger geometry: (max, rms) over the L control values,
        each (..., B)."""
        o = np.asarray(out.detach().cpu().numpy() if isinstance(out, torch.Tensor) else out, dtype=np.float64)
        if o.shape[-1] == 1 and o.shape[-2:] != self.shape:
            o = o[..., 0]
        if o.shape[-2:] != self.shape:
            raise ValueError(f"samples of shape {o.shape} do not end in the designs' {self.shape}")
        diff = np.abs(o - self.designs.astype(np.float64)) * (DECODE_SCALE[self.mode] * 1000.0)
        return diff.max(axis=-1), np.sqrt((diff ** 2).mean(axis=-1))


def load_designs(path: str, batch_size: int, L: int) -> np.ndarray:
    """--edit_from FILE.npy: (n, L) or (n, L, 1) with n >= batch_size -> float32 (n, L).  ValueError otherwise (values are checked by Edit)."""
    try:
        d = np.load(path, allow_pickle=False)
    except Exception as e:
        raise ValueError(f"--edit_from: cannot read '{path}' as a .npy array ({type(e).__name__}: {e})")
    if d.ndim == 3 and d.shape[-1] == 1:
        d = d[..., 0]
    if d.ndim != 2 or d.shape[1] != L:
        raise ValueError(f"--edit_from: '{path}' has shape {d.shape}, expected (n, {L}) or (n, {L}, 1)")
    if d.shape[0] < batch_size:
        raise ValueError(f"--edit_from: '{path}' holds {d.shape[0]} designs, fewer than --batch_size={batch_size}")
    if d.dtype.kind not in "fiu":
        raise ValueError(f"--edit_from: '{path}' holds {d.dtype}, expected float32")
    return np.ascontiguousarray(d, dtype=np.float32)


class EditPlan:
    """What the command line asks for (dynamics/parser.py: --edit_from, --edit_steps, --pin, --edit_band_mm): the designs of all batches
    and the constraints; ``batch(b, B)`` is the Edit of rows [b B, (b + 1) B)."""

    def __init__(self, designs: np.ndarray, pins: Sequence[int] = (), band_mm: Optional[float] = None, steps: Optional[int] = None, mode: str = 'point'):
        self.designs, self.pins, self.band_mm, self.steps, self.mode = designs, tuple(pins), band_mm, steps, mode
        Edit.from_physical(designs, self.pins, band_mm, steps, mode)           # every row is checked at start-up

    def batch(self, batch_idx: int, batch_size: int) -> Edit:
        rows = self.designs[batch_idx * batch_size:(batch_idx + 1) * batch_size]
        if rows.shape[0] != batch_size:
            raise ValueError(f"--edit_from holds {self.designs.shape[0]} designs: none left for batch {batch_idx} of {batch_size}")
        return Edit.from_physical(rows, self.pins, self.band_mm, self.steps, self.mode)


def plan_from_args(args, num_inference_steps: Optional[int] = None) -> Optional[EditPlan]:
    """The EditPlan of the command line, or None.  --pin / --edit_band_mm / --edit_steps without --edit_from: ValueError."""
    path = getattr(args, "edit_from", None)
    pin, band, steps = getattr(args, "pin", None), getattr(args, "edit_band_mm", None), getattr(args, "edit_steps", None)
    if not path:
        given = [f for f, v in (("--pin", pin), ("--edit_band_mm", band), ("--edit_steps", steps)) if v is not None]
        if given:
            raise ValueError(f"{' / '.join(given)} need --edit_from: there is no design to pin, bound or edit")
        return None
    mode = 'point_3d' if getattr(args, "fingers_3d", False) else 'point'
    L = int(args.ctrlpts_dim)
    S = int(num_inference_steps if num_inference_steps is not None else args.num_inference_steps)
    if steps is not None and not 1 <= int(steps) <= S:
        raise ValueError(f"--edit_steps={steps} outside 1..{S} (--num_inference_steps)")
    return EditPlan(load_designs(path, int(args.batch_size), L), parse_pins(pin, L), band, steps, mode)
