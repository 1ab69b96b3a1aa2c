"""Goal-pose objectives: a chosen pose (theta*, x*, y*) the designs should bring the object to.

The reference's 16 objectives are one direction for every pose of the grid ('rotate_clockwise', 'shift_up', ...) or 'convergence',
which pulls the orientation toward a centre the user cannot choose.  A ``Goal`` states the target instead; wherever a chain is an
``(object_index, name)`` pair it may be ``(object_index, Goal)``.  Guidance turns it into a row field (include/dgdm_hip.h,
dgdm_guidance_goal_field): per pose of the cond_fn grid the windowed direction from that pose to the goal, which seeds the trunk's
backward pass for all three outputs.  Scoring (dynamics/predicted.py ``goal_objective``) counts the start orientations whose
predicted roll-out settles at the goal.  No part of this exists in the reference.

Units: ``ori`` and ``pos`` are the dynamics model's normalised inputs (dynamics/dataloader.py:51-52): ori = theta / pi - 1 in
[-1, 1], pos = metres / 0.03.  ``Goal.from_physical`` takes degrees and metres.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Any, Optional, Sequence, Tuple

from .dynamics.dataloader import POS_NORM

PROFILES = {'sign': 0, 'linear': 1}      # DgdmGoalSpec.profile (include/dgdm_hip.h)


@dataclass(frozen=True, eq=False)
class Goal:
    """A goal pose and how strongly, how far and in which shape the guidance pulls toward it.

    ori, pos: the goal in normalised units (see the module docstring).  ``fingers``: a per-finger goal instead - a (B, 3) tensor or
    array of (ori, pos_x, pos_y) rows, one per finger of the batch (``Goal.per_finger``); ori / pos are then not read.
    weight: per output (rotation, shift x, shift y); (1, 0, 0) guides the orientation alone.
    ori_window in (0, 1], pos_window > 0: half-widths, in normalised units, of the band of poses around the goal that are pulled.
    profile: 'sign' - unit pull inside the window, none outside (and none exactly at the goal); 'linear' - proportional to the
    distance, saturating at the window.
    scale: the classifier scale of the chain; None = what ``sampler.classifier_scale(mode, 'convergence', multi)`` returns.  That
    default is borrowed from 'convergence', the one reference objective that also pulls toward a pose; nobody has tuned it for goals."""
    ori: float = 0.0
    pos: Tuple[float, float] = (0.0, 0.0)
    weight: Tuple[float, float, float] = (1.0, 0.0, 0.0)
    ori_window: float = 0.5
    pos_window: float = 1.0
    profile: str = 'sign'
    scale: Optional[float] = None
    fingers: Any = None

    def __post_init__(self):
        fin = lambda v: isinstance(v, numbers.Real) and math.isfinite(v)      # noqa: E731  (numpy scalars included)
        if self.fingers is None:
            if not fin(self.ori) or not -1.0 <= self.ori <= 1.0:
                raise ValueError(f"Goal: ori = {self.ori!r} outside [-1, 1] (ori = theta / pi - 1)")
            if len(self.pos) != 2 or not all(fin(v) for v in self.pos):
                raise ValueError(f"Goal: pos = {self.pos!r} is not two finite numbers (metres / {POS_NORM})")
        else:
            import numpy as np
            f = np.asarray(self.fingers.detach().cpu() if hasattr(self.fingers, "detach") else self.fingers, dtype=np.float64)
            if f.ndim != 2 or f.shape[1] != 3 or not np.isfinite(f).all() or (np.abs(f[:, 0]) > 1.0).any():
                raise ValueError(f"Goal: per-finger goals must be finite (B, 3) rows of (ori in [-1, 1], pos_x, pos_y), got shape {f.shape}")
        if len(self.weight) != 3 or not all(fin(v) for v in self.weight):
            raise ValueError(f"Goal: weight = {self.weight!r} is not three finite numbers")
        if not fin(self.ori_window) or not 0.0 < self.ori_window <= 1.0:
            raise ValueError(f"Goal: ori_window = {self.ori_window!r} outside (0, 1]")
        if not fin(self.pos_window) or not self.pos_window > 0.0:
            raise ValueError(f"Goal: pos_window = {self.pos_window!r} is not a positive number")
        if self.profile not in PROFILES:
            raise ValueError(f"Goal: profile = {self.profile!r} (one of {sorted(PROFILES)})")
        if self.scale is not None and not fin(self.scale):
            raise ValueError(f"Goal: scale = {self.scale!r} is not a finite number")

    @classmethod
    def from_physical(cls, theta_deg: float, x_m: float = 0.0, y_m: float = 0.0, window_deg: Optional[float] = None,
                      window_m: Optional[float] = None, **kw) -> "Goal":
        """theta_deg: the goal orientation in degrees (any angle; taken modulo 360, 0 .. 360 maps onto ori -1 .. 1); x_m, y_m: the goal
        position in metres; window_deg / window_m: the half-widths in degrees / metres (default: ori_window / pos_window's own)."""
        if not all(isinstance(v, numbers.Real) and math.isfinite(v) for v in (theta_deg, x_m, y_m)):
            raise ValueError(f"Goal.from_physical: ({theta_deg!r}, {x_m!r}, {y_m!r}) is not three finite numbers")
        if window_deg is not None:
            kw['ori_window'] = float(window_deg) / 180.0
        if window_m is not None:
            kw['pos_window'] = float(window_m) / POS_NORM
        return cls(ori=(float(theta_deg) % 360.0) / 180.0 - 1.0, pos=(float(x_m) / POS_NORM, float(y_m) / POS_NORM), **kw)

    @classmethod
    def per_finger(cls, fingers, **kw) -> "Goal":
        """One goal per finger: (B, 3) rows of (ori, pos_x, pos_y) in normalised units."""
        return cls(fingers=fingers, **kw)

    def triples(self, batch: int):
        """(batch, 3) float32 tensor of (ori, pos_x, pos_y) per finger."""
        import torch
        if self.fingers is None:
            return torch.tensor([[self.ori, self.pos[0], self.pos[1]]], dtype=torch.float32).expand(int(batch), 3).contiguous()
        f = torch.as_tensor(self.fingers).detach().to(dtype=torch.float32).cpu()
        if f.shape[0] != int(batch):
            raise ValueError(f"Goal: per-finger goals for {f.shape[0]} fingers, the batch has {int(batch)}")
        return f.contiguous()

    def field(self, batch: int, grid_size: int, num_pos: int, ori_range: Sequence[float] = (-1.0, 1.0)):
        """The goal's row field (batch * grid_size * num_pos^2, 3) float32 on the host, row r = cell * B + b, cell = (g * P + px) * P +
        py: the definition of dgdm_guidance_goal_field restated in torch (float32 grids, float64 arithmetic, one rounding).  The
        sampling path builds it on the device; this is for callers that want objective values (Diffusion.deltas_to_objective)."""
        import torch
        B, G, P = int(batch), int(grid_size), int(num_pos)
        ori, pos = _linspace_f32(ori_range[0], ori_range[1], G).double(), _linspace_f32(-1.0, 1.0, P).double()
        goal = self.triples(B).double()                                                  # (B, 3)
        u0 = goal[None, :, 0] - ori[:, None]                                             # (G, B)
        u0 = torch.where(u0 > 1.0, u0 - 2.0, torch.where(u0 < -1.0, u0 + 2.0, u0))
        u1, u2 = goal[None, :, 1] - pos[:, None], goal[None, :, 2] - pos[:, None]        # (P, B)
        shape = (G, P, P, B)
        u = torch.stack([u0[:, None, None, :].expand(shape), u1[None, :, None, :].expand(shape), u2[None, None, :, :].expand(shape)], dim=-1)
        h = torch.tensor([float(torch.tensor(self.ori_window, dtype=torch.float32))] + [float(torch.tensor(self.pos_window, dtype=torch.float32))] * 2,
                         dtype=torch.float64)
        if self.profile == 'sign':
            s = torch.where((u.abs() > 0) & (u.abs() <= h), torch.sign(u), torch.zeros_like(u))
        else:
            s = torch.clamp(u / h, -1.0, 1.0)
        w = torch.tensor(self.weight, dtype=torch.float32).double()
        return (w * s).to(torch.float32).reshape(G * P * P * B, 3)

    @property
    def theta_deg(self) -> float:
        return (self.ori + 1.0) * 180.0

    @property
    def name(self) -> str:
        """The tag of the goal in table keys and directory names, e.g. 'goal_30.0deg_0.00_0.00cm'."""
        if self.fingers is not None:
            return "goal_per_finger"
        return "goal_%.1fdeg_%.2f_%.2fcm" % (self.theta_deg, self.pos[0] * POS_NORM * 100.0, self.pos[1] * POS_NORM * 100.0)

    def __str__(self) -> str:
        return self.name


def _linspace_f32(start: float, end: float, steps: int):
    """The guidance handle's float32 grid (csrc/guidance_api.hip linspace_f32): symmetric around the midpoint, every operation rounded
    to float32 - torch.linspace's CPU kernel fuses its multiply-add and differs in the last bit at some entries."""
    import numpy as np
    import torch
    a, b = np.float32(start), np.float32(end)
    if steps == 1:
        return torch.tensor([a], dtype=torch.float32)
    step, half = np.float32((b - a) / np.float32(steps - 1)), steps // 2
    return torch.from_numpy(np.array([a + step * np.float32(i) if i < half else b - step * np.float32(steps - i - 1) for i in range(steps)],
                                     dtype=np.float32))


def is_goal(o: Any) -> bool:
    return isinstance(o, Goal)


def goal_from_args(args) -> Optional[Goal]:
    """The Goal of the command line (dynamics/parser.py: --goal_pose THETA_DEG,X_CM,Y_CM and the --goal_* flags), or None."""
    pose = getattr(args, "goal_pose", None)
    if not pose:
        return None

    def numbers(text: str, n: int, flag: str) -> Sequence[float]:
        try:
            v = [float(s) for s in str(text).split(",")]
        except ValueError:
            v = []
        if len(v) != n:
            raise ValueError(f"--{flag} {text!r}: {n} comma-separated numbers expected")
        return v
    theta, x_cm, y_cm = numbers(pose, 3, "goal_pose")
    kw = {'weight': tuple(numbers(getattr(args, "goal_weight", None) or "1,0,0", 3, "goal_weight")),
          'profile': getattr(args, "goal_profile", None) or 'sign', 'scale': getattr(args, "goal_scale", None)}
    return Goal.from_physical(theta, x_cm / 100.0, y_cm / 100.0, window_deg=getattr(args, "goal_window_deg", None),
                              window_m=None if getattr(args, "goal_window_cm", None) is None else args.goal_window_cm / 100.0, **kw)
