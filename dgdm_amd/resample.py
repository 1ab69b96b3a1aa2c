"""Resampling the fingers of a chain by predicted objective during stochastic sampling.

The B fingers of a chain are treated as particles of the eta > 0 sampler: every `every` steps they are weighted by the quantity whose
gradient already guides the chain - the dynamics model's objective at (x_t, t), summed over the finger's grid cells -, and when the
weights have degenerated the promising fingers are copied over the poor ones (systematic resampling); the keyed step noise parts the
copies again.  The mechanism is this project's own: the reference has no counterpart, `beta` is untuned, and nothing here shows that it
improves an objective on real checkpoints.  The device recipe is in include/dgdm_hip.h (dgdm_chain_resample); the loop that applies it
is sampler.run_chains.

A second potential, potential='squeeze' (SqueezePotential): the squeeze simulator's objective on every finger's predicted
clean design, over the same pose grid and in the same units - an opinion that does not come from the model whose gradient guides the
chain.  Everything after the values is the same.  Equally this project's own: 2-D only, frictionless, no claim that it improves an
objective under MuJoCo or on real checkpoints.  potential='squeeze_3d' (SqueezePotential3D) is its form for 3-D fingers: the sliced
squeeze of the chain's mesh object (DESIGN.md 4.1d "3-D form"), blind between two planes of the finger grid, frictionless, untuned."""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence


POTENTIALS = ('model', 'squeeze', 'squeeze_3d')


def start_grid(grid_size: int, num_pos: int, ori_range: Sequence[float]):
    """The cells of cond_fn's pose grid (generator/diffusion.py:478) as squeeze starts, (G P^2, 3) float64 = (theta0 rad, x0 m, y0 m) in
    the grid's order n = (io * P + ix) * P + iy: theta0 = (linspace(ori_lo, ori_hi, G)[io] + 1) * pi, x0 = POS_NORM * linspace(-1, 1, P)[ix],
    y0 likewise - the model's inputs in the simulator's units."""
    import numpy as np
    from .dynamics.dataloader import POS_NORM
    G, P = int(grid_size), int(num_pos)
    theta = (np.linspace(float(ori_range[0]), float(ori_range[1]), G) + 1.0) * np.pi
    pos = POS_NORM * np.linspace(-1.0, 1.0, P)
    io, ix, iy = np.meshgrid(np.arange(G), np.arange(P), np.arange(P), indexing="ij")
    return np.ascontiguousarray(np.stack([theta[io], pos[ix], pos[iy]], axis=-1).reshape(G * P * P, 3))


class SqueezePotential:
    """The squeeze simulator's opinion of a predicted clean design: the objective's value per finger from one
    closing of the chain's object by the finger, over the starts of cond_fn's pose grid, in the units of the dynamics model's outputs -
    a potential for Resample that does not come from the model whose gradient guides the chain.  This project's own mechanism: the
    reference has no counterpart; 2-D only, frictionless, and nothing here shows that it improves an objective under MuJoCo or on real
    checkpoints.

    contours (O, nv, 2) float64, metres: the object bank in the guidance handle's object order.  score_std: (theta rad, x m, y m), the
    2-D SCORE_STD by default.  friction: the squeeze's Coulomb coefficient (0: frictionless; the values kernel reads the map's cells
    and y either way).  squeeze_config: engine.SQUEEZE_DEFAULTS' keys.  The rotation table, the bank and the start grid stay on
    the device between evaluations."""

    def __init__(self, contours, score_std=None, num_points: int = 200, friction: float = 0.0, **squeeze_config):
        import numpy as np
        from .dynamics.dataloader import SCORE_STD
        from .sim.squeeze import check_friction
        self.friction = check_friction(friction, "SqueezePotential")
        c = np.ascontiguousarray(np.asarray(contours, dtype=np.float64))
        if c.ndim != 3 or c.shape[2] != 2 or c.shape[0] < 1 or c.shape[1] < 3:
            raise ValueError(f"SqueezePotential: contours (O, nv, 2) with O >= 1, nv >= 3 expected, got {c.shape}")
        std = np.asarray(SCORE_STD[1] if score_std is None else score_std, dtype=np.float64).reshape(-1)
        if std.shape != (3,) or not (np.isfinite(std).all() and (std > 0).all()):
            raise ValueError(f"SqueezePotential: score_std {std.tolist()} is not three finite positive numbers")
        unknown = set(squeeze_config) - {"theta_cells", "x_cells", "x_half", "window", "closing_steps", "travel_max", "finger_half_len"}
        if unknown:
            raise ValueError(f"SqueezePotential: unknown squeeze_config keys {sorted(unknown)}")
        self.contours, self.score_std, self.num_points, self.config = c, tuple(float(v) for v in std), int(num_points), dict(squeeze_config)
        self._bank = self._rot = None
        self._starts: Dict[Any, Any] = {}

    @property
    def n_objects(self) -> int:
        return int(self.contours.shape[0])

    def __repr__(self) -> str:
        tail = f", friction={self.friction}" if self.friction > 0.0 else ""
        return f"SqueezePotential({self.n_objects} contours of {self.contours.shape[1]} vertices, {self.config}{tail})"

    def subset(self, objects: Sequence[int]) -> "SqueezePotential":
        """The same potential over the contours `objects` of the bank, in that order."""
        return SqueezePotential(self.contours[list(objects)], self.score_std, self.num_points, self.friction, **self.config)

    def starts(self, grid_size: int, num_pos: int, ori_range: Sequence[float]):
        """start_grid on the device, made once per grid."""
        import torch
        key = (int(grid_size), int(num_pos), float(ori_range[0]), float(ori_range[1]))
        if key not in self._starts:
            self._starts[key] = torch.from_numpy(start_grid(*key[:2], key[2:])).to(torch.device("cuda", torch.cuda.current_device()))
        return self._starts[key]

    def values(self, x0, objectives: Sequence, rowcoef, n_grad: int, grid_size: int, num_pos: int, ori_range: Sequence[float]):
        """x0 (nc, B, L) float32 on the device: predicted clean designs in sampler units; objectives [n_grad * nc], object-major as
        run_chains holds them, rowcoef (n_grad * nc, G P^2 B) or None -> (n_grad * nc, B) float64 as engine.chain_resample takes them.
        Pair (j * nc + k) * B + b = (finger k * B + b, objectives[j * nc + k].object).  One squeeze map, one values launch."""
        import numpy as np
        import torch
        from . import engine
        from .sim.squeeze import finger_surfaces
        nc, B, L = x0.shape
        n_grad = int(n_grad)
        if len(objectives) != n_grad * nc:
            raise ValueError(f"SqueezePotential.values: {len(objectives)} objectives for {n_grad} x {nc} chains")
        obj = np.array([int(o.object) for o in objectives], dtype=np.int32)
        if obj.min() < 0 or obj.max() >= self.n_objects:
            raise ValueError(f"SqueezePotential.values: an objective names object {int(obj.max())} of a bank of {self.n_objects}")
        dev = x0.device
        if self._bank is None:
            self._bank = torch.from_numpy(self.contours).to(dev)
            self._rot = torch.from_numpy(engine.squeeze_rotation_table(engine.squeeze_config(**self.config).theta_cells)).to(dev)
        st = self.starts(grid_size, num_pos, ori_range)
        sf = finger_surfaces(x0.reshape(nc * B, L), self.num_points)
        finger = (np.arange(nc, dtype=np.int32)[None, :, None] * B + np.arange(B, dtype=np.int32)[None, None, :]).repeat(n_grad, axis=0)
        pairs = np.stack([finger.reshape(-1), np.repeat(obj, B)], axis=1)
        out = engine.squeeze_tables(sf, self._bank, pairs, st, rot=self._rot, friction=self.friction, **self.config)
        return engine.squeeze_objective_values(out["cells"], out["y"], st, B, list(objectives), rowcoef, self.score_std, **self.config)


class SqueezePotential3D:
    """SqueezePotential for 3-D fingers (DESIGN.md 4.3e "potential: squeeze_3d", 4.1d "3-D form"): the sliced squeeze's objective per
    finger of a chain on that chain's object, from one engine.squeeze_values_3d call per evaluation - the tables of a chain's B fingers
    share the per-segment work, and no per-start output is stored.  Equally this project's own mechanism: the sliced model is blind
    between two planes of the finger grid and frictionless; beta, the table size and the closing steps are untuned; nothing here shows
    that it improves an objective under MuJoCo or on real checkpoints.

    meshes: a sequence of (vertices (nv, 3) in metres standing on z = 0, triangles (nt, 3)) in the guidance handle's object order.
    score_std: (theta rad, x m, y m), the 3-D SCORE_STD by default.  sample_size, width: sim.squeeze.finger_surfaces_3d's.
    squeeze_config: engine.SQUEEZE_DEFAULTS' keys; ``friction`` is refused (FRICTION_2D_ONLY).  The meshes are sliced once, at the first
    evaluation, on the levels gz of that decode (the finger grid's z depends on the v index only); the segments, the rotation table and
    the start grid stay on the device between evaluations."""

    def __init__(self, meshes, score_std=None, sample_size: int = 25, width: Optional[float] = None, **squeeze_config):
        import numpy as np
        from .dynamics.dataloader import SCORE_STD
        from .sim.squeeze import FINGER_WIDTH_3D, FRICTION_2D_ONLY
        if "friction" in squeeze_config:
            raise ValueError(f"SqueezePotential3D: {FRICTION_2D_ONLY}")
        try:
            ms = [(np.ascontiguousarray(np.asarray(v, dtype=np.float64)), np.ascontiguousarray(np.asarray(f, dtype=np.int32))) for v, f in meshes]
        except (TypeError, ValueError):
            raise ValueError("SqueezePotential3D: meshes must be a sequence of (vertices (nv, 3), triangles (nt, 3))") from None
        if not ms:
            raise ValueError("SqueezePotential3D: no meshes")
        for i, (v, f) in enumerate(ms):
            if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1 or f.ndim != 2 or f.shape[1] != 3 or not np.isfinite(v).all():
                raise ValueError(f"SqueezePotential3D: mesh {i}: finite vertices (nv, 3) and triangles (nt, 3) expected, got {v.shape} and {f.shape}")
            if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
                raise ValueError(f"SqueezePotential3D: mesh {i}: a triangle names a vertex outside its {v.shape[0]}")
        std = np.asarray(SCORE_STD[0] if score_std is None else score_std, dtype=np.float64).reshape(-1)
        if std.shape != (3,) or not (np.isfinite(std).all() and (std > 0).all()):
            raise ValueError(f"SqueezePotential3D: score_std {std.tolist()} is not three finite positive numbers")
        unknown = set(squeeze_config) - {"theta_cells", "x_cells", "x_half", "window", "closing_steps", "travel_max", "finger_half_len"}
        if unknown:
            raise ValueError(f"SqueezePotential3D: unknown squeeze_config keys {sorted(unknown)}")
        if isinstance(sample_size, bool) or int(sample_size) != sample_size or int(sample_size) < 2:
            raise ValueError(f"SqueezePotential3D: sample_size {sample_size!r} is not an integer >= 2")
        self.meshes, self.score_std, self.sample_size, self.config = ms, tuple(float(v) for v in std), int(sample_size), dict(squeeze_config)
        self.width = FINGER_WIDTH_3D if width is None else float(width)
        self._slices = self._rot = self._gz = None
        self._starts: Dict[Any, Any] = {}

    @property
    def n_objects(self) -> int:
        return len(self.meshes)

    def __repr__(self) -> str:
        return f"SqueezePotential3D({self.n_objects} meshes, sample_size={self.sample_size}, {self.config})"

    def subset(self, objects: Sequence[int]) -> "SqueezePotential3D":
        """The same potential over the meshes `objects` of the bank, in that order."""
        return SqueezePotential3D([self.meshes[int(i)] for i in objects], self.score_std, self.sample_size, self.width, **self.config)

    starts = SqueezePotential.starts

    def values(self, x0, objectives: Sequence, rowcoef, n_grad: int, grid_size: int, num_pos: int, ori_range: Sequence[float]):
        """SqueezePotential.values for 3-D fingers: x0 (nc, B, 42) float32 on the device -> (n_grad * nc, B) float64.  Group j * nc + k
        is chain k's B fingers, k * B .. k * B + B - 1 of the decode, on objectives[j * nc + k].object.  One decode of the nc * B
        designs, one engine.squeeze_values_3d call; no FPS draws, no guid.score call."""
        import numpy as np
        import torch
        from . import engine
        from .sim.squeeze import finger_surfaces_3d
        nc, B, L = x0.shape
        n_grad = int(n_grad)
        if len(objectives) != n_grad * nc:
            raise ValueError(f"SqueezePotential3D.values: {len(objectives)} objectives for {n_grad} x {nc} chains")
        obj = np.array([int(o.object) for o in objectives], dtype=np.int32)
        if obj.min() < 0 or obj.max() >= self.n_objects:
            raise ValueError(f"SqueezePotential3D.values: an objective names object {int(obj.max())} of a bank of {self.n_objects}")
        gx, gz, sf = finger_surfaces_3d(x0.reshape(nc * B, L), self.sample_size, self.width)
        if self._slices is None:
            self._slices = engine.squeeze_slice(self.meshes, gz)
            self._gz = gz
            self._rot = torch.from_numpy(engine.squeeze_rotation_table(engine.squeeze_config(**self.config).theta_cells)).to(x0.device)
        assert np.array_equal(gz, self._gz), "SqueezePotential3D: the finger grid's levels changed between evaluations"
        st = self.starts(grid_size, num_pos, ori_range)
        group_first = np.tile(np.arange(nc, dtype=np.int32) * B, n_grad)
        return engine.squeeze_values_3d(sf, gx, self._slices["segments"], self._slices["offsets"], group_first, B, list(objectives), st, rowcoef,
                                        self.score_std, rot=self._rot, **self.config)


class Resample:
    """every: evaluate after every `every`-th DDIM step (never after the last one).  beta: the inverse temperature of the weights,
    exp(beta * mean objective per grid cell), relative to the previous evaluation; 0 weighs all fingers alike and never resamples.
    ess_frac: resample when the effective sample size falls below ess_frac * B; above 1: whenever evaluated.
    potential: whose objective weighs the fingers - 'model': the dynamics model's at (x_t, t), the quantity whose gradient guides the
    chain; 'squeeze': the squeeze simulator's on the predicted clean design (`squeeze`: a SqueezePotential), a second opinion;
    'squeeze_3d': the same for 3-D fingers, by the sliced squeeze (`squeeze`: a SqueezePotential3D)."""

    def __init__(self, every: int, beta: float, ess_frac: float = 0.5, potential: str = 'model', squeeze=None):
        if isinstance(every, bool) or int(every) != every or int(every) < 1:
            raise ValueError(f"Resample: every {every!r} is not a positive integer")
        beta, ess_frac = float(beta), float(ess_frac)
        if not (math.isfinite(beta) and beta >= 0.0):
            raise ValueError(f"Resample: beta {beta!r} is not a finite non-negative number")
        if not ess_frac > 0.0:
            raise ValueError(f"Resample: ess_frac {ess_frac!r} is not positive")
        if potential not in POTENTIALS:
            raise ValueError(f"Resample: potential {potential!r} is not one of {POTENTIALS}")
        if potential == 'squeeze' and not isinstance(squeeze, SqueezePotential):
            raise ValueError("Resample: potential 'squeeze' needs a SqueezePotential (squeeze=...)")
        if potential == 'squeeze_3d' and not isinstance(squeeze, SqueezePotential3D):
            raise ValueError("Resample: potential 'squeeze_3d' needs a SqueezePotential3D (squeeze=...)")
        if potential == 'model' and squeeze is not None:
            raise ValueError("Resample: a SqueezePotential goes with potential='squeeze', a SqueezePotential3D with potential='squeeze_3d'")
        self.every, self.beta, self.ess_frac, self.potential, self.squeeze = int(every), beta, ess_frac, potential, squeeze

    def __repr__(self) -> str:
        tail = "" if self.potential == 'model' else f", potential={self.potential!r}"
        return f"Resample(every={self.every}, beta={self.beta}, ess_frac={self.ess_frac}{tail})"

    def evaluates(self, si: int, n_steps: int) -> bool:
        """Whether walk step `si` of `n_steps` is followed by an evaluation: every `every`-th step, never the last."""
        return (si + 1) % self.every == 0 and si < n_steps - 1

    def evaluations(self, n_steps: int) -> List[int]:
        return [si for si in range(n_steps) if self.evaluates(si, n_steps)]

    def fps_evaluations(self, n_steps: int) -> int:
        """How many of the evaluations draw FPS starts on a 3-D handle: all of the model's potential, none of a squeeze potential."""
        return len(self.evaluations(n_steps)) if self.potential == 'model' else 0

    def for_objects(self, objects: Sequence[int]) -> "Resample":
        """This Resample for a handle that holds only `objects` of the bank, in that order (a rank's local bank, dist.shard_chains): a
        squeeze potential's bank is cut alike; the model's potential reads the handle and is returned as it is."""
        if self.squeeze is None:
            return self
        return Resample(self.every, self.beta, self.ess_frac, self.potential, self.squeeze.subset(objects))


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


def squeeze_potential_from_args(args) -> Optional[Dict[str, Any]]:
    """--resample_potential squeeze [--resample_squeeze_cells T,X --squeeze_closing_steps K --squeeze_window R --squeeze_friction MU] ->
    SqueezePotential's squeeze_config (and friction), or None for the model's potential.  --resample_potential squeeze_3d (with the
    same companions but --squeeze_friction) -> SqueezePotential3D's squeeze_config.  ValueError: an unknown potential; 'squeeze' with
    --fingers_3d (it is 2-D only: 3-D fingers have squeeze_3d); 'squeeze_3d' without --fingers_3d or with --squeeze_friction
    (FRICTION_2D_ONLY); either with --goal_pose (goal fields have no squeeze form) or without --resample_every; --resample_squeeze_cells
    without either or not two positive integers."""
    potential = getattr(args, "resample_potential", None) or 'model'
    cells = getattr(args, "resample_squeeze_cells", None)
    if potential not in POTENTIALS:
        raise ValueError(f"--resample_potential {potential!r}: choose one of {', '.join(POTENTIALS)}")
    if potential == 'model':
        if cells is not None:
            raise ValueError("--resample_squeeze_cells needs --resample_potential squeeze (or squeeze_3d)")
        return None
    flag = f"--resample_potential {potential}"
    if getattr(args, "resample_every", None) is None:
        raise ValueError(f"{flag} needs --resample_every (and --resample_beta): it is a potential for resampling")
    if potential == 'squeeze' and getattr(args, "fingers_3d", False):
        raise ValueError("--resample_potential squeeze is 2-D only: for --fingers_3d give --resample_potential squeeze_3d (the sliced squeeze)")
    if potential == 'squeeze_3d' and not getattr(args, "fingers_3d", False):
        raise ValueError("--resample_potential squeeze_3d needs --fingers_3d: it is the sliced squeeze of 3-D fingers (--resample_potential squeeze "
                         "is the 2-D one)")
    if getattr(args, "goal_pose", None) is not None:
        raise ValueError(f"{flag} with --goal_pose: goal fields have no squeeze form, not supported")
    config: Dict[str, Any] = {}
    mu = getattr(args, "squeeze_friction", None)
    if mu is not None:
        if potential == 'squeeze_3d':
            from .sim.squeeze import FRICTION_2D_ONLY
            raise ValueError(f"--squeeze_friction with --resample_potential squeeze_3d: {FRICTION_2D_ONLY}")
        from .sim.squeeze import check_friction
        config["friction"] = check_friction(mu, "--squeeze_friction")
    if cells is not None:
        try:
            t, x = (int(v) for v in str(cells).split(","))
        except ValueError:
            raise ValueError(f"--resample_squeeze_cells {cells!r}: two integers T,X expected") from None
        if t < 1 or x < 2:
            raise ValueError(f"--resample_squeeze_cells {cells!r}: need T >= 1 and X >= 2")
        config.update(theta_cells=t, x_cells=x)
    from .sim.squeeze import steps_from_args
    config.update(steps_from_args(args))
    return config


def with_squeeze(resample: Resample, contours, **squeeze_config) -> Resample:
    """`resample` with the squeeze simulator's potential over the contour bank (O, nv, 2) in metres."""
    return Resample(resample.every, resample.beta, resample.ess_frac, 'squeeze', SqueezePotential(contours, **squeeze_config))


def with_squeeze_3d(resample: Resample, meshes, **squeeze_config) -> Resample:
    """`resample` with the sliced squeeze's potential over the meshes (vertices in metres standing on z = 0, triangles)."""
    return Resample(resample.every, resample.beta, resample.ess_frac, 'squeeze_3d', SqueezePotential3D(meshes, **squeeze_config))


def resample_from_args(args) -> Optional[Resample]:
    """--resample_every / --resample_beta / --resample_ess of the generator's entry point, checked before anything is built."""
    r = from_flags(getattr(args, "resample_every", None), getattr(args, "resample_beta", None), getattr(args, "resample_ess", None),
                   bool(getattr(args, "classifier_guidance", False)), float(getattr(args, "eta", 0.0) or 0.0))
    squeeze_potential_from_args(args)       # --resample_potential / --resample_squeeze_cells: refused here too
    if r is None:
        return None
    if getattr(args, "mode", "test") != "test":
        raise ValueError("--resample_*: resampling belongs to the sampling loops of --mode=test")
    if getattr(args, "edit_from", None) is not None:
        raise ValueError("--resample_* with --edit_from: a finger's bounds belong to its slot; resampled edits are not supported")
    if getattr(args, "global_cond", None) is not None or getattr(args, "cond_target", None) is not None:
        raise ValueError("--resample_* with --global_cond / --cond_target: a finger's condition row belongs to its slot; not supported")
    return r
