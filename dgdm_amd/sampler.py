"""Denoise loops of ``generator/diffusion.py`` (:193-201, :249-256, :570-576, :637-647) on the HIP path.

Independent chains - the (object, objective) pairs ``Diffusion.guided_sample`` walks through one after
the other (:561) - are advanced together as an extra batch axis: one U-Net launch, one guidance
launch sequence and one scheduler launch per denoise step for all of them.  The chains do not
interact, so the results equal the reference's sequential evaluation; what has to be preserved is
the order in which the reference consumes the torch CPU generator for the FPS starts
(dynamics/models/pointnet2_utils.py:83), which ``StartStream`` replays.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, engine
from .edit import Edit
from .engine import Guidance, Unet1d, make_objective
from .goal import PROFILES, Goal, is_goal
from .resample import Resample
from .scheduler import DDIMScheduler

SCALE_2D, SCALE_2D_CONV, SCALE_3D, SCALE_3D_CONV = 0.001, 10.0, 0.5, 0.8      # generator/diffusion.py:30-33


def classifier_scale(mode: str, opt_obj: str, multi: bool = False) -> float:
    """generator/diffusion.py:549-560 (per-object loop) and :631-636 (multi-object loop)."""
    if mode == 'point':
        return SCALE_2D_CONV if (opt_obj == 'convergence' and not multi) else SCALE_2D
    if mode == 'point_3d':
        return SCALE_3D_CONV if (opt_obj == 'convergence' and not multi) else SCALE_3D
    return 0.001


def chain_scale(mode: str, opt_obj: Union[str, Goal], multi: bool = False) -> float:
    """The classifier scale of a chain: ``classifier_scale`` for a reference objective; for a Goal its own ``scale``, else the scale of
    'convergence' - a borrowed default that nobody has tuned for goal objectives (dgdm_amd/goal.py)."""
    if is_goal(opt_obj):
        return float(opt_obj.scale) if opt_obj.scale is not None else classifier_scale(mode, 'convergence', multi)
    return classifier_scale(mode, opt_obj, multi)


def chain_objectives(guid: Guidance, chains: Sequence[Tuple[int, Union[str, Goal]]]):
    """[(object index, objective name or Goal), ...] in launch order -> (the launch's objectives, the row field (n, R, 3) the Goal
    chains read at their own index or None when there is no Goal).  The library indexes the field by the chain's place in the launch,
    so it spans all n chains; the rows of the other chains are zero and never read.  Each DISTINCT Goal is built once on the device
    (guided_multi_object hands the same Goal to every object) and copied to its chains' rows."""
    objectives = [make_objective(None, oi, row_field=True) if is_goal(o) else make_objective(o, oi) for oi, o in chains]
    distinct: List[Goal] = []
    for _, o in chains:
        if is_goal(o) and not any(o is d for d in distinct):
            distinct.append(o)
    if not distinct:
        return objectives, None
    B = guid.cfg.batch
    specs = [_lib.GoalSpec((_lib.C.c_float * 3)(*g.weight), g.ori_window, g.pos_window, PROFILES[g.profile]) for g in distinct]
    built = guid.goal_field(torch.stack([g.triples(B) for g in distinct]), specs)
    field = torch.zeros((len(chains), guid.rows, 3), dtype=torch.float32, device=built.device)
    for c, (_, o) in enumerate(chains):
        if is_goal(o):
            field[c] = built[next(k for k, d in enumerate(distinct) if d is o)]
    return objectives, field


class keeps_row_field:
    """``with keeps_row_field(guid):`` - whatever the body hands the handle through Guidance.set_row_field (the Goal chains' field), on the
    way out, by return or by exception, the handle holds what it held before: a field does not outlive its launch, and a field the caller
    set is not lost (the launches are ordered on the stream, and so is the reuse of the field's memory).  guid may be None."""

    def __init__(self, guid: Optional[Guidance]):
        self.guid = guid

    def __enter__(self):
        self.before = self.guid._row_field if self.guid is not None else None
        return self

    def __exit__(self, *exc):
        if self.guid is not None and self.guid._row_field is not self.before:
            self.guid.set_row_field(self.before)
        return False


def _restores_row_field(fn):
    """The loops below run inside keeps_row_field(guid)."""
    import functools

    @functools.wraps(fn)
    def run(unet, guid, *args, **kw):
        with keeps_row_field(guid):
            return fn(unet, guid, *args, **kw)
    return run


class TorchRng:
    """torch's CPU generator replayed by the library on the generator's own state blob (csrc/torch_rng.hip): the same numbers as
    ``torch.randint`` bit for bit, ~3x faster, callable from worker threads (ctypes releases the GIL) and able to SKIP draws.

    ``generator``: a ``torch.Generator``, or None for torch's global CPU generator - every operation then loads the generator's
    state, advances it and stores it back, so torch and this class can be used on the same generator alternately.
    ``seed``: a detached stream instead - the stream of ``torch.Generator().manual_seed(seed)`` without a torch object."""

    BYTES = 5056

    def __init__(self, generator: Optional[torch.Generator] = None, seed: Optional[int] = None, state: Optional[np.ndarray] = None):
        self._gen, self._detached = generator, seed is not None or state is not None
        self._blob = np.zeros(self.BYTES, dtype=np.uint8) if state is None else np.array(state, dtype=np.uint8, copy=True)
        if seed is not None:
            _lib.check(_lib.lib().dgdm_torch_rng_seed(self._blob.ctypes.data, self.BYTES, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def _load(self):
        if not self._detached:
            st = torch.get_rng_state() if self._gen is None else self._gen.get_state()
            self._blob = st.numpy().copy()

    def _store(self):
        if not self._detached:
            st = torch.from_numpy(self._blob.copy())
            torch.set_rng_state(st) if self._gen is None else self._gen.set_state(st)

    def detached_copy(self) -> "TorchRng":
        """A detached stream that starts where the generator stands now (for drawing ahead on a worker thread)."""
        self._load()
        return TorchRng(state=self._blob)

    def adopt(self, other: "TorchRng") -> None:
        """Puts the generator where the detached stream `other` stands."""
        self._blob = other._blob.copy()
        self._store()

    def randint(self, high: int, n: int, skip: bool = False) -> Optional[np.ndarray]:
        self._load()
        out = None if skip else np.empty(n, dtype=np.int64)
        _lib.check(_lib.lib().dgdm_torch_rng_randint(self._blob.ctypes.data, self.BYTES, int(high), int(n), None if skip else out.ctypes.data))
        self._store()
        return out

    def fps_starts(self, num_points: int, sub_batch_size: int, rows: int, n_calls: int = 1, skip: bool = False,
                   out: Optional[np.ndarray] = None) -> Optional[np.ndarray]:
        """The draws of `n_calls` consecutive classifier calls over `rows` rows -> (n_calls, 2 * rows) int64 in the layout
        dgdm_dyn3d_guidance_grad takes, or None when skipped.  out: an int64 view of that shape to fill (rows contiguous; the
        calls may be strided - e.g. one chain's column of a [step][chain][2 * rows] array)."""
        self._load()
        stride = 0
        if skip:
            out = None
        elif out is None:
            out = np.empty((n_calls, 2 * rows), dtype=np.int64)
        else:
            assert out.dtype == np.int64 and out.shape == (n_calls, 2 * rows) and (n_calls == 0 or out.strides[1] == 8) and out.strides[0] % 8 == 0
            stride = out.strides[0] // 8 if n_calls > 1 else 0
        _lib.check(_lib.lib().dgdm_torch_rng_fps_starts(self._blob.ctypes.data, self.BYTES, int(num_points), max(1, int(sub_batch_size)), int(rows),
                                                       int(n_calls), None if out is None else out.ctypes.data, stride))
        self._store()
        return out


_ACTIVE_PLAN: Optional["StartPlan"] = None


class StartPlan:
    """Draws ahead.  The FPS start draws of a sweep do not depend on anything the GPU computes, only on the ORDER in which the
    reference's loops consume the generator; given that order as a list of jobs ``(rows, n_calls, keep)`` a worker thread makes the
    draws while the GPU runs the chains of earlier jobs.  Used as a context manager around code that draws from the GLOBAL generator
    through ``StartStream``: inside it those streams take their numbers from the plan (jobs must be asked for in plan order; a
    request that does not match cancels the plan and the stream continues synchronously from the right state).  On exit the global
    generator stands where the consumed jobs leave it - exactly as if every draw had been a ``torch.randint``."""

    def __init__(self, num_points: int, sub_batch_size: int, jobs: Sequence[Tuple[int, int, bool]], depth: int = 4):
        import queue
        import threading
        self.N, self.sub, self.jobs = int(num_points), int(sub_batch_size), [(int(r), int(n), bool(k)) for r, n, k in jobs]
        self._q: "queue.Queue" = queue.Queue(maxsize=max(1, depth))
        self._stop = threading.Event()
        self._thread: Optional[threading.Thread] = None
        self._pos = 0
        self._rng_after: Optional[TorchRng] = None      # stream position after the last consumed job
        self.draw_seconds = 0.0

    def _put(self, item) -> None:
        while not self._stop.is_set():
            try:
                self._q.put(item, timeout=0.05)
                return
            except Exception:           # queue.Full
                continue

    def _work(self, rng: TorchRng):
        import time
        try:
            for rows, n, keep in self.jobs:
                if self._stop.is_set():
                    return
                t0 = time.perf_counter()
                arr = rng.fps_starts(self.N, self.sub, rows, n, skip=not keep)
                self.draw_seconds += time.perf_counter() - t0
                self._put((arr, TorchRng(state=rng._blob)))
        except BaseException as e:      # a bad blob / argument raises in the library: tell the consumer instead of leaving it waiting
            self._put(e)

    def __enter__(self):
        import threading
        global _ACTIVE_PLAN
        assert _ACTIVE_PLAN is None, "StartPlan contexts do not nest"
        self._base = TorchRng()                              # the global generator
        self._rng_after = self._base.detached_copy()
        self._thread = threading.Thread(target=self._work, args=(self._base.detached_copy(),), daemon=True)
        self._thread.start()
        _ACTIVE_PLAN = self
        return self

    def _close(self):
        global _ACTIVE_PLAN
        if _ACTIVE_PLAN is self:
            _ACTIVE_PLAN = None
            self._stop.set()
            while self._thread is not None and self._thread.is_alive():
                try:
                    self._q.get_nowait()
                except Exception:
                    pass
                self._thread.join(timeout=0.01)
            self._base.adopt(self._rng_after)

    def __exit__(self, *exc):
        self._close()
        return False

    def take(self, num_points: int, sub: int, rows: int, n_calls: int, keep: bool):
        """The next job's draws if it is the job asked for; otherwise cancels the plan (returns False)."""
        if self._pos < len(self.jobs) and (self.N, self.sub) == (int(num_points), int(sub)) and self.jobs[self._pos] == (int(rows), int(n_calls), bool(keep)):
            item = None
            while item is None:
                try:
                    item = self._q.get(timeout=0.5)
                except Exception:       # queue.Empty: still drawing - or the worker died without a word
                    if self._thread is None or not self._thread.is_alive():
                        try:
                            item = self._q.get_nowait()
                        except Exception:
                            item = RuntimeError("the draw-ahead worker ended without delivering this job")
            if isinstance(item, BaseException):      # fall back on the synchronous draw from the last consumed state
                self._close()
                return False, None
            arr, after = item
            self._pos += 1
            self._rng_after = after
            return True, arr
        self._close()
        return False, None


class StartStream:
    """FPS start indices in the reference's draw order.

    One classifier call on ``rows`` rows with sub-batch size ``sub`` draws, per sub-batch, ``torch.randint(0, N, (n,))``
    for sa1 and ``torch.randint(0, 512, (n,))`` for sa2 from the global CPU generator
    (pointnet2_utils.py:83 reached via generator/diffusion.py:495-498 and :524-526).  The numbers are made by the library's
    replay of that generator (``TorchRng``: identical to ``torch.randint``, tests/test_host_logic.py) on the generator's own state.

    ``generator``: a private ``torch.Generator`` instead of the global one; ``seed``: a detached stream (``pair_stream``);
    ``forced``: recorded draws (golden fixtures)."""

    def __init__(self, num_points: int, sub_batch_size: int, forced: Optional[Sequence[torch.Tensor]] = None,
                 generator: Optional[torch.Generator] = None, seed: Optional[int] = None):
        self.N, self.sub = int(num_points), int(sub_batch_size)
        self._forced = list(forced) if forced is not None else None
        self._rng = None if forced is not None else TorchRng(generator, seed)
        self._plannable = forced is None and generator is None and seed is None

    def _forced_call(self, rows: int) -> np.ndarray:
        out = np.empty(2 * rows, dtype=np.int64)
        for r0 in range(0, rows, self.sub):
            n = min(self.sub, rows - r0)
            for k, off in ((0, 2 * r0), (1, 2 * r0 + n)):
                s = self._forced.pop(0)
                assert s.shape == (n,), (s.shape, n)
                out[off:off + n] = s.numpy()
        return out

    def calls(self, rows: int, n_calls: int, keep: bool = True, out: Optional[np.ndarray] = None) -> Optional[np.ndarray]:
        """The indices `n_calls` consecutive classifier calls over `rows` rows consume -> (n_calls, 2 * rows) int64, each row
        [sub-batch 0: sa1 x n0, sa2 x n0 | sub-batch 1: ...] - the layout dgdm_dyn3d_guidance_grad takes.  keep=False: the draws
        are consumed without being materialised (a rank replaying the stream past chains that belong to other ranks).
        out: where to put them (see TorchRng.fps_starts)."""
        arr = None
        if self._forced is not None:
            arr = np.stack([self._forced_call(rows) for _ in range(n_calls)]) if n_calls else np.empty((0, 2 * rows), np.int64)
            if not keep:
                return None
        elif self._plannable and _ACTIVE_PLAN is not None:
            ok, arr = _ACTIVE_PLAN.take(self.N, self.sub, rows, n_calls, keep)
            if ok and not keep:
                return None
            arr = arr if ok else None
        if arr is None:
            return self._rng.fps_starts(self.N, self.sub, rows, n_calls, skip=not keep, out=out)
        if out is not None:
            out[...] = arr
            return out
        return arr

    def call(self, rows: int) -> np.ndarray:
        """One classifier call: 2*rows indices in draw order."""
        return self.calls(rows, 1)[0]

    def skip(self, rows: int, n_calls: int = 1) -> None:
        self.calls(rows, n_calls, keep=False)


def pair_stream(num_points: int, sub_batch_size: int, seed: int, pair_index: int) -> StartStream:
    """A start stream of its own for pair `pair_index` (seed-derived), for workloads that have no reference draw order to keep
    (bench.py's synthetic pair batches): the draws of a pair depend on (seed, pair index) only, not on the rank that runs it or on
    how many ranks there are.  The stream of ``torch.Generator().manual_seed(...)`` with that seed."""
    return StartStream(num_points, sub_batch_size, seed=(int(seed) * 1_000_003 + int(pair_index)) & 0x7FFFFFFFFFFFFFFF)


def edit_start(edit: Optional[Edit], sched: DDIMScheduler, noise: torch.Tensor):
    """(start sample, the timesteps the loop runs, the bounds of its steps or None): the noise and the whole schedule, or what the edit
    makes of them - its designs noised to the first of the schedule's last K timesteps, those K timesteps, its (lo, hi) on the device."""
    if edit is None:
        return noise, sched.timesteps, None
    x, ts = edit.start(sched, noise)
    return x, ts, edit.bounds_on(noise.device)


def step_noise_keys(n_chains: int, shared_step_noise: bool = False, chain_keys: Optional[Sequence[int]] = None) -> List[int]:
    """The noise keys of a launch's chains: `chain_keys` when given (a slice of a larger run: the chains' global indices), else their
    indices; shared_step_noise: key 0 for every chain (common random numbers)."""
    keys = list(range(n_chains)) if chain_keys is None else [int(k) for k in chain_keys]
    if len(keys) != n_chains:
        raise ValueError(f"{len(keys)} chain keys for {n_chains} chains")
    return [0] * n_chains if shared_step_noise else keys


def check_resample(resample: Optional[Resample], eta: float, guid: Optional[Guidance], n_grad: int, scales: Optional[Sequence[float]] = None,
                   bounds=None, edit=None, global_cond=None, grad_fn=None, objectives=None, n_objects: Optional[int] = None) -> None:
    """What a run with `resample` refuses, by ValueError and before any launch: eta == 0 (copies would never part), bounds / an edit
    (a finger's bounds belong to its slot, not to the design that is copied into it), global_cond (likewise its condition row),
    n_grad == 0 or no guidance handle (nothing to weigh by), per-chain scales with n_grad != 1; with the model's potential a bf16 handle
    (score has no bf16 form); with a squeeze potential (which needs no forward-only trunk, so bf16 handles pass) a goal objective among
    `objectives` (names, Goals or the launch's objectives; goal fields have no squeeze form) and a bank of contours / meshes whose
    object count differs from the handle's (`n_objects`: the count to compare with, for a caller whose `guid` is a GuidanceSpec and
    holds no objects); 'squeeze' on a 3-D handle (it is 2-D only: 'squeeze_3d' is the sliced form) and 'squeeze_3d' on a 2-D one."""
    if resample is None:
        return
    if not isinstance(resample, Resample):
        raise ValueError(f"resample: a dgdm_amd.resample.Resample expected, got {type(resample).__name__}")
    if not float(eta) > 0.0:
        raise ValueError("resample: eta == 0 - copies of a finger would never part again; give eta > 0")
    if bounds is not None or edit is not None:
        raise ValueError("resample: bounds / an edit belong to a finger's slot; resampled edits are not supported")
    if global_cond is not None:
        raise ValueError("resample: global_cond rows belong to a finger's slot; resampled conditional rows are not supported")
    if n_grad == 0 or guid is None or grad_fn is not None:
        raise ValueError("resample: needs the guidance handle and its objectives (n_grad >= 1, no grad_fn): there is nothing else to weigh fingers by")
    if resample.potential in ('squeeze', 'squeeze_3d'):
        if resample.potential == 'squeeze' and guid.dyn.kind == 3:
            raise ValueError("resample: the squeeze potential is 2-D only; 3-D fingers have potential='squeeze_3d' (the sliced squeeze)")
        if resample.potential == 'squeeze_3d' and guid.dyn.kind != 3:
            raise ValueError("resample: the squeeze_3d potential is the sliced squeeze of 3-D fingers; 2-D fingers have potential='squeeze'")
        if any(is_goal(o) or getattr(o, "use_rowcoef", 0) == _lib.OBJ_ROWFIELD for o in (objectives or ())):
            raise ValueError("resample: goal objectives have no squeeze form (the squeeze potential reads no row field)")
        have = guid.n_objects if n_objects is None else int(n_objects)
        if resample.squeeze.n_objects != have:
            what = "contours" if resample.potential == 'squeeze' else "meshes"
            raise ValueError(f"resample: the squeeze potential's bank holds {resample.squeeze.n_objects} {what}, the guidance handle "
                             f"{have} objects")
    elif getattr(guid, "contraction_dtype", "f32") == "bf16":
        raise ValueError("resample: the bf16 trunk has no forward-only form (Guidance.score refuses it)")
    if scales is not None and len(set(scales)) > 1 and n_grad != 1:
        raise ValueError(f"resample: per-chain classifier scales ({sorted(set(scales))}) need n_grad == 1, not {n_grad}")


def run_chains(unet: Unet1d, guid: Optional[Guidance], sched: DDIMScheduler, x0: torch.Tensor, n_chains: int, n_grad: int, objectives,
               rowcoef: Optional[torch.Tensor], starts: Optional[np.ndarray], timesteps, scales: Sequence[float],
               global_cond: Optional[torch.Tensor] = None, cfg_weight: float = 1.0, bounds=None, trace: Optional[list] = None,
               on_step=None, grad_fn=None, stepwise: bool = False, eta: float = 0.0, noise_seed: int = 0,
               chain_keys: Optional[Sequence[int]] = None, resample: Optional[Resample] = None, resample_log: Optional[list] = None,
               resample_starts: Optional[np.ndarray] = None) -> torch.Tensor:
    """THE denoise loop, S x [eps-net with the classifier-free mix ; guidance gradient ; DDIM step], of every sampler here and in
    dgdm_amd/dist.py: x0 (B, L) -> (n_chains, B, L).  All n_chains chains start from x0; chain k is guided by the mean of n_grad
    gradients, gradient j of chain k being gradient chain j * n_chains + k of `objectives` (object-major, as dgdm_guided_chains_run
    takes them); n_grad == 0: no guidance.  rowcoef, starts ([step][...], 3-D), scales (one per chain), global_cond ((B, gc) shared or
    (n_chains, B, gc)), cfg_weight, bounds: as engine.guided_chains_run takes them.

    The loop is ONE library call (engine.guided_chains_run) unless something asks to see its steps; then it is walked here, with the
    same bits (tests/test_gpu_parity.py):
      trace: a list that receives (eps, grad, x) per step, each (n_chains, B, L), x being the step's INPUT;
      on_step(si, x, eps): called after each step with its output x;
      grad_fn(si, t, x) -> (n_grad * n_chains, B, L): the step's gradients instead of guid.grad on n_grad copies of x with step si's starts;
      stepwise=True: nothing of these, but walk it all the same.

    eta > 0: stochastic DDIM steps (DDIMScheduler.eta_coefficients).  Step si of chain k adds sigma times the keyed device
    normal of (noise_seed, chain_keys[k], si) - a pure function of those and the element, so the library call, the walk, a run split over
    ranks and a run split into several calls give the same bits as long as a chain keeps its key.  chain_keys None: range(n_chains).
    eta == 0 is the loop of old, launch for launch.

    resample (dgdm_amd/resample.py): a Resample forces the walk.  After the DDIM step of walk step si with
    (si + 1) % every == 0 and si < S - 1 - never after the last step, whose duplicates no noise could part - the step's output is scored
    forward-only at timesteps[si + 1] on n_grad copies, as grad is called; the objectives' values per finger weigh the B fingers of every
    chain, and engine.chain_resample (step_index si, the run's noise_seed and chain keys) copies fingers over fingers where the weights
    have degenerated.  Its output is the x the walk continues with (on_step sees it).  The log weights and last potentials live for the
    run and start at zero.  resample_log: a list that receives (si, ess (n_chains,), did (n_chains,), ancestors (n_chains, B)) per
    evaluation, device tensors.  resample_starts (3-D): the evaluations' FPS draws, [evaluation][n_grad * n_chains][starts_per_call], taken
    from the start stream AFTER all of the run's guidance draws (draw_chain_starts / draw_ensemble_starts, n_potential) - the guidance
    draws are those of the run without resampling.  check_resample lists what is refused, before any launch.
    resample.potential == 'squeeze' (2-D) or 'squeeze_3d' (3-D): the values come from the squeeze simulator instead - one eps-net call on
    the step's output at timesteps[si + 1], x0 = engine.ddim_pred_x0 of it, resample.squeeze.values over the same G P^2 cells in the same
    units; no guid.score call, no FPS draws (resample_starts is not read: Resample.fps_evaluations is 0); everything after the values is
    the same engine.chain_resample call."""
    B, L = x0.shape
    nc = n_chains
    eta = float(eta)
    if eta < 0.0:
        raise ValueError(f"run_chains: eta {eta} is negative")
    if resample is not None:
        check_resample(resample, eta, guid, n_grad, scales, bounds=bounds, global_cond=global_cond, grad_fn=grad_fn, objectives=objectives)
        n_eval = resample.fps_evaluations(len(timesteps))
        if guid.dyn.kind == 3 and n_eval:
            if resample_starts is None or resample_starts.dtype != np.int64 or resample_starts.size != n_eval * n_grad * nc * guid.starts_per_call:
                raise ValueError(f"run_chains: 3-D resampling needs resample_starts, {n_eval} x {n_grad * nc} x {guid.starts_per_call} int64 draws")
            resample_starts = np.ascontiguousarray(resample_starts).reshape(n_eval, -1)
        stepwise = True
    keys = list(range(nc)) if chain_keys is None else [int(k) for k in chain_keys]
    if len(keys) != nc:
        raise ValueError(f"run_chains: {len(keys)} chain keys for {nc} chains")
    eta_coef = [sched.eta_coefficients(int(t), eta) for t in timesteps] if eta != 0.0 else None
    if not stepwise and trace is None and on_step is None and grad_fn is None:
        return engine.guided_chains_run(unet, guid, x0, nc, n_grad, objectives, rowcoef, starts, [int(t) for t in timesteps],
                                        [sched.coefficients(int(t)) for t in timesteps], scales, global_cond, cfg_weight, bounds,
                                        eta_coef, noise_seed, keys if eta_coef is not None else None)
    # one scheduler launch over all chains, or - chains with scales of their own - one per chain, which has no averaged form
    steps = [(slice(None), scales[0])] if len(set(scales)) == 1 else list(enumerate(scales))
    if len(steps) > 1 and n_grad != 1:
        raise ValueError(f"run_chains: per-chain classifier scales ({sorted(set(scales))}) need n_grad == 1, not {n_grad}")
    cond, stride = engine.chain_cond_layout(global_cond, unet.global_cond_dim, nc, B)        # stride 0: one (B, gc) block for all chains, or none
    if cond is not None:
        cond = (cond.reshape(1, B, -1).expand(nc, -1, -1) if stride == 0 else cond).reshape(nc * B, -1)
    x = x0.reshape(1, B, L).expand(nc, -1, -1).contiguous().to(torch.float32)
    if resample is not None:
        logw, vprev = (torch.zeros((nc, B), dtype=torch.float64, device=x.device) for _ in range(2))
        beta_per_cell = resample.beta / float(guid.rows // B)          # a finger has G P^2 cells
        n_seen = 0
    for si, t in enumerate(timesteps):
        t = int(t)
        # every chain starts from the same sample (generator/diffusion.py:570: `sample = noise.clone()` per object), so the first eps-net
        # call has nc identical copies of the B fingers as its batch: evaluate it once (same input, same kernel, same bits) - unless
        # every chain has condition rows of its own
        n = 1 if si == 0 and stride == 0 else nc
        ts = torch.full((n * B,), t, dtype=torch.int32, device=x.device)
        eps = unet.forward_cfg(x[:n].reshape(n * B, L, 1), ts, None if cond is None else cond[:n * B], cfg_weight)
        eps = eps.reshape(n, B, L).expand(nc, -1, -1).contiguous()
        g = None
        if grad_fn is not None:
            g = grad_fn(si, t, x)
        elif n_grad:
            g = guid.grad(x.repeat(n_grad, 1, 1), t, objectives, rowcoef, None if starts is None else starts[si].reshape(-1))
        if trace is not None:
            trace.append((eps.clone(), None if g is None else g.clone(), x.clone()))
        coef = sched.coefficients(t)
        # eta > 0: the launch over all chains takes all keys, a chain's own launch its own key
        noisy = lambda c: {} if eta_coef is None else dict(eta_coef=eta_coef[si], seed=noise_seed, step_index=si,      # noqa: E731
                                                           chain_keys=keys if isinstance(c, slice) else [keys[c]])
        out = [engine.ddim_guided_step(x[c], eps[c], None if g is None else g[c], n_grad, coef, sc, bounds, **noisy(c)) for c, sc in steps]
        x = out[0] if len(out) == 1 else torch.stack(out)
        if resample is not None and resample.evaluates(si, len(timesteps)) and resample.potential in ('squeeze', 'squeeze_3d'):
            # the squeeze model's opinion of the predicted clean design: one eps-net call on the step's output at the next timestep (as the
            # loop calls it; cond is None here), the step's own x0 expression, one squeeze map over cond_fn's grid cells, one values launch
            tn = int(timesteps[si + 1])
            eps_n = unet.forward_cfg(x.reshape(nc * B, L, 1), torch.full((nc * B,), tn, dtype=torch.int32, device=x.device), None, cfg_weight)
            clean = engine.ddim_pred_x0(x, eps_n.reshape(nc, B, L).contiguous(), sched.coefficients(tn)[:2])
            values = resample.squeeze.values(clean, objectives, rowcoef, n_grad, guid.cfg.grid_size, guid.cfg.num_pos,
                                             (guid.cfg.ori_lo, guid.cfg.ori_hi))
            x, anc, ess, did = engine.chain_resample(x, values, n_grad, beta_per_cell, resample.ess_frac, noise_seed, keys, si, logw, vprev)
            n_seen += 1
            if resample_log is not None:
                resample_log.append((si, ess, did, anc))
        elif resample is not None and resample.evaluates(si, len(timesteps)):
            # the forward-only trunk on the step's output; only the logits are used (the tally's thresholds are placeholders)
            st = None if guid.dyn.kind != 3 else resample_starts[n_seen]
            logits = guid.score(x.repeat(n_grad, 1, 1), [int(o.object) for o in objectives], (1.0, 1.0, 1.0), int(timesteps[si + 1]), st,
                                want_logits=True)[2]
            values = guid.objective_values(logits, objectives, rowcoef)
            x, anc, ess, did = engine.chain_resample(x, values, n_grad, beta_per_cell, resample.ess_frac, noise_seed, keys, si, logw, vprev)
            n_seen += 1
            if resample_log is not None:
                resample_log.append((si, ess, did, anc))
        if on_step is not None:
            on_step(si, x, eps)
    return x


def unguided_sample(unet: Unet1d, sched: DDIMScheduler, x: torch.Tensor, on_step=None, global_cond: Optional[torch.Tensor] = None,
                    cfg_weight: float = 1.0, edit: Optional[Edit] = None, eta: float = 0.0, noise_seed: int = 0,
                    shared_step_noise: bool = False) -> torch.Tensor:
    """S x [eps-net ; DDIM step]  (generator/diffusion.py:193-201, :249-256).  on_step(i, x_i, eps_i): the harness's per-step hook
    (plots, noise-prediction loss); it forces a device->host copy per step, as the reference's own plotting does.
    global_cond (B, gc), cfg_weight: the condition rows of a conditional eps-net and the classifier-free guidance weight (the mix is
    the library's: Unet1d.forward_cfg).  edit: x is then the noise the edit's designs are noised with, and the loop runs the edit's K
    bounded steps (dgdm_amd/edit.py).  eta, noise_seed: stochastic steps as in run_chains; the one chain has key 0 (so
    shared_step_noise changes nothing here)."""
    B = x.shape[0]
    engine.check_global_cond(global_cond, unet.global_cond_dim, B)
    x, timesteps, bounds = edit_start(edit, sched, x)
    hook = None if on_step is None else lambda i, xi, eps: on_step(i, xi.reshape(x.shape), eps.reshape(x.shape))
    out = run_chains(unet, None, sched, x.reshape(B, -1), 1, 0, [], None, None, timesteps, [0.0], global_cond, cfg_weight, bounds,
                     on_step=hook, stepwise=True, eta=eta, noise_seed=noise_seed, chain_keys=[0])
    return out.reshape(x.shape)


def convergence_centers(guid: Guidance, mode: str, unguided: torch.Tensor, objects_of_chain: Sequence[int],
                        starts: Optional[np.ndarray] = None) -> torch.Tensor:
    """``Diffusion.get_convergence_centers`` (:506-539) for several objects at once -> (n_chains, B) int64."""
    from .dynamics import metrics
    nc, B = len(objects_of_chain), unguided.shape[0]
    x = unguided.reshape(1, B, -1).expand(nc, -1, -1).contiguous()
    logits = guid.sweep(x, objects_of_chain, starts).cpu()                       # (nc, B*G, 3), row = g*B + b
    if mode == 'point_3d':
        thr = torch.tensor(0.02) / torch.tensor(0.0312)                          # threshold/std (:116-118)
    else:
        thr = torch.tensor(0.03) / torch.tensor(0.0565)
    G = guid.cfg.grid_size
    out = torch.zeros((nc, B), dtype=torch.int64)
    for c in range(nc):
        d0 = logits[c, :, 0]
        prof = torch.where(d0 > thr, 2.0, torch.where(d0 < -thr, 0.0, 1.0))      # :532
        for i in range(B):
            lengths, centers = metrics.convergence_mode_three_class(prof[torch.arange(i, B * G, B)])
            out[c, i] = centers[torch.argmax(lengths)]
    return out


def draw_chain_starts(guid: Guidance, chains: Sequence[Tuple[int, Union[str, Goal]]], n_steps: int, starts: Optional[StartStream] = None,
                      keep: Optional[range] = None, streams: Optional[Sequence[StartStream]] = None, out: Optional[np.ndarray] = None,
                      pool=None, n_potential: int = 0):
    """FPS starts of a batch of 3-D chains in the order the reference's sequential loops consume the generator:
    chain after chain (generator/diffusion.py:561); inside a chain the centre sweep (:563) and then every step's cond_fn (:574).
    A Goal chain draws no sweep, like every objective other than 'convergence'.

    keep: only the chains of this index range are returned (sweep list / step array of len(keep) chains); the draws of the
    others are consumed and dropped, so that a rank holding a block of the chains sees exactly the numbers a single process
    would have handed those chains (dgdm_amd/dist.py).  streams: one StartStream per chain instead of the shared one (then
    nothing has to be skipped: chains outside `keep` are not touched).

    n_potential > 0 (a run with a Resample: its number of evaluations): a third result, (n_potential, len(keep), starts_per_call) - the
    evaluations' draws, taken AFTER all chains' guidance draws, chain after chain (with `streams`, from each chain's own stream behind its
    guidance draws); the first two results are those of n_potential == 0."""
    nc = len(chains)
    keep = range(nc) if keep is None else keep
    if streams is None:
        starts = starts or StartStream(guid.cfg.num_object_points, guid.cfg.sub_batch_size)
    sweep: List[Optional[np.ndarray]] = [None] * len(keep)
    step = out if out is not None else np.empty((n_steps, len(keep), guid.starts_per_call), dtype=np.int64)
    assert step.shape == (n_steps, len(keep), guid.starts_per_call) and step.dtype == np.int64 and step.flags.c_contiguous
    def one(c, o, st, mine):
        k = c - keep.start
        if not is_goal(o) and o == 'convergence':
            sw = st.calls(guid.sweep_rows, 1, keep=mine)
            if mine:
                sweep[k] = sw[0]
        st.calls(guid.rows, n_steps, keep=mine, out=step[:, k] if mine else None)

    if streams is not None:
        # independent streams: the chains' draws can be made side by side (`pool`: a concurrent.futures executor; the library call
        # releases the interpreter lock)
        jobs = [(c, o, streams[c], True) for c, (_, o) in enumerate(chains) if c in keep]
        if pool is not None and len(jobs) > 1:
            list(pool.map(lambda j: one(*j), jobs))
        else:
            for j in jobs:
                one(*j)
    else:
        for c, (_, o) in enumerate(chains):
            one(c, o, starts, c in keep)
    if n_potential > 0:
        pot = np.empty((n_potential, len(keep), guid.starts_per_call), dtype=np.int64)
        for c in range(nc):
            mine = c in keep
            if streams is None or mine:
                (starts if streams is None else streams[c]).calls(guid.rows, n_potential, keep=mine, out=pot[:, c - keep.start] if mine else None)
        return sweep, step, pot
    return sweep, step


@_restores_row_field
def guided_chains(unet: Unet1d, guid: Guidance, sched: DDIMScheduler, mode: str, noise: torch.Tensor,
                  chains: Sequence[Tuple[int, Union[str, Goal]]], unguided: Optional[torch.Tensor] = None,
                  starts: Optional[StartStream] = None, trace: Optional[list] = None, predrawn=None,
                  global_cond: Optional[torch.Tensor] = None, cfg_weight: float = 1.0, edit: Optional[Edit] = None, eta: float = 0.0,
                  noise_seed: int = 0, shared_step_noise: bool = False, chain_keys: Optional[Sequence[int]] = None,
                  resample: Optional[Resample] = None, resample_log: Optional[list] = None) -> torch.Tensor:
    """``Diffusion.guided_sample`` loop bodies (:561-576) for the chains [(object index, opt_obj), ...]; opt_obj: a reference
    objective name or a ``Goal`` (dgdm_amd/goal.py), whose chain is guided by the goal's row field.

    noise (B, L, 1) is shared by all chains (:570).  global_cond: (B, gc) shared by all chains or (n_chains, B, gc); cfg_weight: the
    classifier-free guidance weight of a conditional eps-net.  Returns (n_chains, B, L, 1).

    edit (dgdm_amd/edit.py): every chain then starts from the edit's designs noised with `noise`, runs the schedule's last K steps (the
    3-D start draws are made for K steps) and clips every step's predicted clean sample to the edit's bounds.  The centres of a
    'convergence' chain of an edit come from the SOURCE DESIGNS, not from an unguided sample: `unguided` is not read.

    eta > 0 (run_chains): chain k's steps draw the noise keyed (noise_seed, chain_keys[k]); chain_keys None: the chain's index in
    `chains` (dist.guided_chains_sharded passes the GLOBAL indices of its slice).  A pair may appear several times in `chains`: at
    eta = 0 its replicas are identical, at eta > 0 they diverge through their keys - that is how one asks for several candidate designs
    per task; with an edit, for several edits of one design (the bounded clip is inside the same step).  shared_step_noise=True gives
    every chain key 0: common random numbers, for comparing objectives on equal noise (replicas are then identical again).

    resample, resample_log: run_chains' (every chain resamples among its own B fingers).  3-D: the evaluations' draws follow all
    guidance draws on the start stream; `predrawn` then is draw_chain_starts' triple (n_potential = resample.fps_evaluations(S))."""
    nc, (B, L, _) = len(chains), noise.shape
    check_resample(resample, eta, guid, 1, edit=edit, global_cond=global_cond, objectives=[o for _, o in chains])
    engine.chain_cond_layout(global_cond, unet.global_cond_dim, nc, B)       # a condition of the wrong shape is refused before anything runs
    dev = noise.device
    is3d = mode == 'point_3d'
    noise, timesteps, bounds = edit_start(edit, sched, noise)
    if edit is not None:
        unguided = edit.designs_on(dev)
    S = len(timesteps)
    objectives, field = chain_objectives(guid, chains)
    if field is not None:
        guid.set_row_field(field)
    # --- replay of the reference's RNG consumption: chain after chain; inside a chain the centre sweep, then the steps
    sweep_starts: List[Optional[np.ndarray]] = [None] * nc
    step_starts = pot_starts = None
    if is3d:
        n_pot = 0 if resample is None else resample.fps_evaluations(S)
        if predrawn is None:
            predrawn = draw_chain_starts(guid, chains, S, starts, n_potential=n_pot)
        if n_pot and len(predrawn) != 3:
            raise ValueError("guided_chains: resampling 3-D chains needs the evaluations' draws as well (draw_chain_starts n_potential)")
        sweep_starts, step_starts = predrawn[0], predrawn[1]
        pot_starts = predrawn[2] if n_pot else None
    # --- 'convergence' chains: centres from the unguided sample, then row coefficients
    rowcoef = None
    conv = [c for c, (_, o) in enumerate(chains) if not is_goal(o) and o == 'convergence']
    if conv:
        assert unguided is not None, "opt_obj='convergence' needs the unguided sample (generator/diffusion.py:563)"
        st = np.concatenate([sweep_starts[c] for c in conv]) if is3d else None
        centers = convergence_centers(guid, mode, unguided, [chains[c][0] for c in conv], st)
        rc = np.zeros((nc, guid.rows), dtype=np.float32)
        for k, c in enumerate(conv):
            rc[c] = guid.rowcoef(centers[k])
        rowcoef = torch.from_numpy(rc).to(dev)
    out = run_chains(unet, guid, sched, noise.reshape(B, L), nc, 1, objectives, rowcoef, step_starts, timesteps,
                     [chain_scale(mode, o) for _, o in chains], global_cond, cfg_weight, bounds, trace=trace, eta=eta, noise_seed=noise_seed,
                     chain_keys=step_noise_keys(nc, shared_step_noise, chain_keys), resample=resample, resample_log=resample_log,
                     resample_starts=pot_starts)
    return out.reshape(nc, B, L, 1)


@_restores_row_field
def guided_multi_object(unet: Unet1d, guid: Guidance, sched: DDIMScheduler, mode: str, noise: torch.Tensor,
                        object_indices: Sequence[int], opt_obj: Union[str, Goal], starts: Optional[StartStream] = None,
                        on_step=None, global_cond: Optional[torch.Tensor] = None, cfg_weight: float = 1.0,
                        edit: Optional[Edit] = None, eta: float = 0.0, noise_seed: int = 0, shared_step_noise: bool = False,
                        resample: Optional[Resample] = None, resample_log: Optional[list] = None) -> torch.Tensor:
    """``Diffusion.guided_sample_multi_object`` loop (:637-647): one chain, gradient = mean over the objects.  opt_obj: a reference
    objective name or a ``Goal``.  global_cond (B, gc), cfg_weight, edit: as in guided_chains.  eta, noise_seed: stochastic steps as
    in run_chains; the one chain has key 0 (dist.guided_multi_object_sharded steps it with the same key on every rank).
    resample, resample_log: run_chains' - the fingers are weighed by the mean of the objects' values; 3-D: the evaluations' draws
    (object after object) follow the loop's guidance draws on the start stream."""
    n_obj, (B, L, _) = len(object_indices), noise.shape
    check_resample(resample, eta, guid, n_obj, edit=edit, global_cond=global_cond, objectives=[opt_obj])
    engine.check_global_cond(global_cond, unet.global_cond_dim, B)
    is3d = mode == 'point_3d'
    objectives, field = chain_objectives(guid, [(oi, opt_obj) for oi in object_indices])
    if field is not None:
        guid.set_row_field(field)
    if not is_goal(opt_obj) and opt_obj == 'convergence':
        raise ValueError("the reference never runs the multi-object loop with 'convergence' (generator/diffusion.py:337)")
    if is3d:
        starts = starts or StartStream(guid.cfg.num_object_points, guid.cfg.sub_batch_size)
    noise, timesteps, bounds = edit_start(edit, sched, noise)
    # per step the reference draws object after object (:641-643): one run of draws for the whole loop
    st = starts.calls(guid.rows, len(timesteps) * n_obj).reshape(len(timesteps), -1) if is3d else None
    n_pot = 0 if resample is None else resample.fps_evaluations(len(timesteps))
    pot = starts.calls(guid.rows, n_pot * n_obj).reshape(n_pot, -1) if is3d and n_pot else None
    hook = None if on_step is None else lambda i, x, eps: on_step(i, x.reshape(B, L, 1))      # the harness's per-step plots (:648-674)
    out = run_chains(unet, guid, sched, noise.reshape(B, L), 1, n_obj, objectives, None, st, timesteps, [chain_scale(mode, opt_obj, multi=True)],
                     global_cond, cfg_weight, bounds, on_step=hook, eta=eta, noise_seed=noise_seed, chain_keys=[0], resample=resample,
                     resample_log=resample_log, resample_starts=pot)
    return out.reshape(B, L, 1)


def draw_ensemble_starts(guid: Guidance, n_groups: int, n_obj: int, n_steps: int, streams: Optional[Sequence[StartStream]] = None,
                         out: Optional[np.ndarray] = None, pool=None, n_potential: int = 0):
    """FPS starts of ``n_groups`` independent multi-object chains: every group has its own generator stream and consumes it as
    ``guided_sample_multi_object`` does - step after step, inside a step object after object (generator/diffusion.py:641-643).
    Returned as (n_steps, n_obj, n_groups, starts_per_call): the launch order of ``guided_multi_object_groups``.
    n_potential > 0 (a run with a Resample): every group's stream then goes on with n_potential evaluations' draws, object after object,
    AFTER all its guidance draws, and the result is the pair (steps, (n_potential, n_obj, n_groups, starts_per_call))."""
    streams = streams or [StartStream(guid.cfg.num_object_points, guid.cfg.sub_batch_size) for _ in range(n_groups)]
    out = out if out is not None else np.empty((n_steps, n_obj, n_groups, guid.starts_per_call), dtype=np.int64)
    assert out.shape == (n_steps, n_obj, n_groups, guid.starts_per_call) and out.dtype == np.int64 and out.flags.c_contiguous

    pot = np.empty((n_potential, n_obj, n_groups, guid.starts_per_call), dtype=np.int64) if n_potential > 0 else None

    def one(k):
        for si in range(n_steps):               # a group's stream is consumed step after step, object after object
            streams[k].calls(guid.rows, n_obj, out=out[si, :, k])
        for e in range(n_potential):
            streams[k].calls(guid.rows, n_obj, out=pot[e, :, k])

    if pool is not None and n_groups > 1:
        list(pool.map(one, range(n_groups)))
    else:
        for k in range(n_groups):
            one(k)
    return out if pot is None else (out, pot)


@_restores_row_field
def guided_multi_object_groups(unet: Unet1d, guid: Guidance, sched: DDIMScheduler, mode: str, noise: torch.Tensor,
                               groups: Sequence[Sequence[int]], opt_objs: Sequence[Union[str, Goal]], streams: Optional[Sequence[StartStream]] = None,
                               predrawn: Optional[np.ndarray] = None, python_loop: bool = False, global_cond: Optional[torch.Tensor] = None,
                               cfg_weight: float = 1.0, edit: Optional[Edit] = None, eta: float = 0.0, noise_seed: int = 0,
                               shared_step_noise: bool = False, chain_keys: Optional[Sequence[int]] = None,
                               resample: Optional[Resample] = None, resample_log: Optional[list] = None) -> torch.Tensor:
    """Several independent ``guided_sample_multi_object`` chains (:637-647) in the same launches: chain k averages the guidance
    gradients of the objects ``groups[k]`` for objective ``opt_objs[k]`` (a guidance ensemble: n_obj dynamics-gradient
    evaluations per denoise step).  All groups have the same size.  Launch order of the gradient chains is object-major,
    (j, k) -> j * K + k, so the mean over j is one strided reduction for every group at once.  Returns (K, B, L, 1).
    edit: as in guided_chains - every group edits the same designs, and `predrawn` then holds the draws of the edit's steps.
    eta, noise_seed, shared_step_noise, chain_keys: as in guided_chains, group k being chain k.
    resample, resample_log: run_chains' (the walk, whatever python_loop says); 3-D: `predrawn` then is draw_ensemble_starts' pair."""
    K, n_obj, (B, L, _) = len(groups), len(groups[0]), noise.shape
    check_resample(resample, eta, guid, n_obj, edit=edit, global_cond=global_cond, objectives=opt_objs)
    assert all(len(g) == n_obj for g in groups) and len(opt_objs) == K
    engine.chain_cond_layout(global_cond, unet.global_cond_dim, K, B)       # global_cond: (B, gc) for all groups or (K, B, gc)
    if any(not is_goal(o) and o == 'convergence' for o in opt_objs):
        raise ValueError("the reference never runs the multi-object loop with 'convergence' (generator/diffusion.py:337)")
    is3d = mode == 'point_3d'
    noise, timesteps, bounds = edit_start(edit, sched, noise)
    # (a Goal group reads the row field at its gradient chains' own indices j * K + k)
    objectives, field = chain_objectives(guid, [(groups[k][j], opt_objs[k]) for j in range(n_obj) for k in range(K)])
    if field is not None:
        guid.set_row_field(field)
    n_pot = 0 if resample is None else resample.fps_evaluations(len(timesteps))
    if is3d and predrawn is None:
        predrawn = draw_ensemble_starts(guid, K, n_obj, len(timesteps), streams, n_potential=n_pot)
    pot = None
    if is3d and n_pot:
        if not isinstance(predrawn, tuple) or len(predrawn) != 2:
            raise ValueError("guided_multi_object_groups: resampling 3-D groups needs the evaluations' draws as well (draw_ensemble_starts n_potential)")
        predrawn, pot = predrawn
    scales = {chain_scale(mode, o, multi=True) for o in opt_objs}
    if len(scales) != 1:      # (dgdm_guided_chains_run refuses per-chain scales with averaged gradients; names share one scale, Goals may not)
        raise ValueError(f"guided_multi_object_groups: the groups' classifier scales differ ({sorted(scales)}); give the Goals one scale")
    # K chains x n_obj gradients each, gradient chains object-major
    out = run_chains(unet, guid, sched, noise.reshape(B, L), K, n_obj, objectives, None, predrawn if is3d else None, timesteps, [scales.pop()] * K,
                     global_cond, cfg_weight, bounds, stepwise=python_loop, eta=eta, noise_seed=noise_seed,
                     chain_keys=step_noise_keys(K, shared_step_noise, chain_keys), resample=resample, resample_log=resample_log, resample_starts=pot)
    return out.reshape(K, B, L, 1)
