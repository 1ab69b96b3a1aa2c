"""Host-side helpers of the 'convergence' objective (reference: dynamics/metrics.py:4-38).

These run on B-length / G-length integer profiles on the host, exactly where the reference runs them
(generator/diffusion.py:532-538 builds the profile with a Python loop on the CPU).  ``metric2objective`` and
``convergence_range_from_finals`` score the simulator's roll-outs for the validation harness (host side, further down).
"""
from __future__ import annotations

import numpy as np
import torch


def slicer(a, lower, upper):
    """Wrap-around window a[lower:upper] with Python slice clamping (metrics.py:32-38)."""
    lower, upper, n = int(lower), int(upper), len(a)
    if lower < 0:
        pieces = (a[lower:], a[:upper])
    elif upper > n:
        pieces = (a[lower:], a[:upper - n])
    else:
        return a[lower:upper]
    return torch.cat(pieces) if isinstance(a, torch.Tensor) else np.concatenate(pieces)


def convergence_mode(profile: torch.Tensor):
    """Runs of ones followed by runs of zeros on the circular binary profile (metrics.py:4-21).

    Returns (lengths, points): for every 1->0 transition inside the first period, its index (the last 1)
    and the distance between the surrounding 0->1 transitions measured on the twice-unrolled profile."""
    dev = profile.device
    bits = (profile.detach().cpu().numpy() > 0).astype(np.int64)
    n = bits.size
    ones = int(bits.sum())
    if ones == 0:
        return torch.tensor([n], device=dev), torch.tensor([0], device=dev)
    if ones == n:
        return torch.tensor([n], device=dev), torch.tensor([n - 1], device=dev)
    step = np.diff(np.concatenate([bits, bits]))
    falls = np.nonzero(step < 0)[0]
    falls = falls[falls < n]
    rises = np.nonzero(step > 0)[0]
    marks = np.concatenate([[0], rises[rises > falls[0]], [2 * n]])
    lengths = np.diff(marks)[:falls.size]
    return torch.from_numpy(lengths).to(dev), torch.from_numpy(falls).to(dev)


def convergence_mode_three_class(profile: torch.Tensor):
    """Classes {0: clockwise, 1: static, 2: counter-clockwise}; static cells are dropped first (metrics.py:23-30)."""
    keep = torch.nonzero(profile != 1).reshape(-1)
    if keep.numel() == 0:
        z = torch.tensor([0], device=profile.device)
        return z, z.clone()
    lengths, points = convergence_mode(profile[keep])
    return lengths, keep[points]


# --------------------------------------------------------------------------- harness scoring
# What follows scores SIMULATOR roll-outs on the host (reference: dynamics/metrics.py:40-234, used by
# generator/diffusion.py:304-311).  It is not on the GPU path; it is here so that the reference's validation harness finds the
# names it imports.  Table-driven restatement; tests/test_harness_golden.py replays golden values produced by the reference.
_ROT = {'clockwise': 0, 'counterclockwise': 2}                       # class index in metric['profile']
_SHIFT = {'up': ('x', 0, 0), 'down': ('x', 0, 2), 'left': ('y', 1, 0), 'right': ('y', 1, 2)}     # axis name, column, class index


GOAL_BASIN_DEG = (3, 5, 10)      # the thresholds 'convergence' scores the final angles with (metric2objective)


def convergence_range_from_finals(finals, threshold=0.1):
    """Maximal runs [start, end] of consecutive orientations whose final angles stay within ``threshold`` of each other
    (running min/max since the run began); runs of a single orientation are dropped (metrics.py:40-65)."""
    runs = []
    start = end = 0
    lo = hi = finals[0]
    for i in range(1, len(finals)):
        lo, hi = min(lo, finals[i]), max(hi, finals[i])
        if hi - lo <= threshold:
            end = i
            continue
        if end - start >= 1:
            runs.append((start, end))
        start = end = i
        lo = hi = finals[i]
    if end - start >= 1:
        runs.append((start, end))
    return runs


def _rot_part(metric, rot):
    return {f'num_{rot}_classes': np.sum(metric['profile'] == _ROT[rot], dtype=np.int16),
            'delta_theta': np.mean(metric['delta_theta']), 'final_delta_theta': np.mean(metric['final_delta_theta'])}


def _shift_part(metric, shift):
    ax, col, cls = _SHIFT[shift]
    return {f'num_{shift}_classes': np.sum(metric['profile_' + ax] == cls, dtype=np.int16),
            f'delta_pos_{ax}': np.mean(metric['delta_pos'][:, col]), f'final_pos_{ax}': np.mean(metric['final_pos'][:, col])}


def metric2objective(metric, objective):
    """Scores of one (object, gripper) roll-out for ``objective`` (metrics.py:67-234): a success rate over the orientation grid,
    class counts, and mean motions.  Key names and dtypes as in the reference.  A ``Goal`` (dgdm_amd/goal.py) is scored by
    ``predicted.goal_objective`` on the roll-out's settled poses."""
    from ..goal import is_goal
    if is_goal(objective):
        from .predicted import goal_objective
        return goal_objective(metric, objective)
    if objective == 'rotate':
        p = metric['profile']
        return {'success_rate': np.mean((p == 0) | (p == 2), dtype=np.float32), 'num_zero_classes': np.sum(p == 1, dtype=np.int16),
                'delta_theta_abs': np.mean(np.abs(metric['delta_theta'])), 'final_delta_theta_abs': np.mean(np.abs(metric['final_delta_theta']))}
    if objective == 'convergence':
        out = {}
        for deg in (3, 5, 10):
            runs = convergence_range_from_finals(metric['final_theta'], threshold=deg)
            out[f'max_convergence_range_{deg}deg'] = np.max([b - a for a, b in runs]) if len(runs) > 0 else 0
        return out
    head, _, tail = objective.partition('_')
    if head == 'rotate' and tail in _ROT:
        return {'success_rate': np.mean(metric['profile'] == _ROT[tail], dtype=np.float32), **_rot_part(metric, tail)}
    if head == 'shift' and tail in _SHIFT:
        ax, _, cls = _SHIFT[tail]
        return {'success_rate': np.mean(metric['profile_' + ax] == cls, dtype=np.float32), **_shift_part(metric, tail)}
    if head in _ROT and tail in _SHIFT:
        ax, _, cls = _SHIFT[tail]
        rot, sh = _rot_part(metric, head), _shift_part(metric, tail)
        return {'success_rate': np.mean((metric['profile'] == _ROT[head]) & (metric['profile_' + ax] == cls), dtype=np.float32),
                f'num_{head}_{tail}_classes': rot[f'num_{head}_classes'] + sh[f'num_{tail}_classes'], **rot, **sh}
    raise NotImplementedError


def objective_directions(opt_obj):
    """For every score of ``opt_obj``: +1 if larger is better, -1 if smaller is better - the argmax/argmin choices of
    Diffusion.get_best_ids_all_metrics (generator/diffusion.py:391-428) - plus the key get_average_best_ids ranks by (:354-389).
    A ``Goal``: the scores of ``predicted.goal_objective`` - more start orientations in the basin is better, less error is better."""
    from ..goal import is_goal
    if is_goal(opt_obj):
        return ({**{f'goal_basin_{d}deg': +1 for d in GOAL_BASIN_DEG}, 'goal_error_deg': -1, 'goal_pos_error_cm': -1}, 'goal_basin_5deg')
    if opt_obj in ('rotate', 'rotate_in_place'):
        return {'num_zero_classes': -1, 'delta_theta_abs': +1, 'final_delta_theta_abs': +1}, 'num_zero_classes'
    if opt_obj == 'convergence':
        return {f'max_convergence_range_{d}deg': +1 for d in (3, 5, 10)}, 'max_convergence_range_5deg'
    head, _, tail = opt_obj.partition('_')

    def rot(name):      # clockwise = negative delta theta
        sgn = -1 if name == 'clockwise' else +1
        return {f'num_{name}_classes': +1, 'delta_theta': sgn, 'final_delta_theta': sgn}

    def shift(name):    # up / left = negative x / y
        ax = _SHIFT[name][0]
        sgn = -1 if name in ('up', 'left') else +1
        return {f'num_{name}_classes': +1, f'delta_pos_{ax}': sgn, f'final_pos_{ax}': sgn}

    if head == 'rotate' and tail in _ROT:
        return rot(tail), f'num_{tail}_classes'
    if head == 'shift' and tail in _SHIFT:
        return shift(tail), f'num_{tail}_classes'
    if head in _ROT and tail in _SHIFT:
        return {f'num_{head}_{tail}_classes': +1, **rot(head), **shift(tail)}, f'num_{head}_{tail}_classes'
    raise ValueError('opt obj not supported')
