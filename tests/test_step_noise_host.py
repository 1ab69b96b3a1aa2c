"""Host side of the stochastic DDIM step: the eta coefficients of dgdm_amd/scheduler.py against the float64 closed form
(tests/step_noise_oracle.py), the eta = 0 corner, the noise-source check of DDIMScheduler.step, the chains' noise keys and the flags."""
import struct

import numpy as np
import pytest
import torch

from dgdm_amd import dist as ddist
from dgdm_amd import sampler
from dgdm_amd.scheduler import DDIMScheduler
from tests import step_noise_oracle as orc


def _sched(T, S):
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(S)
    return s


def _bits(v: float) -> bytes:
    return struct.pack("<f", v)


@pytest.mark.parametrize("T,S", [(15, 5), (1000, 1000)])
def test_eta_coefficients_match_closed_form(T, S):
    """sigma^2 and dir^2 against float64, within 16 * 2^-24 absolute.  Where that comes from: the three float32 differences 1 - abar_prev,
    1 - abar_t and 1 - abar_t / abar_prev lie in [0, 1] and carry at most 1, 1 and 2 roundings of values <= 1, i.e. <= 4 * 2^-24
    absolute together; variance = A / B * C with A <= B and C <= B moves by no more than the sum of its operands' errors plus its own
    two roundings (<= 2 * 2^-24); eta^2 <= 1 does not enlarge that; the square root and the squaring back add 3 relative roundings
    (<= 3 * 2^-24), and dir^2 = 1 - abar_prev - sigma^2 adds the error of 1 - abar_prev once more and two roundings: < 16 * 2^-24.
    The squares are compared because sigma itself has no absolute bound of that kind near variance = 0 (d sqrt(v) = dv / 2 sqrt(v))."""
    s = _sched(T, S)
    tol = 16 * 2.0 ** -24
    worst = 0.0
    for eta in (0.3, 0.5, 1.0):
        for t in s.timesteps:
            t = int(t)
            six = s.coefficients(t, eta)
            assert len(six) == 6 and six[:4] == s.coefficients(t) and six[4:] == s.eta_coefficients(t, eta)
            sigma, dirc = six[4:]
            assert np.isfinite(sigma) and np.isfinite(dirc) and sigma >= 0.0 and dirc >= 0.0, (t, eta, sigma, dirc)
            prev = t - T // S
            a_p = float(s.alphas_cumprod[prev]) if prev >= 0 else 1.0
            s64, d64 = orc.eta_coefficients64(float(s.alphas_cumprod[t]), a_p, eta)
            worst = max(worst, abs(sigma ** 2 - s64 ** 2), abs(dirc ** 2 - d64 ** 2))
            assert abs(sigma ** 2 - s64 ** 2) < tol and abs(dirc ** 2 - d64 ** 2) < tol, (t, eta, sigma, s64, dirc, d64)
            if prev >= 0:
                assert sigma > 0.0
    print(f"T = {T}, S = {S}: worst |square - float64 square| = {worst:.3e} (bound {tol:.3e})")


@pytest.mark.parametrize("T,S", [(15, 5), (1000, 1000)])
def test_last_step_has_no_noise_and_eta0_is_todays_tuple(T, S):
    s = _sched(T, S)
    for eta in (0.5, 1.0):
        sigma, dirc = s.eta_coefficients(int(s.timesteps[-1]), eta)
        assert _bits(sigma) == _bits(0.0) and _bits(dirc) == _bits(0.0)            # abar_prev = final_alpha_cumprod = 1
    for t in s.timesteps:
        four, six = s.coefficients(int(t)), s.coefficients(int(t), 0.0)
        assert [_bits(v) for v in six[:4]] == [_bits(v) for v in four]
        assert _bits(six[4]) == _bits(0.0) and _bits(six[5]) == _bits(four[3])     # dir == sqrt_1m_abar_prev, bitwise


def test_step_without_a_noise_source_is_a_value_error():
    s = _sched(15, 5)
    x = torch.zeros(2, 14, 1)
    with pytest.raises(ValueError, match="variance_noise"):
        s.step(x, 12, x, eta=0.5)
    with pytest.raises(ValueError):
        s.step(x, 12, x, eta=0.5, variance_noise=x, noise_key=(0, 0, 0))


def test_chain_keys():
    chains = [(i % 3, 'rotate') for i in range(7)]
    for world in (2, 3):
        keys = []
        for rank in range(world):
            mine, _, local = ddist.shard_chains(chains, rank, world)
            k = ddist.chain_noise_keys(mine)
            assert len(k) == len(local) and sampler.step_noise_keys(len(local), False, k) == k
            keys += k
        assert keys == list(range(7)), (world, keys)
    assert sampler.step_noise_keys(4) == [0, 1, 2, 3]
    assert sampler.step_noise_keys(4, True) == [0, 0, 0, 0] and sampler.step_noise_keys(3, True, [4, 5, 6]) == [0, 0, 0]
    with pytest.raises(ValueError):
        sampler.step_noise_keys(3, False, [0, 1])


def test_parser_flags():
    from dgdm_amd.dynamics.parser import parse
    a = parse([])
    assert a.eta == 0.0 and a.noise_seed is None and a.shared_step_noise is False
    a = parse(["--eta", "0.5", "--noise_seed", "3", "--shared_step_noise"])
    assert a.eta == 0.5 and a.noise_seed == 3 and a.shared_step_noise is True


def test_diffusion_defaults():
    """Diffusion(..., eta=0.0, noise_seed=None): None means `seed`; eta = 0 hands the samplers nothing new."""
    from dgdm_amd.generator.diffusion import Diffusion
    net = torch.nn.Identity()
    d = Diffusion(net, _sched(15, 5), 5, seed=4)
    assert d.eta == 0.0 and d.noise_seed == 4 and d._noise_kw() == {}
    d = Diffusion(net, _sched(15, 5), 5, seed=4, eta=0.5, noise_seed=9)
    assert d._noise_kw() == dict(eta=0.5, noise_seed=9, shared_step_noise=False)
    with pytest.raises(ValueError):
        Diffusion(net, _sched(15, 5), 5, eta=-1.0)
