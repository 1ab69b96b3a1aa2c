"""Host logic of the conditional eps-net that needs no GPU: the command-line flags, --global_cond file validation, the Python layer's shape
errors (raised before the library is touched) and the place of the condition drop-out draw in the generator stream."""
import numpy as np
import pytest
import torch

from dgdm_amd import engine
from dgdm_amd.dynamics.parser import parse
from dgdm_amd.generator import train as gtrain
from dgdm_amd.generator.dataloader import GripperDataset
from dgdm_amd.generator.diffusion import Diffusion
from dgdm_amd.generator.diffusion_utils import ConditionalUnet1D
from dgdm_amd.scheduler import DDIMScheduler


def test_parser_flags():
    a = parse([])
    assert a.global_cond is None and a.cfg_weight == 1.0 and a.cond_drop_prob == 0.0
    a = parse(["--global_cond", "rows.npy", "--cfg_weight", "2.5", "--cond_drop_prob=0.25", "--mode=test"])
    assert a.global_cond == "rows.npy" and a.cfg_weight == 2.5 and a.cond_drop_prob == 0.25 and a.mode == "test"
    gtrain.check_cond_flags(a)
    for bad in (["--cfg_weight", "2"], ["--cond_drop_prob", "0.1"]):                       # nothing to mix or drop without a condition
        with pytest.raises(ValueError, match="need --global_cond"):
            gtrain.check_cond_flags(parse(bad))
    for bad in (["--cond_drop_prob", "1.0"], ["--cond_drop_prob", "-0.1"], ["--cfg_weight", "nan"], ["--cfg_weight", "inf"]):
        with pytest.raises(ValueError):
            gtrain.check_cond_flags(parse(["--global_cond", "rows.npy"] + bad))


def test_global_cond_file_validation(tmp_path):
    f = str(tmp_path / "c.npy")
    good = np.random.RandomState(0).uniform(-1, 1, (12, 6))
    np.save(f, good.astype(np.float32))
    c = gtrain.load_global_cond(f, 12)
    assert c.dtype == np.float32 and c.shape == (12, 6) and np.array_equal(c, good.astype(np.float32))
    np.save(f, good)                                                                       # float64 is converted
    assert gtrain.load_global_cond(f, 12).dtype == np.float32
    with pytest.raises(ValueError, match="12 rows"):
        gtrain.load_global_cond(f, 13)
    np.save(f, good.reshape(12, 3, 2).astype(np.float32))
    with pytest.raises(ValueError, match="rank 2"):
        gtrain.load_global_cond(f, 12)
    np.save(f, good[:, 0].astype(np.float32))
    with pytest.raises(ValueError, match="rank 2"):
        gtrain.load_global_cond(f, 12)
    for v in (np.nan, np.inf):
        bad = good.astype(np.float32)
        bad[7, 2] = v
        np.save(f, bad)
        with pytest.raises(ValueError, match="non-finite.*row 7"):
            gtrain.load_global_cond(f, 12)
    np.save(f, np.zeros((12, 257), np.float32))
    with pytest.raises(ValueError, match="1..256"):
        gtrain.load_global_cond(f, 12)
    np.save(f, np.zeros((12, 0), np.float32))
    with pytest.raises(ValueError, match="1..256"):
        gtrain.load_global_cond(f, 12)
    with pytest.raises(ValueError, match="cannot read"):
        gtrain.load_global_cond(str(tmp_path / "missing.npy"), 12)


def test_dataset_pairs():
    pts = gtrain.finger_control_points(5, False)
    cond = np.arange(10, dtype=np.float32).reshape(5, 2)
    plain, pairs = GripperDataset(pts, 0.12, -0.12, 0.015, -0.045), GripperDataset(pts, 0.12, -0.12, 0.015, -0.045, cond=cond)
    assert len(pairs) == 5
    x, c = pairs[3]
    assert np.array_equal(x, plain[3]) and np.array_equal(c, cond[3])
    batch = next(iter(torch.utils.data.DataLoader(pairs, batch_size=4, shuffle=False)))
    fingers, rows = Diffusion.split_batch(batch)
    assert fingers.shape == (4, 14, 1) and torch.equal(rows, torch.from_numpy(cond[:4]))
    assert Diffusion.split_batch(fingers)[0] is fingers and Diffusion.split_batch(fingers)[1] is None
    with pytest.raises(ValueError):
        GripperDataset(pts, 0.12, -0.12, 0.015, -0.045, cond=cond[:4])
    with pytest.raises(ValueError):
        Diffusion.split_batch((fingers, rows, rows))


def test_shape_errors_before_the_library():
    """Every check below runs on CPU tensors: a call that reached the library (or asked for a handle) would fail for want of a GPU with
    another exception type."""
    c = torch.zeros(4, 6)
    assert engine.check_global_cond(c, 6, 4) is c and engine.check_global_cond(None, 0, 4) is None
    for args in ((None, 6, 4), (c, 0, 4), (c, 5, 4), (c, 6, 3), (torch.zeros(4, 6, 1), 6, 4), (torch.zeros(6), 6, 1)):
        with pytest.raises(ValueError):
            engine.check_global_cond(*args)
    assert engine.chain_cond_layout(None, 0, 3, 4) == (None, 0)
    assert engine.chain_cond_layout(c, 6, 3, 4) == (c, 0)
    c3 = torch.zeros(3, 4, 6)
    assert engine.chain_cond_layout(c3, 6, 3, 4) == (c3, 24)
    for cond, gc in ((None, 6), (c3[:2], 6), (c3, 5), (torch.zeros(3, 5, 6), 6), (torch.zeros(1, 3, 4, 6), 6), (c, 0)):
        with pytest.raises(ValueError):
            engine.chain_cond_layout(cond, gc, 3, 4)
    net = ConditionalUnet1D(input_dim=1, global_cond_dim=6, down_dims=[128, 256], diffusion_step_embed_dim=32)
    assert net.global_cond_dim == 6 and net.mid_modules[0].cond_encoder[1].weight.shape == (512, 38)
    x, t = torch.zeros(4, 14, 1), torch.zeros(4, dtype=torch.int64)
    for cond in (None, torch.zeros(4, 5), torch.zeros(3, 6)):
        with pytest.raises(ValueError):
            net.forward(x, t, cond)
    with pytest.raises(ValueError):
        ConditionalUnet1D(input_dim=1, global_cond_dim=0, down_dims=[128, 256], diffusion_step_embed_dim=32).forward(x, t, torch.zeros(4, 6))
    with pytest.raises(NotImplementedError):
        ConditionalUnet1D(input_dim=2, global_cond_dim=6, down_dims=[128, 256], diffusion_step_embed_dim=32)
    with pytest.raises(ValueError):
        ConditionalUnet1D(input_dim=1, global_cond_dim=257, down_dims=[128, 256], diffusion_step_embed_dim=32)


def _diffusion(gc):
    net = ConditionalUnet1D(input_dim=1, global_cond_dim=gc, down_dims=[128, 256], diffusion_step_embed_dim=32)
    return Diffusion(noise_pred_net=net, noise_scheduler=DDIMScheduler(num_train_timesteps=15), num_inference_steps=5, mode='point', input_dim=1,
                     num_points=14)


def test_dropout_draw_comes_after_the_reference_draws():
    B, L, gc = 6, 14, 4
    x0 = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (B, L, 1)).astype(np.float32))
    cond = torch.from_numpy(np.random.RandomState(2).uniform(0.5, 1, (B, gc)).astype(np.float32))
    # today's stream: randn, randint
    torch.manual_seed(9)
    noise = torch.randn((B, L, 1))
    ts = torch.randint(0, 15, (B,)).long()
    after_two = torch.get_rng_state()
    drop = torch.rand(B) < 0.5
    after_three = torch.get_rng_state()
    assert bool(drop.any()) and not bool(drop.all())
    plain, d = _diffusion(0), _diffusion(gc)
    assert d.cfg_weight == 1.0 and d.cond_drop_prob == 0.0
    torch.manual_seed(9)
    out = plain._training_draws(x0)
    assert len(out) == 5 and torch.equal(out[1], noise) and torch.equal(out[4], ts) and torch.equal(torch.get_rng_state(), after_two)
    # a condition without drop-out: the same two draws, nothing more; the rows pass through
    torch.manual_seed(9)
    out = d._training_draws(x0, cond)
    assert len(out) == 6 and torch.equal(out[1], noise) and torch.equal(out[4], ts) and torch.equal(out[5], cond)
    assert torch.equal(torch.get_rng_state(), after_two)
    # with drop-out: the third draw, after the two; dropped rows are the all-zero row, the others untouched
    d.cond_drop_prob = 0.5
    torch.manual_seed(9)
    out = d._training_draws(x0, cond)
    assert torch.equal(out[1], noise) and torch.equal(out[4], ts) and torch.equal(torch.get_rng_state(), after_three)
    assert torch.equal(out[5], torch.where(drop[:, None], torch.zeros_like(cond), cond))
    # several timesteps per batch: the rows repeat with the fingers
    d.cond_drop_prob, d.num_timesteps_per_batch = 0.0, 2
    out = d._training_draws(x0, cond)
    assert out[0].shape[0] == 2 * B and torch.equal(out[5], cond.repeat(2, 1))
    # a batch is checked against the module before anything is drawn
    st = torch.get_rng_state()
    for batch in (x0, (x0, cond[:, :3]), (x0, cond[:4])):
        with pytest.raises(ValueError):
            d._draws_for(batch)
    with pytest.raises(ValueError):
        plain._draws_for((x0, cond))
    assert torch.equal(torch.get_rng_state(), st)


def test_checkpoint_width_mismatch_names_both_widths():
    a, b = _diffusion(6), _diffusion(0)
    sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    with pytest.raises(ValueError, match="38.*32"):
        b.load_state_dict(sd)
    with pytest.raises(ValueError, match="32.*38"):
        a.load_state_dict({k: v.detach().clone() for k, v in b.state_dict().items()})
    a.load_state_dict(sd)
