"""The eps-net forward (csrc/unet.hip) against the oracle in float64 across the shapes its entry points accept (include/dgdm_hip.h,
"accepted domain"), not only the shipped down_dims (128, 256) / dsed 32 / 8 groups at L = 14, 42, 44.

| down_dims          | groups | dsed             | L                    | form of 'f32'    | reaches                                                          |
|--------------------|--------|------------------|----------------------|------------------|------------------------------------------------------------------|
| (128, 256)         | 8      | 32               | 2, 4, 16, 32, 34     | split            | halo-only second level (L/2 = 1); exactly full tiles; NT = 3 (34) |
| (128, 256)         | 8      | 32               | 46                   | chain (fallback) | the largest L that fits                                          |
| (128, 256)         | 8      | 4, 6, 12, 20, 64 | 14                   | split            | dot_kn's padded step part; half = 2, 3; dsed > 32 (64: largest)  |
| (128, 256)         | 4      | 32               | 42                   | split            | gn_group's looped power-of-two branch (32 ch at 42, 64 at 21)    |
| (128, 256)         | 1      | 32               | 14                   | split            | gn_group's general branch (group = all channels)                 |
| (128, 256)         | 32     | 32               | 14                   | split            | 4- and 8-channel groups (16 and 8 row lanes)                     |
| (128, 128)         | 8      | 32               | 14, 58               | split            | identity residual in down1.0; NT = 4 in the split form (58: largest) |
| (128, 128)         | 8      | 32               | 64                   | chain (fallback) | NT = 4 on the chain                                              |
| (128, 128)         | 2      | 32               | 42                   | split            | 64-channel groups, looped branch on both levels                  |
| (128, 384)         | 8      | 32               | 14                   | split            | 48-channel groups -> general branch; 24 output tiles, ragged MT = 2 round |
| (256, 256)         | 8      | 32               | 26                   | split            | MT = 2 on level 0 in the split form (largest L with the slabs)   |
| (256, 256)         | 8      | 32               | 28                   | chain (fallback) | MT = 2 on level 0; the largest L that fits at this width (164 300 B with the slabs) |
| (256, 512)         | 8      | 32               | 14                   | split            | cmax = 512 in the FiLM stride, 64-channel groups at level 1      |
| (128, 256), gc = 5 | 8      | 12               | 14                   | split            | condition + unpadded dsed together (forward_cond, tests/cond_oracle.py) |

The LDS need behind the "form" column is unet_lds_floats + unet_slab_floats of unet.hip, worked out by hand per case; the
test asserts what `effective_form` reports.  Every case: B = 5 (four samples and a ragged one), timesteps mixed over [0, 1000), randn inputs,
one sample scaled by 1e-3 (the f16x3 input scale is per sample), the three arithmetic modes.

Bounds.  f32 / f32_mfma against float64: relative L2 <= max(1e-6, 2 e32), e32 = the ORACLE evaluated in float32 against itself in float64 on
the same case (a yardstick with none of the code under test in it; 1e-6 is what test_unet_arithmetic_modes_vs_float64 holds at the shipped
shape, the factor 2 allows for another summation order); f32 <= f32_mfma + 1e-7; bit-equal where 'f32' falls back to the chain.  bf16 against
float64 inside (1e-4, max(2e-2, 2 e16)), e16 = the oracle's bf16 statement (orc.contraction('bf16')) against float64 on the same case, and
within 1e-2 of that statement (the bound of tests/test_gpu_bf16.py::test_bf16_unet_vs_oracle; not for the conditional case: tests/cond_oracle.py
has no bf16 form of the down / up convolutions, there the window is (1e-4, 2e-2)).  Finite; a second call returns the same bits."""
import pytest
import torch

from dgdm_amd import _lib, engine, synth
from oracle import dgdm_oracle as orc
from tests import cond_oracle as co

pytestmark = pytest.mark.gpu
B = 5
SPLIT, CHAIN = "f32_f16x3", "f32_mfma"

#        down_dims   groups dsed  L  gc  form of 'f32'
CASES = [((128, 256), 8, 32, L, 0, SPLIT) for L in (2, 4, 16, 32, 34)] + [((128, 256), 8, 32, 46, 0, CHAIN)] + \
        [((128, 256), 8, d, 14, 0, SPLIT) for d in (4, 6, 12, 20, 64)] + [
    ((128, 256), 4, 32, 42, 0, SPLIT),
    ((128, 256), 1, 32, 14, 0, SPLIT),
    ((128, 256), 32, 32, 14, 0, SPLIT),
    ((128, 128), 8, 32, 14, 0, SPLIT),
    ((128, 128), 8, 32, 58, 0, SPLIT),
    ((128, 128), 8, 32, 64, 0, CHAIN),
    ((128, 128), 2, 32, 42, 0, SPLIT),
    ((128, 384), 8, 32, 14, 0, SPLIT),
    ((256, 256), 8, 32, 26, 0, SPLIT),
    ((256, 256), 8, 32, 28, 0, CHAIN),
    ((256, 512), 8, 32, 14, 0, SPLIT),
    ((128, 256), 8, 12, 14, 5, SPLIT),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


def _sd(dims, dsed, gc, seed):
    return synth.synth_state_dict(synth.unet_spec(down_dims=dims, dsed=dsed, global_cond_dim=gc), seed)


@pytest.mark.parametrize("dims,groups,dsed,L,gc,form", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_unet_shapes_vs_float64(dev, dims, groups, dsed, L, gc, form):
    seed = 1000 * groups + 10 * dsed + L
    sd = _sd(dims, dsed, gc, seed % 9973)
    sd64 = {k: v.double() for k, v in sd.items()}
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, 1, generator=g)
    x[B // 2] *= 1e-3
    t = torch.randint(0, 1000, (B,), generator=g)
    c = torch.rand(B, gc, generator=g).mul(2).sub(1) if gc else None

    def oracle(w, xx):
        with torch.no_grad():
            if gc:
                return co.unet1d_forward_cond(w, xx, t, c.to(xx.dtype), n_groups=groups)
            return orc.unet1d_forward(w, xx, t, n_groups=groups)

    ref = oracle(sd64, x.double())
    e32 = _rel(oracle(sd, x), ref)
    ref16, e16 = None, 0.0
    if not gc:                                   # (tests/cond_oracle.py states the down / up convolutions in float32 only)
        with orc.contraction('bf16'):
            ref16 = oracle(sd, x)
        e16 = _rel(ref16, ref)

    net = engine.Unet1d(sd, dims, dsed, 5, groups)
    assert net.global_cond_dim == gc
    xd, td, cd = x.to(dev), t.to(dev), (c.to(dev) if gc else None)
    out = {}
    for mode in ("f32", "f32_mfma", "bf16"):
        net.set_contraction_dtype(mode)
        want = {"f32": form, "f32_mfma": CHAIN, "bf16": "bf16"}[mode]
        assert net.effective_form(B, L) == (want, False), (mode, net.effective_form(B, L))        # what ran is stated, not assumed
        y = net.forward(xd, td, cd)
        assert bool(torch.isfinite(y).all()), mode
        assert torch.equal(net.forward(xd, td, cd), y), mode
        out[mode] = y.cpu().double()
    err = {m: _rel(o, ref) for m, o in out.items()}
    d16 = _rel(out["bf16"], ref16.double()) if ref16 is not None else 0.0
    print(f"dims={dims} groups={groups} dsed={dsed} L={L} gc={gc} {form}: e32 {e32:.2e} f32 {err['f32']:.2e} f32_mfma {err['f32_mfma']:.2e} "
          f"bf16 {err['bf16']:.2e} (oracle bf16 {e16:.2e}, gpu vs oracle bf16 {d16:.2e})")
    bound = max(1e-6, 2 * e32)
    assert err["f32"] <= bound and err["f32_mfma"] <= bound, (err, e32)
    assert err["f32"] <= err["f32_mfma"] + 1e-7, err
    if form == CHAIN:
        assert torch.equal(out["f32"], out["f32_mfma"])
    assert 1e-4 < err["bf16"] < max(2e-2, 2 * e16), (err, e16)
    assert d16 < 1e-2, d16


def test_unet_shape_rejections(dev):
    """What lies outside the accepted domain is EINVAL from the host code, before any launch: the output buffer keeps its fill."""
    lib = _lib.lib()
    x = torch.randn(B, 66, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.arange(B, dtype=torch.int32, device=dev)
    out = torch.full((B, 66, 1), 7.0, device=dev)
    for dims, Ls in (((128, 256), (15, 66, 48)), ((256, 256), (30,)), ((128, 128), (65, 66))):
        net = engine.Unet1d(_sd(dims, 32, 0, 3), dims)
        for mode in ("f32", "f32_mfma", "bf16"):
            net.set_contraction_dtype(mode)
            for L in Ls:
                xl = x[:, :L].contiguous()
                assert lib.dgdm_unet1d_forward(net._h, xl.data_ptr(), t.data_ptr(), out.data_ptr(), B, L, _lib.stream_ptr()) == _lib.EINVAL, (dims, mode, L)
                with pytest.raises(_lib.DgdmError):
                    net.forward(xl, t)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    sd = _sd((128, 256), 32, 0, 3)
    for dims, dsed, groups, w in (((64, 128), 32, 8, None), ((128, 256), 32, 3, sd), ((128, 256), 32, 0, sd), ((128, 256), 5, 8, None), ((128, 256), 2, 8, None),
                                  ((128, 256), 66, 8, None), ((128, 256), 256, 8, None), ((128, 192), 32, 8, None)):
        with pytest.raises(_lib.DgdmError, match="error -1"):
            engine.Unet1d(w or _sd(dims, dsed, 0, 3), dims, dsed, 5, groups)
