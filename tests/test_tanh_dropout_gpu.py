"""GPU: ofa_tanh_dropout_fwd / _bwd (csrc/conv1d.hip) -- p = 0 against float64 tanh, p = 0.5 for the mask's statistics, its values, its
agreement between forward and backward, and its behaviour under graph replay."""
import pytest
import torch

from oracle import recipe

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
ULP = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}    # spacing of the format in [0.5, 1)
F32_SLACK = 8 * 2.0 ** -24                               # a few fp32 roundings (tanhf: ~2 ulp; y*y, 1 - y*y, the product)


def _inputs(n, dtype, tag="td"):
    x = recipe.floats(f"{tag}.x.{n}", (n,)).clamp_(-3, 3)
    x[x.abs() < 1e-3] = 0.5                                                    # (tanh(x) != 0: a zero in the output is a dropped element)
    dy = recipe.floats(f"{tag}.dy.{n}", (n,))
    dy[dy.abs() < 1e-3] = 1.0
    return x.to(dtype), dy.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16", "fp16"))
def test_p0_is_tanh_forward_and_backward(dtype):
    """|tanh| < 1, so a 16-bit output lies within one spacing `ULP` of the float64 value (half of it is the rounding to the format, the
    rest covers a rounding flipped by tanhf's fp32 error); fp32: F32_SLACK absolute.  Backward, from the STORED y: dx = dy (1 - y^2) in
    fp32 -- the rounding of y^2 is relative to 1, not to 1 - y^2, hence F32_SLACK |dy| absolute -- then one rounding to the format, at
    most ULP relative (2 ULP allowed)."""
    from ofasys_amd import kernels as K
    for n in (1, 63, 64, 65, 8 * 80 + 3):
        x, dy = _inputs(n, dtype)
        y = K.tanh_dropout_fwd(x.to(DEV), 0.0, 0, 0, None)
        dx = K.tanh_dropout_bwd(dy.to(DEV), y, 0.0, 0, 0, None).cpu()
        y = y.cpu()
        assert y.shape == x.shape and y.dtype == dtype
        tol = F32_SLACK if dtype == torch.float32 else ULP[dtype]
        assert float((y.double() - torch.tanh(x.double())).abs().max()) <= tol, (n, dtype)
        want = dy.double() * (1 - y.double() ** 2)
        rel = 0.0 if dtype == torch.float32 else 2 * ULP[dtype]
        assert bool(((dx.double() - want).abs() <= rel * want.abs() + F32_SLACK * dy.double().abs()).all()), (n, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16", "fp16"))
def test_p_half_mask_share_values_and_backward_mask(dtype):
    """n = 65539 draws at p = 0.5: the kept count is Binomial(n, 1/2), sigma = sqrt(n) / 2 = 128; it must lie within 5 sigma = 640 of n / 2
    (probability of a false alarm 6e-7; the seed is fixed, so the test is deterministic).  Kept values are tanh / (1 - p) = 2 tanh
    (twice the p = 0 output exactly: a power of two), dropped ones are 0; the backward's zeros are the forward's."""
    from ofasys_amd import kernels as K
    n = 65536 + 3
    x, dy = _inputs(n, dtype, "td5")
    seed, off = 0x1234, 17
    y = K.tanh_dropout_fwd(x.to(DEV), 0.5, seed, off, None)
    y0 = K.tanh_dropout_fwd(x.to(DEV), 0.0, 0, 0, None)
    dx = K.tanh_dropout_bwd(dy.to(DEV), y, 0.5, seed, off, None)
    kept = y != 0
    assert abs(int(kept.sum()) - n / 2) <= 640, int(kept.sum())
    assert torch.equal(y[kept].float(), 2 * y0[kept].float()) and not y[~kept].any()
    assert torch.equal(dx != 0, kept)                                          # (dy != 0 and |t| < 1: a kept element has a gradient)
    t = y.double() * 0.5
    want = dy.to(DEV).double() * 2 * (1 - t * t)
    rel = 0.0 if dtype == torch.float32 else 2 * ULP[dtype]
    assert bool(((dx.double() - want)[kept].abs() <= rel * want[kept].abs() + 2 * F32_SLACK * dy.to(DEV).double()[kept].abs()).all())
    # the same counter gives the same mask, the next one another
    assert torch.equal(K.tanh_dropout_fwd(x.to(DEV), 0.5, seed, off, None), y)
    assert not torch.equal(K.tanh_dropout_fwd(x.to(DEV), 0.5, seed, off + n // 8 + 1, None) != 0, kept)
    assert not torch.equal(K.tanh_dropout_fwd(x.to(DEV), 0.5, seed + 1, off, None) != 0, kept)
    # the mask is dropout_add's at the same position: element e draws halfword e % 8 of counter offset + e / 8
    ones = torch.ones(n, dtype=dtype, device=DEV)
    assert torch.equal(K.dropout_add(ones, None, 0.5, seed, off, None) != 0, kept)


def test_autograd_function_and_graph_replay():
    """ops.tanh_dropout under a captured graph: the position is the device-resident base + the host's relative offset, and the captured
    `rng_advance` moves the base, so two replays draw different masks; eval mode and p = 0 draw nothing."""
    from ofasys_amd import ops
    n = 8 * 80 * 13
    x, dy = _inputs(n, torch.bfloat16, "tdg")
    x, dy = x.to(DEV).view(13 * 8, 80), dy.to(DEV).view(13 * 8, 80)
    ops.manual_seed(7)
    before = ops._Rng.offset
    assert torch.equal(ops.tanh_dropout(x, 0.5, False), ops.tanh_dropout(x, 0.0, True)) and ops._Rng.offset == before
    xg = x.clone().requires_grad_(True)
    y = ops.tanh_dropout(xg, 0.5, True)
    y.backward(dy)
    assert torch.equal(xg.grad != 0, y != 0) and 0.4 < float((y != 0).float().mean()) < 0.6
    ops.rng_advance()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.tanh_dropout(x, 0.5, True)
        ops.rng_advance()
    masks = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        masks.append((out != 0).clone())
    assert not torch.equal(masks[0], masks[1])
    assert all(0.4 < float(m.float().mean()) < 0.6 for m in masks)
