"""GPU: the time-unfold / fold kernels of csrc/conv1d.hip against the plain-torch restatement (tests/tts_oracle.py: F.pad and index,
and its autograd), and ops.conv1d_bn against nn.Conv1d + nn.BatchNorm1d in float64."""
import pytest
import torch

from oracle import recipe
from tests import tts_oracle as O
from tests.golden_util import rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
B = 2
TS, CS, KS = (1, 2, 5, 37), (8, 80, 6), (1, 3, 5)        # C = 8, 80: 16-byte accesses; C = 6: one element per access


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
def test_unfold_moves_values_exactly(dtype):
    from ofasys_amd import kernels as K
    for T in TS:
        for C in CS:
            x = recipe.floats(f"conv1d.x.{T}.{C}", (B, T, C))
            x[0].clamp_(-8, 8)
            x[1] = x[1].abs() + 1000.0                                         # sample 1 is recognisable: nothing of it may reach sample 0
            x = x.to(dtype)
            for k in KS:
                col = K.unfold1d(x.to(DEV).view(B * T, C), B, T, C, k).cpu()
                want = O.unfold1d(x.view(B * T, C), B, T, C, k)
                assert col.shape == want.shape == (B * T, (k * C + 7) // 8 * 8)
                assert torch.equal(col, want), (T, C, k)                       # exact: it only moves values
                half = (k - 1) // 2
                assert not col[:, k * C:].any()                                # pad columns
                for b in range(B):
                    for e in range(min(half, T)):                              # both edges of every sample: the taps that fall outside
                        assert not col[b * T + e, :(half - e) * C].any() and not col[b * T + T - 1 - e, (k - half + e) * C:].any()
                assert float(col[:T].float().abs().max()) <= 8.0               # sample 0's rows hold nothing of sample 1
                assert k == 1 or T == 1 or float(col[T:, :k * C].float().abs().max()) >= 1000.0


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
def test_fold_is_the_adjoint_of_unfold(dtype):
    """Against autograd of the restatement in float64.  16-bit: dcol lies on the grid n / 64, |n| <= 256, so every <= 5-term fp32 sum is
    exact (<= 12 significant bits) and the kernel's one rounding must equal the float64 sum rounded once: exact equality.  fp32: the
    <= k-term sum in a fixed order carries at most (k - 1) roundings of 2^-24 relative to the sum of the terms' magnitudes."""
    from ofasys_amd import kernels as K
    for T in TS:
        for C in CS:
            for k in KS:
                Kpad = (k * C + 7) // 8 * 8
                d = recipe.floats(f"conv1d.d.{T}.{C}.{k}", (B * T, Kpad))
                if dtype != torch.float32:
                    d = (d * 64).round().clamp_(-256, 256) / 64
                d = d.to(dtype)                                                # (the pad columns hold values too: fold must not read them)
                got = K.fold1d(d.to(DEV), B, T, C, k).cpu()
                x = torch.zeros(B * T, C, dtype=torch.float64, requires_grad=True)
                (O.unfold1d(x, B, T, C, k) * torch.cat((d[:, :k * C].double(), torch.zeros(B * T, Kpad - k * C, dtype=torch.float64)), 1)).sum().backward()
                if dtype != torch.float32:
                    assert torch.equal(got, x.grad.to(dtype)), (T, C, k)
                else:
                    xa = torch.zeros(B * T, C, dtype=torch.float64, requires_grad=True)
                    (O.unfold1d(xa, B, T, C, k)[:, :k * C] * d[:, :k * C].double().abs()).sum().backward()
                    assert bool(((got.double() - x.grad).abs() <= (k - 1) * 2.0 ** -24 * xa.grad + 1e-300).all()), (T, C, k)


def _q(t, dtype):
    return t.to(dtype).double()


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("training", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("shape", ((3, 13, 80, 32), (3, 13, 32, 80)), ids=("80to32", "32to80"))
def test_conv1d_bn_against_torch_in_float64(shape, training, dtype):
    """ops.conv1d_bn forward and backward against nn.Conv1d(k = 5, padding 2) + nn.BatchNorm1d in float64 on the same (quantised)
    inputs and parameters.  fp32: the project's parity bound, 1e-3 of the largest element.  bf16: the float64 side rounds the
    convolution's output to bf16 where the kernel path does; what remains is the half-ulp rounding of each stored tensor (2^-9
    relative) -- the output and, going back, BatchNorm's dx, the GEMM's dcol and the fold's dx -- and a rounding of the convolution
    output flipped by the fp32 accumulation order, passed on by gamma * rstd ~ 1: 2^-7 of the largest element forward, 2^-6 backward."""
    from ofasys_amd import ops
    Bn, T, Cin, Cout = shape
    tag = f"conv1dbn.{Cin}.{Cout}"
    conv, bn = torch.nn.Conv1d(Cin, Cout, 5, padding=2), torch.nn.BatchNorm1d(Cout)
    with torch.no_grad():
        conv.weight.copy_(recipe.floats(tag + ".w", (Cout, Cin, 5), 0.1)); conv.bias.copy_(recipe.floats(tag + ".b", (Cout,), 0.1))
        bn.weight.copy_(1 + recipe.floats(tag + ".g", (Cout,), 0.2)); bn.bias.copy_(recipe.floats(tag + ".beta", (Cout,), 0.2))
        bn.running_mean.copy_(recipe.floats(tag + ".rm", (Cout,), 0.1)); bn.running_var.copy_(recipe.floats(tag + ".rv", (Cout,), 0.1).abs() + 0.8)
    x, dout = recipe.floats(tag + ".x", (Bn, T, Cin)), recipe.floats(tag + ".dout", (Bn, T, Cout))
    # float64 side, from the quantised values
    c64, b64 = torch.nn.Conv1d(Cin, Cout, 5, padding=2).double(), torch.nn.BatchNorm1d(Cout).double()
    with torch.no_grad():
        for dst, src in ((c64.weight, conv.weight), (c64.bias, conv.bias), (b64.weight, bn.weight), (b64.bias, bn.bias)):
            dst.copy_(_q(src, dtype))
        b64.running_mean.copy_(_q(bn.running_mean, dtype)); b64.running_var.copy_(_q(bn.running_var, dtype))   # (a bf16 module's buffers are bf16)
    c64.train(training); b64.train(training)
    x64 = _q(x, dtype).requires_grad_(True)
    y64 = c64(x64.transpose(1, 2))
    if dtype != torch.float32:
        y64 = y64 + (y64.detach().to(dtype).double() - y64.detach())           # rounded where the kernel path stores it (straight-through)
    out64 = b64(y64).transpose(1, 2)
    (out64 * _q(dout, dtype)).sum().backward()
    # kernel side
    conv, bn = conv.to(DEV).to(dtype), bn.to(DEV).to(dtype)
    conv.train(training); bn.train(training)
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    out = ops.conv1d_bn(xg.view(Bn * T, Cin), conv, bn, Bn, T)
    assert out.shape == (Bn * T, Cout) and out.dtype == dtype
    (out.view(Bn, T, Cout).float() * dout.to(DEV).to(dtype).float()).sum().backward()
    torch.cuda.synchronize()
    fwd_tol, bwd_tol = (1e-3, 1e-3) if dtype == torch.float32 else (2.0 ** -7, 2.0 ** -6)
    figs = {"out": rel_err(out.view(Bn, T, Cout).float().cpu(), out64.detach()), "dx": rel_err(xg.grad.float().cpu(), x64.grad),
            "dw": rel_err(conv.weight.grad.float().cpu(), c64.weight.grad), "dgamma": rel_err(bn.weight.grad.float().cpu(), b64.weight.grad),
            "dbeta": rel_err(bn.bias.grad.float().cpu(), b64.bias.grad)}
    if not training:                                    # (train mode: the bias cancels in the batch mean, its gradient is rounding noise)
        figs["db"] = rel_err(conv.bias.grad.float().cpu(), c64.bias.grad)
    else:
        figs["running_mean"] = rel_err(bn.running_mean.float().cpu(), b64.running_mean)
        figs["running_var"] = rel_err(bn.running_var.float().cpu(), b64.running_var)
    print(shape, training, str(dtype), {k: f"{v:.2e}" for k, v in figs.items()})
    assert figs["out"] < fwd_tol, figs
    assert all(v < bwd_tol for k, v in figs.items() if k != "out"), figs
