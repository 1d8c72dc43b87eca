"""GPU: the VQGAN decoder's kernels (csrc/vqgan.hip) and their way to the user.

* vq_conv3x3 without the prologue BIT FOR BIT against the float64 restatement on the exact cases of tests/vqgan_case.py, whose sizes
  follow the kernel's own plan (tile seams, one Cin slice and more, one channel block and more), with and without the x2 upsample and
  the residual, both dtypes.
* Sample 1 of a batch of two equal, bit for bit, to the same image run alone, with the norm + swish prologue on.
* vq_groupnorm_stats + vq_conv3x3 with the prologue, vq_norm_rows and vq_conv_out against float64: the relative 2-norm error is at most
  2 x the error of torch's own device composite (F.group_norm -> swish -> F.conv2d) in the same dtype on the same rounded inputs,
  measured in the same test and printed.  The factor allows for another summation order; the kernels round once where the composite
  rounds three times.  Inputs: N(0, 1) scaled and shifted per sample; 4 + N(0, 1) (padding before the activation shows at the border);
  fp16 100 + 0.1 N(0, 1) (E[x^2] - mean^2 in fp32 loses the variance).
* The tiny decoder of the issue end to end through VQGANTokenizer.decode under the same rule, and as PIL images."""
import pytest
import torch
import torch.nn.functional as F

from tests import vqgan_case as C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _plan(*shape):
    from ofasys_amd import kernels as K
    return K.vqgan_conv_plan(*shape)


def _rows(t, dtype):
    return C.rows(t).to(dtype).to(DEV)


def _nchw(y):
    return y.permute(0, 3, 1, 2)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("up", (False, True), ids=("same", "up2"))
@pytest.mark.parametrize("case", C.conv_cases(_plan), ids=lambda c: c[0])
def test_conv3x3_bit_for_bit(case, up, name):
    from ofasys_amd import ops
    from ofasys_amd.module.vqgan import tap_major2d
    dtype, t = DTYPES[name], C.exact_conv(case, up)
    x, w, b = _rows(t["x"], dtype), tap_major2d(t["w"]).to(dtype).to(DEV), t["b"].to(dtype).to(DEV)
    for res, want in ((None, t["want"]), (_rows(t["res"], dtype), t["want_res"])):
        got = ops.vqgan_conv3x3(x, w, b, res=res, upsample=up)
        assert got.dtype == dtype and got.shape == C.rows(want).shape and torch.equal(_nchw(got).double().cpu(), want)


def _chain(x, gamma, beta, w, b, up=False):
    """vq_groupnorm_stats + vq_conv3x3 on NCHW tensors already in the kernels' dtype on the device."""
    from ofasys_amd import ops
    from ofasys_amd.module.vqgan import tap_major2d
    xr = C.rows(x)
    return _nchw(ops.vqgan_conv3x3(xr, tap_major2d(w), b, *ops.vqgan_groupnorm_stats(xr, gamma, beta), upsample=up))


def _operands(gen, kind, dtype, Cin, Cout, H, W):
    x = torch.randn(2, Cin, H, W, generator=gen)
    x = {"plain": x * torch.tensor([1.0, 3.0]).view(2, 1, 1, 1) + torch.tensor([0.0, -2.0]).view(2, 1, 1, 1), "offset": 4 + x, "far": 100 + 0.1 * x}[kind]
    gamma, beta = 1 + 0.3 * torch.randn(Cin, generator=gen), 0.3 * torch.randn(Cin, generator=gen)
    w, b = torch.randn(Cout, Cin, 3, 3, generator=gen) / (9 * Cin) ** 0.5, 0.1 * torch.randn(Cout, generator=gen)
    return [t.to(dtype).to(DEV) for t in (x, gamma, beta, w, b)]                 # the reference is fed these rounded values


@pytest.mark.parametrize("up", (False, True), ids=("same", "up2"))
def test_a_sample_does_not_depend_on_its_batch(up):
    ops_ = _operands(torch.Generator().manual_seed(3), "plain", torch.bfloat16, 64, 64, 17, 19)
    both, alone = _chain(*ops_, up=up), _chain(ops_[0][1:].contiguous(), *ops_[1:], up=up)
    assert torch.equal(both[1:], alone) and not torch.equal(both[:1], alone)


PROLOGUE = [("plain", "bf16", 64, 64, False), ("plain", "fp16", 96, 32, False), ("plain", "fp16", 32, 32, True), ("offset", "bf16", 32, 32, False),
            ("offset", "fp16", 32, 64, True), ("far", "fp16", 32, 32, False), ("far", "fp16", 64, 32, False)]


@pytest.mark.parametrize("kind,name,Cin,Cout,up", PROLOGUE, ids=[f"{k}-{n}-c{ci}to{co}{'-up2' if u else ''}" for k, n, ci, co, u in PROLOGUE])
def test_prologue_chain_within_twice_torchs_error(kind, name, Cin, Cout, up):
    H, W = 19, 35                                                                # two tiles by three, 665 pixels: several statistics chunks
    x, gamma, beta, w, b = _operands(torch.Generator().manual_seed(Cin + Cout), kind, DTYPES[name], Cin, Cout, H, W)
    want = C.conv3x3(x.double().cpu(), w.double().cpu(), b.double().cpu(), norm=(gamma.double().cpu(), beta.double().cpu()), up=up)
    e_new, e_torch = C.rel(_chain(x, gamma, beta, w, b, up=up), want), C.rel(C.conv3x3(x, w, b, norm=(gamma, beta), up=up), want)
    print(f"stats + conv3x3 {kind} {name} {Cin}->{Cout} up={up}: relative error {e_new:.3e}, torch's device composite {e_torch:.3e}")
    assert e_new <= 2 * e_torch


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("Cn", (32, 64))
def test_norm_rows_and_conv_out_within_twice_torchs_error(Cn, name):
    from ofasys_amd import ops
    from ofasys_amd.module.vqgan import tap_major2d
    x, gamma, beta, w, b = _operands(torch.Generator().manual_seed(Cn), "plain", DTYPES[name], Cn, 3, 19, 35)
    xr, n64 = C.rows(x), (gamma.double().cpu(), beta.double().cpu())
    tables = ops.vqgan_groupnorm_stats(xr, gamma, beta)
    want = F.group_norm(x.double().cpu(), 32, *n64, eps=1e-6)
    e_new, e_torch = C.rel(_nchw(ops.vqgan_norm_rows(xr, *tables)), want), C.rel(F.group_norm(x, 32, gamma, beta, eps=1e-6), want)
    print(f"norm_rows {name} C={Cn}: relative error {e_new:.3e}, torch's device composite {e_torch:.3e}")
    assert e_new <= 2 * e_torch
    want = C.conv3x3(x.double().cpu(), w.double().cpu(), b.double().cpu(), norm=n64)
    got = ops.vqgan_conv_out(xr, tap_major2d(w), b, *tables)
    e_new, e_torch = C.rel(got, want), C.rel(C.conv3x3(x, w, b, norm=(gamma, beta)), want)
    print(f"conv_out {name} C={Cn}: relative error {e_new:.3e}, torch's device composite {e_torch:.3e}")
    assert got.dtype == torch.float32 and got.shape == (2, 3, 19, 35) and e_new <= 2 * e_torch


@pytest.mark.parametrize("name", list(DTYPES))
def test_tiny_decoder_end_to_end(name):
    from ofasys_amd import VQGANTokenizer
    tok = VQGANTokenizer(C.TINY, None, code_image_size=16, vqgan_factor=2, dtype=DTYPES[name])
    tokens = torch.randint(0, 64, (2, 65), generator=torch.Generator().manual_seed(1))
    tokens[0, :2], tokens[1, 9] = torch.tensor([-5, 64]), 4000                   # out of range: clamped
    got = tok.decode(tokens.to(DEV), return_pil=False)
    state, codes = tok.vqgan.state_dict(), tokens[:, :64].clamp(0, 63).view(2, 8, 8)
    want = C.decode_code({k: v.double().cpu() for k, v in state.items()}, C.TINY, codes, torch.zeros(1, dtype=torch.float64))
    e_new, e_torch = C.rel(got, want), C.rel(C.decode_code(state, C.TINY, codes, state["post_quant_conv.bias"]), want)
    print(f"tiny decoder {name}: relative error {e_new:.3e}, torch's device composite {e_torch:.3e} (bound {2 * e_torch:.3e})")
    assert got.shape == (2, 3, 16, 16) and got.dtype == torch.float32 and e_new <= 2 * e_torch
    images = tok.decode(tokens.to(DEV))
    assert len(images) == 2 and all(im.mode == "RGB" and im.size == (16, 16) for im in images)
