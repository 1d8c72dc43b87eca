"""CPU: the VQGAN encoder's host side.  The new entry points refuse bad shapes with their status codes before any launch; the plans keep
the LDS images under 80 KiB; the Encoder refuses the configuration flags it does not build; `with_encoder=True` keeps the encode side of
a checkpoint (and only drops `loss.*`) while the default tokenizer is what it was.  Nothing here needs a GPU."""
import pytest
import torch

from tests import vqgan_case as C
from tests import vqgan_encode_case as E

INVALID, UNSUPPORTED = 1, 2
F32, BF16, F16 = 0, 1, 2
BASE = {"ofa_vqgan_downsample": dict(x=None, w=None, bias=None, y=None, B=0, H=4, W=4, Cin=32, Cout=32, dtype=F16, stream=None),
        "ofa_vqgan_conv_in": dict(image=None, w32=None, bias=None, y=None, B=0, in_channels=3, H=4, W=4, Cout=32, dtype=BF16, stream=None),
        "ofa_vqgan_quantize": dict(h=None, w=None, bias=None, out=None, ws=None, ws_bytes=0, N=0, K=32, n_embed=64, seed=-1, dtype=BF16, stream=None)}
REFUSALS = [(n, {}, 0) for n in BASE] + [(n, dict(dtype=F32), UNSUPPORTED) for n in BASE] + [(n, dict(dtype=7), INVALID) for n in BASE] + [
    ("ofa_vqgan_downsample", dict(Cin=48, Cout=48), UNSUPPORTED), ("ofa_vqgan_downsample", dict(Cout=64), UNSUPPORTED),
    ("ofa_vqgan_downsample", dict(H=1), INVALID), ("ofa_vqgan_downsample", dict(B=1), INVALID), ("ofa_vqgan_conv_in", dict(in_channels=4), UNSUPPORTED),
    ("ofa_vqgan_conv_in", dict(Cout=40), UNSUPPORTED), ("ofa_vqgan_conv_in", dict(H=0), INVALID), ("ofa_vqgan_quantize", dict(n_embed=40), UNSUPPORTED),
    ("ofa_vqgan_quantize", dict(K=520), UNSUPPORTED), ("ofa_vqgan_quantize", dict(N=-1), INVALID),
    ("ofa_vqgan_quantize", dict(N=1, n_embed=512, ws_bytes=8), INVALID), ("ofa_vqgan_quantize", dict(N=1), INVALID)]


@pytest.mark.parametrize("name,over,want", REFUSALS, ids=[f"{n[10:]}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'ok'}" for n, o, _ in REFUSALS])
def test_entry_points_refuse_before_any_launch(name, over, want):
    from ofasys_amd.lib import lib
    assert set(over) <= set(BASE[name]) and len(lib().protos[name][1]) == len(BASE[name])
    assert getattr(lib().cdll, name)(*dict(BASE[name], **over).values()) == want
    if want:
        assert lib().cdll.ofa_last_error().decode().startswith(name[4:])


def test_plans_and_conv_in_weight():
    from ofasys_amd import kernels as K
    from ofasys_amd.module.vqgan import conv_in_weight
    assert all(K.vqgan_downsample_plan(c)[4] <= 80 * 1024 and K.vqgan_downsample_plan(c)[:2] == (8, 16) for c in (128, 256, 512))
    assert [K.vqgan_downsample_plan(c)[2:4] for c in (32, 64, 96, 512)] == [(32, 32), (64, 64), (64, 64), (64, 128)] and len(E.down_cases(K.vqgan_downsample_plan)) == 8
    # (row tile, code splits, workspace bytes): the f8 model at B = 8 fills 256 CUs; a split keeps 256 codes; one pair of 8 bytes per row and split
    assert K.vqgan_quantize_plan(8192, 256, 8192)[:3] == (128, 4, 4 * 8192 * 8) and K.vqgan_quantize_plan(1, 32, 256)[:3] == (128, 1, 0)
    assert K.vqgan_quantize_plan(1, 32, 512)[:3] == (128, 2, 16) and K.vqgan_quantize_plan(1 << 20, 512, 8192)[:2] == (64, 1)
    assert all(K.vqgan_quantize_plan(1, k, 8192)[3] <= 80 * 1024 for k in (128, 256, 512))
    with pytest.raises(Exception, match="ofa_vqgan_downsample_plan"):
        K.vqgan_downsample_plan(48)
    w = torch.randn(5, 3, 3, 3)
    w32 = conv_in_weight(w)
    assert w32.shape == (5, 32) and not w32[:, 27:].any() and all(torch.equal(w32[:, 3 * (3 * dy + dx) + c], w[:, c, dy, dx])
                                                                  for dy in range(3) for dx in range(3) for c in range(3))


@pytest.mark.parametrize("over", (dict(dropout=0.1), dict(conv_shortcut=True), dict(resamp_with_conv=False), dict(double_z=True), dict(ch=48),
                                  dict(z_channels=16), dict(in_channels=4)), ids=lambda o: next(iter(o)))
def test_encoder_refuses_what_is_not_built(over):
    from ofasys_amd.module.vqgan import Encoder
    Encoder(**C.TINY["ddconfig"])
    with pytest.raises(ValueError, match="VQGAN Encoder"):
        Encoder(**dict(C.TINY["ddconfig"], **over))


def test_checkpoints_with_and_without_the_encoder(tmp_path):
    from ofasys_amd import VQGANTokenizer
    plain, full = ({k: v.cpu() for k, v in VQGANTokenizer(C.TINY, with_encoder=e).vqgan.state_dict().items()} for e in (False, True))
    new = set(full) - set(plain)
    assert not any(k.startswith(("encoder.", "quant_conv.", "quantize.proj.")) for k in plain) and len(plain) == 91
    assert new and all(k.startswith(("encoder.", "quant_conv.", "quantize.proj.")) for k in new) and all(torch.equal(full[k], v) for k, v in plain.items())
    assert {"encoder.conv_in.weight", "encoder.down.0.downsample.conv.bias", "encoder.down.1.attn.0.q.weight", "encoder.down.1.block.0.nin_shortcut.weight",
            "encoder.mid.attn_1.proj_out.bias", "encoder.norm_out.weight", "encoder.conv_out.bias", "quant_conv.weight", "quantize.proj.bias"} <= new
    assert all(float(full[k].float().std()) > 0 for k in new)            # the seeded initialisation covers them
    state = {k: torch.randn_like(v) for k, v in full.items()}
    torch.save({"state_dict": dict(state, **{"loss.logvar": torch.zeros(1)})}, tmp_path / "last.ckpt")
    tok = VQGANTokenizer(C.TINY, str(tmp_path / "last.ckpt"), 16, 2, fp16=True, with_encoder=True)
    got = tok.vqgan.state_dict()
    assert set(got) == set(state) and all(torch.equal(got[k].cpu(), v.half()) for k, v in state.items())
    assert set(VQGANTokenizer(C.TINY, str(tmp_path / "last.ckpt"), 16, 2).vqgan.state_dict()) == set(plain)     # the default drops the encode side
    torch.save({"state_dict": {k: v for k, v in state.items() if k != "encoder.conv_out.bias"}}, tmp_path / "bad.ckpt")
    with pytest.raises(RuntimeError, match="encoder.conv_out.bias"):
        VQGANTokenizer(C.TINY, str(tmp_path / "bad.ckpt"), 16, 2, with_encoder=True)
