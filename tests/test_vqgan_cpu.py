"""CPU: the VQGAN decoder's host side.  The header declares and the library exports the entry points, which refuse fp32 and bad channel
counts with their status codes before any launch; the Decoder refuses the configuration flags it does not build; the tap-major weight
arrangement round-trips; checkpoints in the reference's format load (and only those); `VQGANTokenizer.decode` drops the last token,
clamps the codes and shapes its output, checked with `decode_code` replaced by the float64 restatement (there is no CPU path through
the kernels); `encode` raises.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from tests import vqgan_case as C

INVALID, UNSUPPORTED = 1, 2                              # OFA_ERR_INVALID, OFA_ERR_UNSUPPORTED
F32, BF16, F16 = 0, 1, 2
BASE = {"ofa_vqgan_groupnorm_stats": dict(x=None, gamma=None, beta=None, scale=None, shift=None, ws=None, ws_bytes=1 << 20, B=0, H=4, W=4, C=32,
                                          dtype=F16, stream=None),
        "ofa_vqgan_norm_rows": dict(x=None, scale=None, shift=None, y=None, B=0, H=4, W=4, C=32, dtype=BF16, stream=None),
        "ofa_vqgan_conv3x3": dict(x=None, w=None, bias=None, res=None, scale=None, shift=None, y=None, B=0, H=4, W=4, Cin=32, Cout=32, upsample=0,
                                  dtype=F16, stream=None),
        "ofa_vqgan_conv_out": dict(x=None, w=None, bias=None, scale=None, shift=None, out=None, B=0, H=4, W=4, C=32, out_ch=3, dtype=BF16,
                                   stream=None)}
REFUSALS = [(n, {}, 0) for n in BASE] + [(n, dict(dtype=F32), UNSUPPORTED) for n in BASE] + [(n, dict(dtype=7), INVALID) for n in BASE] + [
    ("ofa_vqgan_conv3x3", dict(Cin=48), UNSUPPORTED), ("ofa_vqgan_conv3x3", dict(Cout=544), UNSUPPORTED), ("ofa_vqgan_conv3x3", dict(Cin=512, Cout=512), 0),
    ("ofa_vqgan_conv3x3", dict(upsample=1, H=5), INVALID), ("ofa_vqgan_conv3x3", dict(H=0), INVALID), ("ofa_vqgan_conv3x3", dict(B=1), INVALID),
    ("ofa_vqgan_groupnorm_stats", dict(C=40), UNSUPPORTED), ("ofa_vqgan_groupnorm_stats", dict(B=1, ws_bytes=8), INVALID),
    ("ofa_vqgan_norm_rows", dict(C=16), UNSUPPORTED), ("ofa_vqgan_conv_out", dict(out_ch=5), UNSUPPORTED), ("ofa_vqgan_conv_out", dict(C=520), UNSUPPORTED)]


@pytest.mark.parametrize("name,over,want", REFUSALS, ids=[f"{n[10:]}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'ok'}" for n, o, _ in REFUSALS])
def test_entry_points_refuse_before_any_launch(name, over, want):
    from ofasys_amd.lib import lib
    assert set(over) <= set(BASE[name]) and len(lib().protos[name][1]) == len(BASE[name])
    assert getattr(lib().cdll, name)(*dict(BASE[name], **over).values()) == want
    if want:
        assert lib().cdll.ofa_last_error().decode().startswith(name[4:])


def test_plan_and_weight_arrangement():
    from ofasys_amd import kernels as K
    from ofasys_amd.module.vqgan import from_tap_major2d, tap_major2d
    # (tile side, Cin slice, channels per workgroup, LDS bytes): the fewest even slices under 80 KiB, the same with the upsample
    assert [K.vqgan_conv_plan(*s)[:3] for s in ((32, 32), (96, 64), (128, 128), (160, 96), (256, 256), (512, 512))] == \
        [(16, 32, 32), (16, 96, 64), (16, 64, 128), (16, 96, 64), (16, 96, 128), (16, 96, 128)]
    assert all(K.vqgan_conv_plan(c, c, up)[3] <= 80 * 1024 for c in (128, 256, 512) for up in (0, 1))
    assert K.vqgan_conv_plan(512, 512, 1)[1] == 96 and len(C.conv_cases(K.vqgan_conv_plan)) == 9
    with pytest.raises(Exception, match="ofa_vqgan_conv_plan"):
        K.vqgan_conv_plan(48, 32)
    w = torch.randn(5, 3, 3, 3)
    w9 = tap_major2d(w)
    assert w9.shape == (9, 5, 3) and torch.equal(from_tap_major2d(w9), w) and all(torch.equal(w9[3 * dy + dx], w[:, :, dy, dx])
                                                                                 for dy in range(3) for dx in range(3))


@pytest.mark.parametrize("over", (dict(dropout=0.1), dict(conv_shortcut=True), dict(resamp_with_conv=False), dict(give_pre_end=True), dict(ch=48),
                                  dict(z_channels=16), dict(out_ch=5)), ids=lambda o: next(iter(o)))
def test_decoder_refuses_what_is_not_built(over):
    from ofasys_amd.module.vqgan import Decoder
    with pytest.raises(ValueError, match="VQGAN Decoder"):
        Decoder(**dict(C.TINY["ddconfig"], **over))


def test_checkpoint_and_yaml_loading(tmp_path):
    import yaml
    from ofasys_amd import VQGANTokenizer
    cfg = {"model": {"params": dict(C.TINY, ddconfig=dict(C.TINY["ddconfig"], ch_mult=[1, 2]), lossconfig={"target": "x"})}}
    (tmp_path / "model.yaml").write_text(yaml.safe_dump(cfg))
    state = {k: torch.randn_like(v) for k, v in VQGANTokenizer(C.TINY).vqgan.state_dict().items()}
    assert {"quantize.embed.weight", "post_quant_conv.bias", "decoder.up.0.block.0.nin_shortcut.weight", "decoder.up.1.attn.1.proj_out.bias",
            "decoder.up.1.upsample.conv.weight", "decoder.mid.attn_1.q.weight", "decoder.norm_out.weight"} <= set(state)
    extra = {"encoder.conv_in.weight": torch.zeros(1), "loss.logvar": torch.zeros(1), "quant_conv.bias": torch.zeros(1), "quantize.proj.bias": torch.zeros(1)}
    torch.save({"state_dict": dict(state, **extra)}, tmp_path / "last.ckpt")
    tok = VQGANTokenizer(str(tmp_path / "model.yaml"), str(tmp_path / "last.ckpt"), 16, 2, fp16=True)
    got = tok.vqgan.state_dict()
    assert tok.dtype == torch.float16 and all(torch.equal(got[k].cpu(), v.half()) for k, v in state.items())
    for bad in (dict(state, **{"decoder.temb.weight": torch.zeros(1)}), {k: v for k, v in state.items() if k != "decoder.conv_out.bias"}):
        torch.save({"state_dict": bad}, tmp_path / "bad.ckpt")
        with pytest.raises(RuntimeError, match="decoder"):
            VQGANTokenizer(C.TINY, str(tmp_path / "bad.ckpt"), 16, 2)
    with pytest.raises(ValueError, match="no fp32 kernel"):
        VQGANTokenizer(C.TINY, dtype=torch.float32)


def test_decode_semantics_and_encode():
    from ofasys_amd import VQGANTokenizer
    tok, seen = VQGANTokenizer(C.TINY, None, code_image_size=16, vqgan_factor=2), []
    assert tok.dtype == torch.bfloat16
    state = {k: v.double().cpu() for k, v in tok.vqgan.state_dict().items()}

    def restated(codes):
        seen.append(codes.cpu())
        return C.decode_code(state, C.TINY, codes.cpu(), torch.zeros(1, dtype=torch.float64)).float()
    tok.vqgan.decode_code = restated
    tokens = torch.randint(0, 64, (2, 65), generator=torch.Generator().manual_seed(0))
    tokens[0, :3], tokens[1, 5], tokens[:, 64] = torch.tensor([-7, 64, 1000]), -1, 99
    x = tok.decode(tokens, return_pil=False)
    assert x.shape == (2, 3, 16, 16) and x.dtype == torch.float32
    assert seen[0].shape == (2, 8, 8) and torch.equal(seen[0].reshape(2, 64), tokens[:, :64].clamp(0, 63))
    images = tok.decode(tokens)
    assert len(images) == 2 and all(im.mode == "RGB" and im.size == (16, 16) for im in images)
    want = (255 * ((x.clamp(-1, 1) + 1) / 2)).permute(0, 2, 3, 1).numpy().astype("uint8")              # truncation, as the reference
    assert all((np.asarray(im) == w).all() for im, w in zip(images, want)) and want.std() > 0
    with pytest.raises(NotImplementedError, match="encoder is not built.*Gumbel noise"):
        tok.encode(torch.zeros(1, 3, 16, 16))
