"""CPU: the HiFi-GAN vocoder's host side.  The header declares and the library exports the entry points, which refuse bad shapes and
dtypes with their status codes before any launch; the polyphase arrangement of a transposed convolution and the weight-norm folding
against torch in float64; checkpoint loading; the exact cases of the GPU suite are exact (tests/vocoder_case.py); and without a vocoder
Task.build_speech_generator is what it was.  Nothing here needs a GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import vocoder_case as C

INVALID, UNSUPPORTED = 1, 2                              # OFA_ERR_INVALID, OFA_ERR_UNSUPPORTED
F32, BF16, F16 = 0, 1, 2


def _call(name, **over):
    """An entry point on NULL operands and B = 0 (nothing can launch), one argument changed at a time -> its status code."""
    from ofasys_amd.lib import lib
    base = {"ofa_vocoder_conv": dict(x=None, w=None, bias=None, res=None, y=None, lens=None, B=0, L=8, Cin=32, Cout=32, k=3, d=1, len_scale=1,
                                     slope=0.1, accum=0, out_scale=1.0, dtype=F16, stream=None),
            "ofa_vocoder_upsample": dict(x=None, w=None, bias=None, y=None, lens=None, B=0, L=8, Cin=32, Cout=16, u=2, len_scale=1, slope=0.1,
                                         dtype=F16, stream=None),
            "ofa_vocoder_post": dict(x=None, w=None, bias=None, out=None, lens=None, B=0, L=8, C=32, k=7, len_scale=1, slope=0.01, dtype=F16,
                                     stream=None)}[name]
    assert set(over) <= set(base)
    return getattr(lib().cdll, name)(*dict(base, **over).values())


REFUSALS = [("ofa_vocoder_conv", {}, 0), ("ofa_vocoder_conv", dict(dtype=F32), UNSUPPORTED), ("ofa_vocoder_conv", dict(dtype=7), INVALID),
            ("ofa_vocoder_conv", dict(Cin=40), UNSUPPORTED), ("ofa_vocoder_conv", dict(Cout=528), UNSUPPORTED),
            ("ofa_vocoder_conv", dict(Cin=80, dtype=BF16), 0), ("ofa_vocoder_conv", dict(k=4), UNSUPPORTED),
            ("ofa_vocoder_conv", dict(k=11, d=6), UNSUPPORTED), ("ofa_vocoder_conv", dict(k=11, d=5), 0),
            ("ofa_vocoder_conv", dict(L=0), INVALID), ("ofa_vocoder_conv", dict(len_scale=0), INVALID),
            ("ofa_vocoder_conv", dict(B=1), INVALID),                       # null operands with something to do
            ("ofa_vocoder_upsample", {}, 0), ("ofa_vocoder_upsample", dict(u=3), UNSUPPORTED), ("ofa_vocoder_upsample", dict(Cout=24), UNSUPPORTED),
            ("ofa_vocoder_upsample", dict(dtype=F32), UNSUPPORTED), ("ofa_vocoder_upsample", dict(u=8, Cout=256, Cin=512), 0),
            ("ofa_vocoder_post", {}, 0), ("ofa_vocoder_post", dict(C=64), UNSUPPORTED), ("ofa_vocoder_post", dict(k=9), UNSUPPORTED),
            ("ofa_vocoder_post", dict(dtype=F32), UNSUPPORTED), ("ofa_vocoder_post", dict(B=2), INVALID)]


@pytest.mark.parametrize("name,over,want", REFUSALS, ids=[f"{n[12:]}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'ok'}" for n, o, _ in REFUSALS])
def test_entry_points_refuse_before_any_launch(name, over, want):
    from ofasys_amd.lib import lib
    nargs = {"ofa_vocoder_conv": 18, "ofa_vocoder_upsample": 14, "ofa_vocoder_post": 13, "ofa_vocoder_conv_tile": 4, "ofa_vocoder_post_tile": 0}
    for n, count in nargs.items():
        assert n in lib().protos and len(lib().protos[n][1]) == count, n
    assert _call(name, **over) == want
    if want:
        assert lib().cdll.ofa_last_error().decode().startswith(name[4:])


def test_tiles_are_host_only():
    from ofasys_amd import kernels as K
    # NT waves over the channels, 4 / NT over time, MT tiles each: the largest image under 80 KiB
    assert [K.vocoder_conv_tile(*s) for s in ((32, 32, 3, 1), (64, 64, 7, 3), (128, 128, 11, 5), (256, 256, 11, 5), (512, 2048, 3, 1))] == \
        [512, 256, 128, 64, 64]
    assert K.vocoder_conv_tile(40, 32, 3, 1) == 0 and K.vocoder_conv_tile(32, 32, 4, 1) == 0 and K.vocoder_post_tile() == 256


@pytest.mark.parametrize("u", (8, 2))
def test_polyphase_weight_reproduces_conv_transpose1d(u):
    from ofasys_amd.module.hifigan import polyphase_weight
    gen = torch.Generator().manual_seed(u)
    wt, x, b = torch.randn(6, 4, 2 * u, generator=gen).double(), torch.randn(2, 6, 5, generator=gen).double(), torch.randn(4, generator=gen).double()
    want = F.conv_transpose1d(x, wt, b, stride=u, padding=u // 2)                       # [B, Cout, L u]
    w3 = polyphase_weight(wt, u)                                                         # [3, u Cout, Cin]: a 3-tap Conv1d, tap-major
    got = F.conv1d(x, w3.permute(1, 2, 0), b.repeat(u), padding=1)                       # [B, u Cout, L]: row q = output rows q u .. q u + u - 1
    got = got.view(2, u, 4, 5).permute(0, 2, 3, 1).reshape(2, 4, 5 * u)
    assert C.rel(got, want) < 1e-14
    assert int((w3 == 0).sum()) == w3.numel() // 3


@pytest.mark.parametrize("kind", ("conv", "transposed"))
def test_weight_norm_folding_and_checkpoint_loading(kind, tmp_path):
    from ofasys_amd import HiFiGANVocoder
    from ofasys_amd.module.hifigan import fold_weight_norm, polyphase_weight, tap_major
    layer = torch.nn.Conv1d(64, 32, 7) if kind == "conv" else torch.nn.ConvTranspose1d(64, 32, 4, 2, padding=1)
    layer = torch.nn.utils.weight_norm(layer.double())
    g, v = layer.weight_g.detach() * 1.7, layer.weight_v.detach()
    assert g.shape == (v.shape[0], 1, 1) and C.rel(fold_weight_norm(g, v), torch._weight_norm(v, g, 0)) < 1e-14    # (the hook's own function)
    # a checkpoint whose one layer of this kind is weight-normed, the rest plain: the vocoder holds the kernels' layouts
    state = C.generator_state(C.TINY)
    name = "resblocks.0.convs1.1" if kind == "conv" else "ups.0"
    plain = state.pop(name + ".weight").double()
    norm = plain.reshape(plain.shape[0], -1).norm(dim=1).view(-1, 1, 1)
    state[name + ".weight_g"], state[name + ".weight_v"] = norm * 2, plain * 3        # g v / |v| = 2 plain
    torch.save({"generator": state}, tmp_path / "g.pt")
    voc = HiFiGANVocoder(str(tmp_path / "g.pt"), C.TINY, fp16=True)
    held = getattr(voc.model, name.replace(".", "_") + "_w")
    want = tap_major(2 * plain) if kind == "conv" else polyphase_weight(2 * plain, 2)
    assert held.dtype == torch.float16 and held.shape == want.shape and torch.equal(held, want.half())
    assert voc.hop == 4 and torch.equal(voc.model.conv_post_w, state["conv_post.weight"][0].t().half())
    with pytest.raises(ValueError, match="torch.float16.*torch.bfloat16"):
        HiFiGANVocoder(str(tmp_path / "g.pt"), C.TINY)                                  # the reference's default, fp32
    with pytest.raises(KeyError, match="conv_pre"):
        HiFiGANVocoder(None, C.TINY, fp16=True).model.load_state_dict({})


def test_exact_cases_are_exact():
    """What the GPU suite compares bit for bit is representable: every result is exact in bf16 and fp16, every operand as well."""
    from ofasys_amd import kernels as K
    for t in [C.exact_conv(c) for c in C.conv_cases(K.vocoder_conv_tile)] + [C.exact_upsample(c) for c in C.UP_CASES]:
        for dtype in (torch.bfloat16, torch.float16):
            assert torch.equal(t["want"].to(dtype).double(), t["want"]) and float(t["want"].abs().max()) <= 2 * C.NZ + 6
            assert torch.equal(C.lrelu(t["x"], 0.5).to(dtype).double(), C.lrelu(t["x"], 0.5))
        assert float(t["want"].abs().max()) > 2                                         # (and they are not trivially small)


def test_without_a_vocoder_the_speech_generator_is_unchanged():
    from ofasys_amd import AutoRegressiveSpeechGenerator, Dictionary, HiFiGANVocoder, Task
    t = Task(name="tts", instruction="[TEXT:src] -> [AUDIO:fbank]")
    t.initialize(Dictionary())
    g = t.build_speech_generator(max_iter=40)
    assert isinstance(g, AutoRegressiveSpeechGenerator) and g.vocoder is None and g._vocode(None, None) is None and t.generator.vocoder is None
    g = t.build_speech_generator(vocoder_config=C.TINY, vocoder_dtype="bfloat16")
    assert isinstance(g.vocoder, HiFiGANVocoder) and g.vocoder.dtype == torch.bfloat16
    with pytest.raises(ValueError, match="vocoder_checkpoint without vocoder_config"):
        t.build_speech_generator(vocoder_checkpoint="g.pt")
