"""GPU: the HiFi-GAN vocoder's kernels (csrc/vocoder.hip) and its way to the user.

* The convolution and the transposed convolution BIT FOR BIT against the float64 restatement run one utterance at a time, on the
  exact cases of tests/vocoder_case.py (small integers: every fp32 partial sum is exact in any order; tests/test_vocoder_cpu.py proves
  the results representable).  Rows past a sample's end hold 3s in every input and must come out as zeros, untouched by them.
* conv_post per element within the bound of its fp32 fma chain: n = 7 C products, each exact in fp32, so |error of the sum| <=
  n 2^-24 S with S the sum of the products' magnitudes; tanh is 1-Lipschitz and tanhf is good to a few ulp of a value <= 1 (4 x 2^-24).
* A whole tiny generator: its relative error against float64 at most 2 x the error of torch's own device composite in the same 16-bit
  dtype on the same inputs (the project's factor), both printed; and the ragged batch equal, bit for bit, to its
  utterances run alone.
* Task.inference on the tiny text-to-speech model with a tiny vocoder: waveforms fp32, on the CPU, hop x out_len long, equal to the
  vocoder called on the features."""
import json

import pytest
import torch
import torch.nn.functional as F

from tests import vocoder_case as C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _tile(*shape):
    from ofasys_amd import kernels as K
    return K.vocoder_conv_tile(*shape)


def _dev(t, dtype):
    return None if t is None else t.to(dtype).to(DEV)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("case", C.conv_cases(_tile), ids=lambda c: c[0])
def test_conv_bit_for_bit(case, name):
    from ofasys_amd import ops
    from ofasys_amd.module.hifigan import tap_major
    dtype, t = DTYPES[name], C.exact_conv(case)
    lens = torch.tensor(t["lens"], dtype=torch.int32, device=DEV)
    out = _dev(t["y0"], dtype)
    got = ops.vocoder_conv(_dev(t["x"], dtype), _dev(tap_major(t["w"]), dtype), _dev(t["b"], dtype), d=t["d"], lens=lens, slope=t["slope"],
                           res=_dev(t["res"], dtype), out=out, accum=out is not None, out_scale=t["scale"])
    assert got.dtype == dtype and torch.equal(got.double().cpu(), t["want"])
    if t["lens"][0] == case[5] and t["y0"] is None:                       # lens = NULL: sample 0 is full, the same bits for it
        full = ops.vocoder_conv(_dev(t["x"][:1], dtype), _dev(tap_major(t["w"]), dtype), _dev(t["b"], dtype), d=t["d"], slope=t["slope"],
                                res=_dev(None if t["res"] is None else t["res"][:1], dtype), out_scale=t["scale"])
        assert torch.equal(full, got[:1])


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("case", C.UP_CASES, ids=lambda c: c[0])
def test_upsample_bit_for_bit(case, name):
    from ofasys_amd import ops
    from ofasys_amd.module.hifigan import polyphase_weight
    dtype, t = DTYPES[name], C.exact_upsample(case)
    lens = torch.tensor(t["lens"], dtype=torch.int32, device=DEV)
    got = ops.vocoder_upsample(_dev(t["x"], dtype), _dev(polyphase_weight(t["wt"], t["u"]), dtype), _dev(t["b"].repeat(t["u"]), dtype), t["u"],
                               lens=lens, slope=0.5)
    assert got.shape == t["want"].shape and torch.equal(got.double().cpu(), t["want"])


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("Cn", (16, 32))
def test_conv_post_within_its_fma_bound(Cn, name):
    from ofasys_amd import ops
    dtype, gen, L, lens = DTYPES[name], torch.Generator().manual_seed(Cn), 300, (300, 257)     # two workgroups; one ends inside the second
    x = torch.randn(2, L, Cn, generator=gen).to(dtype)
    w, b = (torch.randn(1, Cn, 7, generator=gen) / (7 * Cn) ** 0.5).to(dtype), (torch.randn(1, generator=gen) * 0.1).to(dtype)
    got = ops.vocoder_post(x.to(DEV), w[0].t().contiguous().to(DEV), b.to(DEV), lens=torch.tensor(lens, dtype=torch.int32, device=DEV)).cpu()
    act, x64 = (lambda v: C.lrelu(v, 0.01)), x.double()                   # noqa: E731  (fp32 in the kernel: the activation is not rounded to 16 bits)
    want = C.ragged(lambda u: torch.tanh(F.conv1d(act(u).t()[None], w.double(), b.double(), padding=3))[0].t(), x64, lens).squeeze(-1)
    S = C.ragged(lambda u: F.conv1d(act(u).abs().t()[None], w.double().abs(), b.double().abs(), padding=3)[0].t(), x64, lens).squeeze(-1)
    # (+ the activation's own fp32 rounding of 0.01 v: one more 2^-24 relative on every product)
    bound = (7 * Cn + 2) * 2.0 ** -24 * S + 4 * 2.0 ** -24
    err = (got.double() - want).abs()
    print(f"conv_post {name} C={Cn}: max error {float(err.max()):.3e}, max of the bound {float(bound.max()):.3e}")
    assert got.dtype == torch.float32 and bool((err <= bound).all()) and float(got[1, 257:].abs().max()) == 0.0


@pytest.fixture(scope="module")
def tiny():
    """The tiny generator's state, a ragged batch [2, 12, 80] with lengths (12, 7) and its float64 waveforms, one utterance at a time."""
    state, gen, lens = C.generator_state(C.TINY), torch.Generator().manual_seed(1), (12, 7)
    x = torch.randn(2, 12, 80, generator=gen)
    ref = [C.generator({k: v.double() for k, v in state.items()}, C.TINY, x[b, :l].t()[None].double())[0, 0] for b, l in enumerate(lens)]
    return state, x, lens, ref


def _vocoder(state, cfg, tmp_path, dtype):
    from ofasys_amd import HiFiGANVocoder
    torch.save({"generator": state}, tmp_path / "g.pt")
    return HiFiGANVocoder(str(tmp_path / "g.pt"), cfg, dtype=dtype).to(DEV)


@pytest.mark.parametrize("name", list(DTYPES))
def test_tiny_generator_parity_and_ragged_batch(tiny, tmp_path, name):
    state, x, lens, ref = tiny
    dtype = DTYPES[name]
    voc = _vocoder(state, C.TINY, tmp_path, dtype)
    xd = x.to(dtype).to(DEV)
    got = voc(xd, lengths=lens)
    assert got.shape == (2, 1, 48) and got.dtype == torch.float32
    alone = [voc(xd[b, :l]) for b, l in enumerate(lens)]                   # T x 80 -> 1 x 4 T, the reference's single-utterance form
    torch_arm = [C.generator({k: v.to(DEV) for k, v in state.items()}, C.TINY, xd[b, :l].t()[None])[0, 0] for b, l in enumerate(lens)]
    want = torch.cat(ref)
    e_new, e_torch = C.rel(torch.cat([a[0] for a in alone]), want), C.rel(torch.cat(torch_arm).float(), want)
    print(f"tiny generator {name}: relative error {e_new:.3e}, torch's device composite {e_torch:.3e} (bound {2 * e_torch:.3e})")
    assert e_new <= 2 * e_torch
    for b, l in enumerate(lens):
        assert alone[b].shape == (1, 4 * l) and torch.equal(got[b, 0, :4 * l], alone[b][0]) and float(got[b, 0, 4 * l:].abs().sum()) == 0.0


def test_task_inference_returns_waveforms(tmp_path):
    from ofasys_amd import ModalityType, Slot, Task
    from tests import speech_gen_case as S
    from tests.golden_util import load_golden
    from tests.model_util import build_model
    golden, entry, dtype = load_golden("speech_gen"), "n1", torch.bfloat16
    model, d = build_model(S.case(entry))
    S.apply_eos_affine(model, torch.from_numpy(golden[f"{entry}.eos_scale"]), float(golden[f"{entry}.eos_bias"][0]))
    model = model.to(DEV).to(dtype).eval()
    tgt, tgt_lens = S.target(entry)
    sample = {"net_input": {"slots": [Slot(ModalityType.TEXT, True, S.source_tokens(len(d)).to(DEV)), Slot(ModalityType.AUDIO, False, None)]},
              "target": tgt.to(dtype).to(DEV), "target_lengths": tgt_lens.to(DEV)}
    torch.save({"generator": C.generator_state(C.TINY)}, tmp_path / "g.pt")
    (tmp_path / "g.json").write_text(json.dumps(C.TINY))
    task = Task(name="tts", instruction="[TEXT:src] -> [AUDIO:fbank]")
    task.global_dict = d
    task.cfg.evaluation.generator_args = json.dumps({"max_iter": S.ENTRIES[entry]["max_iter"], "eos_prob_threshold": float(golden[f"{entry}.threshold"][0]),
                                                     "vocoder_config": str(tmp_path / "g.json"), "vocoder_checkpoint": str(tmp_path / "g.pt"),
                                                     "vocoder_dtype": "bfloat16"})
    outs = task.inference(model, sample, has_targ=True)
    voc = task.generator.vocoder
    assert [o.feature.shape[0] for o in outs] == golden[f"{entry}.out_lens"].tolist() and voc.hop == 4
    for o in outs:
        for wav, feat in ((o.waveform, o.feature), (o.targ_waveform, o.targ_feature)):
            assert wav.dtype == torch.float32 and not wav.is_cuda and wav.shape == (4 * feat.shape[0],)
            assert torch.equal(wav, voc(feat.to(DEV))[0].cpu()) and float(wav.abs().max()) > 0
