"""CPU: autoregressive speech generation's host-visible rules.  The plain-torch restatement (tests/speech_gen_oracle.py) against the
reference's own run (tests/golden/speech_gen.npz, tools/gen_speech_gen_golden.py) in float64 at 1e-6 relative; the finish rule's edges;
the user surface (Task.build_speech_generator, Task.generator for an [AUDIO:fbank] target, the refusals that fire before the model runs)
and the step kernel's host-only route.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from tests import speech_gen_case as C
from tests import speech_gen_oracle as O
from tests.golden_util import load_golden, rel_err
from tests.model_util import build_model

TOL = 1e-6


@pytest.fixture(scope="module")
def golden():
    return load_golden("speech_gen")


@pytest.fixture(scope="module")
def models():
    return {entry: build_model(C.case(entry)) for entry in C.ENTRIES}


def _postnet_state(model):
    return {k: v.detach().double() for k, v in model.decoder.adaptor.audio_fbank.postnet.state_dict().items()}


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("entry", list(C.ENTRIES))
def test_restatement_reproduces_the_reference(golden, models, entry):
    """out_lens from the recorded probabilities; feature and eos_prob from the recorded pre-postnet frames and the case's weights."""
    g = lambda k: golden[f"{entry}.{k}"]                                        # noqa: E731
    spec = C.ENTRIES[entry]
    n, max_iter, thr = spec["n_frames_per_step"], spec["max_iter"], float(g("threshold")[0])
    p = torch.from_numpy(g("eos_prob_all"))
    out_lens, T_run = O.finish_rule(p, thr, max_iter)
    assert out_lens.tolist() == g("out_lens").tolist() and T_run == p.shape[1] == g("feature_out").shape[1]
    state = _postnet_state(models[entry][0])
    rows = O.finalize(torch.from_numpy(g("feature_out")).double(), p.double(), None, out_lens, T_run, n,
                      lambda x: O.postnet(x, state, 3), golden["gcmvn_mean"], golden["gcmvn_std"])
    for b, row in enumerate(rows):
        assert row["feature"].shape == g(f"feature.{b}").shape == (int(out_lens[b]) * n, C.RAW)
        assert rel_err(row["feature"], g(f"feature.{b}")) < TOL and rel_err(row["eos_prob"], g(f"eos_prob.{b}")) < TOL
        # the reference keeps the FIRST step's attention map: n columns, and a row's kept part of them
        assert g(f"attn.{b}").shape == (C.TEXT_SHAPE[1], min(n, int(out_lens[b]) * n)) and g(f"alignment.{b}").shape[0] == g(f"attn.{b}").shape[1]
    # the case pins the window: the early row's kept frames depend on what it generated AFTER finishing
    early = int(out_lens.argmin())
    cut = torch.from_numpy(g("feature_out")).double().clone()
    cut[early, int(out_lens[early]):] = 0
    other = O.finalize(cut, p.double(), None, out_lens, T_run, n, lambda x: O.postnet(x, state, 3), golden["gcmvn_mean"], golden["gcmvn_std"])
    assert rel_err(other[early]["feature"], g(f"feature.{early}")) > 1e-3


def test_the_fixture_meets_its_margin_condition(golden):
    for entry, spec in C.ENTRIES.items():
        p, thr = torch.from_numpy(golden[f"{entry}.eos_prob_all"]), float(golden[f"{entry}.threshold"][0])
        lens = golden[f"{entry}.out_lens"].tolist()
        kinds = sorted("early" if l <= 2 else ("never" if l == spec["max_iter"] and not bool((p[b] > thr).any()) else "middle")
                       for b, l in enumerate(lens))
        assert kinds == ["early", "middle", "never"], (entry, lens)


def test_finish_rule_edges():
    thr = 0.5
    p = torch.tensor([[0.5, 0.5, 0.6, 0.9], [0.1, 0.2, 0.3, 0.50001], [0.9, 0.0, 0.0, 0.0]])
    out_lens, T_run = O.finish_rule(p, thr, 4)
    assert out_lens.tolist() == [3, 4, 1] and T_run == 4        # p == threshold does not finish; a finish at the last step; at step 0
    out_lens, T_run = O.finish_rule(torch.full((2, 5), 0.5), thr, 5)
    assert out_lens.tolist() == [5, 5] and T_run == 5           # nobody finishes: every row keeps max_iter, the loop runs it all
    out_lens, T_run = O.finish_rule(torch.tensor([[0.9, 0.0, 0.0], [0.0, 0.9, 0.9]]), thr, 3)
    assert out_lens.tolist() == [1, 2] and T_run == 2           # the loop stops with the last finisher; a finished row keeps its length
    pad = O.padding_flags(torch.tensor([[0.9, 0.0, 0.0], [0.0, 0.0, 0.9]]), thr, 3)
    assert pad.tolist() == [[False, True, True], [False, False, False]]        # the flag lags the finish by one position


def test_gcmvn_from_a_local_statistics_file(tmp_path):
    from ofasys_amd import Dictionary, SpeechGenerator
    mean, std = C.gcmvn_stats()
    path = tmp_path / "gcmvn_stats.npz"
    np.savez(path, mean=mean, std=std)
    gen = SpeechGenerator(Dictionary(), stats_npz_path=str(path))
    x = torch.randn(2, 5, C.RAW, dtype=torch.float64)
    want = x * torch.from_numpy(std).double().view(1, 1, -1) + torch.from_numpy(mean).double().view(1, 1, -1)
    assert rel_err(gen.gcmvn_denormalize(x), want) < 1e-12
    assert SpeechGenerator(Dictionary()).gcmvn_denormalize(x) is x
    rows = O.finalize(x, torch.rand(2, 5).double(), None, torch.tensor([5, 2]), 5, 1, lambda t: torch.zeros_like(t), mean, std)
    assert rel_err(rows[1]["feature"], want[1, :2]) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ the user surface
def _task(instruction="[TEXT:src] -> [AUDIO:fbank]"):
    from ofasys_amd import Dictionary, Task
    t = Task(name="tts", instruction=instruction)
    t.initialize(Dictionary())
    return t


def test_build_speech_generator_defaults_and_pops(tmp_path):
    from ofasys_amd import AutoRegressiveSpeechGenerator
    t = _task()
    g = t.build_speech_generator()
    assert isinstance(g, AutoRegressiveSpeechGenerator)
    assert (g.max_iter, g.eos_prob_threshold, g.gcmvn_stats, g.use_graph, g.fused_step) == (1500, 0.5, None, True, True)
    kw = {"max_iter": 40, "eos_prob_threshold": 0.25, "beam": 5, "max_len_b": 32}
    g = t.build_speech_generator(**kw)                              # (the shared default JSON's beam arguments are ignored, as there)
    assert (g.max_iter, g.eos_prob_threshold) == (40, 0.25)
    mean, std = C.gcmvn_stats()
    np.savez(tmp_path / "s.npz", mean=mean, std=std)
    g = t.build_speech_generator(stats_npz_path=str(tmp_path / "s.npz"), fused_step=False)
    assert g.gcmvn_stats["mean"].shape == (C.RAW,) and g.fused_step is False


def test_task_generator_for_an_audio_target_is_the_speech_generator():
    from ofasys_amd import AutoRegressiveSpeechGenerator, ModalityType
    t = _task()
    assert t.target_modality == ModalityType.AUDIO
    gen = t.generator
    assert isinstance(gen, AutoRegressiveSpeechGenerator) and gen is t.generator and gen.max_iter == 1500
    t2 = _task()
    t2.cfg.evaluation.generator_args = '{"max_iter": 12, "eos_prob_threshold": 0.4}'
    assert (t2.generator.max_iter, t2.generator.eos_prob_threshold) == (12, 0.4)
    other = _task("[TEXT:src] -> [BOX:box]")                        # other non-TEXT targets keep raising
    with pytest.raises(NotImplementedError, match="not implemented"):
        other.generator


def _sample(d, target_modality="AUDIO"):
    from ofasys_amd import ModalityType, Slot
    return {"net_input": {"slots": [Slot(ModalityType.TEXT, True, C.source_tokens(len(d))),
                                    Slot(ModalityType[target_modality], False, None)]}}


def test_max_iter_limits_are_checked_before_the_model_runs(models):
    from ofasys_amd import AutoRegressiveSpeechGenerator
    import copy
    model, d = models["n1"]
    ad = model.decoder.adaptor.audio_fbank
    positions = ad.embed_audio_positions.weight.shape[0]
    with pytest.raises(ValueError, match=f"max_iter={positions + 1} exceeds embed_audio_positions"):
        AutoRegressiveSpeechGenerator(d, max_iter=positions + 1).generate(model, _sample(d))
    m2 = copy.deepcopy(model)
    a2 = m2.decoder.adaptor.audio_fbank
    a2.audio_rp_bucket = a2.audio_rp_bucket[:8, :8].contiguous()
    with pytest.raises(ValueError, match="max_iter=12 exceeds audio_rp_bucket"):
        AutoRegressiveSpeechGenerator(d, max_iter=12).generate(m2, _sample(d))
    m3 = copy.deepcopy(model)
    m3.decoder.cfg.max_target_positions = 8
    with pytest.raises(ValueError, match="max_iter=12 exceeds the decoder's max_target_positions"):
        AutoRegressiveSpeechGenerator(d, max_iter=12).generate(m3, _sample(d))


def test_a_target_that_is_not_audio_is_refused_with_the_reference_message(models):
    from ofasys_amd import AutoRegressiveSpeechGenerator
    model, d = models["n1"]
    with pytest.raises(AssertionError, match="the target slot does not match the generator.*AutoRegressiveSpeechGenerator"):
        AutoRegressiveSpeechGenerator(d, max_iter=4).generate(model, _sample(d, "TEXT"))


def test_outputs_save_fbank_and_audio_needs_soundfile(tmp_path):
    from ofasys_amd import SpeechGeneratorOutput
    o = SpeechGeneratorOutput(feature=torch.ones(3, 80), eos_prob=torch.zeros(3), attn=torch.zeros(4, 3), alignment=torch.zeros(3).long(),
                              targ_feature=torch.zeros(2, 80))
    o.save_fbank(str(tmp_path / "a"))
    o.save_fbank(str(tmp_path / "b.npy"), target=True)
    assert np.load(tmp_path / "a.npy").shape == (3, 80) and np.load(tmp_path / "b.npy").shape == (2, 80)
    assert o.waveform is None and o.text is None


def test_step_kernel_route_is_host_only():
    """Which shapes ofa_speech_step serves (include/ofasys_amd.h): multiples of 8, 1..4 prenet layers, the rows of a workgroup in LDS."""
    from ofasys_amd import kernels as K
    assert K.speech_step_rows() == 4
    assert K.speech_step_ok(768, 80, 256, 768, 2, torch.bfloat16) and K.speech_step_ok(256, 160, 64, 256, 1, torch.float32)
    assert K.speech_step_ok(1024, 80, 256, 1024, 4, torch.float16)
    assert not K.speech_step_ok(768, 84, 256, 768, 2, torch.bfloat16)          # out_dim % 8
    assert not K.speech_step_ok(768, 80, 256, 768, 5, torch.bfloat16)          # a layer count it was not built for
    assert not K.speech_step_ok(768, 80, 256, 768, 0, torch.bfloat16)
    assert not K.speech_step_ok(4096, 80, 256, 4096, 2, torch.bfloat16)        # 2 x 4 rows x 4096 floats exceed the LDS
    assert not K.speech_step_ok(768, 80, 256, 768, 2, torch.int32)
