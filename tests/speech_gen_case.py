"""The speech-generation fixture's case, shared by tools/gen_speech_gen_golden.py (which runs the REFERENCE's own
AutoRegressiveSpeechGenerator on it, CPU, fp32) and the tests (tests/test_speech_gen_cpu.py, tests/test_speech_gen_gpu.py).
TEST INFRASTRUCTURE: plain data and recipe lookups, nothing of the kernels.

The text-to-speech case's model (arch `tiny`, `text` + `audio_fbank`, every dropout 0 including the prenet's, a 3-layer postnet of 32
channels) on [TEXT] -> [AUDIO:fbank], B = 3, text lengths 9 / 6 / 4.  Two entries: `n1` (one frame per step, max_iter 12) and `n2`
(n_frames_per_step = 2, out_dim 160, max_iter 6: the reshape and the three repeat_interleaves).  The tool records, per entry, the
`eos_prob_threshold` and the scale (one factor per input channel) and bias it applied to `eos_proj` after recipe.fill_state so that
the three rows end differently -- one at step 0 or 1, one in the middle, one never; they are DATA of the fixture
(golden["<entry>.eos_scale"], ["<entry>.eos_bias"], ["<entry>.threshold"]).  (One scalar factor cannot do it: under the recipe's weights
the three rows' logits rise together.)"""
import torch

from oracle import recipe
from tests import tts_case as T

B, RAW = 3, 80
TEXT_SHAPE, TEXT_LENGTHS = T.TEXT_SHAPE, T.TEXT_LENGTHS
TARGET_FRAMES, TARGET_LENGTHS = 5, [5, 3, 2]          # the `has_targ` target: [B, 5, out_dim], lengths in steps
MARGIN = 20.0                                         # |eos_prob - threshold| >= MARGIN x the reference's own bf16 gap on eos_prob
PREFIX = T.PREFIX

ENTRIES = {
    "n1": dict(n_frames_per_step=1, max_iter=12),
    "n2": dict(n_frames_per_step=2, max_iter=6),
}


def case(entry):
    """The model case of an entry (the text-to-speech case, with the entry's n_frames_per_step)."""
    audio = dict(T.CASE["adaptor_overrides"]["audio_fbank"], n_frames_per_step=ENTRIES[entry]["n_frames_per_step"])
    return dict(T.CASE, adaptor_overrides={"audio_fbank": audio})


def out_dim(entry):
    return RAW * ENTRIES[entry]["n_frames_per_step"]


def source_tokens(vocab):
    return recipe.tokens("input.speech_gen.src", TEXT_SHAPE, vocab, TEXT_LENGTHS)


def target(entry):
    """(target [B, TARGET_FRAMES, out_dim] fp32, target_lengths [B]) of the `has_targ` run."""
    return recipe.floats(f"input.speech_gen.target.{entry}", (B, TARGET_FRAMES, out_dim(entry))), torch.tensor(TARGET_LENGTHS)


def gcmvn_stats():
    """(mean [RAW], std [RAW]) float32 numpy arrays of the local statistics file."""
    mean = recipe.floats("input.speech_gen.gcmvn.mean", (RAW,), 0.5)
    std = recipe.floats("input.speech_gen.gcmvn.std", (RAW,), 0.25).abs() + 0.5
    return mean.numpy(), std.numpy()


def apply_eos_affine(model, scale, bias, prefix=PREFIX):
    """eos_proj.weight <- scale * eos_proj.weight (per input channel, scale [D] float64), eos_proj.bias <- eos_proj.bias + bias: the
    recorded change to the recipe's weights, applied to the fp32 model before any dtype conversion."""
    sd = model.state_dict()
    with torch.no_grad():
        w, b = sd[prefix + "eos_proj.weight"], sd[prefix + "eos_proj.bias"]
        w.copy_((w.double() * torch.as_tensor(scale, dtype=torch.float64).view(1, -1)).to(w.dtype))
        b.copy_((b.double() + float(bias)).to(b.dtype))


def batch(rows):
    """The rows' (ragged) tensors of one output kind as ONE flat fp32 tensor: what a bf16 gap and a bf16 comparison are taken over, like the
    whole-batch tensors of the text-to-speech fixture."""
    return torch.cat([torch.as_tensor(r).detach().float().reshape(-1) for r in rows])


rel = T.rel
