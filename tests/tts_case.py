"""The text-to-speech fixture's case, shared by tools/gen_tts_golden.py (which runs the REFERENCE on it, CPU) and the tests
(tests/test_tts_cpu.py, tests/test_tts_step_gpu.py).  TEST INFRASTRUCTURE: plain data and recipe lookups, nothing of the kernels.

An arch-`tiny` model with `text` and `audio_fbank` active, every dropout 0 (train mode is then deterministic; BatchNorm takes batch
statistics), a 3-layer postnet of 32 channels -- a first, a tanh-middle and a last layer -- on [TEXT] -> [AUDIO:fbank], B = 3, frame
lengths [11, 7, 1] (a full-length sample, a middle value, a single frame), F = 80, text lengths <= 9."""
import torch

from oracle import recipe

B, F = 3, 80
FRAME_LENGTHS = [11, 7, 1]
TEXT_SHAPE, TEXT_LENGTHS = (B, 9), [9, 6, 4]
BCE_POS_WEIGHT = 5.5
PACK_N = 2                      # pack_frames is recorded for n_frames_per_step = 2 on sample 0 (11 frames: the odd one dropped)
GRAD_SAMPLES = 509

CASE = dict(
    arch="tiny", active={"text", "audio_fbank"}, overrides={"dropout": 0.0},
    adaptor_overrides={"audio_fbank": {"prenet_dropout": 0.0, "postnet_dropout": 0.0, "postnet_conv_dim": 32, "postnet_layers": 3}},
)
PREFIX = "decoder.adaptor.audio_fbank."


def frames():
    """The per-sample target frames [L_i, F] (fp32), as a dataset row would hold them."""
    return [recipe.floats(f"input.tts.fbank.{i}", (n, F)) for i, n in enumerate(FRAME_LENGTHS)]


def source_tokens(vocab):
    return recipe.tokens("input.tts.src", TEXT_SHAPE, vocab, TEXT_LENGTHS)


def stride_of(numel):
    return max(1, numel // GRAD_SAMPLES)


def sample(t):
    """The recorded form of a gradient: evenly strided elements of the flattened tensor."""
    flat = t.detach().reshape(-1)
    return flat[::stride_of(flat.numel())]


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
