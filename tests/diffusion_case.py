"""The motion-diffusion fixture shared by tests/test_diffusion_cpu.py and tests/test_diffusion_step_gpu.py.  TEST INFRASTRUCTURE: plain
data and recipe lookups, nothing of the kernels.

A model of 2 + 2 layers, D = 64, 4 heads, every dropout 0, `text` and `motion_6d` active (max_data_dim 32, 64 noise levels), on
[TEXT] -> [MOTION:...,adaptor=motion_6d]: a text source of 7 tokens, B = 3 target sentences of [9, 1, 6] frames (a full-length one,
a single frame, a middle value) with Dd = 18 columns (two joints), a 50-level cosine schedule, noise and levels supplied."""
import torch

from oracle import recipe

B, DD, T = 3, 18, 9
LENGTHS = [9, 1, 6]
TEXT_SHAPE, TEXT_LENGTHS = (B, 7), [7, 5, 3]
LEVELS = [0, 49, 17]                    # the first, the last and a middle level of the 50
N_LEVELS = 50
DIFFUSER_ARGS = {"num_train_timesteps": N_LEVELS}

CASE = dict(
    arch="tiny", active={"text", "motion_6d"},
    overrides={"dropout": 0.0, "encoder_layers": 2, "decoder_layers": 2, "encoder_embed_dim": 64, "decoder_embed_dim": 64,
               "encoder_ffn_embed_dim": 256, "decoder_ffn_embed_dim": 256, "encoder_attention_heads": 4, "decoder_attention_heads": 4,
               "decoder_input_dim": 64, "decoder_output_dim": 64},
    adaptor_overrides={"motion_6d": {"max_data_dim": 32, "max_noise_levels": 64}},
)
PREFIX = "decoder.adaptor.motion_6d."
ADAPTOR_KEYS = ("frame_encoder.0.weight", "frame_encoder.0.bias", "frame_encoder.2.weight", "frame_encoder.2.bias",
                "frame_decoder.0.weight", "frame_decoder.0.bias", "frame_decoder.2.weight", "frame_decoder.2.bias",
                "noise_level_emb.weight")


def masks():
    return torch.arange(T).unsqueeze(0) >= torch.tensor(LENGTHS).unsqueeze(1)


def frames():
    """x0 fp32 [B, T, Dd], zero at padded frames (as the collation leaves them)."""
    x = recipe.floats("input.diffusion.x0", (B, T, DD))
    return x.masked_fill(masks().unsqueeze(-1), 0.0)


def noise():
    return recipe.floats("input.diffusion.noise", (B, T, DD))


def levels():
    return torch.tensor(LEVELS, dtype=torch.long)


def source_tokens(vocab):
    return recipe.tokens("input.diffusion.src", TEXT_SHAPE, vocab, TEXT_LENGTHS)
