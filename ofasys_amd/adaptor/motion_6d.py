"""Motion6dAdaptor (reference: adaptor/motion_6d.py:23-129): continuous motion frames (3 hip position + 3 hip velocity + 6 per joint
rotation, "rot6d") in and out of the decoder, for diffusion training.  A frame, zero-padded to `max_data_dim` columns, goes through
frame_encoder (Linear - GELU - Linear); with a noise level the result is modulated by the level's row of `noise_level_emb` (scale |
shift); frame_decoder maps the decoder's features back to `max_data_dim` columns, of which the first data_dim are the prediction.

The slot value is the dict the collation builds (preprocessor/motion.py): "value" [B, T, Dd] and "masks" [B, T], optionally "known_w"
[B, T] with "value_0" (in-betweening: known frames replace the noised ones and take level 0) and "noise_level" int64 [B].  The
diffusion route (criterion.py) hands "value" over already mixed, padded and in the model dtype -- [B, T, max_data_dim] from
ops.diffusion_q_sample, marked by "data_dim" -- so the mix and the padding are not repeated here; a plain float [B, T, Dd] value takes
the reference's own steps.  State-dict keys are the text adaptor's plus frame_encoder.{0,2}, frame_decoder.{0,2} and noise_level_emb."""
from dataclasses import dataclass, field
from typing import Any, Dict

import torch
import torch.nn as nn
from torch import Tensor

from .. import ops
from ..configure import register_config
from ..module import Embedding, OfaLinear
from ..module.layers import OfaEmbedding
from ..preprocessor import Dictionary, ModalityType, Slot
from .base import AdaptorOutput
from .text import TextAdaptor, TextAdaptorConfig


@dataclass
class Motion6dAdaptorConfig(TextAdaptorConfig):
    max_data_dim: int = field(default=512, metadata={"help": "columns of a padded frame"})
    max_noise_levels: int = field(default=1024, metadata={"help": "rows of noise_level_emb: num_train_timesteps + 1 at least"})


class _Gelu(nn.Module):
    """The parameter-free middle of frame_encoder / frame_decoder (index 1 of the reference's nn.Sequential)."""

    def forward(self, x):
        return ops.gelu(x)


def _mlp(d_in, d_mid, d_out):
    return nn.Sequential(OfaLinear(d_in, d_mid), _Gelu(), OfaLinear(d_mid, d_out))


@register_config("ofasys.adaptor", "motion_6d", Motion6dAdaptorConfig)
class Motion6dAdaptor(TextAdaptor):
    def __init__(self, embed_tokens: Embedding, dictionary: Dictionary, is_src: bool, general_adaptor, cfg: Motion6dAdaptorConfig):
        super().__init__(embed_tokens, dictionary, is_src, general_adaptor, cfg)
        if cfg.embed_dim % 8:
            raise ValueError(f"motion_6d: embed_dim {cfg.embed_dim} is not a multiple of 8 (the noise-level modulation reads 16-byte vectors)")
        if cfg.max_data_dim % 8:
            raise ValueError(f"motion_6d: max_data_dim {cfg.max_data_dim} is not a multiple of 8 (the padded frames are GEMM rows)")
        self.max_data_dim, self.max_noise_levels = int(cfg.max_data_dim), int(cfg.max_noise_levels)
        self.frame_encoder = _mlp(cfg.max_data_dim, cfg.embed_dim, cfg.embed_dim)
        self.frame_decoder = _mlp(cfg.embed_dim, cfg.embed_dim, cfg.max_data_dim)
        # (nn.Embedding's own N(0, 1) draw, then zeros: the reference's construction order and RNG stream, :65-66.  As there, a model-wide
        #  init_bert_params afterwards redraws the table with std 0.02.)
        self.noise_level_emb = OfaEmbedding(cfg.max_noise_levels, cfg.embed_dim * 2)
        nn.init.constant_(self.noise_level_emb.weight, 0)

    def _padded_input(self, value, known_w, known_v):
        """The reference's own steps on a plain [B, T, Dd] value (:90-97): the in-betweening mix, then zero columns up to max_data_dim."""
        if known_w is not None:
            value = known_w.unsqueeze(-1).to(value.dtype) * known_v.to(value.dtype) + (1.0 - known_w.unsqueeze(-1).to(value.dtype)) * value
        dtype = self.frame_encoder[0].weight.dtype
        return torch.nn.functional.pad(value.to(dtype), (0, self.max_data_dim - value.shape[-1]))

    def forward(self, slot: Slot, **kwargs) -> AdaptorOutput:
        assert slot.modality in (ModalityType.MOTION,)
        v = slot.value
        value, masks = v["value"], v["masks"]
        known_w = v.get("known_w")
        bsz, seq_len = masks.shape
        if v.get("data_dim") is None:
            if value.shape[-1] > self.max_data_dim:
                raise ValueError(f"motion_6d: frames of {value.shape[-1]} columns exceed max_data_dim {self.max_data_dim}")
            value = self._padded_input(value, known_w, v.get("value_0") if known_w is not None else None)
        embed = self.frame_encoder[2](ops.gelu(self.frame_encoder[0](value)))
        level = v.get("noise_level")
        if level is not None:
            # ids: t_b + 1 per sentence (and, in-betweening, one further id 0: the level of every known position); the table's sparse
            # gradient goes through the embedding backward as any other
            ids = level.reshape(bsz) + 1
            row_of = None
            if known_w is not None:
                ids = torch.cat((ids, ids.new_zeros(1)))
                own = torch.arange(bsz, device=masks.device, dtype=torch.int32).unsqueeze(1)
                row_of = torch.where(known_w < 0.5, own, own.new_full((), bsz)).contiguous()
            rows = ops.embedding(ids, self.noise_level_emb.weight)
            embed = ops.film(embed, rows, row_of)
        positions = ops.cached_index(self, ("arange", seq_len), lambda: torch.arange(seq_len, device=masks.device).unsqueeze(0))
        pos_embed = self.embed_positions(positions, range_start=0).expand(bsz, -1, -1)
        return AdaptorOutput(embed, masks, pos_embed, [])

    def forward_output(self, x: Tensor, extra: Dict[str, Any], slot: Slot, **kwargs):
        """[B, T, D] -> the frame decoder's [B, T, max_data_dim] rows; extra["data_dim"] says how many leading columns are the prediction
        (the reference slices them out, :126-127; the diffusion loss reads them in place)."""
        v = slot.value
        data_dim = v.get("data_dim")
        extra["data_dim"] = int(data_dim) if data_dim is not None else int(v["value"].shape[-1])
        return self.frame_decoder[2](ops.gelu(self.frame_decoder[0](x))), extra
