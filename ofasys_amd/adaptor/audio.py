"""AudioFbankAdaptor, source branch (reference: adaptor/audio.py:188-325; Conv2dSubsampling4, module/subsample.py:11-63):
fbank [B,T,80] -> Conv2d(1,D,3,2)+ReLU -> Conv2d(D,D,3,2)+ReLU -> Linear(D*19, D); learned positions; padding mask from
the subsampled lengths; 1-D log-bucket relative-position bias (bucket table [4096,4096], 2*max_position-1 rows).

The target branch (text-to-speech training, :327-336, 468-477, 721-763): fbank frames -> prenet (Linear + ReLU + dropout that draws in
eval mode too) -> Linear(embed_dim) on the way in; on the way out feat_proj / eos_proj and post = feat_out + postnet(feat_out), the
postnet (Conv1d + BatchNorm1d + tanh + dropout) on channels-last rows over the padded layout (ops.conv1d_bn, ops.tanh_dropout).

The whole parameter set of the reference adaptor is mirrored (decoder prenet / postnet / feat_proj / eos_proj / mask_emb)
so checkpoints interchange; is_transformer_layers (a branch the reference itself cannot construct) raises NotImplementedError.
Generation (generator.AutoRegressiveSpeechGenerator) feeds the target branch one position per step through `forward_step`: the prenet
is position-wise and its dropout draws are i.i.d., so only the new frame goes through it (the reference re-runs it over the whole frame
history every step and keeps the last row, model/transformer.py:447-450).  The time / channel mask
DRAWS (get_mask_indices, :401-450) belong to the speech-pretraining criterion, which hands them over in the slot value."""
from dataclasses import dataclass, field

import torch
import torch.nn as nn

from .. import ops
from ..configure import register_config
from ..module import Embedding
from ..preprocessor import Dictionary, ModalityType, Slot
from .base import AdaptorOutput, BaseAdaptor, BaseAdaptorConfig
from .text import make_token_bucket_position

DEFAULT_MAX_WAV_POSITIONS = 4096


def make_audio_bucket_position(bucket_size, max_position=DEFAULT_MAX_WAV_POSITIONS):
    """adaptor/audio.py:50-60 -- the text adaptor's log-bucket rule on a 4096-position grid (integer, bit-exact)."""
    return make_token_bucket_position(bucket_size, max_position)


@dataclass
class AudioFbankAdaptorConfig(BaseAdaptorConfig):
    output_frame_dim: int = field(default=80, metadata={"help": "output_frame_dim"})
    n_frames_per_step: int = field(default=1, metadata={"help": "n_frames_per_step"})
    is_transformer_layers: bool = field(default=False, metadata={"help": "whether encoder prenet have transformer net"})
    prenet_layers: int = field(default=2, metadata={"help": "prenet layers"})
    prenet_dim: int = field(default=256, metadata={"help": "prenet dim"})
    prenet_dropout: float = field(default=0.5, metadata={"help": "prenet dropout"})
    postnet_conv_dim: int = field(default=512, metadata={"help": "postnet_conv_dim"})
    postnet_conv_kernel_size: int = field(default=5, metadata={"help": "postnet_conv_kernel_size"})
    postnet_layers: int = field(default=5, metadata={"help": "postnet_layers"})
    postnet_dropout: float = field(default=0.5, metadata={"help": "postnet_dropout"})
    use_mask: bool = field(default=False, metadata={"help": "use mask"})
    mask_prob: float = field(default=0.65, metadata={"help": "probability of replacing a token with mask"})
    mask_channel_prob: float = field(default=0.0, metadata={"help": "probability of replacing a feature with 0"})
    mask_channel_before: bool = False        # zero the drawn channels before (True) or after (False) the mask_emb rows are written


class Conv2dSubsampling4(nn.Module):
    """module/subsample.py:11-63 on the gfx950 convolution stack (im2col + MFMA GEMM with the bias in the epilogue)."""

    def __init__(self, idim: int, odim: int):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(1, odim, 3, 2), nn.ReLU(), nn.Conv2d(odim, odim, 3, 2), nn.ReLU())
        self.out = nn.Sequential(nn.Linear(odim * (((idim - 1) // 2 - 1) // 2), odim))
        self.subsampling_rate = 4
        self.right_context = 6

    def get_out_seq_lens_tensor(self, in_seq_lens_tensor):
        out = in_seq_lens_tensor.clone()
        for _ in range(2):
            out = ((out.float() - 1) / 2 + 1).floor().long()
        return out

    def forward(self, x: torch.Tensor, x_length: torch.Tensor):
        B, T, Fd = x.shape
        c1, c2 = self.conv[0], self.conv[2]
        img = x.unsqueeze(1)                                                   # [B, 1, T, F] (NCHW, C = 1)
        h, T1, F1 = ops.conv2d(img, c1.weight, c1.bias, B, T, Fd, 2, 0, nchw=True)
        h = ops.relu(h)
        h, T2, F2 = ops.conv2d(h, c2.weight, c2.bias, B, T1, F1, 2, 0)
        h = ops.relu(h)
        C = h.shape[-1]
        # rows are (b, t, f) x c; the reference flattens each frame channel-major: view(b, t, c*f)  (:60-61)
        h = h.view(B, T2, F2, C).permute(0, 1, 3, 2).reshape(B, T2, C * F2)
        lin = self.out[0]
        return ops.linear(h, lin.weight, lin.bias), self.get_out_seq_lens_tensor(x_length)


class Prenet(nn.Module):                                                       # adaptor/audio.py:721-732 (decoder side)
    def __init__(self, in_dim, n_layers, n_units, dropout):
        super().__init__()
        self.layers = nn.ModuleList(
            nn.Sequential(nn.Linear(in_dim if i == 0 else n_units, n_units), nn.ReLU()) for i in range(n_layers))
        self.dropout = dropout

    def forward(self, x):
        for layer in self.layers:
            lin = layer[0]
            # F.dropout(layer(x), p=self.dropout) with the default training=True (:731, "always applies dropout"): eval mode draws too
            x = ops.dropout_add(ops.relu(ops.linear(x, lin.weight, lin.bias)), None, self.dropout, True)
        return x


class Postnet(nn.Module):                                                      # adaptor/audio.py:735-763 (decoder side)
    def __init__(self, in_dim, n_channels, kernel_size, n_layers, dropout):
        super().__init__()
        self.convolutions = nn.ModuleList()
        assert kernel_size % 2 == 1
        for i in range(n_layers):
            cur_layers = ([nn.Conv1d(in_dim if i == 0 else n_channels, n_channels if i < n_layers - 1 else in_dim,
                                     kernel_size=kernel_size, padding=((kernel_size - 1) // 2)),
                           nn.BatchNorm1d(n_channels if i < n_layers - 1 else in_dim)]
                          + ([nn.Tanh()] if i < n_layers - 1 else []) + [nn.Dropout(dropout)])
            nn.init.xavier_uniform_(cur_layers[0].weight, torch.nn.init.calculate_gain("tanh" if i < n_layers - 1 else "linear"))
            self.convolutions.append(nn.Sequential(*cur_layers))

    def forward(self, x, residual=None):
        """x [B, T, C] -> [B, T, C] (+ residual, added in the last layer's dropout kernel).  The layers run on batch-major channels-last
        rows [B*T, C] over the PADDED layout: like the reference, padded frames are convolved and counted in the batch statistics
        (they reach valid frames through the window and through the statistics).  Per layer: ops.conv1d_bn (time-unfold, MFMA GEMM
        with the column-statistics epilogue, BatchNorm), then tanh + dropout in one row kernel, or the last layer's dropout."""
        B, T, C = x.shape
        h = x.contiguous().view(B * T, C)
        last = len(self.convolutions) - 1
        for i, seq in enumerate(self.convolutions):
            h = ops.conv1d_bn(h, seq[0], seq[1], B, T)
            if i < last:
                h = ops.tanh_dropout(h, seq[-1].p, self.training)
        p = self.convolutions[last][-1].p if last >= 0 else 0.0
        return ops.dropout_add(h.view(B, T, -1), residual, p, self.training)


@register_config("ofasys.adaptor", "audio_fbank", AudioFbankAdaptorConfig)
class AudioFbankAdaptor(BaseAdaptor):
    pos_batch_invariant = True          # positions are arange- / grid-derived: identical for every batch row

    def __init__(self, embed_tokens: Embedding, dictionary: Dictionary, is_src: bool, general_adaptor,
                 cfg: AudioFbankAdaptorConfig):
        super().__init__(embed_tokens, dictionary, is_src, general_adaptor, cfg)
        if cfg.is_transformer_layers:
            # adaptor/audio.py:208-217, 338-345 read cfg.encoder_config (no config class defines it) and import
            # ofasys.model.transformer_layer (no such module): the reference cannot construct this branch either
            raise NotImplementedError("audio_fbank.is_transformer_layers: the reference's own branch does not construct "
                                      "(cfg.encoder_config / ofasys.model.transformer_layer do not exist); default False")
        self.audio_bucket_size = cfg.max_position
        self.out_dim = cfg.output_frame_dim * cfg.n_frames_per_step
        self.subsample = Conv2dSubsampling4(self.out_dim, cfg.embed_dim)
        self.is_transformer_layers = False
        self.prenet = nn.Sequential(Prenet(self.out_dim, cfg.prenet_layers, cfg.prenet_dim, cfg.prenet_dropout),
                                    nn.Linear(cfg.prenet_dim, cfg.embed_dim))
        self.embed_audio_positions = Embedding(cfg.max_position, cfg.embed_dim)
        audio_num_rel_dis = 2 * self.audio_bucket_size - 1
        audio_rp_bucket = make_audio_bucket_position(self.audio_bucket_size)
        num_rel_pos_tables = 1 if self.cfg.share_attn_bias else self.num_layers
        self.audio_rel_pos_table_list = nn.ModuleList(
            [Embedding(audio_num_rel_dis, cfg.num_attention_heads, zero_init=True) for _ in range(num_rel_pos_tables)])
        self.register_buffer("audio_rp_bucket", audio_rp_bucket)
        self.n_frames_per_step = cfg.n_frames_per_step
        self.feat_proj = nn.Linear(cfg.embed_dim, self.out_dim)
        self.eos_proj = nn.Linear(cfg.embed_dim, 1)
        self.postnet = Postnet(self.out_dim, cfg.postnet_conv_dim, cfg.postnet_conv_kernel_size, cfg.postnet_layers,
                               cfg.postnet_dropout)
        self.use_mask = cfg.use_mask
        self.mask_emb = nn.Parameter(torch.FloatTensor(cfg.embed_dim).uniform_())
        self.mask_prob = cfg.mask_prob
        self.mask_channel_prob = cfg.mask_channel_prob
        self.mask_channel_before = cfg.mask_channel_before

    def get_rel_pos_bias(self, batch_size, seq_length, idx, **kwargs):
        if seq_length > self.audio_rp_bucket.size(0):                  # the reference fails on the size mismatch (slicing clamps)
            raise ValueError(f"sequence length {seq_length} exceeds the {self.audio_rp_bucket.size(0)} positions of audio_rp_bucket")
        rp_bucket = ops.cached_index(self, ("audio", seq_length), lambda: self.audio_rp_bucket[:seq_length, :seq_length].contiguous())
        return ops.embedding(rp_bucket, self.audio_rel_pos_table_list[idx].weight, plan_key=("audio", ops.owner_token(self)))

    def forward(self, slot: Slot, **kwargs) -> AdaptorOutput:
        assert slot.modality == ModalityType.AUDIO
        fbank = slot.value["fbank"]
        fbank_lengths = slot.value["fbank_lengths"]
        if not slot.is_src:                                                    # adaptor/audio.py:327-336: the decoder's input frames
            if fbank.dim() != 3 or fbank.shape[-1] != self.out_dim:
                raise ValueError(f"audio_fbank: target frames {tuple(fbank.shape)} are not [B, T, {self.out_dim}] "
                                 "(output_frame_dim * n_frames_per_step)")
            pre, proj = self.prenet[0], self.prenet[1]
            feature = ops.linear(pre(fbank), proj.weight, proj.bias)
            T = feature.shape[1]
            if T > self.embed_audio_positions.weight.shape[0]:
                raise ValueError(f"audio_fbank: {T} target frames exceed the {self.embed_audio_positions.weight.shape[0]} audio positions")
            pos = torch.arange(T, device=feature.device)[None, :]
            padding_mask = pos >= fbank_lengths.to(feature.device)[:, None]    # lengths_to_padding_mask, on the device, no sync
            pos_embed = self.embed_audio_positions(pos).expand(feature.shape[0], -1, -1)
            return AdaptorOutput(feature, padding_mask, pos_embed, [])
        mask_indices = slot.value.get("mask_indices", None)
        feature, feature_length = self.subsample(fbank, fbank_lengths)
        T2 = feature.shape[1]
        # adaptor/audio.py:303-310 builds this row by row on the host (one device sync per row); same mask, no sync:
        # positions >= the subsampled length are padding
        padding_mask = torch.arange(T2, device=feature.device)[None, :] >= feature_length[:, None]
        pos = torch.arange(T2, device=feature.device)[None, :]
        pos_embed = self.embed_audio_positions(pos).expand(feature.shape[0], -1, -1)       # one lookup, batch-shared (ops.shared_rows)
        if (slot.has_attr("use_mask") or self.use_mask) and mask_indices is not None:      # apply_mask, :452-466
            mch = None
            if self.mask_channel_prob > 0:          # [B, C] channel draws of get_mask_indices: those channels are zeroed over all T
                if slot.value.get("mask_channel_indices") is None:
                    raise ValueError("audio_fbank.mask_channel_prob > 0: the slot value needs 'mask_channel_indices' ([B, C] bool, "
                                     "adaptor/audio.py:433-446) next to 'mask_indices'")
                mch = slot.value["mask_channel_indices"].to(feature.device).unsqueeze(1)
            if mch is not None and self.mask_channel_before:
                feature = feature.masked_fill(mch, 0.0)
            if self.mask_prob > 0:
                m = mask_indices.to(feature.device).unsqueeze(-1)
                feature = torch.where(m, self.mask_emb.to(feature.dtype).view(1, 1, -1), feature)
            if mch is not None and not self.mask_channel_before:
                feature = feature.masked_fill(mch, 0.0)
        return AdaptorOutput(feature, padding_mask, pos_embed, [])

    def step_weights(self):
        """(head, prenet, proj) as ops.speech_step takes them: the Linear parameters of the output head and of the input prenet."""
        pre, proj = self.prenet[0], self.prenet[1]
        return ((self.feat_proj.weight, self.feat_proj.bias, self.eos_proj.weight, self.eos_proj.bias),
                [(layer[0].weight, layer[0].bias) for layer in pre.layers], (proj.weight, proj.bias))

    def embed_frame(self, frame):
        """frame [B, out_dim] -> [B, embed_dim]: the prenet (its dropout draws, as always) and the projection on ONE frame."""
        pre, proj = self.prenet[0], self.prenet[1]
        return ops.linear(pre(frame), proj.weight, proj.bias)

    def forward_step(self, slot: Slot):
        """The step form of the target branch (generation): slot.value = {"frame_embed": [B, 1, embed_dim], the prenet + projection of the
        frame that enters at position t (`embed_frame`, or the step kernel's output); "step": t (host int); "padded": bool [B, 1], is
        position t a padded key of its row}.  -> what the general adaptor returns for a [B, t + 1] target, reduced to what the decoder's
        incremental path keeps of it: the embedding of position t after the post-forward hook's scale / LayerNorm / dropout, the mask
        column of position t, the (normalised) position embedding of position t, and per bias table the ROW of position t of the
        self-attention bias over the t + 1 keys, [B, A, 1, t + 1] (absolute-position term + the relative-position table row).  The
        decoder builds the cross-attention position bias row from the position embedding.  Inference only."""
        general = self.general_adaptor
        embed, t, padded = slot.value["frame_embed"], int(slot.value["step"]), slot.value["padded"]
        B, n = embed.shape[0], t + 1
        if n > self.embed_audio_positions.weight.shape[0]:
            raise ValueError(f"audio_fbank: {n} target frames exceed the {self.embed_audio_positions.weight.shape[0]} audio positions")
        if self.cfg.entangle_position_embedding or general.cfg.entangle_position_embedding or getattr(general.cfg, "modal_ffn", False):
            raise NotImplementedError("audio_fbank.forward_step: entangle_position_embedding / modal_ffn are not implemented for generation")
        embed = ops.scale(embed, self.embed_scale)
        if self.layernorm_embedding is not None:
            embed = self.layernorm_embedding(embed)
        embed = self.dropout_module(embed)                                     # (eval mode: the identity)
        pos = self.embed_audio_positions(torch.arange(n, device=embed.device)[None, :])          # [1, n, D]
        if self.layernorm_position is not None:
            pos = self.layernorm_position(pos)
        biases = []
        if self.cfg.use_self_attn_bias:
            # the row of position t: pos_q(pos_t) * scaling . pos_k(pos_0..t) per head, + rel_pos_table[bucket[t, 0..t]]
            pos_q = general.pos_q_linear(pos[:, t:], alpha=general.pos_scaling)
            pos_k = general.pos_k_linear(pos)
            abs_row = ops.heads_matmul_nt(pos_q, pos_k, general.num_attention_heads)              # [1, A, 1, n]
            if n > self.audio_rp_bucket.size(0):
                raise ValueError(f"sequence length {n} exceeds the {self.audio_rp_bucket.size(0)} positions of audio_rp_bucket")
            bucket = self.audio_rp_bucket[t, :n]                                                  # (a contiguous view: row t)
            for idx in range(1 if self.cfg.share_attn_bias else self.num_layers):
                rel = ops.embedding(bucket, self.audio_rel_pos_table_list[idx].weight)            # [n, A]
                biases.append((abs_row + rel.t().reshape(1, -1, 1, n)).expand(B, -1, -1, -1).contiguous())
        general.last_pos_shared = True
        return embed, padded, pos[:, t:].expand(B, -1, -1), biases, None

    def forward_output(self, x, extra, slot, **kwargs):
        """adaptor/audio.py:468-477 -> (post, extra) with extra["eos_out"] [B, T, 1] and extra["feature_out"] (before the postnet).
        extra["attn"] stays what the decoder gives: the reference transposes the attention map, the fused attention forms none
        ([None]).  x must be the padded [B, T, D] decoder output: the postnet's window and batch statistics run over padded frames too,
        so packed rows would change the numbers."""
        fbank = slot.value["fbank"]
        if x.dim() != 3 or x.shape[:2] != fbank.shape[:2]:
            raise NotImplementedError(f"audio_fbank output head: decoder rows {tuple(x.shape)} are not the padded [B, T] = "
                                      f"{tuple(fbank.shape[:2])} layout of the target frames (a pack plan with an fbank target slot "
                                      "is not supported: the postnet convolves and normalises padded frames too)")
        attn = extra.get("attn")
        if attn and attn[0] is not None:
            extra["attn"] = [attn[0].transpose(2, 1)]
        x = x.contiguous()                                                     # batch-major rows: the postnet's time axis is T
        feat_out = ops.linear(x, self.feat_proj.weight, self.feat_proj.bias)
        # eos_proj has ONE output row: the projection runs 8 wide on zero-padded copies of its weight and bias (8 * D + 8 elements per
        # step), so that the output rows, the bias gradient's column sum and the weight-gradient GEMM keep whole 16-byte vectors
        w8 = torch.nn.functional.pad(self.eos_proj.weight, (0, 0, 0, 7))
        b8 = torch.nn.functional.pad(self.eos_proj.bias, (0, 7))
        eos_out = ops.linear(x, w8, b8)[..., :1]
        post = self.postnet(feat_out, residual=feat_out)
        extra["eos_out"] = eos_out
        extra["feature_out"] = feat_out
        return post, extra
