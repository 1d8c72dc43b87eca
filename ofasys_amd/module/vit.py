"""CLIP-style pre-LN Vision Transformer backbone of the image_vit adaptor (reference: module/vit.py:22-144), with the reference's
constructor signatures, sizes and state-dict keys (`positional_embedding`, `conv1.weight`, `ln_pre.*`,
`transformer.resblocks.N.{attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.*, ln_1.*, ln_2.*, mlp.c_fc.*, mlp.c_proj.*}`).

Data flow.  The reference goes NLD -> LND through the blocks, back to NLD, then to NCHW, and its adaptor flattens that to [B, T, width]
again: the same rows in the same order.  Here the activations stay batch-major rows [B, T, width] end to end:
  * conv1 is ops.patch_embed (im2col + MFMA GEMM, no bias, no class token);
  * `+ positional_embedding[1:]` is one batch-shared add (its gradient comes back summed over the batch); a grid other than
    input_resolution // patch_size resizes the [n, n, width] table bilinearly first, as the reference does (torch on the device: a
    parameter-side step of n * n * width elements);
  * every residual add emits the next LayerNorm in the same pass (ops.residual_join with ln_b = the next LayerNorm): the stream and its
    normalised copy leave one kernel, and in backward the two gradients meet in one kernel.  The joins also own the bias gradients of
    out_proj and c_proj; QuickGELU's backward owns c_fc's;
  * self-attention reads nn.MultiheadAttention's packed in_proj parameter pair in place (ops.in_proj_self_attention): the fused path for
    16-bit operands at head_dim 64 (vit_base, vit_large, vit_large_336), the unfused tier otherwise (fp32; vit_huge: 1280 / 16 = 80).

DropPath.  The reference builds `DropPath(rate, 0)` and applies it to an LND tensor: axis 0 there is the TOKEN position, so a rate > 0
drops one token position across the whole batch instead of one sample -- a quirk nobody should train on by accident.  The default rate is
0 (identity); any other rate raises NotImplementedError here.
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .layers import LayerNorm, OfaLinear

__all__ = ["QuickGELU", "ResidualAttentionBlock", "Transformer", "VisionTransformer", "vit_base", "vit_large", "vit_large_336",
           "vit_huge"]


class QuickGELU(nn.Module):
    def forward(self, x):
        return ops.quick_gelu(x)


class InProjSelfAttention(nn.Module):
    """Parameter holder with nn.MultiheadAttention(d_model, n_head)'s names, shapes and initial distribution: one packed
    `in_proj_weight` [3D, D] / `in_proj_bias` [3D] in q|k|v order and `out_proj`.  forward: x [B, T, D] batch-major."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        assert embed_dim % num_heads == 0, "embed_dim must be divisible by num_heads"
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = OfaLinear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.0)

    def forward(self, x, out_proj_skip_bias_grad=False):
        a = ops.in_proj_self_attention(x, self.in_proj_weight, self.in_proj_bias, self.num_heads)
        return self.out_proj(a, skip_bias_grad=out_proj_skip_bias_grad)


def _join(branch, bias, stream, next_ln):
    """(stream + branch, next_ln(that)) in one pass; the join takes the bias gradient of the Linear that produced `branch` when every
    parameter involved has a gradient sink (the Linear was then called with skip_bias_grad: see _owns)."""
    return ops.residual_join(branch, stream, None, 0.0, False, next_ln, eps=next_ln.eps if next_ln is not None else 1e-5, x_bias=bias)


def _owns(bias, next_ln):
    return ops.join_takes_bias_grad(bias, *((next_ln.weight, next_ln.bias) if next_ln is not None else ()))


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model: int, n_head: int, attn_mask: torch.Tensor = None, drop_path_rate=0.0):
        super().__init__()
        if attn_mask is not None:
            raise NotImplementedError("the vision blocks take no attention mask")
        if drop_path_rate > 0:
            raise NotImplementedError("vit drop path: the reference drops by token position (DropPath(rate, 0) on an LND tensor), "
                                      "not by sample; only rate 0 is implemented")
        self.attn = InProjSelfAttention(d_model, n_head)
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", OfaLinear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", OfaLinear(d_model * 4, d_model))]))
        self.ln_2 = LayerNorm(d_model)

    def forward_rows(self, stream, normed, next_ln):
        """stream [B, T, D], normed = ln_1(stream) -> (the block's output, next_ln(output) or None)."""
        own = _owns(self.attn.out_proj.bias, self.ln_2)
        a = self.attn(normed, out_proj_skip_bias_grad=own)
        stream, normed = _join(a, self.attn.out_proj.bias if own else None, stream, self.ln_2)
        c_fc, c_proj = self.mlp.c_fc, self.mlp.c_proj
        h = ops.quick_gelu(c_fc(normed, skip_bias_grad=True), c_fc.bias)       # (c_fc.bias' gradient: QuickGELU's backward)
        own = _owns(c_proj.bias, next_ln)
        m = c_proj(h, skip_bias_grad=own)
        return _join(m, c_proj.bias if own else None, stream, next_ln)

    def forward(self, x):
        """x [B, T, D] -> [B, T, D] (one block on its own)."""
        stream, normed = self.ln_1.fork(x)
        return self.forward_rows(stream, normed, None)[0]


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int, attn_mask: torch.Tensor = None, drop_path_rate: float = 0.0):
        super().__init__()
        self.width = width
        self.layers = layers
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, attn_mask, drop_path_rate) for _ in range(layers)])

    def forward(self, x):
        """x [B, T, D] batch-major -> [B, T, D]."""
        blocks = list(self.resblocks)
        if not blocks:
            return x
        stream, normed = blocks[0].ln_1.fork(x)
        for i, blk in enumerate(blocks):
            stream, normed = blk.forward_rows(stream, normed, blocks[i + 1].ln_1 if i + 1 < len(blocks) else None)
        return stream


class VisionTransformer(nn.Module):
    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, drop_path_rate: float = 0.0):
        super().__init__()
        self.input_resolution = input_resolution
        self.patch_size = patch_size
        self.conv1 = nn.Conv2d(in_channels=3, out_channels=width, kernel_size=patch_size, stride=patch_size, bias=False)
        self.width = width
        self.positional_embedding = nn.Parameter(width ** -0.5 * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = LayerNorm(width)
        self.transformer = Transformer(width, layers, heads, drop_path_rate=drop_path_rate)

    def _ofa_plain_conv_weights(self):
        """conv1.weight is read by ops.PatchEmbedFn as a [width, 3*p*p] view: the flat parameter arena keeps torch's order for it."""
        return (self.conv1.weight,)

    def positions(self, h, w, dtype):
        """[h * w, width]: rows 1.. of the table (row 0 is the class position, which this backbone has no token for), resized when the
        grid is not the one the table was made for."""
        n = self.input_resolution // self.patch_size
        pe = self.positional_embedding[1:]
        if (h, w) != (n, n):
            grid = pe.reshape(1, n, n, self.width).permute(0, 3, 1, 2)
            pe = F.interpolate(grid, size=(h, w), mode="bilinear").permute(0, 2, 3, 1).reshape(h * w, self.width)
        return pe.to(dtype)

    def forward(self, x):
        """x [B, 3, H, W] -> (rows [B * h * w, width] batch-major, h, w): the reference's [B, width, h, w] output, flattened as its
        adaptor flattens it."""
        p = self.patch_size
        B, h, w = x.shape[0], x.shape[-2] // p, x.shape[-1] // p
        x = ops.patch_embed(x, self.conv1.weight, None, p)                                  # [B, h*w, width]
        x = ops.add_rowvec_mask(x, self.positions(h, w, x.dtype).unsqueeze(0))
        x = self.transformer(self.ln_pre(x))
        return x.reshape(B * h * w, self.width), h, w


def vit_base(drop_path_rate: float = 0.0):
    return VisionTransformer(224, 16, 768, 9, 12, drop_path_rate)


def vit_large(drop_path_rate: float = 0.0):
    return VisionTransformer(224, 14, 1024, 18, 16, drop_path_rate)


def vit_large_336(drop_path_rate: float = 0.0):
    return VisionTransformer(336, 14, 1024, 18, 16, drop_path_rate)


def vit_huge(drop_path_rate: float = 0.0):
    return VisionTransformer(224, 14, 1280, 24, 16, drop_path_rate)
