"""The VQGAN image decoder (reference: module/taming/modules/diffusionmodules/model.py `Decoder`, models/vqgan.py `GumbelVQ.decode_code`,
preprocessor/tokenizer/vqgan.py `VQGANTokenizer`) on the kernels of csrc/vqgan.hip: inference only, fp16 or bf16.

`Decoder(**ddconfig)` carries the reference's state-dict keys (conv_in, mid.block_1 / attn_1 / block_2, up.{i}.block.{j}.*,
up.{i}.attn.{j}.*, up.{i}.upsample.conv, norm_out, conv_out) with the weights in torch's [Cout, Cin, 3, 3] layout; the kernels' tap-major
[9, Cout, Cin] arrangement is made once after loading (`tap_major2d`).  Activations are NHWC rows [B, H, W, C].  A res block is two
statistics calls and two convolution launches (norm + swish applied while the convolution stages its input, the residual -- or the
nin_shortcut's output -- added in the second one's epilogue); an upsample is ONE convolution launch that reads the source pixels; 1 x 1
convolutions are `ops.linear` on the rows and the attention core is `ops.attention` with one head of dimension C.

`VQGANDecoderModel` adds the codebook (`quantize.embed.weight`) and `post_quant_conv`; `VQGANTokenizer.decode` keeps the reference's
semantics.  Paths are local; nothing is fetched.

The encoder (csrc/vqgan_encode.hip for what the decoder's kernels do not cover) is held only on request: `VQGANTokenizer(...,
with_encoder=True)` adds `encoder.*` (taming's `Encoder`: conv_in, down.{i}.block.{j} / attn.{j} / downsample.conv, mid.*, norm_out,
conv_out), `quant_conv` and `quantize.proj`, and `encode` returns the Gumbel quantizer's codes: conv_in is one launch from the fp32 NCHW
image, a Downsample is one stride-2 launch, and the quantizer's projection, noise and arg-max are one sweep that never forms the
[B h w, n_embed] logits.  Not built: training, `VectorQuantizer` checkpoints, `double_z`, `remap`."""
from typing import Dict, List, Optional, Union

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops

DTYPES = (torch.float16, torch.bfloat16)
DROPPED_PREFIXES = ("encoder.", "loss.", "quant_conv.", "quantize.proj.")


def tap_major2d(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [Cout, Cin, 3, 3] -> [9, Cout, Cin], tap 3 dy + dx first."""
    return w.permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1]).contiguous()


def from_tap_major2d(w9: torch.Tensor) -> torch.Tensor:
    """The inverse of tap_major2d: [9, Cout, Cin] -> [Cout, Cin, 3, 3]."""
    return w9.reshape(3, 3, w9.shape[1], w9.shape[2]).permute(2, 3, 0, 1).contiguous()


def conv_in_weight(w: torch.Tensor) -> torch.Tensor:
    """The encoder's conv_in weight [Cout, 3, 3, 3] -> [Cout, 32] as ofa_vqgan_conv_in reads it: column 3 (3 dy + dx) + c, five zero columns."""
    return F.pad(w.permute(0, 2, 3, 1).reshape(w.shape[0], 27), (0, 5)).contiguous()


def _norm(ch):
    return nn.GroupNorm(32, ch, eps=1e-6, affine=True)


class ResnetBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm1, self.conv1 = _norm(cin), nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2, self.conv2 = _norm(cout), nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.nin_shortcut = nn.Conv2d(cin, cout, 1)


class AttnBlock(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.norm = _norm(ch)
        self.q, self.k, self.v, self.proj_out = (nn.Conv2d(ch, ch, 1) for _ in range(4))


class Upsample(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, padding=1)


class Downsample(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, stride=2, padding=0)            # after a zero pad on the bottom and right only


class _RowsModel(nn.Module):
    """What Decoder and Encoder share: the kernels' weight arrangement, made once, and the res / attention blocks on NHWC rows."""

    def __init__(self):
        super().__init__()
        self._laid = None

    def _apply(self, fn, *args, **kwargs):                                # .to() / .half() / .cuda(): the arrangement is made again
        self._laid = None
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._laid = None
        return super().load_state_dict(*args, **kwargs)

    def _w(self, conv: nn.Conv2d, arrange=None):
        """A convolution's (weight, bias) as the kernels read them, arranged once: 3 x 3 -> [9, Cout, Cin], 1 x 1 -> [Cout, Cin]."""
        if self._laid is None:
            self._laid = {}
        got = self._laid.get(id(conv))
        if got is None:
            w = conv.weight.detach()
            if arrange is not None:
                w = arrange(w)
            else:
                w = tap_major2d(w) if w.shape[2] == 3 else w.reshape(w.shape[0], w.shape[1]).contiguous()
            got = self._laid[id(conv)] = (w, conv.bias.detach().contiguous())
        return got

    @staticmethod
    def _stats(norm, x):
        return ops.vqgan_groupnorm_stats(x, norm.weight.detach(), norm.bias.detach())

    def _res(self, blk: ResnetBlock, x):
        h = ops.vqgan_conv3x3(x, *self._w(blk.conv1), *self._stats(blk.norm1, x))
        skip = ops.linear(x, *self._w(blk.nin_shortcut)) if hasattr(blk, "nin_shortcut") else x
        return ops.vqgan_conv3x3(h, *self._w(blk.conv2), *self._stats(blk.norm2, h), res=skip)

    def _attn(self, blk: AttnBlock, x):
        B, H, W, C = x.shape
        h = ops.vqgan_norm_rows(x, *self._stats(blk.norm, x)).view(B, H * W, C)
        q, k, v = (ops.linear(h, *self._w(p)) for p in (blk.q, blk.k, blk.v))
        a, _ = ops.attention(q, k, v, heads=1, scale=float(C) ** -0.5)
        return ops.dropout_add(ops.linear(a, *self._w(blk.proj_out)).view(B, H, W, C), x, 0.0, False)


class Decoder(_RowsModel):
    """The modules below only HOLD the parameters under the reference's names; `forward_rows` runs the kernels."""

    def __init__(self, *, ch=128, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=2, attn_resolutions=(16,), dropout=0.0, resamp_with_conv=True,
                 in_channels=3, resolution=32, z_channels=256, give_pre_end=False, conv_shortcut=False, **ignorekwargs):
        super().__init__()
        if dropout > 0:
            raise ValueError(f"VQGAN Decoder: dropout={dropout} is not built (the decoder is an inference model)")
        if conv_shortcut or not resamp_with_conv or give_pre_end:
            raise ValueError("VQGAN Decoder: conv_shortcut, resamp_with_conv=False and give_pre_end are not built")
        chans = [ch * m for m in ch_mult]
        if any(c % 32 or not 32 <= c <= 512 for c in chans + [z_channels]) or not 1 <= out_ch <= 4:
            raise ValueError(f"VQGAN Decoder: channel counts {chans} and z_channels={z_channels} must be multiples of 32 in 32..512 "
                             f"(GroupNorm(32) and the MFMA fragments), out_ch={out_ch} in 1..4")
        self.num_resolutions, self.num_res_blocks, self.resolution, self.out_ch = len(ch_mult), num_res_blocks, resolution, out_ch
        self.z_channels = z_channels
        block_in, res = chans[-1], resolution // 2 ** (len(ch_mult) - 1)
        self.z_res = res
        self.conv_in = nn.Conv2d(z_channels, block_in, 3, padding=1)
        self.mid = nn.Module()
        self.mid.block_1, self.mid.attn_1, self.mid.block_2 = ResnetBlock(block_in, block_in), AttnBlock(block_in), ResnetBlock(block_in, block_in)
        self.up = nn.ModuleList()
        for i in reversed(range(self.num_resolutions)):
            up = nn.Module()
            up.block, up.attn = nn.ModuleList(), nn.ModuleList()
            for _ in range(num_res_blocks + 1):
                up.block.append(ResnetBlock(block_in, chans[i]))
                block_in = chans[i]
                if res in attn_resolutions:
                    up.attn.append(AttnBlock(block_in))
            if i != 0:
                up.upsample = Upsample(block_in)
                res *= 2
            self.up.insert(0, up)
        self.norm_out, self.conv_out = _norm(block_in), nn.Conv2d(block_in, out_ch, 3, padding=1)

    @torch.no_grad()
    def forward_rows(self, z: torch.Tensor) -> torch.Tensor:
        """z [B, h, w, z_channels] contiguous NHWC rows of the model's dtype on its device -> fp32 NCHW [B, out_ch, h 2^(levels-1), ...]."""
        dtype = self.conv_in.weight.dtype
        if dtype not in DTYPES:
            raise ValueError(f"the VQGAN decoder runs in torch.float16 or torch.bfloat16, not {dtype}: there is no fp32 kernel and no "
                             "torch fallback")
        if z.dim() != 4 or z.shape[3] != self.z_channels or z.dtype != dtype:
            raise ValueError(f"VQGAN Decoder input must be NHWC rows [B, h, w, {self.z_channels}] of {dtype}, got {z.dtype} {list(z.shape)}")
        h = ops.vqgan_conv3x3(z.contiguous(), *self._w(self.conv_in))
        h = self._res(self.mid.block_1, h)
        h = self._attn(self.mid.attn_1, h)
        h = self._res(self.mid.block_2, h)
        for i in reversed(range(self.num_resolutions)):
            up = self.up[i]
            for j in range(self.num_res_blocks + 1):
                h = self._res(up.block[j], h)
                if len(up.attn):
                    h = self._attn(up.attn[j], h)
            if i != 0:
                h = ops.vqgan_conv3x3(h, *self._w(up.upsample.conv), upsample=True)
        return ops.vqgan_conv_out(h, *self._w(self.conv_out), *self._stats(self.norm_out, h))

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        """The reference's layout: z NCHW [B, z_channels, h, w] -> fp32 NCHW images."""
        return self.forward_rows(z.permute(0, 2, 3, 1).contiguous())


class Encoder(_RowsModel):
    """taming's Encoder under the reference's state-dict keys; like Decoder, the modules only hold the parameters."""

    def __init__(self, *, ch=128, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=2, attn_resolutions=(16,), dropout=0.0, resamp_with_conv=True,
                 in_channels=3, resolution=32, z_channels=256, double_z=True, conv_shortcut=False, **ignorekwargs):
        super().__init__()
        if dropout > 0:
            raise ValueError(f"VQGAN Encoder: dropout={dropout} is not built (the encoder is an inference model)")
        if conv_shortcut or not resamp_with_conv or double_z:
            raise ValueError("VQGAN Encoder: conv_shortcut, resamp_with_conv=False and double_z=True are not built")
        chans = [ch * m for m in ch_mult]
        if any(c % 32 or not 32 <= c <= 512 for c in chans + [z_channels]) or in_channels != 3:
            raise ValueError(f"VQGAN Encoder: channel counts {chans} and z_channels={z_channels} must be multiples of 32 in 32..512 "
                             f"(GroupNorm(32) and the MFMA fragments), in_channels={in_channels} must be 3")
        self.num_resolutions, self.num_res_blocks, self.resolution, self.z_channels = len(ch_mult), num_res_blocks, resolution, z_channels
        self.conv_in = nn.Conv2d(in_channels, ch, 3, padding=1)
        block_in, res = ch, resolution
        self.down = nn.ModuleList()
        for i in range(self.num_resolutions):
            down = nn.Module()
            down.block, down.attn = nn.ModuleList(), nn.ModuleList()
            for _ in range(num_res_blocks):
                down.block.append(ResnetBlock(block_in, chans[i]))
                block_in = chans[i]
                if res in attn_resolutions:
                    down.attn.append(AttnBlock(block_in))
            if i != self.num_resolutions - 1:
                down.downsample = Downsample(block_in)
                res //= 2
            self.down.append(down)
        self.mid = nn.Module()
        self.mid.block_1, self.mid.attn_1, self.mid.block_2 = ResnetBlock(block_in, block_in), AttnBlock(block_in), ResnetBlock(block_in, block_in)
        self.norm_out, self.conv_out = _norm(block_in), nn.Conv2d(block_in, z_channels, 3, padding=1)

    @torch.no_grad()
    def forward_rows(self, x: torch.Tensor) -> torch.Tensor:
        """x fp32 NCHW [B, 3, H, W] on the model's device -> NHWC rows [B, H / 2^(levels-1), W / 2^(levels-1), z_channels] of its dtype."""
        dtype = self.conv_in.weight.dtype
        if dtype not in DTYPES:
            raise ValueError(f"the VQGAN encoder runs in torch.float16 or torch.bfloat16, not {dtype}: there is no fp32 kernel and no "
                             "torch fallback")
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError(f"VQGAN Encoder input must be an fp32 NCHW image [B, 3, H, W], got {x.dtype} {list(x.shape)}")
        h = ops.vqgan_conv_in(x.contiguous(), *self._w(self.conv_in, conv_in_weight))
        for i, down in enumerate(self.down):
            for j in range(self.num_res_blocks):
                h = self._res(down.block[j], h)
                if len(down.attn):
                    h = self._attn(down.attn[j], h)
            if i != self.num_resolutions - 1:
                h = ops.vqgan_downsample(h, *self._w(down.downsample.conv))
        h = self._res(self.mid.block_1, h)
        h = self._attn(self.mid.attn_1, h)
        h = self._res(self.mid.block_2, h)
        return ops.vqgan_conv3x3(h, *self._w(self.conv_out), *self._stats(self.norm_out, h))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The reference's layout: fp32 NCHW image -> NCHW [B, z_channels, h, w] (a view of the rows)."""
        return self.forward_rows(x).permute(0, 3, 1, 2)


def load_config(cfg: Union[str, Dict]) -> Dict:
    """The reference's model.yaml (a local path, read with yaml.safe_load) or the same mapping as a dict -> model.params."""
    if isinstance(cfg, str):
        import yaml
        with open(cfg) as f:
            cfg = yaml.safe_load(f)
    params = cfg["model"]["params"] if "model" in cfg else cfg
    return {k: params[k] for k in ("embed_dim", "n_embed", "ddconfig")}


ENCODER_PREFIXES = ("encoder.", "quant_conv.", "quantize.proj.")


class VQGANDecoderModel(nn.Module):
    """The decode side of the reference's GumbelVQ: quantize.embed.weight [n_embed, embed_dim], post_quant_conv, decoder.*; with
    `with_encoder` also its encode side: encoder.*, quant_conv and quantize.proj."""

    def __init__(self, cfg: Union[str, Dict], seed: int = 0, with_encoder: bool = False):
        super().__init__()
        self.with_encoder = with_encoder
        p = load_config(cfg)
        self.n_embed, self.embed_dim = int(p["n_embed"]), int(p["embed_dim"])
        dd = dict(p["ddconfig"])
        self.quantize = nn.Module()
        self.quantize.embed = nn.Embedding(self.n_embed, self.embed_dim)
        self.post_quant_conv = nn.Conv2d(self.embed_dim, dd["z_channels"], 1)
        self.decoder = Decoder(**dd)
        if with_encoder:
            if dd["z_channels"] != self.embed_dim:
                raise ValueError(f"VQGAN encoder: quantize.proj reads z_channels={dd['z_channels']} channels of quant_conv's embed_dim="
                                 f"{self.embed_dim}: they must be equal (as in the reference's GumbelVQ)")
            self.encoder = Encoder(**dd)
            self.quant_conv = nn.Conv2d(dd["z_channels"], self.embed_dim, 1)
            self.quantize.proj = nn.Conv2d(dd["z_channels"], self.n_embed, 1)
        g = torch.Generator().manual_seed(seed)                              # seeded N(0, 1 / fan_in): activations stay O(1) through the stack
        with torch.no_grad():                                                # (the encode side draws last: the decode side's weights do not move)
            for name, t in sorted(self.named_parameters(), key=lambda nt: nt[0].startswith(ENCODER_PREFIXES)):
                if t.dim() == 4:
                    t.copy_(torch.randn(t.shape, generator=g) / (t.shape[1] * t.shape[2] * t.shape[3]) ** 0.5)
                elif t.dim() == 2:
                    t.copy_(torch.randn(t.shape, generator=g))
                else:
                    norm_w = ".norm" in name and name.endswith("weight")
                    t.copy_(1 + 0.1 * torch.randn(t.shape, generator=g) if norm_w else 0.1 * torch.randn(t.shape, generator=g))
        for t in self.parameters():
            t.requires_grad_(False)

    def load_checkpoint(self, path: str) -> None:
        """The reference's last.ckpt: torch.load(path)["state_dict"], without its encoder / loss / quant_conv / quantize.proj keys (with
        the encoder: without its loss keys only); any other missing or unexpected key fails."""
        sd = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
        dropped = ("loss.",) if self.with_encoder else DROPPED_PREFIXES
        self.load_state_dict({k: v for k, v in sd.items() if not k.startswith(dropped)}, strict=True)

    def _need_encoder(self):
        if not self.with_encoder:
            raise ValueError("this VQGAN model was built without its encoder: pass with_encoder=True")

    @torch.no_grad()
    def encode_rows(self, x: torch.Tensor) -> torch.Tensor:
        """x fp32 NCHW [B, 3, H, W] (any device) -> quant_conv(encoder(x)) as NHWC rows [B, h, w, embed_dim] of the model's dtype."""
        self._need_encoder()
        w = self.quant_conv.weight
        rows = self.encoder.forward_rows(x.to(device=w.device, dtype=torch.float32))
        return ops.linear(rows, w.reshape(w.shape[0], w.shape[1]), self.quant_conv.bias)

    def encode_to_prequant(self, x: torch.Tensor) -> torch.Tensor:
        """GumbelVQ.encode_to_prequant: [B, embed_dim, h, w] in the model's dtype (a view of the rows)."""
        return self.encode_rows(x).permute(0, 3, 1, 2)

    @torch.no_grad()
    def encode(self, x: torch.Tensor, gumbel: bool = True, seed: Optional[int] = None) -> torch.Tensor:
        """The codes of GumbelVQ.encode: int64 [B, h w] on the device.  gumbel: argmax(proj(h) + Gumbel noise), as the reference does
        in eval mode too, from Philox(seed) -- seed None: drawn on the host from torch's default generator; the noise of a sample depends
        on its position in the batch.  gumbel=False: the plain arg-max, reproducible."""
        rows = self.encode_rows(x)
        if gumbel and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())               # a CPU draw: no device sync
        w = self.quantize.proj.weight
        codes = ops.vqgan_quantize(rows.view(-1, rows.shape[3]), w.reshape(w.shape[0], w.shape[1]), self.quantize.proj.bias,
                                   seed if gumbel else None)
        return codes.view(rows.shape[0], -1)

    @torch.no_grad()
    def decode_code(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [B, h, w] (int64, in range) -> fp32 images [B, out_ch, 2^(levels-1) h, 2^(levels-1) w]."""
        emb = self.quantize.embed.weight
        z = ops.embedding(codes.to(emb.device).contiguous(), emb)            # the one-hot einsum of the reference IS this gather; NHWC rows
        w = self.post_quant_conv.weight
        z = ops.linear(z, w.reshape(w.shape[0], w.shape[1]), self.post_quant_conv.bias)
        return self.decoder.forward_rows(z)


class VQGANTokenizer:
    def __init__(self, vqgan_config_path: Union[str, Dict], vqgan_model_path=None, code_image_size: int = 256, vqgan_factor: int = 8,
                 fp16: bool = False, dtype=None, with_encoder: bool = False):
        dtype = getattr(torch, dtype) if isinstance(dtype, str) else dtype
        dtype = torch.float16 if fp16 else (torch.bfloat16 if dtype is None else dtype)
        if dtype not in DTYPES:
            raise ValueError(f"VQGANTokenizer runs in torch.bfloat16 (the default) or torch.float16 (fp16=True), not {dtype}: there is no "
                             "fp32 kernel and no torch fallback")
        self.vqgan = VQGANDecoderModel(vqgan_config_path, with_encoder=with_encoder)
        if vqgan_model_path is not None:                                     # (None: the seeded weights -- tests and benchmarks)
            self.vqgan.load_checkpoint(vqgan_model_path)
        self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.vqgan.to(device=self.device, dtype=dtype).eval()
        self.dtype, self.code_image_size, self.vqgan_factor = dtype, code_image_size, vqgan_factor

    def encode(self, x, gumbel: bool = True, seed: Optional[int] = None, **kwargs):
        """x fp32 [B, 3, S, S] on any device -> int64 codes [B, (S / factor)^2] on the device (needs with_encoder=True).  gumbel=True (the
        default) is the reference's behaviour: Gumbel noise even in eval mode, here from Philox(seed), and the noise a sample draws
        depends on its position in the batch; gumbel=False is the plain arg-max, for reproducible targets."""
        if self.vqgan.with_encoder:
            return self.vqgan.encode(x, gumbel, seed)
        raise NotImplementedError("VQGANTokenizer.encode: the VQGAN encoder is not built (only the decode side is); note that the "
                                  "reference's encode draws Gumbel noise even in eval mode, so its codes are not reproducible either")

    def encode_to_prequant(self, x):
        return self.vqgan.encode_to_prequant(x)

    def decode(self, tokens: torch.Tensor, return_pil: bool = True, **kwargs) -> Union[List, torch.Tensor]:
        side = self.code_image_size // self.vqgan_factor
        codes = tokens[:, :-1].clamp(0, self.vqgan.n_embed - 1).reshape(-1, side, side)
        images = self.vqgan.decode_code(codes.contiguous().to(self.device))
        if not return_pil:
            return images
        from PIL import Image
        x = ((images.clamp(-1.0, 1.0) + 1.0) / 2.0).permute(0, 2, 3, 1).cpu().numpy()
        return [Image.fromarray((255 * im).astype("uint8")).convert("RGB") for im in x]
