"""The HiFi-GAN generator (reference: module/hifigan.py:24-162) on the kernels of csrc/vocoder.hip: inference only, fp16 or bf16.

`Generator(cfg)` reads the reference's configuration keys (upsample_initial_channel, upsample_rates, upsample_kernel_sizes,
resblock_kernel_sizes, resblock_dilation_sizes) and loads the reference's state-dict keys (conv_pre, ups.i, resblocks.n.convs1.m /
convs2.m, conv_post; each as `weight` or as the weight-normed pair `weight_g` / `weight_v`, plus `bias`).  The weights are held as the
kernels read them: a Conv1d as [k, Cout, Cin] (tap-major), a ConvTranspose1d as the 3-tap polyphase form [3, u * Cout, Cin] with its
bias u times, conv_post as [k, C].  Activations are channels-last rows [B, L, C]; a forward is 2 + n_ups * (1 + 6 * n_kernels)
launches and reads no length on the host.  Every upsampler must have kernel size 2 * rate (the released configurations do)."""
from typing import Dict, List, Optional

import torch

from .. import ops

LRELU_SLOPE = 0.1
DTYPES = (torch.float16, torch.bfloat16)


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """torch.nn.utils.weight_norm's weight, g * v / ||v|| with the norm over every dimension but 0 (a Conv1d's output channel, a
    ConvTranspose1d's INPUT channel: the reference wraps both with the default dim), in float64."""
    g, v = g.double(), v.double()
    norm = v.reshape(v.shape[0], -1).norm(dim=1).view(-1, *([1] * (v.dim() - 1)))
    return g * v / norm


def tap_major(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [Cout, Cin, k] -> [k, Cout, Cin]."""
    return w.permute(2, 0, 1).contiguous()


def polyphase_weight(wt: torch.Tensor, u: int) -> torch.Tensor:
    """ConvTranspose1d(k = 2u, stride u, padding u/2) weight [Cin, Cout, 2u] -> the 3-tap convolution [3, u * Cout, Cin] whose output
    row q, read as [u, Cout], is output rows q u .. q u + u - 1: output q u + r takes tap r + u/2 of input row q, and tap r + 3u/2 of row
    q - 1 (phases r < u/2) or tap r - u/2 of row q + 1 (phases r >= u/2); the other blocks are zeros."""
    Cin, Cout, k = wt.shape
    if k != 2 * u or u % 2:
        raise ValueError(f"HiFi-GAN upsampler: kernel size {k} must be twice an even stride, got stride {u}")
    w3 = wt.new_zeros(3, u, Cout, Cin)
    for r in range(u):
        w3[1, r] = wt[:, :, r + u // 2].t()
        if r < u // 2:
            w3[0, r] = wt[:, :, r + 3 * u // 2].t()
        else:
            w3[2, r] = wt[:, :, r - u // 2].t()
    return w3.reshape(3, u * Cout, Cin)


class Generator(torch.nn.Module):
    def __init__(self, cfg: Dict):
        super().__init__()
        self.kernel_sizes = [int(k) for k in cfg["resblock_kernel_sizes"]]
        self.dilations = [[int(d) for d in ds] for ds in cfg["resblock_dilation_sizes"]]
        self.rates = [int(u) for u in cfg["upsample_rates"]]
        self.num_kernels, self.num_upsamples = len(self.kernel_sizes), len(self.rates)
        c0 = int(cfg["upsample_initial_channel"])
        self.in_channels = 80
        self.hop = 1
        for u in self.rates:
            self.hop *= u
        # reference key -> (kind, shape of the reference's weight)
        self.layers: Dict[str, tuple] = {"conv_pre": ("conv", (c0, self.in_channels, 7))}
        ch = c0
        for i, (u, k) in enumerate(zip(self.rates, cfg["upsample_kernel_sizes"])):
            if int(k) != 2 * u or u % 2:
                raise ValueError(f"HiFi-GAN upsampler {i}: kernel size {k} must be twice an even stride, got stride {u}")
            self.layers[f"ups.{i}"] = ("up", (c0 // 2 ** i, c0 // 2 ** (i + 1), 2 * u))
            ch = c0 // 2 ** (i + 1)
            for j, (k, ds) in enumerate(zip(self.kernel_sizes, self.dilations)):
                for m in range(len(ds)):
                    for convs in ("convs1", "convs2"):
                        self.layers[f"resblocks.{i * self.num_kernels + j}.{convs}.{m}"] = ("conv", (ch, ch, k))
        self.layers["conv_post"] = ("post", (1, ch, 7))
        g = torch.Generator().manual_seed(0)
        state = {}
        for name, (kind, shape) in self.layers.items():                 # the reference's init_weights: N(0, 0.01)
            state[name + ".weight"] = torch.randn(*shape, generator=g) * 0.01
            state[name + ".bias"] = torch.zeros(shape[1] if kind == "up" else shape[0])
        for name, (kind, shape) in self.layers.items():
            w, b = self._arrange(name, state[name + ".weight"], state[name + ".bias"])
            self.register_buffer(self._buf(name, "w"), w.float())
            self.register_buffer(self._buf(name, "b"), b.float())

    @staticmethod
    def _buf(name, what):
        return name.replace(".", "_") + "_" + what

    def _arrange(self, name, weight, bias):
        kind, shape = self.layers[name]
        if tuple(weight.shape) != shape:
            raise ValueError(f"HiFi-GAN {name}.weight: expected {list(shape)}, got {list(weight.shape)}")
        weight, bias = weight.double(), bias.double()
        if kind == "conv":
            return tap_major(weight), bias
        if kind == "up":
            u = shape[2] // 2
            return polyphase_weight(weight, u), bias.repeat(u)
        return weight[0].t().contiguous(), bias                        # conv_post [1, C, k] -> [k, C]

    def reference_keys(self) -> List[str]:
        return [f"{name}.{p}" for name in self.layers for p in ("weight", "bias")]

    def load_state_dict(self, state_dict, strict: bool = True):
        """The reference generator's state dict: `<layer>.weight` or the weight-normed `<layer>.weight_g` + `<layer>.weight_v` (folded
        in float64), and `<layer>.bias`.  The arrangement for the kernels happens here, once, in float64."""
        used = set()
        for name in self.layers:
            if name + ".weight" in state_dict:
                weight = state_dict[name + ".weight"]
                used.add(name + ".weight")
            elif name + ".weight_g" in state_dict and name + ".weight_v" in state_dict:
                weight = fold_weight_norm(state_dict[name + ".weight_g"], state_dict[name + ".weight_v"])
                used.update((name + ".weight_g", name + ".weight_v"))
            else:
                raise KeyError(f"HiFi-GAN state dict: neither {name}.weight nor {name}.weight_g / weight_v")
            used.add(name + ".bias")
            w, b = self._arrange(name, weight.cpu(), state_dict[name + ".bias"].cpu())
            wb, bb = getattr(self, self._buf(name, "w")), getattr(self, self._buf(name, "b"))
            wb.copy_(w.to(wb.dtype))
            bb.copy_(b.to(bb.dtype))
        extra = sorted(set(state_dict) - used)
        if strict and extra:
            raise KeyError(f"HiFi-GAN state dict: unexpected keys {extra[:4]}{' ...' if len(extra) > 4 else ''}")

    def _wb(self, name):
        return getattr(self, self._buf(name, "w")), getattr(self, self._buf(name, "b"))

    @torch.no_grad()
    def forward_rows(self, x: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B, T, 80] contiguous rows of the model's dtype on its device; lens int32 [B] on the device or None -> fp32 [B, hop * T].
        Sample b is vocoded as the utterance x[b, :lens[b]] alone would be; its samples from hop * lens[b] on are zeros."""
        w, b = self._wb("conv_pre")
        if w.dtype not in DTYPES:
            raise ValueError(f"HiFi-GAN runs in torch.float16 or torch.bfloat16 (Generator.half() / .bfloat16()), not {w.dtype}: "
                             "there is no fp32 kernel and no torch fallback")
        if x.dim() != 3 or x.shape[2] != self.in_channels or x.dtype != w.dtype:
            raise ValueError(f"HiFi-GAN input must be [B, T, {self.in_channels}] of {w.dtype}, got {x.dtype} {list(x.shape)}")
        h = ops.vocoder_conv(x.contiguous(), w, b, lens=lens)
        scale, nk = 1, self.num_kernels
        for i, u in enumerate(self.rates):
            w, b = self._wb(f"ups.{i}")
            h = ops.vocoder_upsample(h, w, b, u, lens=lens, len_scale=scale, slope=LRELU_SLOPE)
            scale *= u
            xs = None
            for j, ds in enumerate(self.dilations):
                r, blk = h, f"resblocks.{i * nk + j}"
                for m, d in enumerate(ds):
                    xt = ops.vocoder_conv(r, *self._wb(f"{blk}.convs1.{m}"), d=d, lens=lens, len_scale=scale, slope=LRELU_SLOPE)
                    if m + 1 < len(ds):
                        r = ops.vocoder_conv(xt, *self._wb(f"{blk}.convs2.{m}"), lens=lens, len_scale=scale, slope=LRELU_SLOPE, res=r)
                    else:                                               # the block's result: xs (+)= it, / num_kernels with the last
                        xs = ops.vocoder_conv(xt, *self._wb(f"{blk}.convs2.{m}"), lens=lens, len_scale=scale, slope=LRELU_SLOPE, res=r,
                                              out=xs, accum=xs is not None, out_scale=1.0 / nk if j + 1 == nk else 1.0)
            h = xs
        return ops.vocoder_post(h, *self._wb("conv_post"), lens=lens, len_scale=scale, slope=0.01)

    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The reference's layout: x [B, 80, T] -> [B, 1, hop * T] (fp32)."""
        return self.forward_rows(x.transpose(1, 2).contiguous(), lengths).unsqueeze(1)
