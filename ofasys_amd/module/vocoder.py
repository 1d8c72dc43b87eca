"""`HiFiGANVocoder` (reference: module/vocoder.py:154-178): log-mel frames -> waveform through module/hifigan.py's Generator.

The checkpoint (`torch.load(path)["generator"]`, the reference's format) and the JSON configuration are LOCAL paths; nothing is
fetched.  The kernels are fp16 / bf16 only: `fp16=True` runs in torch.float16, `dtype=torch.bfloat16` in bf16, and the reference's
default (fp32) raises -- there is no fp32 kernel and no torch fallback.  Griffin-Lim (`GriffinLimVocoder`) is not built."""
import json
from typing import Dict, Optional, Union

import torch

from .hifigan import DTYPES, Generator


class HiFiGANVocoder(torch.nn.Module):
    def __init__(self, checkpoint_path: Optional[str], model_cfg: Union[Dict, str], fp16: bool = False, dtype=None) -> None:
        super().__init__()
        dtype = getattr(torch, dtype) if isinstance(dtype, str) else dtype
        dtype = torch.float16 if (fp16 and dtype is None) else dtype
        if dtype not in DTYPES:
            raise ValueError(f"HiFiGANVocoder runs in torch.float16 (fp16=True) or torch.bfloat16 (dtype=torch.bfloat16), not "
                             f"{dtype or torch.float32}: there is no fp32 kernel and no torch fallback")
        if isinstance(model_cfg, str):
            with open(model_cfg) as f:
                model_cfg = json.load(f)
        self.model = Generator(model_cfg)
        if checkpoint_path is not None:                                  # (None: the seeded initial weights -- tests and benchmarks)
            state_dict = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
            self.model.load_state_dict(state_dict["generator"])
        self.model.to(dtype)
        self.dtype, self.hop = dtype, self.model.hop

    @torch.no_grad()
    def forward(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """x (B x) T x 80 -> (B x) 1 x hop * T, fp32.  lengths (the frames of every utterance of a padded batch; a tensor or a list):
        utterance b is vocoded as x[b, :lengths[b]] alone would be, and its samples from hop * lengths[b] on are zeros."""
        single = x.dim() == 2
        dev = next(self.model.buffers()).device
        rows = (x.unsqueeze(0) if single else x).to(device=dev, dtype=self.dtype).contiguous()
        lens = None
        if lengths is not None:
            lens = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            if lens.numel() != rows.shape[0]:
                raise ValueError(f"HiFiGANVocoder: {lens.numel()} lengths for a batch of {rows.shape[0]}")
        out = self.model.forward_rows(rows, lens).unsqueeze(1)
        return out.squeeze(0) if single else out

    @classmethod
    def from_data_cfg(cls, args, data_cfg):
        vocoder_cfg = data_cfg.vocoder
        assert vocoder_cfg.get("type", "griffin_lim") == "hifigan", "only the HiFi-GAN vocoder is built (Griffin-Lim is not)"
        return cls(vocoder_cfg["checkpoint"], vocoder_cfg["config"], fp16=args.fp16)


def get_vocoder(args, data_cfg):
    if args.vocoder == "hifigan":
        return HiFiGANVocoder.from_data_cfg(args, data_cfg)
    if args.vocoder == "griffin_lim":
        raise NotImplementedError("the Griffin-Lim vocoder is not built; use vocoder=hifigan")
    raise ValueError("Unknown vocoder")
