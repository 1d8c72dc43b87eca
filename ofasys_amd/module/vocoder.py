"""The vocoders (reference: module/vocoder.py): log-mel frames -> waveform.

`HiFiGANVocoder` (module/vocoder.py:154-178) runs module/hifigan.py's Generator.  The checkpoint (`torch.load(path)["generator"]`, the
reference's format) and the JSON configuration are LOCAL paths; nothing is fetched.  Its kernels are fp16 / bf16 only: `fp16=True` runs in
torch.float16, `dtype=torch.bfloat16` in bf16, and the reference's default (fp32) raises -- there is no fp32 kernel and no torch fallback.

`GriffinLimVocoder` (module/vocoder.py:29-151) needs no weights, only the feature configuration: the pseudo-inverse of the mel filters, then
`spec_bwd_max_iter` Griffin-Lim iterations, each ONE launch of csrc/griffin_lim.hip (per-frame FFTs and the overlap-add inside a workgroup)
instead of the reference's dense Fourier-basis convolutions.

Both have `hop` and `out_len(frames)`, the samples that `frames` frames become."""
import json
import math
from typing import Dict, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from .. import kernels as K
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

    def out_len(self, frames: int) -> int:
        return self.hop * frames

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
        assert vocoder_cfg.get("type", "griffin_lim") == "hifigan", "HiFiGANVocoder.from_data_cfg: the data configuration names another vocoder"
        return cls(vocoder_cfg["checkpoint"], vocoder_cfg["config"], fp16=args.fp16)


# ---------------------------------------------------------------------------------------------------------------- Griffin-Lim
def _hz_to_mel(f):
    """Slaney's scale (librosa's default, htk=False): linear below 1000 Hz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) * (27.0 / np.log(6.4)), f * (3.0 / 200.0))


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)), m * (200.0 / 3.0))


def mel_filters(sample_rate, n_fft, n_mels, f_min, f_max) -> torch.Tensor:
    """`librosa.filters.mel(sample_rate, n_fft, n_mels, f_min, f_max)` at its defaults, restated in numpy float64: triangles between
    n_mels + 2 points equally spaced on Slaney's scale, each scaled to unit area (Slaney's normalisation).  fp32 [n_mels, n_fft / 2 + 1]."""
    freqs = np.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(f_min), _hz_to_mel(f_max), n_mels + 2))
    ramps = pts[:, None] - freqs[None, :]
    lower, upper = -ramps[:-2] / np.diff(pts)[:-1, None], ramps[2:] / np.diff(pts)[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return torch.from_numpy(weights.astype(np.float32))


def get_window(window_fn, n_fft: int, win_length: int) -> torch.Tensor:
    """The window padded to n_fft, (n_fft - win_length) // 2 zeros on the left (utils/audio_utils.py:202-205)."""
    padding = n_fft - win_length
    assert padding >= 0
    return F.pad(window_fn(win_length), (padding // 2, padding - padding // 2))


def window_sum_square(window: torch.Tensor, n_frames: int, hop: int) -> torch.Tensor:
    """GriffinLim.get_window_sum_square (module/vocoder.py:69-79): the squared window added frame by frame, in fp32 and in that order."""
    w_sq, n_fft = window.float() ** 2, window.numel()
    n = n_fft + hop * (n_frames - 1)
    x = torch.zeros(n, dtype=torch.float32)
    for i in range(n_frames):
        x[i * hop: min(n, i * hop + n_fft)] += w_sq[: max(0, min(n_fft, n - i * hop))]
    return x


class GriffinLimVocoder(torch.nn.Module):
    """The reference's constructor.  The kernels are fp32 whatever `fp16` says: `fp16=True` only decides the dtype in which `x` is accepted
    (torch.float16 instead of torch.float32; it is converted on load), where the reference would run the whole transform in half.
    window_fn: torch.hann_window and its like, or the name ("hann").  The tables -- mel filters and their `torch.pinverse`, window,
    twiddles -- are made once here on the host; the window-sum-square once per frame count."""

    def __init__(self, sample_rate, win_size, hop_size, n_fft, n_mels, f_min, f_max, window_fn, spec_bwd_max_iter=32, fp16=False):
        super().__init__()
        if K.griffin_lim_run(n_fft, win_size, hop_size) == 0:
            raise ValueError(f"GriffinLimVocoder: n_fft={n_fft} must be a power of two in 256..2048 with win_size={win_size} <= n_fft and "
                             f"1 <= hop_size={hop_size} <= n_fft")
        window_fn = getattr(torch, window_fn + "_window") if isinstance(window_fn, str) else window_fn
        self.n_fft, self.win, self.hop, self.n_mels, self.n_iter = n_fft, win_size, hop_size, n_mels, spec_bwd_max_iter
        self.dtype = torch.float16 if fp16 else torch.float32
        filters = mel_filters(sample_rate, n_fft, n_mels, f_min, f_max)
        self.register_buffer("pinv_t", torch.pinverse(filters).t().contiguous(), persistent=False)           # [n_mels, K]
        self.register_buffer("window", get_window(window_fn, n_fft, win_size).float().contiguous(), persistent=False)
        ang = 2.0 * math.pi * torch.arange(n_fft // 2, dtype=torch.float64) / n_fft
        self.register_buffer("twiddle", torch.stack([ang.cos(), -ang.sin()], dim=1).float().contiguous(), persistent=False)
        self._wss = {}

    def out_len(self, frames: int) -> int:
        return self.hop * (frames - 1)

    def wss(self, n_frames: int, device) -> torch.Tensor:
        key = (n_frames, str(device))
        if key not in self._wss:
            self._wss[key] = window_sum_square(self.window.cpu(), n_frames, self.hop).to(device)
        return self._wss[key]

    def tables(self, T: int, frames, device):
        """What the two step kernels take after (source, S): window, twiddles, window-sum-square, win, hop, lens.  frames (host values,
        or None: every utterance has T): each utterance gets the window-sum-square row of its own frame count."""
        if frames is None:
            return self.window, self.twiddle, self.wss(T, device), self.win, self.hop, None
        wss = torch.zeros(len(frames), self.n_fft + self.hop * (T - 1), dtype=torch.float32, device=device)
        for b, t in enumerate(frames):
            if t > 0:
                wss[b, :self.n_fft + self.hop * (t - 1)] = self.wss(t, device)
        return self.window, self.twiddle, wss, self.win, self.hop, torch.tensor(frames, dtype=torch.int32, device=device)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, lengths=None, angles=None, seed=None) -> torch.Tensor:
        """x (B x) T x n_mels log-mel frames -> (B x) 1 x hop * (T - 1), fp32.  lengths (host values: a list or a CPU tensor): utterance b
        is vocoded as x[b, :lengths[b]] alone would be, zeros from hop * (lengths[b] - 1) on.  The initial phases are `angles`
        ((B x) n_fft / 2 + 1 x T, the reference's layout) or drawn uniformly in [-pi, pi) on the device from `seed` (None: torch's
        device generator); the reference draws them from numpy on the host.  An utterance of hop * (T - 1) <= n_fft / 2 samples
        cannot be reflect-padded and raises ValueError unless spec_bwd_max_iter is 0."""
        single = x.dim() == 2
        dev = self.window.device
        rows = (x.unsqueeze(0) if single else x).to(device=dev, dtype=self.dtype).contiguous()
        B, T, _ = rows.shape
        frames = [T] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(frames) != B or max(frames) > T:
            raise ValueError(f"GriffinLimVocoder: lengths {frames} for a batch of {B} utterances of {T} frames")
        if self.n_iter > 0 and any(self.hop * (t - 1) <= self.n_fft // 2 for t in frames):
            raise ValueError(f"GriffinLimVocoder: an utterance of {min(frames)} frames has {self.hop * (min(frames) - 1)} samples, too few to "
                             f"reflect-pad by n_fft / 2 = {self.n_fft // 2}")
        S = K.griffin_lim_specgram(rows, self.pinv_t)
        if angles is not None:
            phase = (angles.unsqueeze(0) if single else angles).to(device=dev, dtype=torch.float32).transpose(1, 2).contiguous()
        else:
            gen = None if seed is None else torch.Generator(device=dev).manual_seed(int(seed))
            phase = (torch.rand(S.shape, generator=gen, device=dev) * 2.0 - 1.0) * math.pi
        tables = self.tables(T, None if lengths is None else frames, dev)
        w = K.griffin_lim_inverse(phase, S, *tables)
        other = torch.empty_like(w)
        for _ in range(self.n_iter):
            w, other = K.griffin_lim_project(w, S, *tables, out=other), w
        w = w.unsqueeze(1)
        return w.squeeze(0) if single else w

    @classmethod
    def from_data_cfg(cls, args, data_cfg):
        feat_cfg = data_cfg.config["features"]
        return cls(sample_rate=feat_cfg["sample_rate"], win_size=int(feat_cfg["win_len_t"] * feat_cfg["sample_rate"]),
                   hop_size=int(feat_cfg["hop_len_t"] * feat_cfg["sample_rate"]), n_fft=feat_cfg["n_fft"], n_mels=feat_cfg["n_mels"],
                   f_min=feat_cfg["f_min"], f_max=feat_cfg["f_max"], window_fn=feat_cfg["window_fn"],
                   spec_bwd_max_iter=args.spec_bwd_max_iter, fp16=args.fp16)


def get_vocoder(args, data_cfg):
    if args.vocoder == "griffin_lim":
        return GriffinLimVocoder.from_data_cfg(args, data_cfg)
    if args.vocoder == "hifigan":
        return HiFiGANVocoder.from_data_cfg(args, data_cfg)
    raise ValueError("Unknown vocoder")
