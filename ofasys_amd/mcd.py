"""Mel-cepstral distortion after dynamic time warping: the figure a text-to-speech validation pass reports (task/text_to_speech.py:101-295
of the reference), with the reference's names and return shapes.

The DP is ONE launch of csrc/dtw.hip for the whole ragged batch (`kernels.dtw`), in two forms: `batch_dynamic_time_warping` reads a given
distance tensor, as there; `batch_dtw_features` computes the distances on the fly from two feature sequences and returns only what the
reference logs -- the last DP cell and the length of the optimal path, which the kernel carries along, so nothing is backtraced.  Where the
alignment itself is wanted, `kernels.dtw_backtrace` walks the back pointers on the device.  `MFCC` restates
`torchaudio.transforms.MFCC(sr, n_mfcc=13, log_mels=True, melkwargs=dict(n_fft=int(0.05 sr), win_length=int(0.05 sr), hop_length=
int(0.0125 sr), f_min=20, n_mels=80, window_fn=hann_window))`: `torch.stft` on the device gives |X|^2 (rocFFT serves the lengths that are
no power of two), `kernels.mfcc_rows` does filter bank, log and DCT in one launch; the tables are made here in float64 and rounded once.
No other MFCC configuration is built."""
import math
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import kernels as K
from .module.audio_features import compress_filters

NORMALIZE_TYPES = (None, "len1", "len2", "path")


def htk_mel_filters(sample_rate, n_fft, n_mels=80, f_min=20.0) -> np.ndarray:
    """torchaudio's melscale_fbanks(mel_scale="htk", norm=None) in float64, [n_mels, n_fft // 2 + 1]: n_mels + 2 points equally spaced in
    mel(f) = 2595 log10(1 + f / 700) from mel(f_min) to mel(sample_rate // 2), the triangles evaluated IN HZ at the bin frequencies
    linspace(0, sample_rate // 2, n_fft // 2 + 1); max(0, min(down, up)), peak 1."""
    f_max = float(sample_rate // 2)
    freqs = np.linspace(0.0, f_max, n_fft // 2 + 1)
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)                   # noqa: E731
    pts = 700.0 * (10.0 ** (np.linspace(mel(float(f_min)), mel(f_max), n_mels + 2) / 2595.0) - 1.0)
    diff = pts[1:] - pts[:-1]
    slopes = pts[None, :] - freqs[:, None]                               # [n_bins, n_mels + 2]
    down, up = -slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]
    return np.maximum(0.0, np.minimum(down, up)).T.copy()


def dct_table(n_mfcc=13, n_mels=80) -> np.ndarray:
    """The orthonormal DCT-II in float64, [n_mfcc, n_mels]: cos(pi / n_mels (n + 0.5) k) sqrt(2 / n_mels), row 0 times 1 / sqrt(2)."""
    n, k = np.arange(n_mels, dtype=np.float64)[None, :], np.arange(n_mfcc, dtype=np.float64)[:, None]
    dct = np.cos(math.pi / n_mels * (n + 0.5) * k) * math.sqrt(2.0 / n_mels)
    dct[0] *= 1.0 / math.sqrt(2.0)
    return dct


class MFCC(torch.nn.Module):
    """forward(wav, lengths) -> (fp32 [B, Tmax, 16] on the device: n_mfcc coefficients then zeros, the layout the DTW kernel stages; the
    frame counts, a list of B host ints).  Frames are centred every hop with reflect padding by n_fft // 2 about the utterance's OWN ends,
    periodic Hann window, one-sided |X|^2 not normalised; rows at or past an utterance's own frame count are zeros."""

    def __init__(self, sample_rate, n_mfcc=13, n_mels=80, f_min=20.0):
        super().__init__()
        if not (1 <= n_mfcc <= 16 and n_mfcc <= n_mels <= 128):
            raise ValueError(f"MFCC: n_mfcc={n_mfcc} must be in 1..16 and n_mels={n_mels} in n_mfcc..128")
        self.sample_rate, self.n_mfcc, self.n_mels = sample_rate, int(n_mfcc), int(n_mels)
        self.n_fft, self.hop = int(0.05 * sample_rate), int(0.0125 * sample_rate)
        if not (2 <= self.n_fft <= 4096 and self.hop >= 1):
            raise ValueError(f"MFCC: sample_rate={sample_rate} gives n_fft={self.n_fft}, hop={self.hop}; n_fft must be in 2..4096")
        first, off, w = compress_filters(htk_mel_filters(sample_rate, self.n_fft, self.n_mels, f_min))
        for name, t in (("window", torch.hann_window(self.n_fft, periodic=True, dtype=torch.float64).float()),
                        ("filt_start", torch.from_numpy(first)), ("filt_off", torch.from_numpy(off)), ("filt_w", torch.from_numpy(w)),
                        ("dct", torch.from_numpy(dct_table(self.n_mfcc, self.n_mels)).float())):
            self.register_buffer(name, t.contiguous(), persistent=False)

    def num_frames(self, n_samples: int) -> int:
        return 1 + (n_samples + 2 * (self.n_fft // 2) - self.n_fft) // self.hop

    def power(self, wav, lens):
        """|X|^2 [B, Tmax, n_fft // 2 + 1] of wav fp32 [B, L] on the device; ONE stft over the batch, each utterance reflected about its own ends."""
        pad = self.n_fft // 2
        buf = wav.new_zeros(wav.shape[0], wav.shape[1] + 2 * pad)
        for b, n in enumerate(lens):
            buf[b, :n + 2 * pad] = torch.nn.functional.pad(wav[b, :n].view(1, 1, -1), (pad, pad), mode="reflect").view(-1)
        spec = torch.stft(buf, self.n_fft, self.hop, self.n_fft, self.window, center=False, return_complex=True)
        return (spec.real.square() + spec.imag.square()).transpose(1, 2).contiguous()

    @torch.no_grad()
    def forward(self, wav, lengths=None):
        wav = torch.as_tensor(wav)
        if wav.dim() not in (1, 2) or not wav.is_floating_point():
            raise ValueError(f"MFCC: wav must be (B x) L floating point samples, got {wav.dtype} {tuple(wav.shape)}")
        dev = self.window.device
        wav = (wav.unsqueeze(0) if wav.dim() == 1 else wav).to(device=dev, dtype=torch.float32)
        B, L = wav.shape
        lens = [L] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(lens) != B or (B and (min(lens) < 0 or max(lens) > L)):
            raise ValueError(f"MFCC: lengths {lens} for a batch of {B} utterances of {L} samples")
        if any(n <= self.n_fft // 2 for n in lens):
            raise ValueError(f"MFCC: an utterance of {min(lens)} samples is too short to reflect-pad by n_fft // 2 = {self.n_fft // 2}")
        frames = [self.num_frames(n) for n in lens]
        if B == 0:
            return torch.zeros(0, 0, 16, dtype=torch.float32, device=dev), frames
        power = self.power(wav, lens)[:, :max(frames)].contiguous()
        rows = K.mfcc_rows(power, self.filt_start, self.filt_off, self.filt_w, self.dct)
        live = torch.arange(rows.shape[1], device=dev)[None, :] < torch.tensor(frames, device=dev)[:, None]
        return rows * live[:, :, None], frames


@dataclass
class DtwResult:
    """Device tensors, [B] each: the last DP cell, the number of cells on the optimal path L, nins = L - M (= sum(pathmap.sum(1) - 1) of
    the reference) and ndel = L - N.  path: (int32 [B, maxM + maxN - 1, 2] front-aligned, int32 [B] counts) when asked for."""
    total: Any
    pathlen: Any
    nins: Any
    ndel: Any
    path: Optional[Any] = None
    backptr: Optional[Any] = None


def _shapes(shapes, B, maxM, maxN, device):
    if shapes is None:
        return torch.tensor([[maxM, maxN]] * B, dtype=torch.int32, device=device).reshape(B, 2)
    return torch.as_tensor(shapes).to(device=device, dtype=torch.int32).reshape(B, 2).contiguous()


def batch_dtw_features(x1, x2, shapes, metric="rms", return_path=False, D=None, return_backptr=False):
    """The fused form: x1 fp32 [B, maxM, ld], x2 [B, maxN, ld] (padded buffers: pair b uses the first shapes[b] = (M_b, N_b) rows; the first
    D columns, default all, are the features, D <= 16), metric "l2" (sum of squared differences) or "rms" (sqrt(l2 / D), the reference's
    compute_rms_dist).  The [B, M, N] distances are never formed and nothing is synchronised.  M, N <= 2048."""
    shapes = _shapes(shapes, x1.shape[0], x1.shape[1], x2.shape[1], x1.device)
    total, pathlen, _, bp = K.dtw(shapes, x1=x1, x2=x2, D=D, metric=metric, want_backptr=return_path or return_backptr)
    path = K.dtw_backtrace(bp, shapes) if return_path else None
    return DtwResult(total, pathlen, pathlen - shapes[:, 0], pathlen - shapes[:, 1], path, bp if return_backptr else None)


def batch_dynamic_time_warping(distance, shapes=None, return_path=True, pathmap=False):
    """The reference's signature: distance fp32 [B, maxM, maxN] on the device, shapes [B, 2] (or None: every pair is full) -> (cumdist fp32,
    backptr uint8 with 0 = left, 1 = up-left, 2 = up, the list of B paths int32 [L_b, 2] from (0, 0) to (M_b - 1, N_b - 1)), and with
    pathmap=True a fourth entry, the reference's 0/1 map int32 [B, maxM, maxN].  Cells of cumdist / backptr outside a pair's own
    [:M_b, :N_b] are not written.  return_path=False: None in the list's place and no synchronisation.  M, N <= 4096."""
    B, maxM, maxN = distance.shape
    shapes = _shapes(shapes, B, maxM, maxN, distance.device)
    _, _, cum, bp = K.dtw(shapes, distance=distance, want_cumdist=True, want_backptr=True)
    if not (return_path or pathmap):
        return cum, bp, None
    path, count = K.dtw_backtrace(bp, shapes)
    out = [cum, bp, [path[b, :n] for b, n in enumerate(count.tolist())] if return_path else None]
    if pathmap:                                                          # (entries past a count are (0, 0), which every path holds)
        pm = torch.zeros(B, maxM, maxN, dtype=torch.int32, device=distance.device)
        pm[torch.arange(B, device=pm.device)[:, None], path[..., 0].long(), path[..., 1].long()] = 1
        out.append(pm)
    return tuple(out)


_MFCC = {}


def batch_mel_cepstral_distortion(y1, y2, sr, normalize_type="path", mfcc_fn=None, device="cuda"):
    """y1, y2: lists of 1-D waveforms.  Per pair (distortion, (pathlen, M, N)), host floats and ints: the cumulative RMS distance of the
    13 MFCCs along the DTW path over 1 (None), M ("len1"), N ("len2") or the path's length ("path").  One MFCC pass and one DTW launch for
    the whole batch, one synchronisation at the end."""
    if normalize_type not in NORMALIZE_TYPES:
        raise ValueError(f"normalize_type {normalize_type} not supported")
    if len(y1) != len(y2):
        raise ValueError(f"batch_mel_cepstral_distortion: {len(y1)} waveforms against {len(y2)}")
    B = len(y1)
    if B == 0:
        return []
    if mfcc_fn is None or mfcc_fn.sample_rate != sr:
        if (sr, str(device)) not in _MFCC:
            _MFCC[(sr, str(device))] = MFCC(sr).to(device)
        mfcc_fn = _MFCC[(sr, str(device))]
    waves = [torch.as_tensor(w).reshape(-1).float() for w in list(y1) + list(y2)]
    lens = [int(w.numel()) for w in waves]
    batch = torch.nn.utils.rnn.pad_sequence([w.to(waves[0].device) for w in waves], batch_first=True)
    rows, frames = mfcc_fn(batch, lengths=lens)
    M, N = frames[:B], frames[B:]
    x1, x2 = rows[:B, :max(M)].contiguous(), rows[B:, :max(N)].contiguous()
    res = batch_dtw_features(x1, x2, list(zip(M, N)), metric="rms", D=mfcc_fn.n_mfcc)
    total, pathlen = torch.stack([res.total, res.pathlen.float()]).tolist()             # the one synchronisation (a path length is exact in fp32)
    div = {None: lambda b: 1, "len1": lambda b: M[b], "len2": lambda b: N[b], "path": lambda b: int(pathlen[b])}[normalize_type]
    return [(total[b] / div(b), (int(pathlen[b]), M[b], N[b])) for b in range(B)]
