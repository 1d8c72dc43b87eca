"""Waveforms -> log-mel frames on the device: the audio INPUT end (preprocessor/default/audio.py:297-328, 485-565 of the reference).

`LogMelExtractor.kaldi` is `torchaudio.compliance.kaldi.fbank` at its defaults -- the reference's fallback route, dither 0 -- for
speech-to-text sources; `LogMelExtractor.tts` is `extract_logmel_spectrogram` for text-to-speech targets.  Both are ONE launch of
csrc/audio_features.hip per batch (plus one of ofa_utterance_cmvn where that is asked for); the tables -- window, twiddles, the compressed
filter bank -- are made here on the host in float64 and rounded once.  PyKaldi's own default is dither 1.0, which draws random numbers:
that default is not built, nor is any Kaldi option other than the defaults named here."""
import math

import numpy as np
import torch

from .. import kernels as K
from .vocoder import get_window, mel_filters

KALDI_LOW_FREQ, KALDI_WIN_T, KALDI_SHIFT_T = 20.0, 0.025, 0.010


def _htk_mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def kaldi_mel_banks(sample_rate, n_fft, n_mels, low_freq=KALDI_LOW_FREQ) -> np.ndarray:
    """torchaudio's get_mel_banks at its defaults in float64: n_mels + 2 points equally spaced in HTK mel from low_freq to Nyquist, the
    triangles evaluated IN MEL at the bin frequencies k sample_rate / n_fft, k < n_fft / 2; peak 1.  [n_mels, n_fft / 2 + 1], the Nyquist
    column zero."""
    mel_low, mel_high = _htk_mel(low_freq), _htk_mel(0.5 * sample_rate)
    delta = (mel_high - mel_low) / (n_mels + 1)
    left = mel_low + np.arange(n_mels, dtype=np.float64)[:, None] * delta
    mel = _htk_mel(sample_rate / n_fft * np.arange(n_fft // 2, dtype=np.float64))[None, :]
    bank = np.maximum(0.0, np.minimum((mel - left) / delta, (left + 2.0 * delta - mel) / delta))
    return np.pad(bank, ((0, 0), (0, 1)))


def compress_filters(dense):
    """A dense [n_mels, n_bins] filter bank -> (first bin int32 [n_mels], offsets int32 [n_mels + 1], packed fp32 weights): filter m weighs
    bins first[m] + j by w[off[m] + j], j < off[m + 1] - off[m] -- everything between its first and last non-zero after fp32 rounding."""
    dense = np.asarray(dense, dtype=np.float64).astype(np.float32)
    first, off, w = [], [0], []
    for row in dense:
        nz = np.flatnonzero(row)
        lo, hi = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
        first.append(lo)
        w.append(row[lo:hi])
        off.append(off[-1] + hi - lo)
    w = np.concatenate(w) if off[-1] else np.zeros(0, dtype=np.float32)
    return np.asarray(first, dtype=np.int32), np.asarray(off, dtype=np.int32), w.astype(np.float32)


class LogMelExtractor(torch.nn.Module):
    """Use the two constructors.  forward(wav, lengths) -> (fp32 [B, Tmax, n_mels] on the device, int64 [B] frame counts on the host)."""

    def __init__(self, kind, sample_rate, n_fft, win, shift, n_mels, window, filters, mean=None, std=None, utterance_cmvn=False):
        super().__init__()
        if K.logmel_run(kind, n_fft, win, shift) == 0 or not 1 <= n_mels <= 128:
            raise ValueError(f"LogMelExtractor.{kind}: n_fft={n_fft} must be a power of two in 256..2048 with window length {win} <= n_fft, "
                             f"1 <= frame shift {shift} <= n_fft and 1 <= n_mels={n_mels} <= 128")
        self.kind, self.sample_rate, self.n_fft, self.win, self.shift, self.n_mels = kind, sample_rate, n_fft, win, shift, n_mels
        self.utterance_cmvn = bool(utterance_cmvn)
        first, off, w = compress_filters(filters)
        ang = 2.0 * math.pi * torch.arange(n_fft // 2, dtype=torch.float64) / n_fft
        for name, t in (("window", window.float()), ("twiddle", torch.stack([ang.cos(), -ang.sin()], dim=1).float()),
                        ("filt_start", torch.from_numpy(first)), ("filt_off", torch.from_numpy(off)), ("filt_w", torch.from_numpy(w)),
                        ("mean", None if mean is None else torch.as_tensor(mean).float().reshape(-1)),
                        ("std", None if std is None else torch.as_tensor(std).float().reshape(-1))):
            self.register_buffer(name, None if t is None else t.contiguous(), persistent=False)
        if (self.mean is None) != (self.std is None) or (self.mean is not None and (self.mean.numel() != n_mels or self.std.numel() != n_mels)):
            raise ValueError(f"LogMelExtractor.{kind}: the global CMVN statistics must be a mean and a std of {n_mels} entries each")

    @classmethod
    def kaldi(cls, sample_rate=16000, n_mels=80, utterance_cmvn=False):
        """fbank at torchaudio's defaults: 25 ms povey windows every 10 ms, snip edges, DC removal, pre-emphasis 0.97, power spectrum,
        HTK-mel triangles from 20 Hz to Nyquist, log floor 1.1920929e-07, no dither.  utterance_cmvn: UtteranceCMVN (means and variances)."""
        win, shift = int(sample_rate * KALDI_WIN_T), int(sample_rate * KALDI_SHIFT_T)
        n_fft = 1 << max(win - 1, 1).bit_length()
        window = torch.zeros(n_fft, dtype=torch.float64)
        window[:win] = torch.hann_window(win, periodic=False, dtype=torch.float64).pow(0.85)
        return cls("kaldi", sample_rate, n_fft, win, shift, n_mels, window, kaldi_mel_banks(sample_rate, n_fft, max(int(n_mels), 1)),
                   utterance_cmvn=utterance_cmvn)

    @classmethod
    def tts(cls, sample_rate, win_length, hop_length, n_fft, n_mels, f_min, f_max, window_fn="hann", stats_npz_path=None):
        """extract_logmel_spectrogram: reflect-padded frames of n_fft every hop_length, the window padded to n_fft, magnitudes, Slaney's
        filters, log floor 1e-5.  stats_npz_path: a local .npz with `mean` and `std` per mel column (global_cmvn), applied in the launch."""
        window_fn = getattr(torch, window_fn + "_window") if isinstance(window_fn, str) else window_fn
        if win_length > n_fft:
            raise ValueError(f"LogMelExtractor.tts: win_length={win_length} exceeds n_fft={n_fft}")
        mean = std = None
        if stats_npz_path is not None:
            stats = np.load(stats_npz_path)
            mean, std = stats["mean"], stats["std"]
        return cls("tts", sample_rate, n_fft, win_length, hop_length, n_mels, get_window(window_fn, n_fft, win_length),
                   mel_filters(sample_rate, n_fft, max(int(n_mels), 1), f_min, f_max).double().numpy(), mean=mean, std=std)

    def num_frames(self, n_samples: int) -> int:
        if self.kind == "kaldi":
            return 0 if n_samples < self.win else 1 + (n_samples - self.win) // self.shift
        return 1 + n_samples // self.shift

    @torch.no_grad()
    def forward(self, wav, lengths=None):
        """wav (B x) L: floating point or int16, on the reference's int16 scale either way.  lengths (host values): utterance b is
        wav[b, :lengths[b]].  A batch whose every utterance has 0 frames gives an empty [B, 0, n_mels] without a launch; a tts utterance
        of at most n_fft / 2 samples cannot be reflect-padded and raises ValueError."""
        wav = torch.as_tensor(wav)
        if wav.dim() not in (1, 2) or not (wav.is_floating_point() or wav.dtype == torch.int16):
            raise ValueError(f"LogMelExtractor: wav must be (B x) L floating point or int16 samples, got {wav.dtype} {tuple(wav.shape)}")
        dev = self.window.device
        wav = (wav.unsqueeze(0) if wav.dim() == 1 else wav).to(device=dev, dtype=torch.float32).contiguous()
        B, L = wav.shape
        lens = [L] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(lens) != B or (B and (min(lens) < 0 or max(lens) > L)):
            raise ValueError(f"LogMelExtractor: lengths {lens} for a batch of {B} utterances of {L} samples")
        if self.kind == "tts" and any(n <= self.n_fft // 2 for n in lens):
            raise ValueError(f"LogMelExtractor.tts: an utterance of {min(lens)} samples is too short to reflect-pad by n_fft / 2 = {self.n_fft // 2}")
        frames = [self.num_frames(n) for n in lens]
        T = max(frames, default=0)
        if T == 0:
            return torch.zeros(B, 0, self.n_mels, dtype=torch.float32, device=dev), torch.tensor(frames, dtype=torch.long)
        lens_dev = None if lengths is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        out = K.logmel(wav, lens_dev, self.window, self.twiddle, self.filt_start, self.filt_off, self.filt_w, self.kind, self.win, self.shift, T,
                       self.mean, self.std)
        if self.utterance_cmvn:
            K.utterance_cmvn(out, None if lengths is None else torch.tensor(frames, dtype=torch.int32, device=dev))
        return out, torch.tensor(frames, dtype=torch.long)
