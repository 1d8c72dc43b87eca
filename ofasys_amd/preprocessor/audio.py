"""Target-side fbank slots (preprocessor/default/audio.py:398-476): the collation of a text-to-speech batch.

A target-side AUDIO slot carries {"fbank": [L_i, F] float frames, "fbank_lengths": L_i} per sample.  `FbankPreprocess.collate` pads the
frames with zeros to [B, Lmax, F]; the decoder's input slot is the target shifted right by one zero frame, and the sample gets `target`,
`target_lengths` and `ntokens` (the sum of the lengths) -- what the ofa_tacotron2 criterion reads.  Source-side slots and plain tensor
values collate as TensorPreprocess always did.

Frames arrive as arrays, or are extracted here: a slot value {"wav": 1-D samples on the int16 scale} keeps its samples through `map`, and
`collate` pads the batch's waveforms and runs module/audio_features.py LogMelExtractor ONCE on the device -- the Kaldi fbank (plus
utterance CMVN as configured) for a source slot, the text-to-speech log-mel (plus global CMVN from `stats_npz_path`) for a target slot --
then packs and emits what ready frames give.  File loading, resampling and speed perturbation, volume normalisation, SpecAugment, dither
and Kaldi options other than torchaudio's defaults are not built: each is refused where it is asked for."""
import copy
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from .collate import CollateOutput, PreprocessConfig, SafeBasePreprocess, TensorPreprocess
from .instruction import Slot


def pack_frames(feature: torch.Tensor, n_frames_per_step: int = 1) -> torch.Tensor:
    """[L, F] -> [L // n, n * F]: n consecutive frames per decoder step, the remainder dropped (preprocessor/default/audio.py:467-476)."""
    n = int(n_frames_per_step)
    if n == 1:
        return feature
    if n < 1:
        raise ValueError(f"pack_frames: n_frames_per_step={n}")
    packed = feature.shape[0] // n
    return feature[: n * packed].reshape(packed, n * feature.shape[1])       # (explicit width: a sample shorter than n packs to 0 frames)


def collate_frames(frames: List[torch.Tensor]) -> torch.Tensor:
    """A list of [L_i, F] frames -> [B, max L_i, F], zero padded (:409-423)."""
    max_len = max(f.size(0) for f in frames)
    out = frames[0].new_zeros((len(frames), max_len, frames[0].size(1)))
    for i, v in enumerate(frames):
        out[i, : v.size(0)] = v
    return out


def _is_frames(v):
    return isinstance(v, dict) and "fbank" in v


def _is_wav(v):
    return isinstance(v, dict) and "wav" in v


@dataclass
class AudioPreprocessConfig(PreprocessConfig):         # preprocessor/default/audio.py:156-203 (the fields in scope)
    target_sr: int = 16000
    win_length: int = 1024                             # (the four window fields and f_min / f_max: the text-to-speech target side)
    hop_length: int = 256
    n_fft: int = 1024
    f_min: float = 0
    f_max: float = 8000
    output_frame_dim: int = 80
    n_frames_per_step: int = 1
    utterance_cmvn: bool = False                       # source side: UtteranceCMVN after the Kaldi fbank
    stats_npz_path: Optional[str] = None               # target side: a local .npz of `mean` and `std` per column (global_cmvn)


# what the reference's audio preprocessor also does with a waveform and this one refuses, by the key a user would ask for it with
NOT_BUILT = {"path": "file loading is not built: decode the file and pass its samples as 'wav'",
             "speed": "speed perturbation is not built (it resamples)",
             "normalize_volume": "volume normalisation is not built",
             "specaugment": "SpecAugment is not built",
             "dither": "dither is not built: it draws random numbers; the fbank is torchaudio's default, dither 0",
             "kaldi_options": "Kaldi options other than torchaudio's fbank defaults are not built"}


class FbankPreprocess(TensorPreprocess):
    """AUDIO slots.  A slot whose value is {"fbank", "fbank_lengths"} (or, on the target side, a bare [L, F] array) carries ready frames;
    one whose value is {"wav"} carries samples from which `collate` extracts the frames on the device; a target-side slot of either
    kind is a text-to-speech target.  Everything else is TensorPreprocess."""

    def __init__(self, global_dict, cfg, modality_type, sanity_check: bool = True):
        super().__init__(global_dict, cfg, modality_type, sanity_check)
        self.audio = cfg if isinstance(cfg, AudioPreprocessConfig) else AudioPreprocessConfig()
        self._extractors = {}

    def extractor(self, is_src: bool):
        """The side's LogMelExtractor, built on first use: Kaldi fbank for a source, the text-to-speech log-mel for a target."""
        if is_src not in self._extractors:
            from ..module.audio_features import LogMelExtractor            # (lazily: the module loads the library)
            a = self.audio
            self._extractors[is_src] = LogMelExtractor.kaldi(a.target_sr, a.output_frame_dim, a.utterance_cmvn) if is_src else \
                LogMelExtractor.tts(a.target_sr, a.win_length, a.hop_length, a.n_fft, a.output_frame_dim, a.f_min, a.f_max, "hann", a.stats_npz_path)
        return self._extractors[is_src]

    def _steps(self, slot: Slot) -> int:
        return slot.get_attr("n_frames_per_step", int) or self.audio.n_frames_per_step

    def _map_wav(self, slot: Slot) -> Slot:
        v, who = slot.value, f"audio slot '{slot.column_name}'"
        for key in v:
            if key in NOT_BUILT:
                raise ValueError(f"{who}: {NOT_BUILT[key]}")
            if key not in ("wav", "sample_rate"):
                raise ValueError(f"{who}: unknown key {key!r} next to 'wav' (known: 'sample_rate')")
        if v.get("sample_rate") is not None and int(v["sample_rate"]) != self.audio.target_sr:
            raise ValueError(f"{who}: resampling is not built: the samples are at {v['sample_rate']} Hz, the configuration's target_sr is "
                             f"{self.audio.target_sr}")
        wav = v["wav"]
        if isinstance(wav, str):
            raise ValueError(f"{who}: {NOT_BUILT['path']}")
        wav = torch.from_numpy(wav) if isinstance(wav, np.ndarray) else wav
        if not torch.is_tensor(wav) or wav.dim() != 1 or not (wav.is_floating_point() or wav.dtype == torch.int16):
            raise ValueError(f"{who}: expected 1-D floating point or int16 samples on the int16 scale, got {type(wav).__name__}")
        frames = self.extractor(slot.is_src).num_frames(wav.shape[0]) // self._steps(slot)
        slot.value = {"wav": wav, "wav_lengths": wav.shape[0], "fbank_lengths": frames}
        return slot

    def map(self, slot: Slot) -> Slot:
        super().map(slot)
        v = slot.value
        if _is_wav(v):
            return self._map_wav(slot)
        if v is None or (slot.is_src and not _is_frames(v)):
            return slot
        fbank = v["fbank"] if _is_frames(v) else v
        if isinstance(fbank, np.ndarray):
            fbank = torch.from_numpy(fbank)
        if not torch.is_tensor(fbank) or fbank.dim() != 2 or not fbank.is_floating_point():
            raise ValueError(f"audio target slot '{slot.column_name}': expected [L, F] float frames (or {{'fbank', 'fbank_lengths'}}), "
                             f"got {type(fbank).__name__}")
        n = slot.get_attr("n_frames_per_step", int)
        length = int(v["fbank_lengths"]) if _is_frames(v) and v.get("fbank_lengths") is not None else fbank.shape[0]
        fbank = fbank[:length].float()
        fbank = pack_frames(fbank, n or 1)
        slot.value = {"fbank": fbank, "fbank_lengths": fbank.shape[0]}
        return slot

    def _extract(self, slots: List[Slot]) -> torch.Tensor:
        """The batch's waveforms, padded -> frames [B, Tmax, n F] on the device in one extractor call, packed as pack_frames packs each
        utterance alone: rows from an utterance's own packed count on are zero."""
        if not torch.cuda.is_available():
            raise RuntimeError("FbankPreprocess: extracting frames from 'wav' values runs on the GPU -- there is no CPU path")
        ext = self.extractor(slots[0].is_src).to("cuda")
        lens = [int(s.value["wav_lengths"]) for s in slots]
        wav = torch.zeros(len(slots), max(lens), dtype=torch.float32)
        for i, s in enumerate(slots):
            wav[i, :lens[i]] = s.value["wav"]
        feat, frames = ext(wav, lens)
        n = self._steps(slots[0])
        if n > 1:
            packed = frames // n
            T = int(packed.max())
            feat = feat[:, :n * T].reshape(len(slots), T, n * feat.shape[2])
            dead = torch.arange(T, device=feat.device)[None, :] >= packed.to(feat.device)[:, None]
            feat = feat.masked_fill(dead[:, :, None], 0.0)
        return feat

    def collate(self, slots: List[Slot]) -> CollateOutput:
        is_wav = _is_wav(slots[0].value)
        if not is_wav and not _is_frames(slots[0].value):
            return super().collate(slots)
        SafeBasePreprocess.collate(self, slots)                                # (the sanity checks)
        feat = self._extract(slots) if is_wav else collate_frames([torch.as_tensor(s.value["fbank"]) for s in slots])
        target_length = torch.tensor([int(s.value["fbank_lengths"]) for s in slots], dtype=torch.long)
        proto = slots[0]
        if is_wav:                                                             # (the copies below need not carry the samples)
            proto = copy.copy(slots[0])
            proto.value = None
        if slots[0].is_src:
            proto.value = {"fbank": feat, "fbank_lengths": target_length}
            return CollateOutput(proto)
        input_slot, target_slot = copy.deepcopy(proto), copy.deepcopy(proto)
        bsz, _, d = feat.size()
        prev_outputs = torch.cat((feat.new_zeros((bsz, 1, d)), feat[:, :-1, :]), dim=1)
        input_slot.value = {"fbank": prev_outputs, "fbank_lengths": target_length}
        target_slot.value = {"fbank": feat, "fbank_lengths": target_length}
        extra = {"target": feat, "target_lengths": target_length, "ntokens": target_length.sum().item(), "type": "fbank"}
        return CollateOutput(input_slot, target_slot, extra)
