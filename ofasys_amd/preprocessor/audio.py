"""Target-side fbank slots (preprocessor/default/audio.py:398-476): the collation of a text-to-speech batch.

A target-side AUDIO slot carries {"fbank": [L_i, F] float frames, "fbank_lengths": L_i} per sample.  `FbankPreprocess.collate` pads the
frames with zeros to [B, Lmax, F]; the decoder's input slot is the target shifted right by one zero frame, and the sample gets `target`,
`target_lengths` and `ntokens` (the sum of the lengths) -- what the ofa_tacotron2 criterion reads.  Source-side slots and plain tensor
values collate as TensorPreprocess always did.  Feature extraction, CMVN and augmentation are out of scope: frames arrive as arrays."""
import copy
from typing import List

import numpy as np
import torch

from .collate import CollateOutput, SafeBasePreprocess, TensorPreprocess
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


class FbankPreprocess(TensorPreprocess):
    """AUDIO slots.  A target-side slot whose value is {"fbank", "fbank_lengths"} (or a bare [L, F] array) is a text-to-speech target;
    everything else is TensorPreprocess."""

    def map(self, slot: Slot) -> Slot:
        super().map(slot)
        v = slot.value
        if slot.is_src or v is None:
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

    def collate(self, slots: List[Slot]) -> CollateOutput:
        if slots[0].is_src or not _is_frames(slots[0].value):
            return super().collate(slots)
        SafeBasePreprocess.collate(self, slots)                                # (the sanity checks)
        input_slot, target_slot = copy.deepcopy(slots[0]), copy.deepcopy(slots[0])
        feat = collate_frames([torch.as_tensor(s.value["fbank"]) for s in slots])
        bsz, _, d = feat.size()
        prev_outputs = torch.cat((feat.new_zeros((bsz, 1, d)), feat[:, :-1, :]), dim=1)
        target_length = torch.tensor([int(s.value["fbank_lengths"]) for s in slots], dtype=torch.long)
        input_slot.value = {"fbank": prev_outputs, "fbank_lengths": target_length}
        target_slot.value = {"fbank": feat, "fbank_lengths": target_length}
        extra = {"target": feat, "target_lengths": target_length, "ntokens": target_length.sum().item(), "type": "fbank"}
        return CollateOutput(input_slot, target_slot, extra)
