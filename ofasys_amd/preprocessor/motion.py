"""MOTION slots as continuous rot6d frames (preprocessor/default/motion_6d.py:199-391), for diffusion training: selected by a slot's
`preprocess=motion_6d` attribute, as in the reference.

The value of a sample is frames that are ALREADY rot6d -- an ndarray / tensor [T, Dd] (Dd = 6 + 6 * joints), or {"frames": [T, Dd],
"known_w": [T] or None} for in-betweening.  `map` applies the slot's `min_length` (default 10) / `max_length` (default 1000) /
`sample_rate` attributes and builds `interp_w` [T, T] from `known_w` (the reference's `_get_interpolate_weight`: a known frame keeps
itself, an unknown one interpolates linearly between its known neighbours, or copies the only one it has).  `collate` pads with zeros to
the longest sample and hands the adaptor {"value" [B, T, Dd], "masks" bool [B, T] (True at padding), optional "known_w" [B, T] and
"interp_w" [B, T, T], "value_0": the same tensor as "value"}, with `ntokens` = the sum of the lengths.

Not built -- each raises NotImplementedError: a file path as the value, BVH / Euler input, `anchor_frame`, `soft_trim` / `window`
sampling and `batch_decode`.  They all need the BVH header and its kinematics (joint hierarchy, rotation order, forward kinematics)."""
import copy
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from ..configure import register_config
from .collate import CollateOutput, PreprocessConfig, SafeBasePreprocess
from .instruction import ModalityType, Slot

_NEEDS_BVH = "it needs the BVH header and its kinematics, which are not built"


@dataclass
class Motion6dPreprocessConfig(PreprocessConfig):
    inbetween_args: str = ""          # (the reference samples an in-betweening region from it; only an empty value is accepted)


def interpolate_weight(known_w) -> torch.Tensor:
    """known_w [n] -> interp_w fp32 [n, n]: row k is the weights that rebuild frame k from the known frames (known_w > 0.5)."""
    known = [float(v) > 0.5 for v in known_w]
    n = len(known)
    last_k: List[Optional[int]] = [None] * n
    for k in range(n):
        last_k[k] = k if known[k] else (last_k[k - 1] if k > 0 else None)
    next_k: List[Optional[int]] = [None] * n
    for k in range(n - 1, -1, -1):
        next_k[k] = k if known[k] else (next_k[k + 1] if k + 1 < n else None)
    w = torch.zeros(n, n, dtype=torch.float32)
    for k in range(n):
        i, j = last_k[k], next_k[k]
        if known[k]:
            w[k, k] = 1.0
        elif i is None and j is None:
            raise ValueError("known_w marks no frame as known: nothing to interpolate from")
        elif i is None:
            w[k, j] = 1.0
        elif j is None:
            w[k, i] = 1.0
        else:
            c = (k - i) / (j - i)
            w[k, i], w[k, j] = 1.0 - c, c
    return w


@register_config("ofasys.preprocess", "motion_6d", Motion6dPreprocessConfig)
class Motion6dPreprocess(SafeBasePreprocess):
    def __init__(self, global_dict, cfg: Motion6dPreprocessConfig = None, sanity_check: bool = True):
        cfg = Motion6dPreprocessConfig() if cfg is None else cfg
        if cfg.inbetween_args:
            raise NotImplementedError("motion_6d: inbetween_args (sampling an in-betweening region) is not implemented: supply known_w "
                                      "with the frames")
        super().__init__(global_dict, cfg, ModalityType.MOTION, sanity_check)

    def map(self, slot: Slot) -> Slot:
        super().map(slot)
        data = slot.value
        if isinstance(data, str):
            raise NotImplementedError(f"motion_6d slot '{slot.column_name}': loading a motion file is not implemented: {_NEEDS_BVH}; "
                                      "pass rot6d frames [T, 6 + 6 * joints]")
        for attr in ("anchor_frame", "soft_trim", "window"):
            if slot.has_attr(attr):
                raise NotImplementedError(f"motion_6d slot '{slot.column_name}': the attribute {attr} is not implemented: {_NEEDS_BVH}"
                                          if attr == "anchor_frame" else
                                          f"motion_6d slot '{slot.column_name}': {attr} sampling is not implemented: the reference draws it "
                                          f"around its BVH conversion; {_NEEDS_BVH}")
        if data is None:
            raise NotImplementedError(f"motion_6d slot '{slot.column_name}': an empty value (the generator's dummy frames) is not "
                                      f"implemented: get_data_dim reads the BVH header; {_NEEDS_BVH}")
        frames, known_w = (data.get("frames"), data.get("known_w")) if isinstance(data, dict) else (data, None)
        frames = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
        if not torch.is_tensor(frames) or frames.dim() != 2 or not frames.is_floating_point():
            raise ValueError(f"motion_6d slot '{slot.column_name}': expected rot6d frames [T, Dd] (float array / tensor, or "
                             f"{{'frames', 'known_w'}}), got {type(frames).__name__}")
        if frames.shape[1] < 12 or (frames.shape[1] - 6) % 6:
            raise NotImplementedError(f"motion_6d slot '{slot.column_name}': frames of {frames.shape[1]} columns are not rot6d (6 + 6 * joints); "
                                      f"converting BVH / Euler frames is not implemented: {_NEEDS_BVH}")
        frames = frames.float()
        if known_w is not None:
            known_w = torch.as_tensor(np.asarray(known_w), dtype=torch.float32) if not torch.is_tensor(known_w) else known_w.float()
            if known_w.shape != frames.shape[:1]:
                raise ValueError(f"motion_6d slot '{slot.column_name}': known_w {tuple(known_w.shape)} is not [T] = [{frames.shape[0]}]")
        min_length = slot.get_attr("min_length", int) or 10
        max_length = slot.get_attr("max_length", int) or 1000
        sample_rate = slot.get_attr("sample_rate", int) or 1
        if sample_rate < 1:
            raise ValueError(f"motion_6d slot '{slot.column_name}': sample_rate={sample_rate}")
        if sample_rate > 1:
            beg = int(np.random.randint(0, sample_rate))
            frames = frames[beg::sample_rate]
            known_w = known_w[beg::sample_rate] if known_w is not None else None
        if frames.shape[0] < min_length:
            raise ValueError(f"motion_6d slot '{slot.column_name}': {frames.shape[0]} frames are fewer than min_length={min_length}")
        frames = frames[:max_length]
        sample = {"value": frames.contiguous()}
        if known_w is not None:
            known_w = known_w[:max_length].contiguous()
            sample["known_w"] = known_w
            sample["interp_w"] = interpolate_weight(known_w)
        slot.value = sample
        return slot

    def collate(self, slots: List[Slot]) -> CollateOutput:
        super().collate(slots)
        lengths = [int(s.value["value"].shape[0]) for s in slots]
        if min(lengths) < 1:
            raise ValueError("motion_6d: a sample without frames: every sentence needs at least one unmasked frame")
        if len({int(s.value["value"].shape[1]) for s in slots}) != 1:
            raise ValueError("motion_6d: the samples of a batch differ in data_dim")
        bsz, max_len = len(slots), max(lengths)
        masks = torch.arange(max_len).unsqueeze(0) >= torch.tensor(lengths, dtype=torch.long).unsqueeze(-1)

        def pad(key):
            out = []
            for s in slots:
                v = s.value[key]
                out.append(torch.cat((v, v.new_zeros((max_len - v.shape[0],) + tuple(v.shape[1:]))), dim=0))
            return torch.stack(out, dim=0)

        input_slot = copy.copy(slots[0])
        value = {"value": pad("value"), "masks": masks}
        if "known_w" in slots[0].value:
            value["known_w"] = pad("known_w")
        if "interp_w" in slots[0].value:
            interp_w = torch.zeros(bsz, max_len, max_len)
            for i, s in enumerate(slots):
                n = s.value["interp_w"].shape[0]
                interp_w[i, :n, :n] = s.value["interp_w"]
            value["interp_w"] = interp_w
        value["value_0"] = value["value"]            # the clean frames: diffusion noises "value" (a copy of the dict), never these
        input_slot.value = value
        if input_slot.is_src:
            return CollateOutput(input_slot)
        return CollateOutput(input_slot, None, {"ntokens": sum(lengths)})

    def batch_decode(self, *args, **kwargs):
        raise NotImplementedError(f"motion_6d: batch_decode (rot6d frames -> BVH) is not implemented: {_NEEDS_BVH}")
