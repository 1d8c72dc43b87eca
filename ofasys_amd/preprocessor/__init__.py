from .collate import (CollateOutput, DefaultBoxPreprocess, DefaultTextPreprocess, GeneralPreprocess, Instruction,
                      TensorPreprocess, collate_others, collate_tokens, group_by_predicator, to_device)
from .audio import FbankPreprocess, collate_frames, pack_frames
from .motion import Motion6dPreprocess, Motion6dPreprocessConfig
from .dictionary import Dictionary
from .instruction import ModalityType, Slot

__all__ = ["Dictionary", "ModalityType", "Slot", "Instruction", "CollateOutput", "GeneralPreprocess", "DefaultTextPreprocess",
           "DefaultBoxPreprocess", "TensorPreprocess", "FbankPreprocess", "Motion6dPreprocess", "Motion6dPreprocessConfig", "collate_frames", "pack_frames", "collate_tokens", "collate_others", "group_by_predicator", "to_device"]
