"""ImageVitAdaptor (reference: adaptor/image_vit.py:45-181): a CLIP-style Vision Transformer backbone (module/vit.py: vit_base /
vit_large / vit_large_336 / vit_huge) -> Linear(width, D), with the 2-D position ids, position embedding and relative-position bias
of the ResNet adaptor (shared code: adaptor/image_resnet.py ImageGridAdaptor).  `sample_patch_num` is treated as image_resnet treats it."""
from dataclasses import dataclass, field

from ..configure import ChoiceEnum, register_config
from ..module import Embedding
from ..module.vit import vit_base, vit_huge, vit_large, vit_large_336
from ..preprocessor import Dictionary
from .base import BaseAdaptorConfig
from .image_resnet import ImageGridAdaptor


@dataclass
class ImageVitAdaptorConfig(BaseAdaptorConfig):
    vit_type: ChoiceEnum(["vit_base", "vit_large", "vit_large_336", "vit_huge"]) = field(default="vit_base", metadata={"help": "vit type"})
    # the reference's drop path drops by token position, not by sample (module/vit.py): only 0 is implemented, anything else raises
    vit_drop_path_rate: float = field(default=0.0, metadata={"help": "vit drop path rate"})
    image_bucket_size: int = field(default=42, metadata={"help": "image bucket size"})
    pretrained_ckpt_path: str = field(default="", metadata={"help": "path of pretrained ckpt"})


@register_config("ofasys.adaptor", "image_vit", ImageVitAdaptorConfig)
class ImageVitAdaptor(ImageGridAdaptor):
    def __init__(self, embed_tokens: Embedding, dictionary: Dictionary, is_src: bool, general_adaptor, cfg: ImageVitAdaptorConfig):
        super().__init__(embed_tokens, dictionary, is_src, general_adaptor, cfg)
        backbone = {"vit_base": vit_base, "vit_large": vit_large, "vit_large_336": vit_large_336, "vit_huge": vit_huge}[cfg.vit_type]
        self._build_grid(cfg, lambda: backbone(cfg.vit_drop_path_rate), None)
