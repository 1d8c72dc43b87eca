"""Case definitions of the image_vit fixtures, shared by tools/gen_vit_golden.py (which runs the REFERENCE on them, CPU) and the
tests (tests/test_vit_cpu.py, tests/test_vit_gpu.py).  TEST INFRASTRUCTURE: plain data and recipe lookups, nothing of the kernels.

Backbone cases: VisionTransformer(input_resolution, patch_size, width, layers, heads) on a [B, 3, H, W] image, weights from the shared
recipe under the key "vit.<case>.<state-dict key>", loss = sum(output * dout) with a recipe `dout`.
Model case: an arch-`tiny` model with `image_vit` (vit_base) active, an [IMAGE] + text source and a text target, B = 2, 224 x 224.
"""
import torch

from oracle import recipe

B = 2
BACKBONE_CASES = {
    # name: (constructor arguments, (H, W))
    "t16": ((32, 8, 128, 2, 2), (32, 32)),        # 16 tokens
    "t196": ((56, 4, 128, 2, 2), (56, 56)),       # 196 tokens: crosses an attention tile seam
    "interp": ((32, 8, 128, 2, 2), (48, 32)),     # a 6 x 4 grid on a 4 x 4 table: interpolated positions, 24 tokens
    "hd80": ((32, 8, 160, 1, 2), (32, 32)),       # head_dim 80: the unfused tier
}
GRAD_SAMPLES = 509          # gradients are recorded as their norm and about this many evenly strided elements


def grid_of(name):
    (res, p, width, layers, heads), (H, W) = BACKBONE_CASES[name]
    return H // p, W // p


def backbone_inputs(name):
    (res, p, width, layers, heads), (H, W) = BACKBONE_CASES[name]
    h, w = grid_of(name)
    return recipe.floats(f"vit.{name}.image", (B, 3, H, W)), recipe.floats(f"vit.{name}.dout", (B, h * w, width), 0.1)


def fill_backbone_state(name, state_dict):
    """In-place recipe fill of a VisionTransformer state dict (tensors keep dtype and device)."""
    with torch.no_grad():
        for k, v in state_dict.items():
            v.copy_(recipe.value_for(f"vit.{name}.{k}", tuple(v.shape)).to(dtype=v.dtype, device=v.device))
    return state_dict


def stride_of(numel):
    return max(1, numel // GRAD_SAMPLES)


def sample(t):
    """The recorded form of a gradient: evenly strided elements of the flattened tensor."""
    flat = t.detach().reshape(-1)
    return flat[::stride_of(flat.numel())]


MODEL_CASE = dict(
    arch="tiny", active={"text", "image_vit"}, overrides={}, adaptor_overrides={"image_vit": {"vit_type": "vit_base"}},
    slots=[("IMAGE", True, ("img", "vit_image", (B, 3, 224, 224)), ["adaptor=image_vit"]),
           ("TEXT", True, ("tok", "src", (B, 10), [10, 6]), None),
           ("TEXT", False, ("tok", "prev", (B, 8), [8, 5]), None)],
)
MODEL_PREFIX = "encoder.adaptor.image_vit."
# parameters whose gradients the model tests compare: the whole adaptor (the ViT, image_proj, the position and relative-position tables)
EMBED_STRIDE = 7            # image_proj's output [B, 196, 256] is recorded every 7th element
