"""A plain-torch restatement of one motion sampling step as the reference writes it (module/diffusion.py:133-152 with the post-processing
of preprocessor/default/motion_6d.py:394-419 and the scheduler's two-stage step), in the dtype of its inputs: float64 is the tests'
reference, the same code in fp32 measures what fp32 arithmetic costs.  TEST INFRASTRUCTURE: nothing of the kernels."""
import math

import torch
import torch.nn.functional as F


def levels(acp, N, n, ddim, steps_offset=0, set_alpha_to_one=True):
    """-> [(t, a_t, a_prev)] per step, python ints / floats from the float64 table `acp`."""
    r = N // n
    out = []
    for i in reversed(range(n)):
        t = int(round(i * r)) + (steps_offset if ddim else 0)
        p = t - r
        out.append((t, float(acp[t]), float(acp[p]) if p >= 0 else (float(acp[0]) if ddim and not set_alpha_to_one else 1.0)))
    return out


def scheduler_step(ddim, x0, x_t, noise, t, a_t, a_prev):
    if ddim:                                                      # eta = 0, use_clipped_model_output=True
        eps = (x_t - math.sqrt(a_t) * x0) / math.sqrt(1.0 - a_t)
        return math.sqrt(a_prev) * x0 + math.sqrt(1.0 - a_prev) * eps
    beta = 1.0 - a_t / a_prev
    mean = math.sqrt(a_prev) * beta / (1.0 - a_t) * x0 + math.sqrt(1.0 - beta) * (1.0 - a_prev) / (1.0 - a_t) * x_t
    sigma = math.sqrt(max((1.0 - a_prev) / (1.0 - a_t) * beta, 1e-20)) if t > 0 else 0.0
    return mean + sigma * noise


def rectify(x):
    """rotmat_to_rot6d(rot6d_to_rotmat(x)) on the joint columns [..., 6 * joints]."""
    a = x.reshape(*x.shape[:-1], -1, 6)
    b1 = F.normalize(a[..., :3], dim=-1, eps=1e-12)
    b2 = F.normalize(a[..., 3:] - (b1 * a[..., 3:]).sum(-1, keepdim=True) * b1, dim=-1, eps=1e-12)
    return torch.cat((b1, b2), dim=-1).reshape(x.shape)


def x0_hat(pred, value_0=None, known_w=None, interp_w=None, guidance=0.0, clip=False, masks=None):
    """pred [B, T, Dd] -> the step's x0_hat: guidance, rectification, the dense infill, the clip; zeros at padded frames."""
    x = pred.clone()
    if guidance != 0.0:
        x[0::2] = (1 + guidance) * pred[0::2] - guidance * pred[1::2]
    x = torch.cat((x[..., :6], rectify(x[..., 6:])), dim=-1)
    if interp_w is not None:
        x = x + torch.matmul(interp_w.to(x.dtype), value_0.to(x.dtype) - x)
        kw = known_w.to(x.dtype).unsqueeze(-1)
        x = kw * value_0.to(x.dtype) + (1.0 - kw) * x
    if clip:
        x = x.clamp(-1.0, 1.0)
    return x if masks is None else x.masked_fill(masks.unsqueeze(-1), 0.0)


def step(ddim, level, pred, x_t, noise, guidance=0.0, masks=None, **post):
    """-> (x_prev, img).  Under guidance the odd rows take the even rows' new state; padded frames are zeros."""
    img = x0_hat(pred, guidance=guidance, masks=masks, **post)
    x = scheduler_step(ddim, img, x_t, torch.zeros_like(x_t) if noise is None else noise.to(x_t.dtype), *level)
    if masks is not None:
        x = x.masked_fill(masks.unsqueeze(-1), 0.0)
    if guidance != 0.0:
        x[1::2] = x[0::2]
    return x, img


def denoiser_input(x_t, value_0=None, known_w=None, masks=None):
    """The adaptor's in-betweening mix [B, T, Dd] (not rounded, not padded); zeros at padded frames."""
    if known_w is not None:
        kw = known_w.to(x_t.dtype).unsqueeze(-1)
        x_t = kw * value_0.to(x_t.dtype) + (1.0 - kw) * x_t
    return x_t if masks is None else x_t.masked_fill(masks.unsqueeze(-1), 0.0)
