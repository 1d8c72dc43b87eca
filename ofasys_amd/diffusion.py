"""The noise schedule of diffusion training (reference: module/diffusion.py:80-100 `DiffusionWrapper.__init__` and :156-173 `p_losses`,
which build a `diffusers` DDIMScheduler / DDPMScheduler).  `diffusers` is not required: what training reads of either scheduler -- the
betas, their cumulative product and `add_noise` -- is restated here; the two schedulers do not differ in any of it.

    betas   linear             linspace(beta_start, beta_end, N)
            scaled_linear      linspace(sqrt(beta_start), sqrt(beta_end), N) ** 2
            squaredcos_cap_v2  beta_i = min(1 - ab((i + 1) / N) / ab(i / N), 0.999),  ab(t) = cos((t + 0.008) / 1.008 * pi / 2) ** 2
    acp     cumprod(1 - beta)

Everything is computed in float64 on the host; three fp32 tables go to the device, each rounded once:
    sqrt_acp[t] = sqrt(acp[t])     sqrt_1m_acp[t] = sqrt(1 - acp[t])     w[t] = sqrt(snr + 1) = 1 / sqrt(1 - acp[t])
A documented difference: the reference keeps acp in fp32 and forms 1 - acp from that.  At t = 0 of the cosine schedule
1 - acp is 4.1e-5 and the fp32 spacing of acp is 1.4e-3 of it, so the reference's w[0] carries about 7e-4 relative error; these tables
do not.  Sampling (the scheduler step, DDIM / DDPM) is not built: `clip_sample`, `num_inference_steps`, `set_alpha_to_one` and
`steps_offset` are accepted and unused."""
import math
from typing import NamedTuple

import numpy as np
import torch

SCHEDULERS = ("DDIMScheduler", "DDPMScheduler")
BETA_SCHEDULES = ("squaredcos_cap_v2", "linear", "scaled_linear")
PREDICTION_TYPES = ("sample", "epsilon")
_DEFAULTS = {"scheduler": "DDIMScheduler", "num_train_timesteps": 1000, "beta_start": 1e-4, "beta_end": 2e-2,
             "beta_schedule": "squaredcos_cap_v2", "prediction_type": "sample"}
_UNUSED_IN_TRAINING = ("clip_sample", "num_inference_steps", "set_alpha_to_one", "steps_offset")


class Tables(NamedTuple):
    """The three fp32 [N] tables on one device."""
    sqrt_acp: torch.Tensor
    sqrt_1m_acp: torch.Tensor
    w: torch.Tensor


def make_betas(beta_schedule, n, beta_start, beta_end):
    """float64 [n] betas of a `diffusers` schedule name."""
    if beta_schedule == "linear":
        return np.linspace(beta_start, beta_end, n, dtype=np.float64)
    if beta_schedule == "scaled_linear":
        return np.linspace(math.sqrt(beta_start), math.sqrt(beta_end), n, dtype=np.float64) ** 2
    if beta_schedule == "squaredcos_cap_v2":
        i = np.arange(n + 1, dtype=np.float64) / n
        ab = np.cos((i + 0.008) / 1.008 * math.pi / 2) ** 2
        return np.minimum(1.0 - ab[1:] / ab[:-1], 0.999)
    raise NotImplementedError(f"diffuser_args: beta_schedule {beta_schedule!r} is not implemented (one of {', '.join(BETA_SCHEDULES)})")


class NoiseSchedule:
    """The training side of the reference's DiffusionWrapper: NoiseSchedule(**diffuser_args).  `acp` is the float64 cumulative product;
    `on(device)` hands out the fp32 tables (built once per device and kept: a captured step addresses them)."""

    def __init__(self, **kwargs):
        unknown = sorted(set(kwargs) - set(_DEFAULTS) - set(_UNUSED_IN_TRAINING))
        if unknown:
            raise ValueError(f"diffuser_args: unknown key(s) {', '.join(unknown)} (accepted: "
                             f"{', '.join(list(_DEFAULTS) + list(_UNUSED_IN_TRAINING))})")
        cfg = dict(_DEFAULTS, **{k: v for k, v in kwargs.items() if k in _DEFAULTS})
        if cfg["scheduler"] not in SCHEDULERS:
            raise ValueError(f"diffuser_args: scheduler {cfg['scheduler']!r} is not supported (one of {', '.join(SCHEDULERS)})")
        if cfg["prediction_type"] == "v_prediction":
            raise NotImplementedError("diffuser_args: prediction_type 'v_prediction' is not implemented (module/diffusion.py:171-172 "
                                      "raises for it too)")
        if cfg["prediction_type"] not in PREDICTION_TYPES:
            raise ValueError(f"diffuser_args: prediction_type {cfg['prediction_type']!r} is not one of {', '.join(PREDICTION_TYPES)}")
        n = int(cfg["num_train_timesteps"])
        if n < 1:
            raise ValueError(f"diffuser_args: num_train_timesteps={n}")
        self.scheduler, self.prediction_type, self.beta_schedule = cfg["scheduler"], cfg["prediction_type"], cfg["beta_schedule"]
        self.num_train_timesteps = n
        self.beta_start, self.beta_end = float(cfg["beta_start"]), float(cfg["beta_end"])
        self.betas = make_betas(self.beta_schedule, n, self.beta_start, self.beta_end)
        self.acp = np.cumprod(1.0 - self.betas)
        one_minus = 1.0 - self.acp                       # float64: 1 - acp keeps 11 more digits than the reference's fp32 difference
        self.sqrt_acp, self.sqrt_1m_acp, self.w = np.sqrt(self.acp), np.sqrt(one_minus), 1.0 / np.sqrt(one_minus)
        self._dev = {}

    def on(self, device) -> Tables:
        key = torch.device(device)
        if key not in self._dev:
            self._dev[key] = Tables(*(torch.from_numpy(a.astype(np.float32)).to(key) for a in (self.sqrt_acp, self.sqrt_1m_acp, self.w)))
        return self._dev[key]

    # What the step engine reads of the object in a micro-batch (trainer._walk, sample_structure): the tables are constants -- a replay
    # has nothing to copy, and a captured graph that addresses them keeps them alive through its pins -- and the objective and the
    # number of levels are part of the step's structure.
    capture_constant = True

    def structure(self):
        return ("diffusion", self.prediction_type, self.num_train_timesteps)


def parse_diffuser_args(spec):
    """TaskConfig.diffuser_args (a JSON string, a dict or None) -> the keyword dict of NoiseSchedule, checked."""
    import json
    args = {} if spec in (None, "") else (json.loads(spec) if isinstance(spec, str) else dict(spec))
    if not isinstance(args, dict):
        raise ValueError(f"diffuser_args must be a JSON object, got {type(args).__name__}")
    NoiseSchedule(**args)
    return args
