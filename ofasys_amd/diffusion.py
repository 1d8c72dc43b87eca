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
do not.

Sampling (module/diffusion.py:102-154 `sample`, which calls the scheduler's `set_timesteps` and `step`): `sampling_plan()` restates what
the loop reads of either scheduler as a list of timesteps and one coefficient row (c0, c1, sigma) per step,
    x_prev = c0 * x0_hat + c1 * x_t + sigma * noise,
with N = num_train_timesteps, n = num_inference_steps (default N), r = N // n, a = acp:
    timesteps  t_i = round(i * r), i = n - 1 .. 0 (+ steps_offset, DDIM only); a t_i >= N raises
    previous   p = t - r; a_prev = a[p] if p >= 0, else 1 (DDIM with set_alpha_to_one=False: a[0])
    DDIM       (the reference's call: eta = 0, use_clipped_model_output=True)  eps = (x_t - sqrt(a_t) x0_hat) / sqrt(1 - a_t),
               x_prev = sqrt(a_prev) x0_hat + sqrt(1 - a_prev) eps, i.e. c1 = sqrt(1 - a_prev) / sqrt(1 - a_t),
               c0 = sqrt(a_prev) - c1 sqrt(a_t), sigma = 0: no noise is drawn
    DDPM       (ancestral, fixed_small variance) beta = 1 - a_t / a_prev:  c0 = sqrt(a_prev) beta / (1 - a_t),
               c1 = sqrt(1 - beta) (1 - a_prev) / (1 - a_t), sigma = sqrt(max((1 - a_prev) / (1 - a_t) beta, 1e-20)) for t > 0, else 0
`clip_sample` clamps x0_hat to [-1, 1] (after the rectification and the infill: csrc/diffusion_step.hip).  Only prediction_type "sample"
samples, as in the reference.  The coefficients are float64 here and rounded once to fp32 for the device (`sampling_on`); the
coefficient form is algebraically the reference's two-stage form."""
import math
from typing import NamedTuple

import numpy as np
import torch

SCHEDULERS = ("DDIMScheduler", "DDPMScheduler")
BETA_SCHEDULES = ("squaredcos_cap_v2", "linear", "scaled_linear")
PREDICTION_TYPES = ("sample", "epsilon")
_DEFAULTS = {"scheduler": "DDIMScheduler", "num_train_timesteps": 1000, "beta_start": 1e-4, "beta_end": 2e-2,
             "beta_schedule": "squaredcos_cap_v2", "prediction_type": "sample"}
_UNUSED_IN_TRAINING = ("clip_sample", "num_inference_steps", "set_alpha_to_one", "steps_offset")      # the sampling side reads them


class SamplingPlan(NamedTuple):
    """timesteps int64 [n], descending; coef [n, 3] = (c0, c1, sigma) per step: float64 numpy from `sampling_plan`, an int64 and an fp32
    device tensor from `sampling_on`."""
    timesteps: object
    coef: object


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
    """The reference's DiffusionWrapper, training (`on`) and sampling (`sampling_plan`) side: NoiseSchedule(**diffuser_args).  `acp` is the float64 cumulative product;
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
        infer = kwargs.get("num_inference_steps")
        self.num_inference_steps = n if infer is None else int(infer)
        self.clip_sample = bool(kwargs.get("clip_sample", False))
        self.set_alpha_to_one = bool(kwargs.get("set_alpha_to_one", True))
        self.steps_offset = int(kwargs.get("steps_offset", 0))
        self._plan_dev = {}

    def sampling_plan(self) -> SamplingPlan:
        """The sampling loop's timesteps and coefficient rows in float64 (the module docstring has the formulas)."""
        if self.prediction_type != "sample":
            raise NotImplementedError(f"sampling with prediction_type {self.prediction_type!r} is not implemented: the reference asserts "
                                      "prediction_type == 'sample' whenever there is a post-processing function (module/diffusion.py:"
                                      "140-143), and motion always has one")
        N, n = self.num_train_timesteps, self.num_inference_steps
        if not 1 <= n <= N:
            raise ValueError(f"diffuser_args: num_inference_steps={n} must be in [1, num_train_timesteps={N}]")
        ddim = self.scheduler == "DDIMScheduler"
        r = N // n
        ts = np.round(np.arange(n, dtype=np.float64) * r)[::-1].astype(np.int64) + (self.steps_offset if ddim else 0)
        if ts.max() >= N or ts.min() < 0:
            raise ValueError(f"diffuser_args: timestep {int(ts.max() if ts.max() >= N else ts.min())} (steps_offset={self.steps_offset}) is "
                             f"outside the {N} training levels")
        a = self.acp
        a_t = a[ts]
        prev = ts - r
        final = 1.0 if (self.set_alpha_to_one or not ddim) else a[0]
        a_prev = np.where(prev >= 0, a[np.maximum(prev, 0)], final)
        if ddim:
            c1 = np.sqrt(1.0 - a_prev) / np.sqrt(1.0 - a_t)
            c0 = np.sqrt(a_prev) - c1 * np.sqrt(a_t)
            sigma = np.zeros(n)
        else:
            beta = 1.0 - a_t / a_prev
            c0 = np.sqrt(a_prev) * beta / (1.0 - a_t)
            c1 = np.sqrt(1.0 - beta) * (1.0 - a_prev) / (1.0 - a_t)
            sigma = np.where(ts > 0, np.sqrt(np.maximum((1.0 - a_prev) / (1.0 - a_t) * beta, 1e-20)), 0.0)
        return SamplingPlan(ts, np.stack((c0, c1, sigma), axis=1))

    def sampling_on(self, device) -> SamplingPlan:
        """The plan on one device: timesteps int64 [n], coef fp32 [n, 3] (rounded once; built once per device and kept, as `on`)."""
        key = torch.device(device)
        if key not in self._plan_dev:
            plan = self.sampling_plan()
            self._plan_dev[key] = SamplingPlan(torch.from_numpy(plan.timesteps.copy()).to(key),
                                               torch.from_numpy(plan.coef.astype(np.float32)).to(key))
        return self._plan_dev[key]

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
