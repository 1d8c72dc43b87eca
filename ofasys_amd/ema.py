"""Exponential moving average of the weights (reference: engine/ema/ema.py, stepped from engine/trainer.py:934-939, configured by
`EMAConfig`, configure/configs.py:849-860), kept on the device and updated inside the train step.

The reference walks `model.state_dict()` on the host after every update.  Here the trainable parameters already live in one flat
arena (trainer.FlatParams), so the average is one streaming kernel over a second arena of the same layout (ofa_ema_step), launched at
the end of `TrainStep._update` and captured with it.  Whether an update averages, and with which decay, is decided by that kernel
from the schedule state on the device (`ema_schedule` is the same rule on the host): a captured step replays the rule.

    state   fp32 with ema_fp32 (the reference's `fp32_params`), else the model dtype; ONE array with the shadow for an fp32 model
    shadow  the model-dtype arena the averaged model's parameters are views of (`get_model()`); = round(state)

Floating-point state-dict entries outside the arena (BatchNorm running statistics, frozen parameters) are averaged by ONE launch per
dtype over a device-resident table (ofa_ema_segments_step); their state is fp32 with ema_fp32, else their own dtype, as the
reference's.  Non-floating entries are copied when the average is applied; keys containing "version" are left alone (ema.py:157).
"""
import copy
from dataclasses import dataclass
from typing import Optional

import torch

from . import kernels as K


@dataclass
class EMAConfig:                          # configure/configs.py:849-860: the reference's names and defaults
    store_ema: bool = False
    ema_decay: float = 0.9999
    ema_start_update: int = 0
    ema_seed_model: Optional[str] = None  # a checkpoint to seed the EMA from: refused (checkpoints are out of scope)
    ema_update_freq: int = 1
    ema_fp32: bool = False


def as_config(ema) -> Optional[EMAConfig]:
    """None, an EMAConfig or a dict of its fields -> a validated EMAConfig, or None when no EMA is stored."""
    if ema is None:
        return None
    cfg = EMAConfig(**ema) if isinstance(ema, dict) else ema
    if not cfg.store_ema:
        return None
    if cfg.ema_seed_model is not None:
        raise NotImplementedError("ema_seed_model loads the EMA from a checkpoint file; checkpoints are out of scope here -- "
                                  "seed it with EMA.restore(state_dict) instead")
    if not (0.0 <= float(cfg.ema_decay) <= 1.0) or int(cfg.ema_start_update) < 0 or int(cfg.ema_update_freq) < 1:
        raise ValueError(f"bad EMA configuration: {cfg}")
    return cfg


def ema_schedule(t, skipped, cfg):
    """(apply, decay) of the EMA after an attempted update: t = the number of completed updates, `skipped` = this one was skipped
    (non-finite gradients, empty batch, loss-scale overflow).  The rule the kernels evaluate on the device: ema.py:187 for the decay;
    ema.py:188-192's counter, which only advances on stepped updates and starts at 0 with the trainer, restated as t % freq."""
    decay = 0.0 if t < cfg.ema_start_update else cfg.ema_decay
    return (not skipped) and t % max(int(cfg.ema_update_freq), 1) == 0, decay


def _rebase(t, src, dst):
    """The window `t` is of the flat array `src`, taken of `dst` instead (same element offset, shape and strides; `dst` may be of
    another dtype: the fp32 state next to a 16-bit arena)."""
    off = (t.data_ptr() - src.data_ptr()) // src.element_size()
    extent = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride())) if t.numel() else 0
    assert t.dtype == src.dtype and off >= 0 and off + extent <= src.numel() == dst.numel()
    return torch.as_strided(dst, t.shape, t.stride(), dst.storage_offset() + off)


class _Group:
    """The floating-point state-dict entries outside the arena that share one dtype: a flat state, a flat shadow, a device table."""

    def __init__(self, dtype, keys, tensors, fp32):
        self.dtype, self.keys, self.sources = dtype, keys, [t.detach() for t in tensors]
        self.offsets, off = [], 0
        for t in self.sources:
            self.offsets.append(off)
            off += t.numel()
        dev = self.sources[0].device
        self.shadow = torch.cat([t.reshape(-1) for t in self.sources]).clone()
        self.state = self.shadow.float() if fp32 and dtype != torch.float32 else self.shadow
        self.table, self.max_len = K.ema_segment_table(self.sources, self.offsets, dev)

    def view(self, arr, i):
        t = self.sources[i]
        return arr[self.offsets[i]:self.offsets[i] + t.numel()].view(t.shape)


class EMA:
    """The EMA of `model`, whose trainable parameters are the arena `fp` (trainer.FlatParams).  Built by TrainStep(ema=...); the
    reference's host-side `step` has no counterpart -- the device does it."""

    def __init__(self, model, fp, config: EMAConfig, step_t=None):
        self.config = config
        self.decay = config.ema_decay
        self._live, self._fp, self._step_t = model, fp, step_t
        T = fp.flat.dtype
        self.shadow = fp.flat.clone()
        self.state = self.shadow.float() if config.ema_fp32 and T != torch.float32 else self.shadow
        in_arena = {id(p) for p in fp.params}
        self._kind, groups = {}, {}
        self._copies, self._copy_src = {}, {}
        self._live_sd = model.state_dict(keep_vars=True)          # key -> the live Parameter / buffer
        for key, t in self._live_sd.items():
            if id(t) in in_arena:
                self._kind[key] = "arena"
            elif "version" in key:                                   # ema.py:157: never averaged, never copied
                self._kind[key] = "fixed"
                self._copies[key] = t.detach().clone()
            elif torch.is_floating_point(t):
                if not t.is_contiguous():
                    raise NotImplementedError(f"EMA: {key} is a non-contiguous tensor outside the parameter arena")
                self._kind[key] = "seg"
                groups.setdefault(t.dtype, ([], []))
                groups[t.dtype][0].append(key)
                groups[t.dtype][1].append(t)
            else:
                self._kind[key] = "copy"
                self._copies[key] = t.detach().clone()
                self._copy_src[key] = t.detach()
        self._groups = [_Group(dt, ks, ts, config.ema_fp32) for dt, (ks, ts) in groups.items()]
        self._seg_of = {k: (g, i) for g in self._groups for i, k in enumerate(g.keys)}
        self._keys = list(self._kind)
        self._model = None

    # ------------------------------------------------------------------ the device side
    def arenas(self):
        """Every device array this object owns and a captured step addresses."""
        out = [self.shadow, self.state]
        for g in self._groups:
            out += [g.shadow, g.state, g.table]
        return out + list(self._copies.values())

    def _enqueue(self, step_t, sched):
        """The launches of one update, on the current stream (TrainStep._update calls this last; captured with it)."""
        c = self.config
        sep = self.state is not self.shadow
        K.ema_step(self.state, self._fp.flat, self.shadow if sep else None, step_t, sched, c.ema_decay, c.ema_start_update,
                   c.ema_update_freq)
        for g in self._groups:
            K.ema_segments_step(g.state, g.table, len(g.sources), g.max_len, g.shadow if g.state is not g.shadow else None, g.dtype,
                                step_t, sched, c.ema_decay, c.ema_start_update, c.ema_update_freq)
        if self._copy_src:
            # non-floating entries (ema.py:163-169) follow the model when -- and only when -- the average is applied: the same rule,
            # from the same device words, as integer arithmetic over all of them at once
            apply = sched[3] == 0
            if c.ema_update_freq > 1:
                apply = apply & (torch.remainder(step_t[0], float(c.ema_update_freq)) == 0)
            ints = [k for k in self._copy_src if self._copies[k].dtype != torch.bool]
            for k in self._copy_src:
                if self._copies[k].dtype == torch.bool:
                    self._copies[k].copy_(torch.where(apply, self._copy_src[k], self._copies[k]))
            by_dtype = {}
            for k in ints:
                by_dtype.setdefault(self._copies[k].dtype, []).append(k)
            for dt, ks in by_dtype.items():
                dst = [self._copies[k] for k in ks]
                diff = torch._foreach_sub([self._copy_src[k] for k in ks], dst)
                torch._foreach_mul_(diff, apply.to(dt))
                torch._foreach_add_(dst, diff)

    # ------------------------------------------------------------------ the reference's methods
    def _shadow_tensor(self, key):
        kind = self._kind[key]
        if kind == "arena":
            return _rebase(self._live_sd[key].detach(), self._fp.flat, self.shadow)
        if kind == "seg":
            g, i = self._seg_of[key]
            return g.view(g.shadow, i)
        return self._copies[key]

    def _state_tensor(self, key):
        kind = self._kind[key]
        if kind == "arena":
            return _rebase(self._live_sd[key].detach(), self._fp.flat, self.state)
        if kind == "seg":
            g, i = self._seg_of[key]
            return g.view(g.state, i)
        return self._copies[key]

    def get_model(self):
        """The averaged model: a copy of the live one whose parameters are views of the shadow arena at the live arena's offsets
        (channels-last convolution weights and the packed k|v|q / all-layer k|v attention views included), whose buffers are the
        averaged buffers; eval mode, no gradients.  It follows every later update: the same memory."""
        if self._model is not None:
            return self._model
        memo = {}
        for key, t in self._live_sd.items():
            if id(t) in memo:
                continue
            s = self._shadow_tensor(key)
            memo[id(t)] = torch.nn.Parameter(s, requires_grad=False) if isinstance(t, torch.nn.Parameter) else s
        for m in self._live.modules():            # the arena views FlatParams hung on the attention modules
            packs = [getattr(m, "_pack", None) or {}]
            if getattr(m, "_cross_all", None) is not None:
                packs.append(m._cross_all[0])
            for pack in packs:
                for name in ("w", "b"):
                    if torch.is_tensor(pack.get(name)):
                        memo[id(pack[name])] = _rebase(pack[name], self._fp.flat, self.shadow)
                for name in ("gw", "gb"):         # gradient windows: the copy has no gradient arena
                    if torch.is_tensor(pack.get(name)):
                        memo[id(pack[name])] = None
        with torch.no_grad():
            model = copy.deepcopy(self._live, memo)
        from .adaptor.base import BaseAdaptor
        for m in model.modules():                 # deepcopy copies closures by reference: they still reach the LIVE token embedding
            if isinstance(m, BaseAdaptor):
                m._bind_embed_tokens(m._general_adaptor[0].embed_tokens)
        model.requires_grad_(False)
        model.eval()
        self._model = model
        return model

    def get_decay(self):
        """The decay of the latest update (ema.py:187).  Reads the device's update counter: one sync."""
        if self._step_t is None:
            return self.decay
        t = int(self._step_t.item())
        if t > 0:
            self.decay = ema_schedule(t, False, self.config)[1]
        return self.decay

    def build_fp32_params(self, state_dict=None):
        """(Re)fill the fp32 state from `state_dict`, or from the shadow model (ema.py:101-126)."""
        if not self.config.ema_fp32:
            raise RuntimeError("build_fp32_params should not be called if ema_fp32=False. "
                               "Use ema_fp32=True if this is really intended.")
        with torch.no_grad():
            for key in self._keys:
                if state_dict is not None and key not in state_dict:
                    continue
                src = self._shadow_tensor(key) if state_dict is None else state_dict[key]
                dst = self._state_tensor(key)
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)

    def restore(self, state_dict, build_fp32_params=False):
        """Load a state dict into the shadow model (strict=False: unknown keys are ignored) and, on request, into the fp32 state."""
        with torch.no_grad():
            for key in self._keys:
                if key in state_dict:
                    dst = self._shadow_tensor(key)
                    if dst.shape != state_dict[key].shape:
                        raise ValueError(f"incompatible tensor shapes between model param and ema param: {key} "
                                         f"{tuple(state_dict[key].shape)} vs. {tuple(dst.shape)}")
                    dst.copy_(state_dict[key])
        if build_fp32_params:
            self.build_fp32_params(state_dict)

    def reverse(self, model):
        """Load the averaged weights into `model` (inference or fine-tuning from the EMA, ema.py:196-202).  For a model that is NOT
        being stepped: a TrainStep updates its fp32 master weights and rewrites the model's parameters from them, so weights loaded
        into the model of a running step are gone after its next update.  To fine-tune from the average, reverse into the model
        first and build the TrainStep from it."""
        model.load_state_dict(self.state_dict()["ema"], strict=False)
        return model

    def state_dict(self):
        """{"ema": the shadow model's state dict, "ema_fp32_params": the fp32 state (None without ema_fp32)} under the model's own
        keys -- the shape of the reference's checkpoint `extra_state` (trainer.py: extra_state["ema"], ["ema_fp32_params"]).  The
        tensors are views of the live arenas, as a torch state dict's are: clone them to keep a snapshot."""
        out = {"ema": {k: self._shadow_tensor(k) for k in self._keys}, "ema_fp32_params": None}
        if self.config.ema_fp32:
            out["ema_fp32_params"] = {k: self._state_tensor(k) for k in self._keys}
        return out
