"""Train-step harness around the hot path (reference: engine/trainer.py:737-979 `Trainer.train_step`,
engine/criterion/cross_entropy.py:50-67, engine/optim/fp16_optimizer.py + adam.py).  Only the arithmetic the measured
step needs is here -- the reference's CLI, checkpointing, logging and data loading are out of scope.

Step arithmetic reproduced:
    for task in tasks: for micro-batch:  loss = CE_sum(model(slots), target); loss.backward()   (grads accumulate)
    grads   <- all_reduce_sum(grads)                      (DDP: bucketed, overlapped with the last backward)
    n       <- all_reduce_sum(sum of sample_size)         (sample_size = non-pad target tokens)
    grads   *= 1 / n                                      (== world/n after DDP's division by world, trainer.py:857-860)
    gnorm    = ||grads||_2 ; grads *= min(1, clip/(gnorm+1e-6))       (module/utils.py:342-384)
    Adam on the fp32 master copy, cast back to the model dtype        (fp16_optimizer.py:32-71, adam.py:192-212)
The multiply, the clip coefficient and Adam are ONE kernel pass over the flat arena (coef stays on the device: no host
sync anywhere in the step).
"""
import contextlib
import os
import warnings
from typing import List

import torch
import torch.utils._python_dispatch          # noqa: F401  (TorchDispatchMode: the capture audit's view of torch-native ops)

from . import criterion
from . import kernels as K
from . import ops
from .distributed import GradBucketReducer, all_reduce_scalars
from .ema import EMA, as_config
from .lib import capture_audit


class FlatParams:
    """All trainable parameters as views of one flat buffer (model dtype), with a matching flat gradient arena."""

    def __init__(self, model: torch.nn.Module):
        from .module.multihead_attention import MultiheadAttention
        # arena order = registration order, except that each attention's k|v|q (self) or k|v (cross) projection weights
        # and biases are made adjacent so ONE packed GEMM can use them (and their gradients) without any copy
        mha_of, mhas = {}, []
        for m in model.modules():
            if isinstance(m, MultiheadAttention) and m.q_proj.bias is not None:
                mhas.append(m)
                for p in (m.k_proj.weight, m.v_proj.weight, m.q_proj.weight, m.k_proj.bias, m.v_proj.bias, m.q_proj.bias):
                    mha_of[id(p)] = m
        # ... and the k|v projections of ALL the decoder layers' encoder-decoder attentions are made adjacent across layers: they
        # all read the encoder output, so the stack runs them as ONE GEMM (N = layers * 2D; ops.CrossKVShared)
        cross = [m for m in mhas if getattr(m, "encoder_decoder_attention", False) and not m.self_attention]
        cross_ok = len(cross) > 1 and len({tuple(m.k_proj.weight.shape) for m in cross}) == 1 and \
            all(m.kdim == m.vdim and m.k_proj.weight.shape == m.v_proj.weight.shape for m in cross) and \
            all(q.requires_grad for m in cross for q in (m.k_proj.weight, m.v_proj.weight, m.k_proj.bias, m.v_proj.bias))
        cross_group = []
        if cross_ok:
            cross_group = [w for m in cross for w in (m.k_proj.weight, m.v_proj.weight)] + \
                [b for m in cross for b in (m.k_proj.bias, m.v_proj.bias)]
        cross_ids = {id(q) for q in cross_group}
        seen, params = set(), []
        for p in model.parameters():
            if not p.requires_grad or id(p) in seen:
                continue
            m = mha_of.get(id(p))
            group = [p]
            if id(p) in cross_ids:
                group = cross_group
            elif m is not None:
                if m.self_attention:
                    group = [m.k_proj.weight, m.v_proj.weight, m.q_proj.weight, m.k_proj.bias, m.v_proj.bias, m.q_proj.bias]
                elif cross_ok and m in cross:
                    group = [m.q_proj.weight, m.q_proj.bias]
                else:
                    group = [m.k_proj.weight, m.v_proj.weight, m.k_proj.bias, m.v_proj.bias, m.q_proj.weight, m.q_proj.bias]
                if not all(g.requires_grad for g in group):
                    group = [p]
            for g in group:
                if id(g) not in seen:
                    seen.add(id(g))
                    params.append(g)
        assert params, "no trainable parameters"
        self.params = params
        # 4-D weights NOT consumed by ops.Conv2dFn keep torch's contiguous layout (the patch-embedding projection: ops.PatchEmbedFn
        # reshapes it to [D, C*p*p] as a view and its im2col emits columns in (c, ph, pw) order -- ADVICE r3)
        self._plain4d = {id(w) for m in model.modules() for w in getattr(m, "_ofa_plain_conv_weights", lambda: ())()}
        dtype, device = params[0].dtype, params[0].device
        self.offsets, off = [], 0
        for p in params:
            assert p.dtype == dtype and p.device == device
            self.offsets.append(off)
            off += (p.numel() + 7) // 8 * 8          # keep every view 16-byte aligned
        self.numel = off
        self.flat = torch.zeros(off, dtype=dtype, device=device)
        self.grad = torch.zeros(off, dtype=dtype, device=device)
        with torch.no_grad():
            for p, o in zip(params, self.offsets):
                self._view(self.flat, o, p).copy_(p.data)
                p.data = self._view(self.flat, o, p)
                p.grad = self._view(self.grad, o, p)
                p._ofa_grad = p.grad          # backward kernels accumulate straight into the arena (ops._sink)
                # a gradient that autograd itself delivers (a parameter used through torch's own ops) is ADDED to the arena view by
                # AccumulateGrad: a partial writer as far as the step's first-touch rule goes (ops.grad_mode) -- asked just before
                # (the engine also runs the hook with no gradient at all -- the sinks' own `return None` -- which touches nothing)
                old = getattr(p, "_ofa_grad_hook", None)
                if old is not None:                  # (an earlier FlatParams over the same parameter: its hook goes)
                    old.remove()
                p._ofa_grad_hook = p.register_hook(lambda g, v=p._ofa_grad: None if g is None else (ops.grad_mode(v, False) and None))
        off_of = {id(p): o for p, o in zip(params, self.offsets)}
        for m in mhas:
            n = 3 if m.self_attention else 2
            kw, kb = m.k_proj.weight, m.k_proj.bias
            if id(kw) not in off_of or kw.shape[0] != kw.shape[1] and not m.self_attention and m.kdim != m.embed_dim:
                continue
            D, Kin = kw.shape
            ow, ob = off_of[id(kw)], off_of[id(kb)]
            ws = [m.k_proj.weight, m.v_proj.weight, m.q_proj.weight][:n]
            bs = [m.k_proj.bias, m.v_proj.bias, m.q_proj.bias][:n]
            ok = all(off_of.get(id(w)) == ow + i * D * Kin for i, w in enumerate(ws)) and \
                all(off_of.get(id(b)) == ob + i * D for i, b in enumerate(bs)) and (D * Kin) % 8 == 0 and D % 8 == 0
            if ok:
                m._pack = {"w": self.flat[ow:ow + n * D * Kin].view(n * D, Kin), "b": self.flat[ob:ob + n * D],
                           "gw": self.grad[ow:ow + n * D * Kin].view(n * D, Kin), "gb": self.grad[ob:ob + n * D]}
        if cross_ok:
            L = len(cross)
            D, Kin = cross[0].k_proj.weight.shape
            ow, ob = off_of[id(cross[0].k_proj.weight)], off_of[id(cross[0].k_proj.bias)]
            ok = all(off_of.get(id(w)) == ow + i * D * Kin for i, w in enumerate(cross_group[:2 * L])) and \
                all(off_of.get(id(b)) == ob + i * D for i, b in enumerate(cross_group[2 * L:])) and (D * Kin) % 8 == 0 and D % 8 == 0
            if ok:
                pack = {"w": self.flat[ow:ow + 2 * L * D * Kin].view(2 * L * D, Kin), "b": self.flat[ob:ob + 2 * L * D],
                        "gw": self.grad[ow:ow + 2 * L * D * Kin].view(2 * L * D, Kin), "gb": self.grad[ob:ob + 2 * L * D],
                        "params": tuple(cross_group), "layers": L, "D": D}
                for i, m in enumerate(cross):
                    m._cross_all = (pack, i)

    def _view(self, buf, o, p):
        """Parameter p's window of an arena.  Spatial convolution weights ([Cout, Cin, kh, kw], kh * kw > 1) live in the arena in
        the order the im2col GEMM reads them -- [Cout][kh][kw][Cin], i.e. torch's channels_last strides for the same logical
        shape -- so the forward needs no permuted copy of the weight and the weight-gradient GEMM writes the arena directly
        (state dicts hold values, not strides: checkpoints interchange unchanged).  Only weights that ops.Conv2dFn consumes:
        a module lists the others in `_ofa_plain_conv_weights()`."""
        n = p.numel()
        if p.dim() == 4 and p.shape[2] * p.shape[3] > 1 and (p.shape[1] * p.shape[2] * p.shape[3]) % 8 == 0 \
                and id(p) not in self._plain4d:
            Cout, Cin, kh, kw = p.shape
            return buf[o:o + n].view(Cout, kh, kw, Cin).permute(0, 3, 1, 2)
        return buf[o:o + n].view(p.shape)

    def zero_grad(self):
        self.grad.zero_()
        self.repoint()

    def repoint(self):
        for p, o in zip(self.params, self.offsets):      # autograd may have replaced .grad; re-point it at the arena
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + o * self.grad.element_size():
                p.grad = self._view(self.grad, o, p)
                p._ofa_grad = p.grad


class _AtenAudit(torch.utils._python_dispatch.TorchDispatchMode):
    """Shows the capture audit the tensor arguments of torch-native ops too (masks, cached index tensors consumed by aten indexing or
    `cat`): the C ABI sees only its own arguments.  Thread-local, i.e. the forward pass and whatever backward work runs on the calling
    thread; the autograd engine's device thread runs this package's Functions, whose launches the audit sees through lib.ptr()."""

    def __init__(self, audit):
        super().__init__()
        self.audit = audit

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        for a in args:
            if torch.is_tensor(a):
                if a.is_cuda:
                    self.audit.see(a)
            elif isinstance(a, (list, tuple)):
                for b in a:
                    if torch.is_tensor(b) and b.is_cuda:
                        self.audit.see(b)
        self.audit.label("aten::" + getattr(func, "__name__", str(func)))
        return func(*args, **(kwargs or {}))


# Capture mode: other threads of the process (the RCCL watchdog of torch.distributed polls events) must not invalidate a
# capture in progress -- only this thread's stream is being recorded.
_CAPTURE_MODE = "thread_local"


_KEEP_ALIVE = []        # CUDAGraph objects are never destroyed: the destructor of one whose capture failed aborts the process


class _Uncapturable(Exception):
    """A sample holds something the static-input walker does not understand: the step must stay eager."""


def _walk(obj, path, out):
    """Collect every tensor of a sample (slot values may be tensors, dicts or lists of tensors -- audio slots carry
    {fbank, fbank_lengths, mask_indices}) as (path, tensor), depth first, in a deterministic order."""
    if torch.is_tensor(obj):
        out.append((path, obj))
    elif isinstance(obj, dict):
        for k in obj:                                  # insertion order: the same code builds every batch of a structure
            _walk(obj[k], path + (k,), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _walk(v, path + (i,), out)
    elif hasattr(obj, "modality") and hasattr(obj, "is_src"):           # a Slot
        _walk(obj.value, path + ("value",), out)
    elif hasattr(obj, "tensors") and hasattr(obj, "structure"):         # a packing.PackPlan: index / segment tables
        for i, t in enumerate(obj.tensors()):
            out.append((path + (i,), t))
    elif obj is None or isinstance(obj, (str, int, float, bool)) or getattr(obj, "capture_constant", False):
        pass                                           # (capture_constant: a diffusion.NoiseSchedule -- its device tables never change)
    else:
        raise _Uncapturable(f"{'/'.join(map(str, path))}: {type(obj).__name__}")


def sample_tensors(samples):
    """[(path, tensor)] over every micro-batch: all slot values, `target`, `constraint_masks` and any other tensor-valued
    entry of the sample dict (what a replay must copy into the graph's static inputs)."""
    out = []
    for i, s in enumerate(samples):
        for k in s:
            _walk(s[k], (i, k), out)
    return out


def sample_structure(samples):
    """Hashable structure of a step: per micro-batch the task key, per slot (modality, side, attributes), and per tensor
    (path, shape, dtype).  Two steps with the same structure run the same kernels on the same shapes -- the key of the graph
    cache and of the reducer's learned contribution counts."""
    sig = []
    for i, s in enumerate(samples):
        slots = tuple((getattr(sl.modality, "name", str(sl.modality)), bool(sl.is_src), tuple(sl.attributes or ()))
                      for sl in s["slots"])
        scal = tuple((k, s[k]) for k in sorted(s) if isinstance(s[k], (str, int, float, bool)))
        plan = s["pack"].structure() if s.get("pack") is not None else None          # launch bounds of a ragged batch
        diff = s["diffusion"].structure() if s.get("diffusion") is not None else None    # (the objective chooses the loss kernel's inputs)
        sig.append((slots, scal, plan) if diff is None else (slots, scal, plan, diff))
    tens = tuple((p, tuple(t.shape), str(t.dtype)) for p, t in sample_tensors(samples))
    return (tuple(sig), tens)


class TrainStep:
    """One optimisation step = `train_step(samples)`.

    use_graph: capture the step into a hipGraph (torch.cuda.graphs) and replay it.  The eager step is HOST-bound on an
    MI355X (~600 kernel launches + autograd bookkeeping take as long as the kernels themselves); a replay costs one
    launch.  Everything a replay must see fresh lives on the device: the Philox stream position (ops._Rng.base), the
    Adam step counter / bias corrections / lr (self._sched), the clip coefficient.  Each distinct batch structure
    (`sample_structure`: slot modalities / attributes, every tensor's shape and dtype) gets its own graph after
    `graph_warmup` eager steps; new batches of a captured structure are copied into the graph's static input tensors (every
    tensor of the sample: slot values incl. dict-valued audio slots, target, constraint masks).

    Data parallel (world > 1), `dp_graph`:
      "full"  (default) ONE graph holds forward, backward, the bucketed gradient all-reduces -- launched from inside backward
              as each bucket completes, so RCCL traffic over xGMI overlaps the remaining backward kernels -- the scalar
              all-reduce, clip and Adam.  RCCL collectives are captured like any other stream work.
      "split" two graphs (forward+backward, clip+Adam) around an eager bucket-by-bucket all-reduce: no overlap.  Chosen
              automatically when the process group's backend is not nccl (gloo's host-side collectives cannot be captured), or
              with dp_graph="split" / OFA_DP_GRAPH=split.
      Do not keep an autograd graph of this model alive from BEFORE the capture (outputs of an earlier forward on another
      stream): it pins the parameters' AccumulateGrad nodes to that stream and torch routes the captured backward through
      it, which invalidates the capture (ROCm: a crash in hipStreamEndCapture).  `del` such outputs first.
      A capture that fails cannot be retried in the same process (torch leaves the CUDA generator in its capturing state:
      "Cannot register the state during capturing stage" on every later capture), so there is no full -> split retry: the step
      engine warns, keeps the half-built graph objects alive (their destructor would abort the process) and runs eagerly from
      then on -- identically on every rank, the failure being structural."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_norm=1.0, process_group=None,
                 bucket_bytes: int = 64 << 20, use_graph: bool = False, graph_warmup: int = 2,
                 label_smoothing: float = 0.0, constraint_range=None, drop_worst_ratio: float = 0.0, dp_graph: str = None,
                 loss_scale=None, max_graphs: int = 16, shard_optimizer: bool = False, ema=None,
                 closed_set_edge_head: bool = False):
        """closed_set_edge_head (opt-in): a micro-batch that carries "constraint_nodes" runs the decoder for FEATURES and
        ops.trie_head_cross_entropy (csrc/trie_head.hip) -- the logits of each row's trie node's children, the loss and both gradients
        without the [rows, V] vocabulary projection -- and, in valid_step, ops.trie_head_eval.  Every other micro-batch takes the dense
        head in the same step.  Off (the default): every launch is what it was.
        ema: an ema.EMAConfig (or a dict of its fields) with store_ema set keeps an exponential moving average of the weights
        (engine/ema/ema.py), updated on the device as the last launches of every update; `self.ema` is the ema.EMA object.  Fixed at
        construction: a captured step holds exactly the launches `_update` made when it was recorded.
        shard_optimizer (data parallel, opt-in): gradients are reduce-SCATTERED, every rank clips and updates only the 1 / world of
        the arena it owns, and the updated 16-bit parameters are all-gathered (distributed.GradBucketReducer, "sharded exchange") --
        the optimizer pass (0.6 ms of an 11 ms cfg-2 step) shrinks by the world size at the all-reduce's wire volume.  The optimizer
        state arrays keep their full length (what a rank does not own is never touched); the global gradient norm is the sum of the
        ranks' partial sums of squares.  Default off: the all-reduce form is what has run on hardware."""
        self.model = model
        self.fp = FlatParams(model)
        dev = self.fp.flat.device
        self.master = self.fp.flat.float().clone() if self.fp.flat.dtype != torch.float32 else self.fp.flat
        self.exp_avg = torch.zeros(self.fp.numel, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.fp.numel, dtype=torch.float32, device=dev)
        self.betas, self.eps, self.weight_decay, self.clip_norm = betas, eps, weight_decay, clip_norm
        self.num_updates = 0
        self.group = process_group
        self.shard_optimizer = bool(shard_optimizer)
        self.reducer = GradBucketReducer(self.fp.params, self.fp.grad, self.fp.offsets, process_group, bucket_bytes,
                                         shard=self.shard_optimizer)
        self.world = self.reducer.world
        self.pad = model.global_dict.pad()
        # criterion: plain cross entropy (engine/criterion/cross_entropy.py) or, with any of these set, the label-smoothed
        # one (label_smoothed_cross_entropy.py); a sample may carry its own "constraint_masks" [B, Tt, V]
        self.label_smoothing, self.constraint_range, self.drop_worst_ratio = label_smoothing, constraint_range, drop_worst_ratio
        self.closed_set_edge_head = bool(closed_set_edge_head)
        # ... gathered in the record every route of criterion.py reads its settings from, handed in per call
        self.criterion = criterion.Settings(self.pad, model.global_dict.eos(), label_smoothing, constraint_range, drop_worst_ratio,
                                            self.closed_set_edge_head)
        self._stats = torch.zeros(3, dtype=torch.float64, device=dev)      # [sample_size, loss_sum, ntokens]
        self._ctc_stat = torch.zeros(1, dtype=torch.float64, device=dev)   # sum of the step's CTC losses (speech-to-text micro-batches)
        self._tts_stat = torch.zeros(3, dtype=torch.float64, device=dev)   # the step's [l1, mse, eos] terms (text-to-speech micro-batches)
        self._diffusion_stat = torch.zeros(1, dtype=torch.float64, device=dev)   # the step's summed main_loss (motion-diffusion micro-batches)
        self._gsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._gnorm_t = torch.zeros(1, dtype=torch.float32, device=dev)
        # device-resident schedule: _step_t = number of updates done; _lr_t = learning rate; _sched = [grad multiplier,
        # lr*sqrt(1-b2^t)/(1-b1^t), lr, skip flag of this update, count of skipped updates] consumed by ofa_adam_step(step = 0)
        self._step_t = torch.zeros(1, dtype=torch.float64, device=dev)
        self._lr_t = torch.full((1,), float(lr), dtype=torch.float64, device=dev)
        self._sched = torch.zeros(5, dtype=torch.float32, device=dev)
        self._lr = float(lr)
        self.use_graph = bool(use_graph) and dev.type == "cuda"
        # LayerDrop: the kept layers -- hence the autograd graph and every parameter's contribution count -- change per step and
        # per rank, so the step structure key says nothing about them: never captured, and the bucket reducer is never armed
        self.dynamic_autograd = any(float(getattr(m, "layerdrop", 0.0) or 0.0) > 0.0 for m in model.modules())
        if self.use_graph and self.dynamic_autograd:
            warnings.warn("ofasys_amd.TrainStep: LayerDrop draws the kept layers on the host every step; the step is not captured")
            self.use_graph = False
        # SyncBatchNorm layers exchange statistics in the middle of forward AND backward.  They do so on their own communicator
        # (ops.sync_bn_process_group, created here while every rank is at the same point), and with them in the model the bucket
        # reducer is never armed: ranks learn step structures at different times (padded lengths are part of the key), and a rank
        # that launches buckets from inside backward next to one that launches them at finish() would interleave the two kinds of
        # collectives differently -- harmless across communicators only as long as nobody's stream waits on both.  Every bucket
        # goes out at finish(), in index order, on every rank.
        self.sync_collectives = any(getattr(m, "_ofa_sync", None) not in (None, False) for m in model.modules())
        if self.sync_collectives and self.world > 1 and any(getattr(m, "_ofa_sync", None) is True for m in model.modules()):
            ops.sync_bn_process_group()
        self.graph_warmup = graph_warmup
        default_dp = "full"
        if self.world > 1:
            import torch.distributed as dist
            if dist.get_backend(process_group) != "nccl":
                default_dp = "split"
        self.dp_graph = dp_graph or os.environ.get("OFA_DP_GRAPH") or default_dp
        assert self.dp_graph in ("full", "split"), self.dp_graph
        # loss_scale: None, or a dict for the reference's DYNAMIC loss scaler (engine/optim/dynamic_loss_scaler.py; the fp16
        # trainer default, default_trainer.yaml:7-9): {"init_scale": 128, "scale_factor": 2, "scale_window": 2000, "tolerance": 0,
        # "threshold": None, "min_loss_scale": 1e-4}.  The whole state machine runs on the device (ofa_step_schedule_scaled):
        # the loss gradient is seeded with the scale, an overflowing update is skipped and the scale halved, and it grows back
        # every scale_window clean updates.  (The compute dtypes of this build are bf16 / fp32, whose exponent range makes the
        # scale numerically idle; it is here so that a reference fp16 recipe runs unchanged.)
        self.loss_scale_cfg = None
        if loss_scale is not None:
            cfg = {"init_scale": 2.0 ** 7, "scale_factor": 2.0, "scale_window": 2000, "tolerance": 0.0, "threshold": None,
                   "min_loss_scale": 1e-4}
            cfg.update(loss_scale if isinstance(loss_scale, dict) else {})
            self.loss_scale_cfg = cfg
            self._ls = torch.tensor([cfg["init_scale"], 0, -1, -1, 0, 0, 0, 0], dtype=torch.float64, device=dev)
        self._graphs = {}                           # batch structure -> dict(graphs, static samples, seen count)
        self._gsq_cleared = False
        self._rng_pending = None                    # (Philox counter, its step's advance): added by the fused norm / schedule launch
        self._tail_ticket = torch.zeros(2, dtype=torch.int32, device=dev)     # tickets of the two fused tails (they reset themselves)
        self._ce_stats = ops.StepStats(self._stats, self._tail_ticket[1:2])
        self._prezero = {}                          # batch structure -> gradient-arena ranges its partial writers need cleared up front
        # Every captured structure pins its activations: the captures share ONE memory pool (step graphs replay one at a time and
        # consume nothing of each other, so the pool's blocks are reused across them) and at most `max_graphs` structures are
        # captured -- the rest run eagerly.  Variable-length data should arrive bucketed (pad_to_multiple / packing buckets).
        self.max_graphs = int(max_graphs)
        self._pool = None
        self._warned_cap = False
        self._skipped_seen = 0.0
        self._seed = torch.ones((), dtype=torch.float32, device=dev)   # the backward seed of a micro-batch's loss (autograd's default: one fill per call)
        self.last = {}
        # validation (valid_begin / valid_step / valid_result): its accumulator [ntokens, loss_sum, nll_sum, n_correct] and its own
        # table of forward-only graphs; nothing of the training state above is written by it
        self._valid_acc = torch.zeros(4, dtype=torch.float64, device=dev)
        self._valid_ctc = torch.zeros(1, dtype=torch.float64, device=dev)      # summed CTC loss of the pass (speech-to-text micro-batches)
        # text-to-speech micro-batches: [sample_size, sample_size * (loss, l1, mse, eos), ntokens] of the pass, and whether it held any
        self._valid_tts = torch.zeros(6, dtype=torch.float64, device=dev)
        self._valid_has_tts = False
        # motion-diffusion micro-batches: [sample_size (1 each), loss, ntokens] of the pass
        self._valid_diffusion = torch.zeros(3, dtype=torch.float64, device=dev)
        self._valid_has_diffusion = False
        self._valid_decodes = []                    # per such micro-batch (greedy tokens, their lengths, encoder_target, ds), on the device
        self._valid_graphs = {}                     # (batch structure, use_ema) -> dict(graphs, static samples, seen count)
        self._warned_valid_cap = False
        ema_cfg = as_config(ema)
        self.ema = EMA(model, self.fp, ema_cfg, step_t=self._step_t) if ema_cfg is not None else None

    # ------------------------------------------------------------------ learning rate (host -> device scalar)
    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        self._lr = float(value)
        self._lr_t.fill_(self._lr)                  # outside any captured region: replays read the new value

    # ------------------------------------------------------------------ the three phases of a step
    def _fwd_bwd(self, samples, routes, overlap_reduce, structure=None):
        model = self.model
        model.train()
        ops.drop_pending()
        if self._rng_pending:                            # (a forward / backward whose update never ran: its counter advance is still due)
            self._rng_pending[0].add_(self._rng_pending[1])
            self._rng_pending = None
        # gradients: no arena-wide fill.  The first full writer of a gradient in the step stores, every later one adds (ops.grad_mode);
        # what this batch structure's partial writers need cleared is cleared here, in one launch, and what nobody writes at the end.
        # (Data parallel: the reducer reads buckets from inside backward, unwritten parameters included -- the arena is filled as before.
        #  The debug library's OFA_STEP_TAIL_OLD bit 0 selects the fill too.)
        first_touch = self.world == 1 and not K.tail_old(K.TAIL_FIRST_TOUCH)
        if first_touch:
            self.fp.repoint()
            # (structure None: eager steps share one list.  The step's statistics and the sum of squares are cleared by the same launch.)
            # (a step without a speech-to-text micro-batch launches exactly what it launched before: its CTC statistic is not touched)
            stt = (self._ctc_stat,) if "speech_to_text" in routes else ()
            if "tacotron2" in routes:                # (likewise: the text-to-speech terms are cleared only by a step that adds to them)
                stt += (self._tts_stat,)
            if "diffusion" in routes:
                stt += (self._diffusion_stat,)
            ops.grad_begin(self.fp.grad, self._prezero.get(structure, ()), also=(self._stats, self._gsq) + stt)
            self._gsq_cleared = True
        else:
            ops.grad_abort()
            self.fp.zero_grad()
            self._stats.zero_()
            if "speech_to_text" in routes:
                self._ctc_stat.zero_()
            if "tacotron2" in routes:
                self._tts_stat.zero_()
            if "diffusion" in routes:
                self._diffusion_stat.zero_()
        self.reducer.overlap = overlap_reduce
        # gradients are only read after backward unless buckets are all-reduced from inside it: fold lazily, in batches
        ops.defer_reductions(self.world == 1 or not overlap_reduce)
        self.reducer.begin_step(structure, dynamic=self.dynamic_autograd or self.sync_collectives)
        try:
            self._micro_batches(samples, routes)
            ops.flush_folds()
        except BaseException:
            ops.grad_abort()                         # (every sink adds again: nothing of this step's touched set outlives it)
            raise
        if first_touch:
            demand, _ = ops.grad_end()               # (before the gradient norm: clears what nobody wrote)
            if demand:
                if len(self._prezero) >= 256 and structure not in self._prezero:
                    self._prezero.clear()
                self._prezero[structure] = sorted(set(self._prezero.get(structure, ())) | set(demand))
        # (one owned range and no collective between the norm and the schedule: the counter add rides in that launch, see _update)
        self._rng_pending = ops.rng_defer() if self._fused_norm() else ops.rng_advance()

    def _fused_norm(self):
        return self.world == 1 and not K.tail_old(K.TAIL_NORM_SCHEDULE)

    output_projection = staticmethod(criterion.output_projection)

    def _criterion_inputs(self, model, s, features=False, encoder_out=False):
        """criterion.forward with the engine's settings, under the name and with the tuple the tests' oracles take:
        (logits or features, target, masks, nodes, pack plan[, the encoder's output dict])."""
        kind = "trie_head" if features else "speech_to_text" if encoder_out else "plain"
        x = criterion.forward(model, s, kind, self.criterion)
        return x[:5] + ((x.encoder_out,) if encoder_out else ())

    def _loss_seed(self, loss=None):
        """The backward seed of a micro-batch's loss: the engine's constant ones tensor (autograd's default is one fill per call), which
        the criteria that write the logits' gradient in their forward are told in advance (ops._SeededGrad).  None under loss scaling:
        the seed is then the scale (FP16Optimizer.backward: loss * loss_scale, fp16_optimizer.py:92-102), a device value.
        loss: the loss about to be seeded -- one of another shape, dtype or device gets a new constant."""
        if self.loss_scale_cfg is not None:
            return None
        if loss is not None and (self._seed.shape != loss.shape or self._seed.dtype != loss.dtype or self._seed.device != loss.device):
            self._seed = torch.ones_like(loss)
        return self._seed

    def _micro_batches(self, samples, routes):
        """Forward, the routed criterion (criterion.py), backward and the step statistics of every micro-batch."""
        cfg = self.criterion
        fused = self._ce_stats if (self.fp.flat.is_cuda and not K.tail_old(K.TAIL_CRITERION_STATS)) else None
        for s, kind in zip(samples, routes):
            x = criterion.forward(self.model, s, kind, cfg)
            loss, n, size = criterion.train_loss(self.model, s, kind, x, cfg, seed=self._loss_seed(), stats=fused, ctc_stat=self._ctc_stat,
                                                      tts_stat=self._tts_stat, diffusion_stat=self._diffusion_stat)
            counted = False
            if n is None:                            # the plain route: its statistics are added before the backward
                if fused is not None and fused.done:     # (the criterion kernel's last block added them)
                    counted = True
                elif loss.is_cuda and loss.dtype == torch.float32 and x.target.is_contiguous() and x.target.dtype == torch.int64:
                    # [sample_size, loss_sum, ntokens] += (non-pad targets, loss, non-pad targets) in one launch
                    K.step_stats_add(self._stats, loss.detach(), x.target, self.pad)
                    counted = True
                else:
                    n = x.target.ne(self.pad).sum()
            seed = self._loss_seed(loss)
            loss.backward(seed if seed is not None else self._ls[0].to(loss.dtype))
            if not counted:
                self._stats[0] += n if size is None else size
                self._stats[1] += loss.detach().double()
                self._stats[2] += n

    def _reduce(self):
        self.reducer.finish()
        all_reduce_scalars(self._stats, self.group)

    def _update(self):
        # coef = (1/sample_size) * min(1, clip / (||g/sample_size|| + 1e-6)), all on the device; a non-finite norm or an empty
        # batch sets the skip flag instead (ofa_step_schedule) and ofa_adam_step leaves weights and moments untouched
        owned = self.reducer.owned_ranges()              # the whole arena, or (sharded optimizer) this rank's pieces of the buckets
        pending, self._rng_pending = self._rng_pending, None
        if self._fused_norm() and len(owned) == 1 and owned[0][2] and owned[0][1] > owned[0][0]:
            # the sum of squares, its fold, the schedule and the Philox counter add in one launch (ofa_sumsq_schedule)
            lo, hi, _ = owned[0]
            c = self.loss_scale_cfg or {}
            K.sumsq_schedule(self.fp.grad[lo:hi], self._gsq, self._tail_ticket[0:1], self._stats, self._step_t, self._lr_t, self._sched,
                             self._gnorm_t, self.clip_norm, self.betas[0], self.betas[1],
                             loss_scaler=self._ls if self.loss_scale_cfg is not None else None,
                             scale_factor=c.get("scale_factor", 2.0), scale_window=c.get("scale_window", 2000),
                             tolerance=c.get("tolerance", 0.0), threshold=c.get("threshold"), min_loss_scale=c.get("min_loss_scale", 1e-4),
                             counter=pending[0] if pending else None, counter_add=pending[1] if pending else 0)
            self._gsq_cleared = False
            self._finish_update(owned)
            return
        if pending:
            pending[0].add_(pending[1])
        if not self._gsq_cleared:                        # (a first-touch step cleared it with its gradients: nothing wrote it since)
            self._gsq.zero_()
        self._gsq_cleared = False
        for lo, hi, counted in owned:
            if counted:
                K.sumsq(self.fp.grad[lo:hi], self._gsq)
        if self.shard_optimizer and self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(self._gsq, op=dist.ReduceOp.SUM, group=self.group)      # the global norm: every element counted once
        if self.loss_scale_cfg is None:
            K.step_schedule(self._gsq, self._stats, self._step_t, self._lr_t, self._sched, self._gnorm_t, self.clip_norm,
                            self.betas[0], self.betas[1])   # adam.py:205-207 + the clip coefficient, one device thread
        else:
            c = self.loss_scale_cfg
            K.step_schedule_scaled(self._gsq, self._stats, self._step_t, self._lr_t, self._sched, self._gnorm_t, self._ls,
                                   self.clip_norm, self.betas[0], self.betas[1], c["scale_factor"], c["scale_window"],
                                   c["tolerance"], c["threshold"], c["min_loss_scale"])
        self._finish_update(owned)

    def _finish_update(self, owned):
        for lo, hi, _ in owned:
            K.adam_step(self.master[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], self.fp.grad[lo:hi], self.fp.flat[lo:hi],
                        self._sched, 0.0, self.betas[0], self.betas[1], self.eps, self.weight_decay, 0)
        self.reducer.gather_params(self.fp.flat)         # (sharded optimizer: the other ranks' updated parameters)
        self._gnorm = self._gnorm_t
        if self.ema is not None:                         # after the gather: every rank averages the full, updated parameters
            self.ema._enqueue(self._step_t, self._sched)

    def check(self):
        """Host-side poll of the device guard (ONE sync): raises FloatingPointError as engine/trainer.py:866-876 does when an
        update since the last call saw a non-finite gradient norm or no target token (that update was skipped on the device)."""
        if self.loss_scale_cfg is not None:          # overflows are the scaler's business (trainer.py:957-960 logs and goes on) ...
            if float(self._ls[5]) != 0.0:            # ... until the scale hits the floor (dynamic_loss_scaler.py:58-66)
                raise FloatingPointError(f"Minimum loss scale reached ({self.loss_scale_cfg['min_loss_scale']}). Your loss is "
                                         "probably exploding. Try lowering the learning rate, using gradient clipping or "
                                         "increasing the batch size.")
            return
        skipped = float(self._sched[4])
        if skipped > self._skipped_seen:
            n = int(skipped - self._skipped_seen)
            self._skipped_seen = skipped
            raise FloatingPointError(f"gradients are Nan/Inf (or sample_size == 0) in {n} update(s): skipped on the device")

    # ------------------------------------------------------------------ graph plumbing
    def captured_graphs(self):
        return sum(1 for e in self._graphs.values() if "graphs" in e)

    def _capture(self, samples, routes, structure, mode):
        import gc
        gc.collect()                      # drop unreachable autograd graphs (see the class docstring) before recording
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        pool = self._pool
        entry = {"static": samples, "graphs": [], "mode": mode}
        # A captured kernel node holds raw addresses.  What the capture allocates lives in the graphs' private pool; everything older
        # lives in the default pool and stays mapped only while Python holds it.  lib.capture_audit records every such tensor a
        # C-ABI call of the capture addresses (and _AtenAudit the inputs of the forward's torch-native ops); the entry PINS them, so
        # that no cache that later drops or regrows a tensor (ops.cached_index, SegmentPlan, a grown mask) can unmap memory a graph
        # still reads -- the allocator flush at the entry of the NEXT capture would otherwise hand it back to the driver.
        with capture_audit() as audit, _AtenAudit(audit):
            if self.world == 1 or mode == "full":
                g = torch.cuda.CUDAGraph()
                _KEEP_ALIVE.append(g)
                with torch.cuda.graph(g, pool=pool, capture_error_mode=_CAPTURE_MODE):
                    self._fwd_bwd(samples, routes, overlap_reduce=self.world > 1, structure=structure)
                    if self.world > 1:
                        self._reduce()
                    self._update()
                entry["graphs"] = [g]
            else:
                ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                _KEEP_ALIVE.extend((ga, gb))
                with torch.cuda.graph(ga, pool=pool, capture_error_mode=_CAPTURE_MODE):
                    self._fwd_bwd(samples, routes, overlap_reduce=False)
                with torch.cuda.graph(gb, pool=pool, capture_error_mode=_CAPTURE_MODE):
                    self._update()
                entry["graphs"] = [ga, gb]
        entry["audit"] = audit
        if os.environ.get("OFA_CAPTURE_PINS", "1") != "0":          # (0: the audit tool's negative control -- reproduces a dangling pointer)
            entry["pins"] = audit.tensors()
        return entry

    def owned_tensors(self):
        """Tensors whose lifetime is the step engine's / the model's own (what a capture may address without a pin)."""
        own = list(self.model.parameters()) + list(self.model.buffers())
        own += [self.fp.flat, self.fp.grad, self.master, self.exp_avg, self.exp_avg_sq, self._stats, self._gsq, self._gnorm_t,
                self._step_t, self._lr_t, self._sched, self._seed, getattr(self, "_ls", None), self._valid_acc, self._ctc_stat,
                self._valid_ctc, self._tts_stat, self._valid_tts, self._diffusion_stat, self._valid_diffusion]
        own += list(ops._Rng.base.values())
        if self.ema is not None:
            own += self.ema.arenas()
        return own

    def audit_report(self, entry):
        """[(first C-ABI call, shape, dtype, storage bytes)]: default-pool tensors the captured graphs of `entry` address that neither
        the engine, the model nor the entry's static inputs own -- each one is kept alive by entry["pins"] only."""
        own = self.owned_tensors() + [t for _, t in sample_tensors(entry["static"])]
        return entry["audit"].foreign(own)

    def _replay(self, entry, samples):
        if samples is not entry["static"]:
            # ONE batched copy launch (K.copy_batched) instead of one ~3.5 us copy launch per tensor (34 per cfg-2 step, 77 per cfg-2b step)
            K.copy_batched([(dst, src) for (_, dst), (_, src) in zip(entry["static_tensors"], sample_tensors(samples)) if dst is not src])
        entry["graphs"][0].replay()
        if len(entry["graphs"]) == 2:
            self.reducer.overlap = False
            self.reducer.begin_step(None)
            self._reduce()
            entry["graphs"][1].replay()

    def train_step(self, samples: List[dict], eager: bool = False):
        """samples: one dict per (task, micro-batch): {"slots": [...], "target": LongTensor[B,Tt], optional "task", "pack"} and the keys
        that choose its criterion (criterion.py has the table): "constraint_masks"; "reward" (fp32, one value per row of `target`: SCST,
        optional "constraint_range": "start,end" and "sentence_avg": True); "constraint_nodes" (int32 [B, Tt], -1 where no closed set
        applies) with "constraint_trie" (Task.constraint_trie_on; optional "constraint_nodes_packed" as "target_packed"); "encoder_target"
        with "ctc_range"; "target_lengths" (int64 [B]) with a floating-point "target" [B, T, F] of fbank frames: text-to-speech, the
        ofa_tacotron2 criterion (optional "bce_pos_weight", "sentence_avg"), whose step reports l1_loss / mse_loss / eos_loss in `last`.
        "diffusion" (a diffusion.NoiseSchedule) with one target slot of continuous motion frames (adaptor/motion_6d.py): diffusion training
        (optional "noise" / "noise_level": the draws; "scale_main_loss", "criterion_weight"), whose step reports main_loss in `last`.
        criterion.route names each micro-batch's criterion, or refuses the dict, before anything runs."""
        routes = [criterion.route(s, self.criterion) for s in samples]
        done = False
        structure = None
        if (self.use_graph and not eager) or self.world > 1:
            try:
                structure = sample_structure(samples)
            except _Uncapturable as e:
                if self.use_graph:
                    warnings.warn(f"ofasys_amd.TrainStep: a sample holds an object the static-input walker does not know ({e}); "
                                  "running eagerly")
                    self.use_graph = False
        if self.use_graph and not eager and structure is not None:
            entry = self._graphs.get(structure)
            if entry is None:
                if len(self._graphs) >= 64 * max(self.max_graphs, 1):       # bound the bookkeeping of never-captured structures too
                    self._graphs = {k: e for k, e in self._graphs.items() if "graphs" in e}
                entry = self._graphs[structure] = {"seen": 0}
            if "graphs" not in entry and entry["seen"] >= self.graph_warmup and self.captured_graphs() >= self.max_graphs:
                if not self._warned_cap:
                    warnings.warn(f"ofasys_amd.TrainStep: {self.max_graphs} batch structures are captured already; further ones run "
                                  "eagerly (bucket the padded lengths -- pad_to_multiple / packing buckets -- or raise max_graphs)")
                    self._warned_cap = True
            elif "graphs" in entry:
                self._replay(entry, samples)
                done = True
            elif entry["seen"] >= self.graph_warmup and (self.world == 1 or self.dp_graph != "full"
                                                         or self.reducer.knows(structure) or self.graph_warmup == 0):
                mode = "full" if (self.world > 1 and self.dp_graph == "full") else "split"
                rng_state = ops._Rng.offset
                try:
                    torch.cuda.synchronize()
                    cap = self._capture(samples, routes, structure, mode)
                except Exception as e:              # anything uncapturable (a custom adaptor, a collective): eager from now on
                    warnings.warn(f"ofasys_amd.TrainStep: hipGraph capture ({mode}) failed ({type(e).__name__}: {e}); a failed "
                                  "capture cannot be retried in this process -- running eagerly")
                    ops._Rng.offset = rng_state
                    ops.defer_reductions(False)
                    self.use_graph = False
                else:
                    cap["static_tensors"] = sample_tensors(cap["static"])
                    entry.update(cap)
                    self._replay(entry, samples)
                    done = True
            else:
                entry["seen"] += 1
        if not done:
            self._fwd_bwd(samples, routes, overlap_reduce=True, structure=structure)
            self._reduce()
            self._update()
        self.num_updates += 1
        self.last = {"stats": self._stats, "gnorm": self._gnorm, "skipped": self._sched[3:5]}
        if "speech_to_text" in routes:
            self.last["ctc_loss"] = self._ctc_stat          # (the step's summed CTC term; other steps report what they always did)
        if "tacotron2" in routes:                           # (the terms of the step's text-to-speech micro-batches, summed over them)
            self.last["l1_loss"], self.last["mse_loss"], self.last["eos_loss"] = self._tts_stat[0:1], self._tts_stat[1:2], self._tts_stat[2:3]
        if "diffusion" in routes:                           # (the summed loss of the step's motion-diffusion micro-batches: sample_size 1 each)
            self.last["main_loss"] = self._diffusion_stat
        if self.loss_scale_cfg is not None:
            self.last["loss_scale"] = self._ls[0:1]
        return self.last

    # ------------------------------------------------------------------ validation: forward only, no training state touched
    def valid_begin(self):
        """Start a validation pass: zero the accumulator [ntokens, loss_sum, nll_sum, n_correct] (a device tensor the engine owns)."""
        self._valid_acc.zero_()
        self._valid_ctc.zero_()
        self._valid_tts.zero_()
        self._valid_has_tts = False
        self._valid_diffusion.zero_()
        self._valid_has_diffusion = False
        self._valid_decodes = []

    @contextlib.contextmanager
    def _valid_mode(self, model):
        """`model` as a validation forward runs it: eval mode, no autograd, and the decoder layers' `need_attn` off -- in eval mode a
        layer otherwise returns its cross-attention weights (the reference's layers do: its generators turn that off with
        make_generation_fast_), which nobody reads here and which takes attention off the fused kernels (packed batches run on those
        alone).  On exit the mode and the flags are as they were found, and so is the host side of the Philox position (eval mode
        draws nothing unless a module says apply_during_inference)."""
        was_training = model.training
        flagged = [m for m in model.modules() if getattr(m, "need_attn", None) is True]
        rng = ops._Rng.offset
        model.eval()
        for m in flagged:
            m.need_attn = False
        try:
            with torch.no_grad():
                yield model
        finally:
            for m in flagged:
                m.need_attn = True
            ops._Rng.offset = rng
            model.train(was_training)

    def _valid_forward(self, samples, routes, model):
        """The micro-batches through `model` (see _valid_mode) and through criterion.evaluate into the accumulator (and `_valid_ctc`).
        Nothing here reads or writes the gradient arena, the step statistics, the optimizer or EMA state or the device counters.
        -> [(tokens, lengths, encoder_target, ds)], the greedy CTC decodes of the speech-to-text micro-batches: the caller keeps
        copies until the pass ends."""
        outs = []
        with self._valid_mode(model):
            for s, kind in zip(samples, routes):
                x = criterion.forward(model, s, kind, self.criterion)
                decode = criterion.evaluate(model, s, kind, x, self.criterion, self._valid_acc, self._valid_ctc, self._valid_tts,
                                            self._valid_diffusion)
                if decode is not None:
                    outs.append(decode)
        return outs

    def _keep_decodes(self, outs):
        """Copies of a batch's greedy decodes (a replayed graph writes the same buffers again) wait on the device for valid_result."""
        self._valid_decodes += [(t.clone(), n.clone(), et.clone(), ds) for t, n, et, ds in outs]

    def captured_valid_graphs(self):
        return sum(1 for e in self._valid_graphs.values() if "graphs" in e)

    def _capture_valid(self, samples, routes, model):
        import gc
        gc.collect()
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        entry = {"static": samples, "graphs": []}
        with capture_audit() as audit, _AtenAudit(audit):          # (the pins: see _capture)
            g = torch.cuda.CUDAGraph()
            _KEEP_ALIVE.append(g)
            with torch.cuda.graph(g, pool=self._pool, capture_error_mode=_CAPTURE_MODE):
                entry["decodes"] = self._valid_forward(samples, routes, model)
            entry["graphs"] = [g]
        entry["audit"] = audit
        entry["pins"] = audit.tensors()
        return entry

    def _replay_valid(self, entry, samples):
        if samples is not entry["static"]:
            K.copy_batched([(dst, src) for (_, dst), (_, src) in zip(entry["static_tensors"], sample_tensors(samples)) if dst is not src])
        entry["graphs"][0].replay()
        self._keep_decodes(entry["decodes"])

    def valid_step(self, samples: List[dict], eager: bool = False, use_ema: bool = False):
        """One validation batch: the micro-batch dicts `train_step` takes (pack plans, target_packed, constraint_masks,
        constraint_nodes + constraint_trie [+ constraint_nodes_packed], with the same refusals), forward only, accumulated on the device
        (engine/trainer.py:982-1030 `valid_step`; the criterion in eval mode, label_smoothed_cross_entropy.py:114-198).  A micro-batch
        with "reward" (SCST) is refused: the reference validates those by generating.  use_ema: the forward runs on the averaged
        model (`self.ema.get_model()`).  With use_graph, one forward-only hipGraph per (batch structure, use_ema) is captured after
        `graph_warmup` eager visits -- its own table and its own cap of `max_graphs`, the engine's memory pool -- and replayed.
        Nothing is returned and nothing synchronises: `valid_result()` reads the pass."""
        routes = [criterion.route(s, self.criterion, training=False) for s in samples]
        self._valid_has_tts = self._valid_has_tts or "tacotron2" in routes
        self._valid_has_diffusion = self._valid_has_diffusion or "diffusion" in routes
        if use_ema:
            if self.ema is None:
                raise RuntimeError("valid_step(use_ema=True) needs an EMA of the weights: build the engine with ema={'store_ema': True}")
            model = self.ema.get_model()
        else:
            model = self.model
        structure = None
        if self.use_graph and not eager:
            try:
                structure = (sample_structure(samples), bool(use_ema))
            except _Uncapturable:
                structure = None                    # (train_step warns about such samples; validation just runs them eagerly)
        if structure is not None:
            entry = self._valid_graphs.get(structure)
            if entry is None:
                if len(self._valid_graphs) >= 64 * max(self.max_graphs, 1):
                    self._valid_graphs = {k: e for k, e in self._valid_graphs.items() if "graphs" in e}
                entry = self._valid_graphs[structure] = {"seen": 0}
            if "graphs" in entry:
                self._replay_valid(entry, samples)
                return
            if entry["seen"] >= self.graph_warmup:
                if self.captured_valid_graphs() >= self.max_graphs:
                    if not self._warned_valid_cap:
                        warnings.warn(f"ofasys_amd.TrainStep: {self.max_graphs} validation batch structures are captured already; "
                                      "further ones run eagerly (bucket the padded lengths or raise max_graphs)")
                        self._warned_valid_cap = True
                else:
                    try:
                        torch.cuda.synchronize()
                        cap = self._capture_valid(samples, routes, model)
                    except Exception as e:
                        warnings.warn(f"ofasys_amd.TrainStep: hipGraph capture (validation) failed ({type(e).__name__}: {e}); a failed "
                                      "capture cannot be retried in this process -- running eagerly")
                        self.use_graph = False
                    else:
                        cap["static_tensors"] = sample_tensors(cap["static"])
                        entry.update(cap)
                        self._replay_valid(entry, samples)
                        return
            else:
                entry["seen"] += 1
        self._keep_decodes(self._valid_forward(samples, routes, model))

    def valid_result(self):
        """The pass since valid_begin(): ONE synchronisation (and, data parallel, one all-reduce of the accumulator) ->
        dict(loss, nll_loss, ppl, ntokens, sample_size, n_correct, total, accuracy); see `valid_metrics`.  A pass that held
        speech-to-text micro-batches with ctc_weight > 0 also reports ctc_loss (the summed CTC loss, natural log), c_errors and
        c_total: the unit-level edit distance of the greedy CTC decode against the labels and the label count
        (speech_to_text_loss.py:294-300), computed here on the host with ops.edit_distance -- this rank's figures.  Word-level WER,
        post_process and the KenLM decoder are out of scope."""
        res = valid_metrics(self._valid_acc, self.group if self.world > 1 else None, self.world)
        if self._valid_decodes:
            res["ctc_loss"] = float(self._valid_ctc)
            pad, eos = self.pad, self.model.global_dict.eos()
            errs = total = 0
            for toks, n, et, ds in self._valid_decodes:
                toks, n, et = toks.tolist(), n.tolist(), et.tolist()
                for b in range(len(n)):
                    ref = [v - ds for v in et[b] if v != pad and v != eos]
                    errs += ops.edit_distance(toks[b][:n[b]], ref)
                    total += len(ref)
            res["c_errors"], res["c_total"] = errs, total
        if self._valid_has_tts:
            # text-to-speech batches (tacotron2_loss.py:201-214 `reduce_metrics`): every value is the batches' mean weighted by their
            # sample_size, natural units (no base-2 conversion there); a pass of such batches alone reports these as its loss
            acc = self._valid_tts
            if self.world > 1:
                acc = all_reduce_scalars(acc.clone(), self.group)
            ss, loss, l1, mse, eos, ntok = acc.tolist()
            d = ss + 1e-8
            res.update({"l1_loss": l1 / d, "mse_loss": mse / d, "eos_loss": eos / d})
            if res["ntokens"] == 0:
                res.update({"loss": loss / d, "ntokens": ntok, "sample_size": ss})
            else:
                res["tts_loss"] = loss / d
        if self._valid_has_diffusion:
            # motion-diffusion batches (diffusion_loss.py:88-102 `reduce_metrics`): the losses' sum over sample_size (1 per batch),
            # natural units; a pass of such batches alone reports it as its loss
            acc = self._valid_diffusion
            if self.world > 1:
                acc = all_reduce_scalars(acc.clone(), self.group)
            ss, loss, ntok = acc.tolist()
            res["main_loss"] = loss / max(ss, 1.0)
            if res["ntokens"] == 0:
                res.update({"loss": loss / max(ss, 1.0), "ntokens": ntok, "sample_size": ss})
        return res


def valid_metrics(acc, group=None, world=1):
    """The accumulator [ntokens, loss_sum, nll_sum, n_correct] (fp64 [4]; summed over the ranks of `group` when world > 1, on a copy)
    -> the reference's validation log (label_smoothed_cross_entropy.py:200-238 `reduce_metrics`): loss per sample_size and nll_loss
    per token in base 2, ppl = 2 ** nll_loss, accuracy = 100 n_correct / total.  sample_size = ntokens (sentence_avg is off).
    An empty pass gives zeros, not NaN."""
    if world > 1:
        acc = all_reduce_scalars(acc.clone(), group)
    ntokens, loss_sum, nll_sum, n_correct = acc.tolist()            # the one synchronisation
    ln2 = 0.6931471805599453
    nll = nll_sum / max(ntokens, 1.0) / ln2
    return {"loss": loss_sum / max(ntokens, 1.0) / ln2, "nll_loss": nll, "ppl": 2.0 ** nll if nll < 1000.0 else float("inf"), "ntokens": ntokens, "sample_size": ntokens,
            "n_correct": n_correct, "total": ntokens, "accuracy": 100.0 * n_correct / max(ntokens, 1.0)}


Trainer = TrainStep           # the name round-1 code and tests use; `ofasys_amd.Trainer` is the fit() facade (engine.py)
