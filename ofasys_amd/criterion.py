"""Which criterion a micro-batch takes, and the host code that applies it (the kernels and autograd Functions are ops.py's).

A micro-batch is the dict `TrainStep.train_step` / `valid_step` take.  `route` reads its keys and scalars -- no tensor data, no model,
no device -- and names the criterion or refuses the dict; `forward` runs the model and lays the criterion's inputs out; `train_loss`
and `evaluate` apply the routed criterion in the two directions.  The engine computes the routes of a step's micro-batches once, up
front, so a refusal fires BEFORE the model forward of the step (it used to fire after the refused micro-batch's own forward); types,
messages and precedence are what they were.

    route            keys of the micro-batch                                 training                       validation
    speech_to_text   encoder_target + ctc_range                              label-smoothed CE + CTC        criterion_eval, CTC loss + greedy decode
    trie_head        constraint_nodes (+ constraint_trie), edge_head set     trie_head_cross_entropy        trie_head_eval
    trie_nodes       constraint_nodes (+ constraint_trie)                    trie_label_smoothed_c._e.      criterion_eval(nodes)
    scst             reward                                                  scst_loss                      refused
    label_smoothed   constraint_masks, or any of label_smoothing /           label_smoothed_cross_entropy   criterion_eval
                     constraint_range / drop_worst_ratio set
    plain            none of these                                           cross_entropy_sum              criterion_eval

A text-to-speech micro-batch -- "target_lengths" next to a floating-point "target" [B, T, F] of fbank frames -- takes the one route outside
that table, "tacotron2" (EXTRA_ROUTES): the model returns (post, extra) and ops.tacotron2_loss applies the reference's ofa_tacotron2
criterion (engine/criterion/tacotron2_loss.py) with reduction "mean"; validation is the same kernel without the gradient.  It carries
none of the token criteria's keys and no pack plan (the postnet runs over the padded layout), and the reference criterion's guided
attention loss and its own CTC term are refused.

A motion-diffusion micro-batch -- "diffusion" (a diffusion.NoiseSchedule) next to ONE target slot whose value is a dict with a
floating-point "value" [B, T, Dd] (adaptor/motion_6d.py) -- takes the route "diffusion" (DIFFUSION_ROUTES): the reference's diffusion_criterion
(engine/criterion/diffusion_loss.py, module/diffusion.py `p_losses`).  `forward` draws the noise and one level per sentence on the
device (or takes "noise" / "noise_level" from the micro-batch: tests and reproduction), noises the frames (ops.diffusion_q_sample) into
a COPY of the slot value and runs the model with full_context_alignment=True (a denoiser's decoder is not causal); ops.diffusion_loss
is the weighted L1 loss and the criterion's reduction in one launch, sample_size 1.  The token criteria's keys, a pack plan, a second
target slot, a slot value that already holds "noise_level" and the two auxiliary losses (they need the BVH forward kinematics) are refused.
"""
from typing import NamedTuple, Optional, Tuple

import torch

from . import ops

ROUTES = ("speech_to_text", "trie_head", "trie_nodes", "scst", "label_smoothed", "plain")
EXTRA_ROUTES = ("tacotron2",)           # routes whose target is not a token sequence: keyed by "target_lengths", never reached without it
DIFFUSION_ROUTES = ("diffusion",)       # ... keyed by "diffusion" (kept apart: tests/test_tts_cpu.py pins EXTRA_ROUTES as it stood)


class Settings(NamedTuple):
    """The criterion's settings, handed to every function here per call (the engine builds one from its constructor arguments)."""
    pad: int
    eos: int
    label_smoothing: float = 0.0
    constraint_range: Optional[Tuple[int, int]] = None
    drop_worst_ratio: float = 0.0
    edge_head: bool = False             # a well-formed node micro-batch takes the trie-edge head (TrainStep(closed_set_edge_head=True))


class Inputs(NamedTuple):
    """What `forward` hands a criterion: by padded position, or (pack plan) by packed decoder row."""
    logits: torch.Tensor                # (trie_head: the decoder's features [.., D] stand here; the head projects them itself)
    target: torch.Tensor
    masks: Optional[torch.Tensor]
    nodes: Optional[torch.Tensor]
    plan: object
    encoder_out: Optional[dict]         # (speech_to_text alone)
    extra: Optional[dict] = None        # (tacotron2 alone: the output head's eos_out / feature_out; `logits` holds the postnet's frames)
    # (diffusion: `logits` holds the frame decoder's [B, T, max_data_dim] rows, `target` x0 or the noise (fp32), `masks` the padding
    #  mask, `extra` {"noise_level": the drawn levels})


def output_projection(model):
    """(weight [V, D], bias or None) of the decoder's text output projection: the tied token embedding, or the adaptor's own
    Linear (adaptor/text.py:72)."""
    ga = model.decoder.adaptor
    text = ga.name2adaptor["text"]
    if text.share_input_output_embed:
        return ga.embed_tokens.weight, None
    proj = text.output_projection
    return proj.weight, getattr(proj, "bias", None)


def route(s, settings, training=True):
    """Micro-batch dict -> one of ROUTES, or the refusal of a malformed one.  An absent key and a key set to None are the same.
    A malformed node micro-batch under `edge_head` is no head batch: it meets the dense path's refusal."""
    def has(k):
        return s.get(k) is not None
    if has("diffusion"):
        return _route_diffusion(s, has)
    if has("target_lengths"):
        for k in ("reward", "constraint_nodes", "constraint_masks", "encoder_target"):
            if has(k):
                raise NotImplementedError(f"a text-to-speech micro-batch (target_lengths) cannot carry {k}: its criterion is "
                                          "ofa_tacotron2 on fbank frames (engine/criterion/tacotron2_loss.py), not a token criterion")
        if has("pack"):
            raise NotImplementedError("a text-to-speech micro-batch (target_lengths) cannot carry a pack plan: the postnet convolves and "
                                      "normalises padded frames too, a packed layout would change the numbers")
        if s.get("use_guided_attention_loss"):
            raise NotImplementedError("use_guided_attention_loss is not supported: the fused attention forms no [B, A, Tt, Ts] weights "
                                      "for the guided attention loss to read")
        if float(s.get("ctc_weight", 0.0) or 0.0) > 0:
            raise NotImplementedError("ofa_tacotron2 with its own ctc_weight > 0 is not supported (tacotron2_loss.py:135-152); "
                                      "CTC training is the speech_to_text_loss criterion's")
        return "tacotron2"
    if not training and has("reward"):
        raise NotImplementedError("an SCST micro-batch (reward) cannot be validated by the criterion: the reference validates "
                                  "such tasks by generating (engine/criterion/scst_loss.py)")
    if has("pack") and has("constraint_masks"):
        raise NotImplementedError("constraint masks are laid out by padded position: run such samples without a pack plan")
    if has("constraint_nodes"):
        if has("constraint_masks"):
            raise ValueError("a micro-batch carries its closed set as constraint_masks or as constraint_nodes, not both")
        if has("reward"):
            raise NotImplementedError("an SCST micro-batch (reward) cannot carry constraint_nodes: its criterion takes a "
                                      "constraint range only (engine/criterion/scst_loss.py:214-217)")
        if not has("constraint_trie"):
            raise ValueError("constraint_nodes need \"constraint_trie\": the device arrays of the answer trie "
                             "(Task.constraint_trie_on(device))")
    if has("encoder_target") and has("ctc_range"):
        if training:                    # (validation reads the weights' signs alone and ignores the nodes: as it always did)
            ce_w, ctc_w = float(s.get("ce_weight", 1.0)), float(s.get("ctc_weight", 0.0))
            if ce_w < 0 or ctc_w < 0 or ce_w + ctc_w == 0:
                raise ValueError(f"speech_to_text_loss: ce_weight={ce_w}, ctc_weight={ctc_w}: one of them must be positive, none negative")
            if has("reward") or has("constraint_nodes"):
                raise NotImplementedError("a speech-to-text micro-batch (encoder_target) carries neither a reward nor constraint_nodes")
        return "speech_to_text"
    if has("constraint_nodes"):
        return "trie_head" if settings.edge_head else "trie_nodes"
    if has("reward"):
        if has("constraint_masks"):
            raise NotImplementedError("an SCST micro-batch (reward) cannot carry constraint_masks: its criterion takes a "
                                      "constraint range only (engine/criterion/scst_loss.py:214-217)")
        return "scst"
    if settings.label_smoothing > 0 or settings.constraint_range is not None or settings.drop_worst_ratio > 0 or has("constraint_masks"):
        return "label_smoothed"
    return "plain"


def _diffusion_slot(s):
    """The one target slot of a motion-diffusion micro-batch (module/diffusion.py:19-33), or its refusal."""
    targets = [sl for sl in s["slots"] if not sl.is_src]
    if len(targets) != 1:
        raise NotImplementedError(f"a diffusion micro-batch has {len(targets)} target slots: the diffusion decoder supports exactly one "
                                  "(module/diffusion.py:21-24)")
    v = targets[0].value
    if not (isinstance(v, dict) and torch.is_tensor(v.get("value")) and v["value"].is_floating_point() and v["value"].dim() == 3):
        raise ValueError("a diffusion micro-batch needs a target slot whose value is a dict with a floating-point \"value\" [B, T, Dd] "
                         "(the motion_6d collation: preprocessor/motion.py)")
    if v.get("masks") is None:
        raise ValueError("a diffusion micro-batch's slot value needs \"masks\" (bool [B, T], True at padding)")
    if "noise_level" in v:
        raise ValueError("the slot value of a diffusion micro-batch already holds \"noise_level\": the criterion corrupts \"value\" and injects "
                         "the level itself (module/diffusion.py:27-33); supply a level as the micro-batch's own \"noise_level\"")
    return targets[0]


def _route_diffusion(s, has):
    for k in ("reward", "constraint_nodes", "constraint_masks", "constraint_trie", "encoder_target", "target_lengths"):
        if has(k):
            raise NotImplementedError(f"a diffusion micro-batch cannot carry {k}: its criterion is diffusion_criterion on continuous "
                                      "frames (engine/criterion/diffusion_loss.py), not a token criterion")
    if has("pack"):
        raise NotImplementedError("a diffusion micro-batch cannot carry a pack plan: the denoiser's decoder attends without a causal "
                                  "mask (full_context_alignment), which the packed layout does not serve")
    for k in ("scale_aux_loss_1", "scale_aux_loss_2"):
        if float(s.get(k, 0.0) or 0.0) > 0:
            raise NotImplementedError(f"diffusion_criterion with {k} > 0 is not supported: custom_reg_loss needs the BVH header's forward "
                                      "kinematics, which is not built")
    _diffusion_slot(s)
    return "diffusion"


def _forward_diffusion(model, s):
    import copy
    sched = s["diffusion"]
    slot = _diffusion_slot(s)
    v = slot.value
    adaptor = model.decoder.adaptor.get_adaptor(slot)
    width = getattr(adaptor, "max_data_dim", None)
    if width is None:
        raise ValueError("a diffusion micro-batch's target slot must select the motion_6d adaptor ([MOTION:...,adaptor=motion_6d])")
    if adaptor.max_noise_levels < sched.num_train_timesteps + 1:
        raise ValueError(f"motion_6d: max_noise_levels {adaptor.max_noise_levels} < num_train_timesteps + 1 = {sched.num_train_timesteps + 1}")
    x0 = v["value_0"] if v.get("value_0") is not None else v["value"]
    x0 = x0 if x0.dtype == torch.float32 else x0.float()
    B = x0.shape[0]
    # the draws of p_losses (module/diffusion.py:158-159), on the device with torch's generator -- capture-aware: a replayed step draws
    # anew -- unless the micro-batch supplies them
    noise = s["noise"] if s.get("noise") is not None else torch.randn_like(x0)
    t = s["noise_level"] if s.get("noise_level") is not None else \
        torch.randint(0, sched.num_train_timesteps, (B,), device=x0.device, dtype=torch.long)
    noise = noise if noise.dtype == torch.float32 else noise.float()
    dtype = adaptor.frame_encoder[0].weight.dtype
    known_w = v.get("known_w")
    if known_w is not None and known_w.dtype != torch.float32:
        known_w = known_w.float()
    value = ops.diffusion_q_sample(x0, noise, t, sched, width, dtype, known_w=known_w, masks=v["masks"])
    noised = copy.copy(slot)
    noised.value = dict(v, value=value, noise_level=t, data_dim=int(x0.shape[-1]))
    slots = [noised if sl is slot else sl for sl in s["slots"]]
    pred, _ = model(slots, full_context_alignment=True)[:2]
    target = x0 if sched.prediction_type == "sample" else noise
    return Inputs(pred, target, v["masks"], None, None, None, {"noise_level": t})


def _diffusion_scale(s):
    """scale_main_loss times the criterion's weight (diffusion_loss.py:57, :85)."""
    return float(s.get("scale_main_loss", 1.0)) * float(s.get("criterion_weight", 1.0))


def _diffusion_ntokens(x):
    return x.masks.numel() - x.masks.sum()


def forward(model, s, kind, settings):
    """One micro-batch through `model` -> Inputs.  The train step and the validation step share it."""
    if kind == "diffusion":
        return _forward_diffusion(model, s)
    if kind == "tacotron2":                      # (no pack plan: route refused one) -> the frames after the postnet, and the head's extras
        post, extra = model(s["slots"])
        return Inputs(post, s["target"], None, None, None, None, extra)
    plan = s.get("pack")
    kw = {"features_only": True} if kind == "trie_head" else {"return_encoder_out": True} if kind == "speech_to_text" else {}
    if plan is not None:                         # ragged batch (packing.py): logits and targets by packed decoder row
        kw["pack"] = plan
    out = model(s["slots"], **kw)
    target = s["target"]
    if plan is not None:
        target = s.get("target_packed")
        if target is None:
            idx = plan.dec_index
            target = s["target"].reshape(-1)[idx.clamp_min(0)].masked_fill(idx < 0, settings.pad).view(1, -1)
    # closed-set targets by trie node (collate's closed_set_nodes): one int32 per target position instead of a mask row, and
    # "constraint_trie", the task's device arrays of the answer trie; the nodes follow the targets into a packed layout
    nodes = s.get("constraint_nodes")
    if nodes is not None and plan is not None:
        packed = s.get("constraint_nodes_packed")
        if packed is None:
            idx = plan.dec_index
            packed = nodes.reshape(-1)[idx.clamp_min(0)].masked_fill(idx < 0, -1)
        nodes = packed.view(1, -1)
    return Inputs(out[0], target, s.get("constraint_masks"), nodes, plan, out[2] if kind == "speech_to_text" else None)


def _ctc(model, s, x, settings, stat):
    """The CTC side of a speech-to-text micro-batch -> (loss, the CTC logits: the encoder output's projection onto rows ds:de of the
    token embedding, their ops.CtcLayout, ds); the summed loss is added to `stat` on the device."""
    ds, de = (int(v) for v in s["ctc_range"].split(","))
    enc = x.encoder_out["encoder_out"][0]                # T x B x C, or packed rows [rows, 1, C]
    weight = model.decoder.adaptor.embed_tokens.weight   # (:218: rows ds:de of the decoder's token embedding)
    y = ops.encoder_ctc_logits(enc, weight, ds, de)
    if x.plan is not None:
        lay = ops.CtcLayout.packed(x.plan.enc_self)
    else:
        # input lengths: the non-pad encoder positions of a sentence, counted over the whole source (:347-350); like the
        # reference, the first `length` time steps are the ones read
        masks = x.encoder_out["encoder_padding_mask"][0]
        lengths = masks.shape[1] - masks.sum(1) if masks is not None else torch.full((enc.shape[1],), enc.shape[0], device=enc.device)
        bm = not y.is_contiguous() and y.transpose(0, 1).is_contiguous()
        lay = ops.CtcLayout.padded(lengths, y.shape[0], batch_major=bm)
    loss, _ = ops.ctc_loss(y, lay, s["encoder_target"], ds, settings.pad, settings.eos, bool(s.get("zero_infinity", False)),
                           stat=stat)                    # (the statistic takes the fp64 sum, before its rounding to fp32)
    return loss, y, lay, ds


def _tacotron_size(s):
    """sample_size of a text-to-speech micro-batch on the device (tacotron2_loss.py:155): nsentences under sentence_avg, else ntokens =
    the sum of the target lengths -> (ntokens, sample_size or None: ntokens)."""
    n = s["target_lengths"].sum()
    return n, (s["target"].shape[0] if s.get("sentence_avg") else None)


def train_loss(model, s, kind, x, cfg, seed=None, stats=None, ctc_stat=None, tts_stat=None, diffusion_stat=None):
    """The routed criterion on x = forward(...) -> (loss, ntokens, sample_size or None: ntokens).  ntokens is None on the plain route:
    its statistics are the caller's (with `stats`, an ops.StepStats, the criterion kernel may have added them: stats.done).
    seed: the tensor the caller will hand to loss.backward (ops._SeededGrad), None when it is not known yet (loss scaling); the routes
    whose forward can write the logits' gradient take it."""
    size = None
    if kind == "diffusion":
        # the weighted L1 loss, the per-sentence masked mean and the prediction's gradient in one launch; sample_size is 1
        # (diffusion_loss.py:59); the loss is added to `diffusion_stat` (fp64 [1]) on the device: the step's main_loss
        loss = ops.diffusion_loss(x.logits, x.target, x.extra["noise_level"], s["diffusion"], masks=x.masks, scale=_diffusion_scale(s),
                                  seed=seed)
        if diffusion_stat is not None:
            diffusion_stat += loss.detach()
        return loss, _diffusion_ntokens(x), 1
    if kind == "tacotron2":
        # l1 + mse + eos under reduction "mean" (what task.train_step -> criterion(model, sample, update_num=) uses), loss and the three
        # gradients in one launch; the terms are added to `tts_stat` (fp64 [3]: l1, mse, eos) on the device
        loss, terms = ops.tacotron2_loss(x.extra["feature_out"], x.logits, x.extra["eos_out"], x.target, s["target_lengths"],
                                         float(s.get("bce_pos_weight", 1.0)), "mean", seed=seed)
        if tts_stat is not None:
            tts_stat += terms
        n, size = _tacotron_size(s)
        return loss, n, size
    if kind == "speech_to_text":
        # ce_weight * (the label-smoothed loss on the decoder) + ctc_weight * CTC(encoder output . embed_tokens[ds:de]^T), one backward on
        # the weighted sum (engine/criterion/speech_to_text_loss.py).  A weight of 0 launches nothing of its side's criterion.  The CE
        # side is ops.label_smoothed_cross_entropy whatever label_smoothing is (0 included: not the fused cross_entropy_sum a plain
        # micro-batch takes).  The CTC loss is added to `ctc_stat`, this rank's sum: it is not all-reduced with the step statistics.
        ce_w, ctc_w = float(s.get("ce_weight", 1.0)), float(s.get("ctc_weight", 0.0))
        loss, n = None, None
        if ce_w > 0:
            loss, _, n = ops.label_smoothed_cross_entropy(x.logits, x.target, cfg.pad, cfg.label_smoothing, cfg.constraint_range, x.masks,
                                                          cfg.drop_worst_ratio)
            if ce_w != 1.0:
                loss = loss * ce_w
        if ctc_w > 0:
            lc = _ctc(model, s, x, cfg, ctc_stat)[0]
            lc = lc if ctc_w == 1.0 else lc * ctc_w
            loss = lc if loss is None else loss + lc
        if n is None:
            n = x.target.ne(cfg.pad).sum()
        if s.get("sentence_avg"):                # sample_size = nsentences (speech_to_text_loss.py:241)
            size = s["target"].shape[0]
    elif kind == "trie_head":
        # (the features stand in x.logits; loss scaling reaches the gradient kernels through backward's seed)
        weight, bias = output_projection(model)
        loss, _, n = ops.trie_head_cross_entropy(x.logits, weight, bias, x.target, x.nodes, s["constraint_trie"], cfg.pad,
                                                 cfg.label_smoothing, cfg.constraint_range, cfg.drop_worst_ratio)
    elif kind == "trie_nodes":
        loss, _, n = ops.trie_label_smoothed_cross_entropy(x.logits, x.target, x.nodes, s["constraint_trie"], cfg.pad, cfg.label_smoothing,
                                                           cfg.constraint_range, cfg.drop_worst_ratio, seed=seed)
    elif kind == "scst":
        # self-critical sequence training (scst.ScstRewardCriterion builds such a micro-batch): the generated tokens' NLL weighted
        # by the sentence's reward, loss and logits gradient in one pass (engine/criterion/scst_loss.py:24-36)
        row_seq = None
        if x.plan is not None:                   # packed decoder rows: the sentence of padded row i is i // Tt (filler rows: -1)
            row_seq = torch.div(x.plan.dec_index, s["target"].shape[1], rounding_mode="floor").to(torch.int32)
        cr = s.get("constraint_range")
        cr = tuple(int(v) for v in cr.split(",")) if cr is not None else cfg.constraint_range
        loss, n = ops.scst_loss(x.logits, x.target, s["reward"], cfg.pad, cr, row_seq, seed=seed)
        if s.get("sentence_avg"):                # sample_size = nsentences (scst_loss.py:93)
            size = s["reward"].numel()
    elif kind == "label_smoothed":
        loss, _, n = ops.label_smoothed_cross_entropy(x.logits, x.target, cfg.pad, cfg.label_smoothing, cfg.constraint_range, x.masks,
                                                      cfg.drop_worst_ratio)
    else:
        # (the backward seed is known here: the criterion kernel writes the logits' gradient in its one pass over them)
        loss, n = ops.cross_entropy_sum(x.logits, x.target, cfg.pad, seed=seed, stats=stats), None
    return loss, n, size


def evaluate(model, s, kind, x, cfg, acc, ctc_stat=None, tts_acc=None, diffusion_acc=None):
    """The routed criterion in eval mode on x = forward(...): adds [ntokens, loss_sum, nll_sum, n_correct] to `acc` (label_smoothing /
    constraint_range; no drop_worst: the reference's eval call never drops).  A speech-to-text micro-batch
    (speech_to_text_loss.py:259-322) evaluates the decoder side if ce_weight > 0 and, if ctc_weight > 0, adds its CTC loss to
    `ctc_stat` and decodes greedily on the device -> (tokens, lengths, encoder_target, ds); every other call returns None.
    A text-to-speech micro-batch adds [sample_size, sample_size * (loss, l1, mse, eos), ntokens] to `tts_acc` (fp64 [6]): the
    reference's reduce_metrics weighs a batch's values by its sample_size (tacotron2_loss.py:201-214).
    A motion-diffusion micro-batch adds [sample_size = 1, loss, ntokens] to `diffusion_acc` (fp64 [3]; diffusion_loss.py:88-102)."""
    if kind == "diffusion":
        out = ops.diffusion_eval(x.logits, x.target, x.extra["noise_level"], s["diffusion"], masks=x.masks, scale=_diffusion_scale(s))
        diffusion_acc[0:1] += 1.0
        diffusion_acc[1:2] += out.double()
        diffusion_acc[2:3] += _diffusion_ntokens(x)
        return
    if kind == "tacotron2":
        out = ops.tacotron2_eval(x.extra["feature_out"], x.logits, x.extra["eos_out"], x.target, s["target_lengths"],
                                 float(s.get("bce_pos_weight", 1.0)), "mean")
        n, size = _tacotron_size(s)
        w = n.double() if size is None else torch.full((), float(size), dtype=torch.float64, device=out.device)
        tts_acc[0:1] += w
        tts_acc[1:5] += out.double() * w
        tts_acc[5:6] += n
        return
    if kind == "speech_to_text":
        decode = None
        if float(s.get("ce_weight", 1.0)) > 0:
            ops.criterion_eval(x.logits, x.target, cfg.pad, cfg.label_smoothing, cfg.constraint_range, x.masks, None, None, acc=acc)
        if float(s.get("ctc_weight", 0.0)) > 0:
            _, y, lay, ds = _ctc(model, s, x, cfg, ctc_stat)
            decode = (*ops.ctc_greedy_decode(y, lay), s["encoder_target"], ds)
        return decode
    if kind == "trie_head":
        weight, bias = output_projection(model)
        ops.trie_head_eval(x.logits, weight, bias, x.target, x.nodes, s["constraint_trie"], cfg.pad, cfg.label_smoothing,
                           cfg.constraint_range, acc=acc)
        return
    ops.criterion_eval(x.logits, x.target, cfg.pad, cfg.label_smoothing, cfg.constraint_range, x.masks, x.nodes,
                       s["constraint_trie"] if x.nodes is not None else None, acc=acc)
