"""Generate tests/golden/tts.npz (+ tts.manifest.json) by RUNNING THE REFERENCE on the CPU (build container only) on the case of
tests/tts_case.py.

TEST INFRASTRUCTURE.  Usage:  python tools/gen_tts_golden.py
Only data is stored -- no reference source:
  * the collation of the case's frames by the reference's own audio preprocessor (prev_outputs, target, target_lengths, ntokens) and its
    pack_frames on sample 0;
  * the reference GeneralistModel (tiny, text + audio_fbank, every dropout 0, train mode) on [TEXT] -> [AUDIO:fbank]: post, feature_out,
    eos_out, the decoder's output in front of the head (`hidden`) and the prenet's output (`embed`);
  * the reference criterion's compute_loss on them: (loss, l1, mse, eos) under "mean" and under "sum";
  * the gradient of the "mean" loss for every parameter that receives one, as (norm, evenly strided sample);
  * the key|shape list of the decoder-side adaptor's state dict;
  * for every recorded tensor and gradient sample the reference's OWN bf16-vs-fp32 gap (the same run with the module and the frames in
    bfloat16), as max |a - b| / max |b| -- the bf16 tests hold the implementation to twice that gap.
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import recipe  # noqa: E402
from oracle.cases import VOCAB_EXTRA  # noqa: E402
from oracle.ref_import import build_reference_model, install  # noqa: E402
from tests import tts_case as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tts.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "tts.manifest.json")


def reference_collate():
    """The reference's DefaultAudioPreprocess.collate / pack_frames on the case's frames (the object is made without its constructor,
    which wants feature-extraction settings: collate reads output_type and the dictionary alone)."""
    from ofasys import ModalityType
    from ofasys.preprocessor import Dictionary, Slot
    from ofasys.preprocessor.default.audio import DefaultAudioPreprocess
    d = Dictionary()
    d.add_symbol("<phone>_dict_begin")
    d.add_symbol("<phone>_dict_end")
    pre = object.__new__(DefaultAudioPreprocess)
    pre.global_dict, pre.output_type, pre._sanity_check, pre.n_frames_per_step = d, "fbank", True, 1
    slots = [Slot(ModalityType.AUDIO, False, {"fbank": f, "fbank_lengths": f.shape[0]}) for f in C.frames()]
    out = pre.collate(slots)
    packed = pre.pack_frames(C.frames()[0], n_frames_per_step=C.PACK_N)
    return out.net_input_slot.value, out.net_target_slot.value, out.sample_extra, packed


def run_model(dtype, prev, lengths, target, rec):
    from ofasys import ModalityType
    from ofasys.engine.criterion.tacotron2_loss import OFATacotron2Criterion
    from ofasys.preprocessor import Slot
    case = C.CASE
    model, d = build_reference_model(case["arch"], VOCAB_EXTRA, case["active"], case["overrides"], case["adaptor_overrides"])
    recipe.fill_state(model.state_dict())
    model = model.to(dtype)
    model.train()
    slots = [Slot(ModalityType.TEXT, True, C.source_tokens(len(d))),
             Slot(ModalityType.AUDIO, False, {"fbank": prev.to(dtype), "fbank_lengths": lengths})]
    ad = model.decoder.adaptor.audio_fbank
    hooks = [ad.prenet.register_forward_hook(lambda m, i, o: rec.__setitem__("embed", o.detach().float())),
             ad.feat_proj.register_forward_hook(lambda m, i, o: rec.__setitem__("hidden", i[0].detach().float()))]
    post, extra = model(slots)[:2]
    for h in hooks:
        h.remove()
    crit = types.SimpleNamespace(bce_pos_weight=C.BCE_POS_WEIGHT)
    T = target.shape[1]
    eos_tgt = (torch.arange(T).view(1, T).expand(C.B, -1) == (lengths.view(C.B, 1).expand(-1, T) - 1)).float()   # (:104-107)
    losses = {}
    for reduction in ("mean", "sum"):
        l1, mse, eos = OFATacotron2Criterion.compute_loss(crit, extra["feature_out"].float(), post.float(), extra["eos_out"].float(),
                                                          target.float(), eos_tgt, lengths, reduction)
        losses[reduction] = torch.stack([l1 + mse + eos, l1, mse, eos]).detach().double()
        if reduction == "mean":
            model.zero_grad()
            (l1 + mse + eos).backward(retain_graph=True)
    rec.update(post=post.detach().float(), feature_out=extra["feature_out"].detach().float(), eos_out=extra["eos_out"].detach().float())
    return model, losses


def main():
    install()
    import ofasys  # noqa: F401
    out, manifest = {}, {}
    inp, tgt, extra, packed = reference_collate()
    prev, lengths, target = inp["fbank"], tgt["fbank_lengths"], extra["target"]
    assert torch.equal(inp["fbank_lengths"], lengths) and torch.equal(extra["target_lengths"], lengths) and torch.equal(tgt["fbank"], target)
    out["prev_outputs"], out["target"], out["target_lengths"] = prev.numpy(), target.numpy(), lengths.numpy()
    out["ntokens"] = np.array([extra["ntokens"]], np.int64)
    out["packed0"] = packed.numpy()

    rec32, rec16 = {}, {}
    model, losses = run_model(torch.float32, prev, lengths, target, rec32)
    model16, losses16 = run_model(torch.bfloat16, prev, lengths, target, rec16)
    gaps = {}
    for k in ("post", "feature_out", "eos_out", "hidden", "embed"):
        out[k] = rec32[k].numpy()
        gaps[k] = C.rel(rec16[k], rec32[k])
        out["gap_" + k] = np.array([gaps[k]])
    for r in ("mean", "sum"):
        out["loss_" + r] = losses[r].numpy()
        gaps["loss_" + r] = C.rel(losses16[r], losses[r])
        out["gap_loss_" + r] = np.array([gaps["loss_" + r]])
    named = [(k, p) for k, p in model.named_parameters() if p.grad is not None]
    g16 = {k: p.grad.detach().float() for k, p in model16.named_parameters() if p.grad is not None}
    keys = [k for k, _ in named]
    assert set(keys) == set(g16)
    grads = [p.grad.detach().float() for _, p in named]
    out["gkeys"] = np.array(keys)
    out["gnorm"] = np.array([float(g.double().norm()) for g in grads], np.float64)
    samples = [C.sample(g) for g in grads]
    out["gcount"] = np.array([s.numel() for s in samples], np.int64)
    out["gsample"] = torch.cat(samples).numpy()
    out["gap_g"] = np.array([C.rel(C.sample(g16[k]), C.sample(g)) for k, g in zip(keys, grads)], np.float64)
    out["gap_gnorm"] = np.array([abs(float(g16[k].double().norm()) - float(g.double().norm())) / max(float(g.double().norm()), 1e-30)
                                 for k, g in zip(keys, grads)], np.float64)
    state = model.decoder.adaptor.audio_fbank.state_dict()
    out["state_keys"] = np.array([f"{k}|{tuple(v.shape)}" for k, v in state.items()])
    manifest = {"case": {k: (sorted(v) if isinstance(v, set) else v) for k, v in C.CASE.items()}, "frame_lengths": C.FRAME_LENGTHS,
                "bce_pos_weight": C.BCE_POS_WEIGHT, "loss_mean": losses["mean"].tolist(), "loss_sum": losses["sum"].tolist(),
                "gaps": gaps, "gap_g_max": float(out["gap_g"].max()), "params_with_grad": len(keys), "state_keys": len(state),
                "inputs": "recipe keys: input.tts.fbank.<i>, input.tts.src; weights: oracle.recipe.fill_state"}
    print("loss (mean)", losses["mean"].tolist(), "ref bf16 gaps", gaps, "grads max", manifest["gap_g_max"])
    np.savez_compressed(OUT, **out)
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
