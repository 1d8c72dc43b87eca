"""Generate tests/golden/validation.npz by RUNNING THE REFERENCE's LabelSmoothedCrossEntropyCriterion in eval mode on the CPU (build
container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_validation_golden.py
The criterion object is the reference's own (engine/criterion/label_smoothed_cross_entropy.py:95-198), built with report_accuracy and
called as its forward calls it: compute_loss(model, net_output, sample, update_num=0) and compute_accuracy(model, net_output, sample).
The "model" is the two methods the criterion asks of one: get_normalized_probs (the fp32 log-softmax, model/ofa.py:287-299) and
get_targets.  Logits [3, 6, 48] are recipe values; so that the accuracy is neither 0 nor 1, two thirds of the live positions have
their target raised above the row, and two positions hold two EQUAL maxima -- the target the lower column in one, the higher in the
other -- which pins the reference's tie rule (argmax on the CPU: the lowest column).  Targets carry <pad> = 1.  Settings: eps 0 and
0.1; no constraint, the constraint range "8,40" (targets it would remove are set to <pad>, so no live target leaves the allowed set),
and sample["constraint_masks"] (random, every live target allowed, one raised non-target column masked off).  Only data is stored: the
logits (fp32 values on the bf16 grid; `logits_masked` for the mask settings), the mask (bit-packed along V), and per setting the
target and `rec` = [eps, cstart, cend, loss, nll_loss, ntokens, n_correct, total] as recorded.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import recipe  # noqa: E402
from oracle.ref_import import install  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "validation.npz")
B, T, V, PAD = 3, 6, 48, 1
RANGE = (8, 40)
SETTINGS = [(f"{kind}_eps{str(eps).replace('.', '')}", eps, kind) for kind in ("none", "range", "mask") for eps in (0.0, 0.1)]


class _Model:
    @staticmethod
    def get_normalized_probs(net_output, log_probs):
        y = torch.log_softmax(net_output[0].float(), dim=-1)
        return y if log_probs else y.exp()

    @staticmethod
    def get_targets(sample, net_output):
        return sample["target"]


def main():
    install()
    from ofasys.engine.criterion.label_smoothed_cross_entropy import (LabelSmoothedCrossEntropyCriterion,
                                                                      LabelSmoothedCrossEntropyCriterionConfig)
    task = SimpleNamespace(target_dictionary=SimpleNamespace(pad=lambda: PAD))
    g = torch.Generator().manual_seed(7)
    target = torch.randint(4, V, (B, T), generator=g)
    target[0, 4:] = PAD
    target[1, 5:] = PAD
    target[2, 3:] = PAD
    logits = recipe.floats("validation.logits", (B, T, V), 2.0).bfloat16().float()     # (on the bf16 grid: exact in every kernel dtype)
    live = [(b, t) for b in range(B) for t in range(T) if int(target[b, t]) != PAD]
    for i, (b, t) in enumerate(live):
        if i % 3 != 2:
            logits[b, t, target[b, t]] = 9.0                 # the arg-max
    (b0, t0), (b1, t1) = live[0], live[1]
    target[b0, t0], target[b1, t1] = 12, 30                  # two equal maxima at columns 12 and 30 (inside the range)
    logits[b0, t0, 12] = logits[b0, t0, 30] = logits[b1, t1, 12] = logits[b1, t1, 30] = 11.0
    out = {"pad": np.array([PAD]), "range": np.array(RANGE)}
    for name, eps, kind in SETTINGS:
        cfg = LabelSmoothedCrossEntropyCriterionConfig(label_smoothing=eps, report_accuracy=True,
                                                       constraint_range=f"{RANGE[0]},{RANGE[1]}" if kind == "range" else None)
        crit = LabelSmoothedCrossEntropyCriterion(task, cfg)
        crit.eval()
        tg = target.clone()
        sample = {"target": tg}
        mask = None
        if kind == "range":
            inside = (tg < 4) | ((tg >= RANGE[0]) & (tg < RANGE[1]))
            tg[~inside] = PAD
        elif kind == "mask":
            mask = torch.rand(B, T, V, generator=torch.Generator().manual_seed(11)) < 0.6
            mask.scatter_(2, tg[..., None], True)
            mask[b0, t0, 30] = mask[b1, t1, 12] = True       # (the tie columns stay in)
            b2, t2 = live[2]
            other = (int(tg[b2, t2]) + 5) % V
            logits_m = logits.clone()
            logits_m[b2, t2, other] = 20.0                   # a dominant column the mask takes away
            mask[b2, t2, other] = False
            sample["constraint_masks"] = mask
        x = logits_m if kind == "mask" else logits
        net_output = (x.clone(),)
        with torch.no_grad():
            loss, nll, ntok = crit.compute_loss(_Model, net_output, sample, update_num=0)
            n_correct, total = crit.compute_accuracy(_Model, net_output, sample)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(nll)) and int(total) == int(ntok) == int((tg != PAD).sum())
        assert 0 < int(n_correct) < int(total), (name, n_correct, total)
        out["logits_masked" if kind == "mask" else "logits"] = x.numpy()
        # rec: [eps, cstart, cend (-1: no range), loss, nll_loss, ntokens, n_correct, total]
        out[f"{name}.target"] = tg.numpy().astype(np.int16)
        out[f"{name}.rec"] = np.array([eps, RANGE[0] if kind == "range" else -1, RANGE[1] if kind == "range" else -1, float(loss.double()),
                                       float(nll.double()), int(ntok), int(n_correct), int(total)], np.float64)
        if mask is not None:
            out["mask"] = np.packbits(mask.numpy(), axis=-1)
        print(name, "loss", float(loss), "nll", float(nll), "ntokens", int(ntok), "n_correct", int(n_correct), "total", int(total))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
