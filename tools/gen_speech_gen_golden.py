"""Generate tests/golden/speech_gen.npz (+ speech_gen.manifest.json) by RUNNING THE REFERENCE's own AutoRegressiveSpeechGenerator on the
CPU in fp32 (build container only) on the case of tests/speech_gen_case.py.

TEST INFRASTRUCTURE.  Usage:  python tools/gen_speech_gen_golden.py
Only data is stored -- no reference source.  Per entry (`n1`, `n2`):
  * the scale (per input channel) and bias applied to eos_proj after recipe.fill_state and the eos_prob_threshold, chosen HERE so that
    the three rows end differently: one at step 1, one in the middle, one never.  What the decoder hands to eos_proj up to a row's
    finish does not depend on eos_proj (a finished row only pads its OWN later keys), so the choice is made on the eos_proj inputs of
    one run that finishes nobody;
  * per row feature, eos_prob, attn (as the reference returns it: the first step's map), alignment, out_lens, and targ_feature of
    the `has_targ` run; the pre-postnet feature_out of all T_run steps and the eos_prob of all T_run steps;
  * the reference's OWN bf16-vs-fp32 gaps (the same run with the module in bfloat16), as max |a - b| / max |b| over the batch (for the
    ragged outputs: over the rows' kept parts together).
Asserted here (a condition on the INPUTS, so that no 16-bit test can flip a finish): the bf16 run gives the same out_lens, and over
every (row, step) up to the row's finish |eos_prob - threshold| >= 20 x the absolute bf16 gap on eos_prob.
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import recipe  # noqa: E402
from oracle.cases import VOCAB_EXTRA  # noqa: E402
from oracle.ref_import import build_reference_model, install  # noqa: E402
from tests import speech_gen_case as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "speech_gen.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "speech_gen.manifest.json")


def build(entry, dtype, affine):
    case = C.case(entry)
    model, d = build_reference_model(case["arch"], VOCAB_EXTRA, case["active"], case["overrides"], case["adaptor_overrides"])
    recipe.fill_state(model.state_dict())
    if affine is not None:
        C.apply_eos_affine(model, *affine)
    return model.to(dtype).eval(), d


def run(entry, dtype, affine, threshold, stats_path, has_targ=False):
    """The reference generator on the entry -> (outputs, feature_out [B, T_run, out_dim], eos_prob [B, T_run])."""
    from ofasys import ModalityType
    from ofasys.generator.speech_generator import AutoRegressiveSpeechGenerator
    from ofasys.preprocessor import Slot
    model, d = build(entry, dtype, affine)
    gen = AutoRegressiveSpeechGenerator(d, stats_npz_path=stats_path, max_iter=C.ENTRIES[entry]["max_iter"], eos_prob_threshold=threshold)
    slots = [Slot(ModalityType.TEXT, True, C.source_tokens(len(d))), Slot(ModalityType.AUDIO, False, None)]
    sample = {"net_input": {"slots": slots}}
    if has_targ:
        tgt, lens = C.target(entry)
        sample["target"], sample["target_lengths"] = tgt.to(dtype), lens
    rec = {"feat": [], "eos": [], "hidden": []}
    ad = model.decoder.adaptor.audio_fbank
    hooks = [ad.feat_proj.register_forward_hook(lambda m, i, o: rec["feat"].append(o.detach().float())),
             ad.eos_proj.register_forward_hook(lambda m, i, o: (rec["eos"].append(o.detach().float()), rec["hidden"].append(i[0].detach().float())) and None)]
    outs = gen.generate(model, sample, has_targ=has_targ)
    for h in hooks:
        h.remove()
    run.hidden = torch.cat(rec["hidden"], 1)
    return outs, torch.cat(rec["feat"], 1), torch.cat(rec["eos"], 1).squeeze(2)


def choose(x, w, b0, max_iter, level, swing=5.0):
    """x [B, T, D]: the inputs of eos_proj in a run that finishes nobody (they do not depend on eos_proj up to a row's finish); w [D], b0:
    the recipe's eos_proj.  -> (scale [D] float64, bias): the smallest change (in the 2-norm of the weight change and the bias change) after
    which row 0's logit is level - swing at step 0 and level + swing at step 1, row 1's is level + swing at step max_iter // 2 and
    level - swing before, and row 2's is level - swing at every step.  Steps after a row's finish are left free."""
    rows, want = [], []
    plan = {0: 1, 1: max_iter // 2, 2: None}
    for r, fin in plan.items():
        for t in range(max_iter if fin is None else fin + 1):
            rows.append(torch.cat([x[r, t].double(), torch.ones(1, dtype=torch.float64)]))
            want.append(level + (swing if t == fin else -swing))
    A, y = torch.stack(rows), torch.tensor(want, dtype=torch.float64)
    resid = y - (A[:, :-1] @ w.double() + b0)
    sol = torch.linalg.pinv(A) @ resid                                          # minimum norm
    scale = (w.double() + sol[:-1]) / w.double()
    return scale, float(sol[-1])


def to_np(t):
    return t.detach().float().numpy() if t.is_floating_point() else t.detach().numpy()


def main():
    install()
    import ofasys  # noqa: F401
    out, manifest = {}, {"entries": {}}
    mean, std = C.gcmvn_stats()
    tmp = tempfile.mkdtemp()
    stats_path = os.path.join(tmp, "gcmvn_stats.npz")
    np.savez(stats_path, mean=mean, std=std)
    for entry, spec in C.ENTRIES.items():
        max_iter, n = spec["max_iter"], spec["n_frames_per_step"]
        _, _, z = run(entry, torch.float32, None, 2.0, stats_path)              # threshold 2: nobody finishes, the raw logits of every step
        assert z.shape == (C.B, max_iter)
        threshold = 0.4
        ref0, _ = build(entry, torch.float32, None)
        sd = ref0.state_dict()
        affine = choose(run.hidden, sd[C.PREFIX + "eos_proj.weight"][0], float(sd[C.PREFIX + "eos_proj.bias"][0]), max_iter,
                        float(np.log(threshold / (1 - threshold))))
        outs, feat, eosz = run(entry, torch.float32, affine, threshold, stats_path, has_targ=True)
        outs16, feat16, eosz16 = run(entry, torch.bfloat16, affine, threshold, stats_path, has_targ=True)
        out_lens = [int(o.eos_prob.shape[0]) // n for o in outs]                # steps (never-finishing rows: max_iter)
        lens16 = [int(o.eos_prob.shape[0]) // n for o in outs16]
        assert out_lens == lens16, (out_lens, lens16)
        T_run = feat.shape[1]
        assert T_run == max(out_lens) and feat16.shape[1] == T_run
        p, p16 = torch.sigmoid(eosz), torch.sigmoid(eosz16)
        kinds = sorted("early" if f <= 2 else ("never" if f >= max_iter and not bool((p[b] > threshold).any()) else "middle")
                       for b, f in enumerate(out_lens))
        assert kinds == ["early", "middle", "never"], (out_lens, kinds)
        decide = torch.zeros_like(p, dtype=torch.bool)
        for b, f in enumerate(out_lens):
            decide[b, :f] = True
        gap_abs = float((p16 - p)[decide].abs().max())
        margin = float((p - threshold)[decide].abs().min())
        assert margin >= C.MARGIN * gap_abs, (entry, margin, gap_abs)
        pre = entry + "."
        out[pre + "eos_scale"] = affine[0].numpy()
        out[pre + "eos_bias"] = np.array([affine[1]], np.float64)
        out[pre + "threshold"] = np.array([threshold], np.float64)
        out[pre + "out_lens"] = np.array(out_lens, np.int64)
        out[pre + "feature_out"] = feat.numpy()
        out[pre + "eos_prob_all"] = p.numpy()
        gaps = {"feature_out": C.rel(feat16, feat), "eos_prob_all": C.rel(p16, p)}
        for k in ("feature", "eos_prob", "attn", "targ_feature"):                # over the batch, as gen_tts_golden.py's gaps: the rows' kept parts together
            gaps[k] = C.rel(C.batch(getattr(a, k) for a in outs16), C.batch(getattr(b, k) for b in outs))
        for b, (o, o16) in enumerate(zip(outs, outs16)):
            for k in ("feature", "eos_prob", "attn", "alignment", "targ_feature"):
                out[f"{pre}{k}.{b}"] = to_np(getattr(o, k))
        for k, v in gaps.items():
            out[pre + "gap_" + k] = np.array([v])
        manifest["entries"][entry] = {"case": {k: (sorted(v) if isinstance(v, set) else v) for k, v in C.case(entry).items()},
                                      "max_iter": max_iter, "eos_bias": affine[1], "eos_scale_absmax": float(affine[0].abs().max()), "threshold": threshold, "out_lens": out_lens,
                                      "T_run": T_run, "margin": margin, "bf16_gap_abs_eos_prob": gap_abs, "gaps": gaps}
        print(entry, "out_lens", out_lens, "T_run", T_run, "margin", margin, "gap", gap_abs, "gaps", gaps)
    out["gcmvn_mean"], out["gcmvn_std"] = mean, std
    manifest["inputs"] = "recipe keys: input.speech_gen.src, input.speech_gen.target.<entry>, input.speech_gen.gcmvn.*; weights: oracle.recipe.fill_state, then eos_scale / eos_bias"
    np.savez_compressed(OUT, **out)
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
