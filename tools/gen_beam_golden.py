"""Generate tests/golden/beam_search.npz by RUNNING THE REFERENCE's SequenceGenerator.generate on the CPU (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_beam_golden.py
The reference GeneralistModel (`tiny_text` case, recipe weights, eval mode) generates for the case's two source sentences under
the configurations of tests/beam_case.py.  With V = 204 and random weights EOS almost never wins, so the EOS row of the tied
output projection (= the token embedding) gets EOS_BOOST * its row of the `input.beam_eos_dir` recipe direction added first
(beam_case.boost_eos); the HIP test applies the same change.  Only data is stored: per configuration the hypotheses' tokens,
scores and positional scores.  The script asserts that the fixture covers what the test is meant to pin (hypotheses
finalised at >= 3 distinct steps, one sentence finishing before another, an EOS among the 2K candidates but outside the
top K, n-gram bans that change a result).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import recipe  # noqa: E402
from oracle.cases import CASES, VOCAB_EXTRA, make_value  # noqa: E402
from oracle.ref_import import build_reference_model, install  # noqa: E402
from tests.beam_case import CONFIGS, boost_eos  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "beam_search.npz")


def run(model, d, src_slots, cfg, log=None):
    from ofasys import ModalityType
    from ofasys.generator.sequence_generator import SequenceGenerator
    from ofasys.preprocessor import Slot
    gen = SequenceGenerator(d, **cfg)
    if log is not None:
        step_fn, fin_fn = gen.search.step, gen.finalize_hypos

        def step(step_i, lprobs, *a, **k):
            out = step_fn(step_i, lprobs, *a, **k)
            sc, idx, _ = out
            K = lprobs.shape[1]
            top_eos = (idx[:, :K] == d.eos()) & torch.isfinite(sc[:, :K])
            low_eos = (idx[:, K:] == d.eos()) & torch.isfinite(sc[:, K:])
            log["eos_outside_topk"] += int((low_eos.any(1) & ~top_eos.any(1)).sum())
            return out

        def fin(step_i, *a, **k):
            finished_before = list(a[5])
            out = fin_fn(step_i, *a, **k)
            for s, (b, f) in enumerate(zip(finished_before, a[5])):
                if f and not b:
                    log["finish_step"][s] = step_i
            return out
        gen.search.step, gen.finalize_hypos = step, fin
    slots = list(src_slots) + [Slot(ModalityType.TEXT, False, torch.zeros(len(src_slots[0].value), 1, dtype=torch.long))]
    return gen.generate(model, {"net_input": {"slots": slots}})


def flatten(result, n_best, max_len):
    """[bsz, n_best, max_len + 1] tokens (pad 1), lengths, scores, positional scores."""
    bsz = len(result)
    toks = np.full((bsz, n_best, max_len + 1), 1, np.int64)
    pos = np.zeros((bsz, n_best, max_len + 1), np.float32)
    lens, scores = np.zeros((bsz, n_best), np.int64), np.zeros((bsz, n_best), np.float32)
    for b, r in enumerate(result):
        hyps = r if isinstance(r, list) else [r]
        for i, h in enumerate(hyps):
            n = h.tokens.numel()
            toks[b, i, :n], pos[b, i, :n] = h.tokens.numpy(), h.positional_scores.numpy()
            lens[b, i], scores[b, i] = n, float(h.score)
    return toks, lens, scores, pos


def main():
    install()
    import ofasys  # noqa: F401
    from ofasys import ModalityType
    from ofasys.preprocessor import Slot
    case = CASES["tiny_text"]
    model, d = build_reference_model(case["arch"], VOCAB_EXTRA, case["active"], case["overrides"], case["adaptor_overrides"])
    recipe.fill_state(model.state_dict())
    with torch.no_grad():
        boost_eos(model.state_dict()["decoder.adaptor.embed_tokens.weight"], d.eos())
    model.eval()
    V = len(d)
    src = [Slot(ModalityType[m], True, make_value(spec, V), attributes=a) for m, s, spec, a in case["slots"] if s]
    arrays, steps_seen, eos_outside, finish_order = {}, set(), 0, False
    for name, cfg in CONFIGS.items():
        log = {"eos_outside_topk": 0, "finish_step": {}}
        res = run(model, d, src, cfg, log)
        n_best = cfg.get("return_n_best", 1) if cfg.get("return_n_best", -1) != -1 else cfg["beam_size"]
        toks, lens, scores, pos = flatten(res, n_best, cfg["max_len"])
        arrays.update({f"{name}.tokens": toks, f"{name}.lens": lens, f"{name}.scores": scores, f"{name}.pos": pos})
        steps_seen |= set(int(x) - 1 for x in lens.ravel() if x > 0)
        eos_outside += log["eos_outside_topk"]
        fs = log["finish_step"]
        if len(set(fs.values())) > 1:
            finish_order = True
        print(name, "lengths", lens.tolist(), "finish steps", fs, "eos outside top K", log["eos_outside_topk"])
        if cfg.get("no_repeat_ngram_size", 0) > 0:
            plain = run(model, d, src, dict(cfg, no_repeat_ngram_size=0))
            t2, l2, _, _ = flatten(plain, n_best, cfg["max_len"])
            assert not (np.array_equal(t2, toks) and np.array_equal(l2, lens)), f"{name}: the n-gram bans change nothing"
    assert len(steps_seen) >= 3, f"hypotheses finalised at only {sorted(steps_seen)}"
    assert finish_order, "no sentence finishes before another"
    assert eos_outside > 0, "no step with EOS among the 2K candidates but outside the top K"
    arrays["configs"] = np.array(json.dumps(CONFIGS))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; finalisation steps", sorted(steps_seen))


if __name__ == "__main__":
    main()
