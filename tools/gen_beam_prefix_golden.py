"""Generate tests/golden/beam_prefix.npz by RUNNING THE REFERENCE's SequenceGenerator.generate with `prefix_tokens` on the CPU
(build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_beam_prefix_golden.py
Same scenario as tools/gen_beam_golden.py (`tiny_text` model, recipe weights, the EOS boost of tests/beam_case.py), under the
configurations and forced prefixes of tests/beam_prefix_case.py.  Only data is stored: per configuration the prefix, the
hypotheses' tokens, scores and positional scores, and for one configuration the lprobs of step 0 with what the reference's
search.step made of them.

Inside a forced row all tokens but one tie, and torch.topk leaves the order of ties open, so only hypotheses that follow their
sentence's prefix are defined by the reference.  The script therefore ASSERTS, per configuration, that
  - every returned hypothesis begins with its sentence's prefix,
  - from each sentence's first free step on every active beam begins with it,
  - running the reference again with search.step's torch.topk replaced by the project's tie rule (value descending, flat index
    ascending) returns the same hypotheses,
and stores the facts in the fixture.  A configuration that fails is given other inputs; the comparison stays.
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
from tests.beam_case import boost_eos  # noqa: E402
from tests.beam_prefix_case import CONFIGS, LPROBS_OF, PAD  # noqa: E402
from tools.gen_beam_golden import flatten  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "beam_prefix.npz")


_topk = torch.topk


def tie_rule_topk(x, k, dim=-1, largest=True, sorted=True):
    """torch.topk with ties to the lower index (the largest-first calls: search.step's)."""
    if not largest:
        return _topk(x, k, dim=dim, largest=False, sorted=sorted)
    order = torch.sort(x, dim=dim, descending=True, stable=True).indices.narrow(dim, 0, k)
    return x.gather(dim, order), order


def run(model, d, src_slots, cfg, prefix, tie_rule=False, log=None):
    from ofasys import ModalityType
    from ofasys.generator.sequence_generator import SequenceGenerator
    from ofasys.preprocessor import Slot
    gen = SequenceGenerator(d, **cfg)
    beam = gen.beam_size
    plen = (prefix != PAD).sum(1)
    step_fn, pre_fn = gen.search.step, gen._prefix_tokens

    def step(step_i, lprobs, scores, prev, batch_idxs):
        out = step_fn(step_i, lprobs, scores, prev, batch_idxs)
        if log is not None:
            if step_i == 0:
                log["step0_masked"] = lprobs.clone()
                log["step0_cand"] = tuple(o.clone() for o in out)
            # the beams entering this step were made active at step_i - 1: off the prefix they may be only while it lasts (the
            # K - 1 beams next to the first one at step 0 hold tie tokens, and stay forced along until the prefix ends)
            for r in range(prev.shape[0]):
                s = int(batch_idxs[r // beam])
                n = int(plen[s])
                if step_i - 1 >= n and prev[r, 1:n + 1].tolist() != prefix[s, :n].tolist():
                    log["stray_active"].append((s, step_i, prev[r].tolist()))
        return out

    def pre(step_i, lprobs, *a, **k):
        if log is not None and step_i == 0:
            log["step0_lprobs"] = lprobs.clone()
        return pre_fn(step_i, lprobs, *a, **k)

    gen.search.step, gen._prefix_tokens = step, pre
    slots = list(src_slots) + [Slot(ModalityType.TEXT, False, torch.zeros(len(src_slots[0].value), 1, dtype=torch.long))]
    if tie_rule:
        torch.topk = tie_rule_topk
    try:
        return gen.generate(model, {"net_input": {"slots": slots}, "prefix_tokens": prefix.clone()})
    finally:
        torch.topk = _topk


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
    arrays = {}
    for name, c in CONFIGS.items():
        cfg, prefix = c["gen"], torch.tensor(c["prefix"], dtype=torch.long)
        log = {"stray_active": []}
        res = run(model, d, src, cfg, prefix, log=log)
        n_best = cfg.get("return_n_best", 1) if cfg.get("return_n_best", -1) != -1 else cfg["beam_size"]
        toks, lens, scores, pos = flatten(res, n_best, cfg["max_len"])
        print(name, "lengths", lens.tolist(), "scores", np.round(scores, 3).tolist())
        follows = True
        for b in range(toks.shape[0]):
            want = [t for t in c["prefix"][b] if t != PAD]
            assert (lens[b] > 0).any(), (name, b, "no hypothesis")
            for i in range(toks.shape[1]):
                if lens[b, i] > 0 and toks[b, i, :len(want)].tolist() != want:
                    follows = False
                    print("  hypothesis off its prefix:", b, i, toks[b, i, :lens[b, i]].tolist())
        assert follows, f"{name}: a returned hypothesis does not begin with its sentence's prefix"
        assert not log["stray_active"], f"{name}: active beams off their prefix after it ended: {log['stray_active'][:4]}"
        t2, l2, s2, p2 = flatten(run(model, d, src, cfg, prefix, tie_rule=True), n_best, cfg["max_len"])
        assert np.array_equal(t2, toks) and np.array_equal(l2, lens), f"{name}: the result depends on the order of ties"
        assert np.abs(s2 - scores).max() < 1e-5 and np.abs(p2 - pos).max() < 1e-5, name
        arrays.update({f"{name}.tokens": toks, f"{name}.lens": lens, f"{name}.scores": scores, f"{name}.pos": pos,
                       f"{name}.prefix": prefix.numpy(), f"{name}.hyps_follow_prefix": np.array(True),
                       f"{name}.active_follow_prefix": np.array(True), f"{name}.tie_order_free": np.array(True)})
        if name == LPROBS_OF:
            sc, idx, beams = log["step0_cand"]
            arrays.update({"step0.lprobs": log["step0_lprobs"].numpy(), "step0.masked": log["step0_masked"].numpy(),
                           "step0.cand_scores": sc.numpy(), "step0.cand_tokens": idx.numpy(), "step0.cand_beams": beams.numpy()})
    arrays["configs"] = np.array(json.dumps(CONFIGS))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
