"""Generate tests/golden/trie_beam.npz by RUNNING THE REFERENCE's SequenceGenerator.generate with its own Trie as `constraint_trie`
on the CPU (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_trie_beam_golden.py
The reference GeneralistModel (`tiny_text` case, recipe weights, eval mode) generates for the case's two source sentences under the
closed sets and configurations of tests/trie_beam_case.py.  Only data is stored: per configuration the hypotheses' tokens, lengths,
scores and positional scores, the label of the best hypothesis, and the number of steps the reference ran.  The script asserts that
the fixture covers what the tests are meant to pin: a sentence that returns fewer hypotheses than the beam, an answer that is a
strict prefix of another with both returned, configurations whose result the n-gram ban / max_len / unk penalty changes, beam 1
missing the exact arg-max, beam 16 reproducing the scores of tests/golden/traverse.npz, and adjacent hypothesis scores at least
1e-2 apart (so exact token comparisons are meaningful).
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
from tests.trie_beam_case import CLOSED_SETS, CONFIGS, WIDTH, distinct, generator_args, label_of  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "trie_beam.npz")
MIN_GAP = 1e-2


def ref_kwargs(cfg):
    """Task-level names (task/base.py:475-486) -> the reference generator's keywords; normalize_scores False as build_generator."""
    a = generator_args(cfg)
    return dict(beam_size=a.pop("beam", 5), return_n_best=a.pop("return_n_best", 1), max_len=a.pop("max_len", 256),
                min_len=a.pop("min_len", 1), normalize_scores=a.pop("normalize_scores", False), len_penalty=a.pop("lenpen", 1),
                unk_penalty=a.pop("unkpen", 0), temperature=a.pop("temperature", 1.0),
                no_repeat_ngram_size=a.pop("no_repeat_ngram_size", 0), **a)


def run(model, d, src_slots, answers, cfg):
    from ofasys import ModalityType
    from ofasys.generator.sequence_generator import SequenceGenerator
    from ofasys.preprocessor import Slot
    from ofasys.utils.trie import Trie
    trie = Trie(d.eos())
    for a in answers:
        trie.insert([d.bos()] + list(a) + [d.eos()])
    gen = SequenceGenerator(d, constraint_trie=trie, **ref_kwargs(cfg))
    steps = [0]
    step_fn = gen.search.step

    def step(step_i, *a, **k):
        steps[0] = step_i + 1
        return step_fn(step_i, *a, **k)
    gen.search.step = step
    slots = list(src_slots) + [Slot(ModalityType.TEXT, False, torch.zeros(len(src_slots[0].value), 1, dtype=torch.long))]
    res = gen.generate(model, {"net_input": {"slots": slots}})
    return [r if isinstance(r, list) else [r] for r in res], steps[0]


def flatten(result, n_best):
    bsz = len(result)
    toks = np.full((bsz, n_best, WIDTH), 1, np.int64)
    pos = np.zeros((bsz, n_best, WIDTH), np.float32)
    lens, scores = np.zeros((bsz, n_best), np.int64), np.zeros((bsz, n_best), np.float32)
    for b, hyps in enumerate(result):
        for i, h in enumerate(hyps):
            n = h.tokens.numel()
            toks[b, i, :n], pos[b, i, :n] = h.tokens.numpy(), h.positional_scores.numpy()
            lens[b, i], scores[b, i] = n, float(h.score)
    return toks, lens, scores, pos


def seqs(result):
    return [[h.tokens[:-1].tolist() for h in hyps] for hyps in result]


def main():
    install()
    import ofasys  # noqa: F401
    from ofasys import ModalityType
    from ofasys.preprocessor import Slot
    case = CASES["tiny_text"]
    model, d = build_reference_model(case["arch"], VOCAB_EXTRA, case["active"], case["overrides"], case["adaptor_overrides"])
    recipe.fill_state(model.state_dict())
    model.eval()
    V = len(d)
    src = [Slot(ModalityType[m], True, make_value(spec, V), attributes=a) for m, s, spec, a in case["slots"] if s]
    arrays, results, min_gap = {}, {}, float("inf")
    for name, cfg in CONFIGS.items():
        answers = CLOSED_SETS[cfg["set"]]
        res, steps = run(model, d, src, answers, cfg)
        results[name] = res
        n_best = cfg.get("return_n_best", 1)
        toks, lens, scores, pos = flatten(res, n_best)
        best = np.array([label_of(answers, hyps[0].tokens[:-1].tolist()) for hyps in res], np.int64)
        arrays.update({f"{name}.tokens": toks, f"{name}.lens": lens, f"{name}.scores": scores, f"{name}.pos": pos,
                       f"{name}.best": best, f"{name}.ref_steps": np.array(steps)})
        for b in range(len(res)):
            s = scores[b][lens[b] > 0].astype(np.float64)
            assert np.all(np.diff(s) < 0), (name, b)
            if len(s) > 1:
                min_gap = min(min_gap, float(-np.diff(s).max()))
        print(name, "hypotheses", [(lens[b] > 0).sum() for b in range(len(res))], "best", best.tolist(), "reference steps", steps)
    assert min_gap >= MIN_GAP, f"adjacent hypothesis scores only {min_gap} apart: change the scenario, not the tolerance"
    # ---- coverage
    main_set = distinct(CLOSED_SETS["main"])
    full = seqs(results["beam16"])
    assert all(sorted(s) == sorted(main_set) for s in full), "beam 16 does not return the whole closed set"
    assert all(len(s) < 16 for s in full)                                             # fewer hypotheses than the beam
    assert all([17, 23] in s and [17, 23, 99] in s for s in full)                     # a strict prefix of another, both returned
    short = seqs(results["beam16_max_len3"])
    assert all(sorted(s) == sorted(a for a in main_set if len(a) <= 3) for s in short) and len(short[0]) == len(main_set) - 2
    trav = np.load(os.path.join(ROOT, "tests", "golden", "traverse.npz"))["scores"]   # the exact route, recorded from the reference
    for b, hyps in enumerate(results["beam16"]):
        for h in hyps:
            want = float(trav[b, label_of(CLOSED_SETS["main"], h.tokens[:-1].tolist())])
            assert abs(float(h.score) - want) < 1e-4, (b, h.tokens.tolist(), float(h.score), want)
    exact = trav.argmax(1).tolist()
    assert arrays["beam16.best"].tolist() == exact
    assert arrays["beam1.best"].tolist() != exact, "beam 1 finds the arg-max everywhere: no case of beam search missing it"
    extra = distinct(CLOSED_SETS["extra"])
    plain, cut = seqs(results["beam16_extra_plain"]), seqs(results["beam16_unk_ngram"])
    assert all(sorted(s) == sorted(extra) for s in plain)
    assert all([40, 8, 40, 8] in p and [40, 8, 40, 8] not in c for p, c in zip(plain, cut)), "the n-gram ban changes nothing"
    unk_moves = False
    for b in range(len(plain)):                                                        # the unk penalty lowers the <unk> answers' scores
        sp = {tuple(h.tokens.tolist()): float(h.score) for h in results["beam16_extra_plain"][b]}
        sc = {tuple(h.tokens.tolist()): float(h.score) for h in results["beam16_unk_ngram"][b]}
        for k in sc:
            if 3 in k:
                assert abs(sp[k] - 0.75 - sc[k]) < 1e-4, (k, sp[k], sc[k])
                unk_moves = True
    assert unk_moves
    small = seqs(results["beam5_small"])
    assert all(sorted(s) == sorted(CLOSED_SETS["small"]) for s in small)
    arrays["configs"] = np.array(json.dumps(CONFIGS))
    arrays["closed_sets"] = np.array(json.dumps(CLOSED_SETS))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; smallest gap between adjacent hypothesis scores", round(min_gap, 4))


if __name__ == "__main__":
    main()
