"""Generate tests/golden/diverse_search_steps.npz and tests/golden/diverse_beam.npz by RUNNING THE REFERENCE on the CPU (build
container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_diverse_golden.py
(a) diverse_search_steps.npz: the reference's DiverseBeamSearch.step / DiverseSiblingsSearch.step on the small random inputs of
    tests/diverse_case.py (inputs and the three outputs).
(b) diverse_beam.npz: the reference's SequenceGenerator.generate with those strategies on the `tiny_text` recipe model with the
    EOS boost of tests/beam_case.py, under the configurations of tests/diverse_case.py (tokens, lengths, scores, positional scores).
Only data is stored.  The script refuses to write unless the fixtures pin what the tests are meant to pin: every group
configuration differs from plain beam search on the same inputs, a group and a sibling configuration change tokens, some step has a
finite EOS candidate among the first K positions that comes from a group other than 0, and no selection of any step was decided by
less than diverse_case.MIN_GAP -- measured by tests/diverse_oracle.py on the lprobs the reference's step saw, which must also
reproduce that step's outputs.
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
from tests import diverse_case as dc  # noqa: E402
from tests import diverse_oracle as do  # noqa: E402
from tests.beam_case import boost_eos  # noqa: E402
from tools.gen_beam_golden import flatten  # noqa: E402

OUT_STEPS = os.path.join(ROOT, "tests", "golden", "diverse_search_steps.npz")
OUT_GEN = os.path.join(ROOT, "tests", "golden", "diverse_beam.npz")
MAX_BYTES = 96 * 1024                             # tens of KB, as the other generation goldens


class _Dict:                                      # what Search.__init__ reads of a dictionary
    def pad(self): return do.PAD
    def unk(self): return do.UNK
    def eos(self): return do.EOS
    def __len__(self): return dc.STEP_V


def oracle_step(strategy, step, lprobs, scores, gaps):
    if strategy[0] == "groups":
        return do.group_step(step, lprobs, scores, strategy[1], strategy[2], gaps)
    return do.sibling_step(step, lprobs, scores, strategy[1], gaps)


def steps_fixture(search):
    arrays, worst = {}, float("inf")
    cases = [("groups", K, G, s) for K, G, s in dc.STEP_GROUPS] + [("siblings", K, None, r) for K, r in dc.STEP_SIBLINGS]
    for n, (kind, K, G, amount) in enumerate(cases):
        for step in dc.STEP_STEPS:
            lprobs, scores = dc.step_inputs(K, step, dc.STEP_SEED + 10 * n + step)
            ref = search.DiverseBeamSearch(_Dict(), G, amount) if kind == "groups" else search.DiverseSiblingsSearch(_Dict(), amount)
            sc, idx, beams = ref.step(step, lprobs.clone(), scores.clone())
            gaps = []
            strategy = ("groups", G, amount) if kind == "groups" else ("siblings", amount)
            osc, oidx, obeams = oracle_step(strategy, step, lprobs, scores, gaps)
            key = dc.step_key(kind, K, G, amount, step)
            assert torch.equal(idx, oidx) and torch.equal(beams, obeams) and torch.equal(sc, osc), f"{key}: the oracle differs"
            assert min(gaps) >= dc.MIN_GAP, f"{key}: a selection decided by {min(gaps):.2e}"
            worst = min(worst, min(gaps))
            arrays.update({f"{key}.lprobs": lprobs.numpy(), f"{key}.scores": scores.numpy(), f"{key}.out_scores": sc.numpy(),
                           f"{key}.out_indices": idx.numpy(), f"{key}.out_beams": beams.numpy()})
    print(f"(a) {len(arrays) // 5} steps, smallest gap {worst:.3e}")
    arrays["min_gap"] = np.array(worst, np.float64)
    return arrays


def run(model, d, src_slots, gen_cfg, strategy=None, log=None):
    """generate() of the reference; log: per step, the oracle's check of the strategy's step and what the fixture must cover."""
    from ofasys import ModalityType
    from ofasys.generator.sequence_generator import SequenceGenerator
    from ofasys.preprocessor import Slot
    gen = SequenceGenerator(d, search_strategy=strategy, **gen_cfg)
    if log is not None:
        step_fn, K = gen.search.step, gen_cfg["beam_size"]

        def step(step_i, lprobs, scores, *a, **k):
            lp, scs = lprobs.clone(), None if scores is None else scores.clone()
            out = step_fn(step_i, lprobs, scores, *a, **k)
            sc, idx, beams = out
            osc, oidx, obeams = oracle_step(log["strategy"], step_i, lp, scs, log["gaps"])
            assert torch.equal(idx, oidx) and torch.equal(beams, obeams), f"step {step_i}: the oracle picks other candidates"
            assert torch.allclose(sc, osc, rtol=0, atol=1e-6), f"step {step_i}: the oracle's scores differ"
            G = log["strategy"][1] if log["strategy"][0] == "groups" else 1
            eos_top = (idx[:, :K] == d.eos()) & torch.isfinite(sc[:, :K])
            log["eos_other_group"] += int((eos_top & (torch.arange(K) % G != 0)).sum())
            return out
        gen.search.step = step
    slots = list(src_slots) + [Slot(ModalityType.TEXT, False, torch.zeros(len(src_slots[0].value), 1, dtype=torch.long))]
    return gen.generate(model, {"net_input": {"slots": slots}})


def generate_fixture(search):
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
    arrays, tokens_changed, eos_other, gap_of = {}, {"groups": False, "siblings": False}, 0, {}
    for name, cfg in dc.CONFIGS.items():
        gen_cfg, s = cfg["gen"], cfg["strategy"]
        kind = "groups" if "diverse_beam_groups" in s else "siblings"
        strategy = ("groups", s["diverse_beam_groups"], s["diverse_beam_strength"]) if kind == "groups" else ("siblings", s["diversity_rate"])
        log = {"strategy": strategy, "gaps": [], "eos_other_group": 0}
        res = run(model, d, src, gen_cfg, dc.strategy_of(cfg, d, search.DiverseBeamSearch, search.DiverseSiblingsSearch), log)
        n_best, max_len = gen_cfg["return_n_best"], gen_cfg["max_len"]
        toks, lens, scores, pos = flatten(res, n_best, max_len)
        arrays.update({f"{name}.tokens": toks, f"{name}.lens": lens, f"{name}.scores": scores, f"{name}.pos": pos})
        t2, l2, s2, _ = flatten(run(model, d, src, gen_cfg), n_best, max_len)
        same_tokens = np.array_equal(t2, toks) and np.array_equal(l2, lens)
        if kind == "groups":
            assert not (same_tokens and np.allclose(s2, scores, rtol=0, atol=1e-6)), f"{name}: equals plain beam search"
        tokens_changed[kind] |= not same_tokens
        eos_other += log["eos_other_group"]
        gap_of[name] = min(log["gaps"])
        print(f"{name}: lengths {lens.tolist()} tokens {'differ from' if not same_tokens else 'equal'} plain beam search, "
              f"EOS from another group {log['eos_other_group']}, smallest gap {gap_of[name]:.3e}")
        assert gap_of[name] >= dc.MIN_GAP, f"{name}: a selection decided by {gap_of[name]:.2e} < {dc.MIN_GAP}"
    assert tokens_changed["groups"] and tokens_changed["siblings"], f"tokens changed: {tokens_changed}"
    assert eos_other > 0, "no step with a finite EOS candidate among the first K positions from a group other than 0"
    arrays["configs"] = np.array(json.dumps(dc.CONFIGS))
    arrays["gaps"] = np.array(json.dumps(gap_of))
    return arrays


def main():
    install()
    import ofasys  # noqa: F401
    from ofasys.utils import search
    for out, arrays in ((OUT_STEPS, steps_fixture(search)), (OUT_GEN, generate_fixture(search))):
        np.savez_compressed(out, **arrays)
        size = os.path.getsize(out)
        if size > MAX_BYTES:
            os.remove(out)
            raise AssertionError(f"{out}: {size} bytes, above the scale of the other goldens")
        print("wrote", out, size, "bytes")


if __name__ == "__main__":
    main()
