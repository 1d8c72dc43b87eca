"""Generate tests/golden/sampling.npz by RUNNING THE REFERENCE's SequenceGenerator.generate with search_strategy=Sampling(...) on the
CPU (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_sampling_golden.py
The reference GeneralistModel (`tiny_text` case, recipe weights, the beam golden's EOS boost, eval mode) samples for the case's
two source sentences under the configurations of tests/sampling_case.py.  The ONE change to the reference's run: for the duration
of Sampling.step, torch.multinomial is replaced by the project's draw rule (tests/sampling_case.py: inverse CDF of the kept
weights in vocabulary order) fed from a recorded table of uniform numbers, [steps + 1, rows] with the rows of the FIXED batch --
the reference's shrinking batch is mapped back through original_batch_idxs.  `RecordedSampling` works out the token ids of the
kept columns for the mode first (topk indices, _sample_topp on a clone, or arange) and then calls the reference's step unchanged.

Only data is stored, per configuration and run: the uniforms, the hypotheses (tokens, lengths, scores, positional scores), and for
every step what Sampling.step saw and returned in fixed rows (lprobs, kept-set size, kept token ids, drawn token, drawn lprob,
cumulative score, parent slot).  Seeds of the tables are searched from 0 upward until the margin conditions hold for every draw of
the run; the script then asserts the coverage the tests are meant to pin.
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
from tests.sampling_case import (CONFIGS, DRAW_MARGIN, RUNS, TOPP_MARGIN, boost_eos, draw, kept_set, topk_margin_ok,  # noqa: E402
                                 topp_margin_ok)

OUT = os.path.join(ROOT, "tests", "golden", "sampling.npz")
MAX_KEPT = 64               # kept token ids are stored for sets up to this size (top-k / top-p at V = 204)


class MarginError(Exception):
    pass


def make_strategy(d, topk, topp, K, bsz, uniforms, log):
    from ofasys.utils.search import Sampling

    class RecordedSampling(Sampling):
        def step(self, step, lprobs, scores, prev_output_tokens=None, original_batch_idxs=None):
            nb, beam, V = lprobs.shape
            orig = original_batch_idxs.tolist()
            seen = lprobs[:, ::beam] if step == 0 else lprobs                      # what the draws read
            if self.sampling_topp > 0:
                probs, ids = self._sample_topp(seen.clone())
                ids = torch.where(probs > 0, ids, torch.full_like(ids, -1))         # trimmed columns weigh nothing
            elif self.sampling_topk > 0:
                ids = seen.topk(self.sampling_topk)[1]
            else:
                ids = torch.arange(V).expand(seen.shape[0], seen.shape[1], V)
            ids2d = ids.reshape(-1, ids.shape[-1])
            # fixed row of every (row of probs2d, sample)
            if step == 0:
                fixed = [[orig[i] * K + j for j in range(beam)] for i in range(nb)]
            else:
                fixed = [[orig[i // beam] * K + i % beam] for i in range(nb * beam)]
            real = torch.multinomial

            def multinomial(probs2d, num, replacement=True):
                out = torch.zeros(probs2d.shape[0], num, dtype=torch.long)
                for i in range(probs2d.shape[0]):
                    tok = ids2d[i]
                    cols = torch.argsort(torch.where(tok >= 0, tok, torch.full_like(tok, V)), stable=True)   # vocabulary order
                    w = probs2d[i].double()[cols]
                    W, cdf = float(w.sum()), w.cumsum(0)
                    for j in range(num):
                        t = float(uniforms[step, fixed[i][j]]) * W
                        hit = ((cdf > t) & (w > 0)).nonzero()
                        out[i, j] = cols[int(hit[0]) if hit.numel() else int((w > 0).nonzero()[-1])]
                return out
            torch.multinomial = multinomial
            try:
                sc, idx, beams = super().step(step, lprobs.clone(), scores, prev_output_tokens, original_batch_idxs)
            finally:
                torch.multinomial = real
            # ---- record, in fixed rows, and check the margins with the shared restatement
            for i in range(nb):
                for j in range(beam):
                    r = orig[i] * K + j
                    row = lprobs[i, 0 if step == 0 else j]
                    kept, facts = kept_set(row, self.sampling_topk if self.sampling_topp <= 0 else -1, self.sampling_topp)
                    if self.sampling_topp > 0 and not topp_margin_ok(facts, self.sampling_topp, TOPP_MARGIN):
                        raise MarginError(f"step {step} row {r}: top-p boundary {facts}")
                    if self.sampling_topp <= 0 and not topk_margin_ok(facts):
                        raise MarginError(f"step {step} row {r}: tie at the top-k boundary")
                    c, m = draw(row, kept, float(uniforms[step, r]))
                    if m < DRAW_MARGIN:
                        raise MarginError(f"step {step} row {r}: draw margin {m:.2e}")
                    assert c == int(idx[i, j]), (step, r, c, int(idx[i, j]))        # the restatement draws what the reference drew
                    log["margin"] = min(log["margin"], m)
                    log["lprobs"][step, r] = lprobs[i, j].numpy()
                    n = int(kept.sum())
                    log["kept_n"][step, r] = n
                    if n <= MAX_KEPT:
                        log["kept_ids"][step, r, :n] = kept.nonzero().flatten().numpy()
                    log["tok"][step, r], log["beam"][step, r] = int(idx[i, j]), int(beams[i, j])
                    log["lp"][step, r], log["score"][step, r] = float(row[idx[i, j]]), float(sc[i, j])
            log["steps"] = max(log["steps"], step + 1)
            return sc, idx, beams
    return RecordedSampling(d, topk, topp)


def run(model, d, src_slots, cfg, uniforms, bsz):
    from ofasys import ModalityType
    from ofasys.generator.sequence_generator import SequenceGenerator
    from ofasys.preprocessor import Slot
    gen_cfg = cfg["gen"]
    K, T, V = gen_cfg["beam_size"], gen_cfg["max_len"] + 1, len(d)
    rows = bsz * K
    log = {"margin": np.inf, "steps": 0, "lprobs": np.full((T, rows, V), np.nan, np.float32),
           "kept_n": np.zeros((T, rows), np.int64), "kept_ids": np.full((T, rows, MAX_KEPT), -1, np.int64),
           "tok": np.full((T, rows), -1, np.int64), "beam": np.full((T, rows), -1, np.int64),
           "lp": np.full((T, rows), np.nan, np.float32), "score": np.full((T, rows), np.nan, np.float32), "finish_step": {}}
    gen = SequenceGenerator(d, search_strategy=make_strategy(d, cfg["topk"], cfg["topp"], K, bsz, uniforms, log), **gen_cfg)
    fin_fn = gen.finalize_hypos

    def fin(step_i, *a, **k):
        before = list(a[5])
        out = fin_fn(step_i, *a, **k)
        for s, (b, f) in enumerate(zip(before, a[5])):
            if f and not b:
                log["finish_step"][s] = step_i
        return out
    gen.finalize_hypos = fin
    slots = list(src_slots) + [Slot(ModalityType.TEXT, False, torch.zeros(bsz, 1, dtype=torch.long))]
    return gen.generate(model, {"net_input": {"slots": slots}}), log


def flatten(result, n_best, max_len):
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
    bsz = int(src[0].value.shape[0])
    arrays, steps_seen, finish_order, reorder_seen, worst = {}, set(), False, False, np.inf
    for name, cfg in CONFIGS.items():
        g = cfg["gen"]
        K, T = g["beam_size"], g["max_len"] + 1
        seed, found = 0, 0
        while found < RUNS:
            uniforms = np.random.default_rng(seed).random((T, bsz * K), dtype=np.float32)
            seed += 1
            try:
                res, log = run(model, d, src, cfg, uniforms, bsz)
            except MarginError as e:
                print(name, "seed", seed - 1, "skipped:", e)
                continue
            n_best = g.get("return_n_best", -1) if g.get("return_n_best", -1) != -1 else K
            toks, lens, scores, pos = flatten(res, n_best, g["max_len"])
            key = f"{name}.{found}"
            n = log["steps"]
            arrays.update({f"{key}.uniforms": uniforms, f"{key}.tokens": toks, f"{key}.lens": lens, f"{key}.scores": scores,
                           f"{key}.pos": pos, f"{key}.seed": np.array(seed - 1), f"{key}.steps": np.array(n)})
            arrays.update({f"{key}.step_{k}": log[k][:n] for k in ("lprobs", "kept_n", "kept_ids", "tok", "beam", "lp", "score")})
            steps_seen |= set(int(x) - 1 for x in lens.ravel() if x > 0)
            fs = log["finish_step"]
            finish_order |= len(set(fs.values())) > 1
            # a slot that ends while another of its sentence goes on: the next step's slots were compacted
            for t in range(n - 1):
                for s in range(bsz):
                    tk = log["tok"][t, s * K:(s + 1) * K]
                    went_on = log["tok"][t + 1, s * K] >= 0
                    if went_on and K > 1 and (tk[:-1] == d.eos()).any() and (tk != d.eos()).any():
                        first_eos = int(np.argmax(tk == d.eos()))
                        reorder_seen |= bool((tk[first_eos + 1:] != d.eos()).any())
            worst = min(worst, log["margin"])
            print(key, "seed", seed - 1, "lengths", lens.tolist(), "finish steps", fs, "draw margin", log["margin"])
            found += 1
    assert len(steps_seen) >= 3, f"hypotheses finalised at only {sorted(steps_seen)}"
    assert finish_order, "no sentence finishes before another"
    assert reorder_seen, "no slot ends while a later slot of its sentence goes on (no non-identity reorder)"
    arrays["configs"] = np.array(json.dumps(CONFIGS))
    arrays["margins"] = np.array([DRAW_MARGIN, TOPP_MARGIN])
    arrays["worst_draw_margin"] = np.array(worst)
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; finalisation steps", sorted(steps_seen), "worst draw margin", worst)


if __name__ == "__main__":
    main()
