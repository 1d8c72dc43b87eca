"""The diverse-decoding golden scenarios shared by tools/gen_diverse_golden.py (reference, CPU) and tests/test_diverse_beam_*.py.
TEST INFRASTRUCTURE.

(a) STEP_*: single calls of the reference's DiverseBeamSearch.step / DiverseSiblingsSearch.step on small random inputs
    (tests/golden/diverse_search_steps.npz).
(b) CONFIGS: SequenceGenerator.generate on the `tiny_text` recipe model with the EOS boost of tests/beam_case.py
    (tests/golden/diverse_beam.npz).  "strategy" is what builds the search strategy, "gen" the generator's keywords.
"""
import torch

# the project's fp32 parity bound: below it a GPU run may legitimately order two candidates the other way
MIN_GAP = 1e-3

# ---------------------------------------------------------------- (a) single steps
STEP_BSZ, STEP_V, STEP_STEPS = 2, 40, (0, 3)
STEP_SEED = 19000         # (of the random inputs; chosen so that no selection is decided by less than MIN_GAP -- the tool asserts it)
STEP_GROUPS = [(K, G, s) for (K, G) in ((4, 2), (4, 4), (6, 3), (8, 1)) for s in (0.5, 2.0)]
STEP_SIBLINGS = [(K, r) for K in (2, 5) for r in (0.0, 0.5, 3.0)]


def step_key(kind, K, x, amount, step):
    return f"{kind}.K{K}" + (f".G{x}" if kind == "groups" else "") + f".a{amount}.s{step}"


def step_inputs(K, step, seed):
    """lprobs [bsz, K, V] (a log-softmax of random logits) and the cumulative scores [bsz, K, step + 1] of one recorded step."""
    g = torch.Generator().manual_seed(seed)
    lprobs = torch.log_softmax(torch.randn(STEP_BSZ, K, STEP_V, generator=g) * 2.0, -1)
    scores = torch.zeros(STEP_BSZ, K, step + 1)
    if step > 0:
        scores[:, :, :step] = -torch.rand(STEP_BSZ, K, step, generator=g).cumsum(-1) * 2
    return lprobs, scores


# ---------------------------------------------------------------- (b) generate
CONFIGS = {
    "groups2": dict(strategy=dict(diverse_beam_groups=2, diverse_beam_strength=0.5),
                    gen=dict(beam_size=4, max_len=10, normalize_scores=False, return_n_best=4)),
    "groups4": dict(strategy=dict(diverse_beam_groups=4, diverse_beam_strength=1.5),
                    gen=dict(beam_size=4, max_len=10, normalize_scores=False, return_n_best=4)),
    "groups2_ngram": dict(strategy=dict(diverse_beam_groups=2, diverse_beam_strength=0.5),
                          gen=dict(beam_size=4, max_len=10, no_repeat_ngram_size=2, unk_penalty=0.5, temperature=0.7,
                                   normalize_scores=True, return_n_best=4)),
    "groups3_beam6": dict(strategy=dict(diverse_beam_groups=3, diverse_beam_strength=1.0),
                          gen=dict(beam_size=6, max_len=8, min_len=2, normalize_scores=False, return_n_best=6)),
    "siblings_half": dict(strategy=dict(diversity_rate=0.5),
                          gen=dict(beam_size=4, max_len=10, normalize_scores=False, return_n_best=4)),
    "siblings_two": dict(strategy=dict(diversity_rate=2.0),
                         gen=dict(beam_size=4, max_len=10, normalize_scores=True, len_penalty=1.0, return_n_best=4)),
}


def strategy_of(cfg, tgt_dict, groups_cls, siblings_cls):
    """The search strategy of a configuration, built from the caller's classes (the reference's, or this project's holders)."""
    s = cfg["strategy"]
    if "diverse_beam_groups" in s:
        return groups_cls(tgt_dict, s["diverse_beam_groups"], s["diverse_beam_strength"])
    return siblings_cls(tgt_dict, s["diversity_rate"])
