"""The trie-constrained beam-search golden scenario shared by tools/gen_trie_beam_golden.py (reference, CPU) and
tests/test_trie_beam_*.py: closed sets and generator configurations run on the two source sentences of the `tiny_text` case (recipe
weights as they are: no EOS boost, so the unnormalised scores are those of tests/golden/traverse.npz).  TEST INFRASTRUCTURE."""
from tests.traverse_case import ANSWERS

SCORE_TOL = 1e-3              # the project's standing fp32 bound against the reference (relative, floor absolute)
UNK = 3

CLOSED_SETS = {
    "main": ANSWERS,                                           # 14 answers, 13 distinct, 1-4 tokens (tests/traverse_case.py)
    "small": [[17], [40, 8], [90, 12, 64]],                    # fewer answers than beams
    # <unk> as an answer and inside one (unk_penalty), and an answer that repeats a bigram (no_repeat_ngram_size = 2 cuts it)
    "extra": ANSWERS + [[UNK], [17, UNK], [40, 8, 40, 8]],
}

# Generator arguments under the names Task.generator_kwargs takes (beam, lenpen, unkpen, ...); `set`: the closed set.
CONFIGS = {
    "beam1": dict(set="main", beam=1, max_len=10),
    "beam3_norm": dict(set="main", beam=3, max_len=10, normalize_scores=True, return_n_best=3),
    "beam5_ngram_temp": dict(set="main", beam=5, max_len=10, no_repeat_ngram_size=2, temperature=0.7, return_n_best=5),
    "beam16": dict(set="main", beam=16, max_len=10, return_n_best=16),
    "beam16_max_len3": dict(set="main", beam=16, max_len=3, return_n_best=16),
    "beam5_long": dict(set="main", beam=5, max_len=256, return_n_best=5),
    "beam16_unk_ngram": dict(set="extra", beam=16, max_len=10, unkpen=0.75, no_repeat_ngram_size=2, return_n_best=16),
    "beam16_extra_plain": dict(set="extra", beam=16, max_len=10, return_n_best=16),
    "beam5_small": dict(set="small", beam=5, max_len=10, return_n_best=5),
}
WIDTH = 8                     # stored token columns: the longest answer + EOS fits


def generator_args(cfg):
    """The configuration without its closed-set name."""
    return {k: v for k, v in cfg.items() if k != "set"}


def distinct(answers):
    out = []
    for a in answers:
        if list(a) not in out:
            out.append(list(a))
    return out


def label_of(answers, tokens):
    """The lowest label whose answer is `tokens` (without EOS)."""
    return [list(a) for a in answers].index(list(tokens))
