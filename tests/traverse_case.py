"""The closed-set golden scenario shared by tools/gen_traverse_golden.py (reference, CPU) and tests/test_traverse_*.py: the answer
set scored for the two source sentences of the `tiny_text` case.  TEST INFRASTRUCTURE."""

# Token-id sequences from the '<text>_i' range of the 204-symbol test dictionary (ids 4 .. 203), in label order: 1-4 tokens, shared
# first tokens (17, 40, 90), [17, 23] a strict prefix of [17, 23, 99] and of [17, 23, 99, 5], [40, 8] given twice.
ANSWERS = [
    [17],
    [17, 23, 99],
    [40, 8],
    [17, 23],
    [61],
    [40, 8, 120, 33],
    [90, 12],
    [40, 8],
    [17, 23, 99, 5],
    [90, 150, 7],
    [134, 20],
    [40, 77],
    [90, 12, 64],
    [188, 4],
]
VALID_BATCH_SIZE = 5          # the reference's chunk size: 14 answers -> ragged chunks of 5, 5, 4
SCORE_TOL = 1e-3              # the project's standing fp32 bound against the reference (relative, floor absolute)


def score_err(got, want):
    """max over all entries of |got - want| / max(|want|, 1): relative with an absolute floor."""
    import numpy as np
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1.0)).max())


def random_answers(rng, C, V=204, max_len=5, pool=12, p_dup=0.1, p_ext=0.45):
    """Answers of 1 .. max_len tokens with shared prefixes, prefixes that are answers themselves, and duplicates (p_dup: a copy
    of an earlier answer; p_ext: a prefix of an earlier answer plus tokens from a small pool; else a fresh first token)."""
    answers = []
    for _ in range(C):
        r = rng.random()
        if answers and r < p_dup:
            a = list(answers[rng.integers(len(answers))])                        # a duplicate
        elif answers and r < p_dup + p_ext:
            base = answers[rng.integers(len(answers))]
            keep = int(rng.integers(1, len(base) + 1))
            a = list(base[:keep])
            if len(a) < max_len:
                a += [int(4 + rng.integers(pool)) for _ in range(rng.integers(0, max_len - len(a) + 1))]
        else:
            a = [int(rng.integers(4, V))] + [int(4 + rng.integers(pool)) for _ in range(rng.integers(0, max_len))]
        answers.append(a)
    return answers
