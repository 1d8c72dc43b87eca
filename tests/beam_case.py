"""The beam-search golden scenario shared by tools/gen_beam_golden.py (reference, CPU) and tests/test_beam_search_*.py:
generator configurations and the EOS boost applied to the `tiny_text` recipe weights.  TEST INFRASTRUCTURE."""
import math

from oracle import recipe

# With V = 204 and random recipe weights EOS (id 2) almost never wins a step: its row of the tied output projection / token
# embedding gets EOS_BOOST * (a recipe direction, unit norm) added, so hypotheses end at several different steps.
EOS_BOOST = -4.0          # (sign and size chosen so that hypotheses end at steps 1-10; tools/gen_beam_golden.py asserts the coverage)

CONFIGS = {
    "beam1": dict(beam_size=1, max_len=10, normalize_scores=False),
    "beam3_norm": dict(beam_size=3, max_len=10, min_len=2, normalize_scores=True, len_penalty=1.0),
    "beam4_ngram": dict(beam_size=4, max_len=10, no_repeat_ngram_size=2, unk_penalty=0.5, temperature=0.7, return_n_best=4,
                        normalize_scores=False),
    "beam3_range": dict(beam_size=3, max_len=9, constraint_range="(4, 120)", return_n_best=3, normalize_scores=False),
}


def boost_eos(embed_weight, eos):
    """In place: embed_weight[eos] += EOS_BOOST * u, u the unit `input.beam_eos_dir` recipe vector."""
    D = embed_weight.shape[1]
    u = recipe.floats("input.beam_eos_dir", (D,))
    u = u / math.sqrt(float((u * u).sum()))
    embed_weight[eos] += (EOS_BOOST * u).to(embed_weight.dtype).to(embed_weight.device)
