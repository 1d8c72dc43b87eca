"""CPU: beam search under a forced target prefix without a GPU -- the C ABI of the prefix entry points, their register
allocation, the restatement of tests/beam_prefix_case.py against what the reference recorded for one step, the fixture's facts,
and check_sample's accept / refuse table."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.beam_prefix_case import CONFIGS, EOS, LPROBS_OF, PAD, mask_lprobs, select
from tests.golden_util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRY_POINTS = ("ofa_beam_prefix_topk", "ofa_beam_prefix_fill", "ofa_beam_prefix_select")


def test_header_declares_and_library_exports_prefix_entry_points():
    import ctypes
    from ofasys_amd import kernels as Kn, lib as L
    protos = L.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos
        getattr(ctypes.CDLL(L.LIB_PATH), name)
        assert callable(getattr(Kn, name[len("ofa_"):]))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_prefix_kernels_compile_without_spills(tmp_path):
    out = tmp_path / "beam_search.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "ofasys_amd", "csrc", "beam_search.hip"), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("vgpr_spill_count", "private_segment_fixed_size", "vgpr_count", "wavefront_size")}
    row = [k for k in meta if "beam_prefix_row_kernel" in k]
    fill = [k for k in meta if "beam_prefix_fill_kernel" in k]
    assert len(row) == 3 and len(fill) == 1, sorted(meta)
    for k in row + fill:                         # wave64, no scratch, the register budget of DESIGN.md 5g (two workgroups per SIMD pair)
        assert meta[k]["wavefront_size"] == 64
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_count"] <= 128, (k, meta[k])


def test_fixture_facts_and_self_consistency():
    g = load_golden("beam_prefix")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(CONFIGS))
    beams = {c["gen"]["beam_size"] for c in CONFIGS.values()}
    widths = {len(c["prefix"][0]) for c in CONFIGS.values()}
    assert {1, 5} <= beams and {1, 3} <= widths
    assert any(PAD in c["prefix"][1] and PAD not in c["prefix"][0] for c in CONFIGS.values())          # a ragged batch
    assert any(c["gen"].get("no_repeat_ngram_size") == 2 for c in CONFIGS.values())
    for name, c in CONFIGS.items():
        assert bool(g[f"{name}.hyps_follow_prefix"]) and bool(g[f"{name}.active_follow_prefix"]) and bool(g[f"{name}.tie_order_free"])
        toks, lens, scores, pos = g[f"{name}.tokens"], g[f"{name}.lens"], g[f"{name}.scores"], g[f"{name}.pos"]
        assert np.array_equal(g[f"{name}.prefix"], np.array(c["prefix"]))
        for b in range(toks.shape[0]):
            want = [t for t in c["prefix"][b] if t != PAD]
            assert (lens[b] > 0).all()
            for i in range(toks.shape[1]):
                n = int(lens[b, i])
                assert toks[b, i, :len(want)].tolist() == want and toks[b, i, n - 1] == EOS
                raw = pos[b, i, :n].astype(np.float64).sum()
                if c["gen"].get("normalize_scores", True):
                    raw /= n ** c["gen"].get("len_penalty", 1.0)
                assert abs(raw - float(scores[b, i])) < 1e-4, (name, b, i)


def test_restatement_reproduces_the_recorded_first_step():
    """The reference's lprobs of step 0 (beam 1, width 1) through the restatement: the masked lprobs search.step received, and its
    first candidate -- the forced token with its own lprob; the second candidate's value is the fill f = min g - 1 (its token is
    one of the ties)."""
    g = load_golden("beam_prefix")
    c = CONFIGS[LPROBS_OF]
    K, bsz = c["gen"]["beam_size"], len(c["prefix"])
    assert K == 1
    lp = torch.from_numpy(g["step0.lprobs"]).clone()
    V = lp.shape[1]
    cfg = dict(min_len=1, max_len=c["gen"]["max_len"], unk_penalty=0.0, ngram=0, normalize=False, len_penalty=1.0)
    i32 = torch.int32
    st = {"tokens": torch.full((bsz, 10), PAD, dtype=torch.long), "scores": torch.zeros(bsz, 10), "ignore": torch.zeros(bsz, K, dtype=i32),
          "done": torch.zeros(bsz, dtype=i32), "nfin": torch.zeros(1, dtype=i32), "reorder": torch.arange(bsz),
          "fin_tok": torch.zeros(bsz, K, 10, dtype=torch.long), "fin_pos": torch.zeros(bsz, K, 10), "fin_score": torch.zeros(bsz, K),
          "fin_len": torch.zeros(bsz, K, dtype=i32), "fin_cnt": torch.zeros(bsz, dtype=i32)}
    st["tokens"][:, 0] = 0
    prefix = torch.tensor(c["prefix"])
    gvals = lp.gather(1, prefix[:, :1]).squeeze(1)
    masked = mask_lprobs(lp, st, K, 0, cfg, prefix[:, 0], (prefix != PAD).sum(1))
    assert torch.equal(masked, torch.from_numpy(g["step0.masked"]).reshape(bsz, V))
    new = select(masked, st, K, 0, cfg)
    assert new["tokens"][:, 1].tolist() == g["step0.cand_tokens"][:, 0].tolist() == prefix[:, 0].tolist()
    assert torch.equal(new["scores"][:, 0], torch.from_numpy(g["step0.cand_scores"][:, 0]))
    assert torch.equal(torch.from_numpy(g["step0.cand_scores"][:, 1]), (gvals.min() - 1).expand(bsz))


def _gen(**kw):
    from ofasys_amd import Dictionary
    from ofasys_amd.generator import SequenceGenerator
    d = Dictionary()
    for i in range(40):
        d.add_symbol(f"<text>_{i}")
    return SequenceGenerator(d, **dict(dict(beam_size=2), **kw)), d


ACCEPTED = [None, torch.zeros(2, 0, dtype=torch.long), [[17], [33]], [[17, 20, 9], [33, 8, PAD]], [[17, 20, 9], [33, PAD, PAD]]]
REFUSED = [([[17, EOS], [33, 8]], "<eos>"), ([[0, 17], [33, 8]], "<bos>"), ([[17, 9000], [33, 8]], "outside the dictionary"),
           ([[17, 20], [PAD, 8]], "<pad> in front"), ([[17, PAD], [33, PAD]], "only <pad>"), ([[PAD], [PAD]], "only <pad>")]


@pytest.mark.parametrize("prefix", ACCEPTED)
def test_check_sample_accepts(prefix):
    gen, _ = _gen()
    sample = {"net_input": {"slots": []}}
    if prefix is not None:
        sample["prefix_tokens"] = torch.as_tensor(prefix, dtype=torch.long)
    assert gen.check_sample(sample) is True
    got = gen._prefix_of(sample)
    if prefix is None or len(sample["prefix_tokens"][0]) == 0:
        assert got is None
    else:
        assert torch.equal(got[0], sample["prefix_tokens"]) and got[1].tolist() == [sum(t != PAD for t in row) for row in prefix]


@pytest.mark.parametrize("prefix,what", REFUSED)
def test_check_sample_refuses(prefix, what):
    gen, _ = _gen()
    with pytest.raises(NotImplementedError, match=what):
        gen.check_sample({"net_input": {"slots": []}, "prefix_tokens": torch.tensor(prefix)})


def test_check_sample_keeps_the_other_refusals_and_the_ngram_rule():
    gen, _ = _gen(no_repeat_ngram_size=1)
    assert gen.check_sample({"net_input": {"slots": []}}) is True
    assert gen.check_sample({"net_input": {"slots": []}, "prefix_tokens": torch.zeros(2, 0, dtype=torch.long)}) is False
    with pytest.raises(NotImplementedError, match="constraints"):
        gen.check_sample({"net_input": {"slots": []}}, constraints=torch.zeros(1, 1))


def test_trie_generator_keeps_refusing_a_prefix():
    from ofasys_amd import Dictionary, TraversePlan
    from ofasys_amd.generator import TrieBeamGenerator
    d = Dictionary()
    for i in range(40):
        d.add_symbol(f"<text>_{i}")
    gen = TrieBeamGenerator(d, TraversePlan([[5, 6], [5, 7, 8]], d.bos(), d.eos(), d.pad()), beam_size=2)
    with pytest.raises(NotImplementedError, match="TrieBeamGenerator: prefix"):
        gen.check_sample({"net_input": {"slots": []}, "prefix_tokens": torch.tensor([[17], [33]])})


def test_step_decoder_keys_graphs_by_variant():
    """`step` takes a variant; the default keeps the plain step number as the key."""
    import inspect
    from ofasys_amd.generator import StepDecoder
    sig = inspect.signature(StepDecoder.step)
    assert list(sig.parameters)[-1] == "variant" and sig.parameters["variant"].default is None
