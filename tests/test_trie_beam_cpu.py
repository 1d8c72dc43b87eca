"""CPU: trie-constrained beam search without a GPU -- TraversePlan.edge_child / max_degree against walks of the collater's Trie,
the C ABI of csrc/trie_beam.hip (exports, argument validation before any launch, register allocation), the option handling of
TrieBeamGenerator and TraverseTask(search=...), and the reference-recorded golden's self-consistency."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.golden_util import load_golden
from tests.traverse_case import ANSWERS, random_answers
from tests.trie_beam_case import CLOSED_SETS, CONFIGS, WIDTH, distinct, generator_args, label_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BOS, PAD, EOS = 0, 1, 2


# ------------------------------------------------------------------------------------------------ the plan
def _trie(answers):
    from ofasys_amd.preprocessor.collate import Trie
    trie = Trie(EOS)
    for a in answers:
        trie.insert([BOS] + list(a) + [EOS])
    return trie


def _check_children(plan, answers):
    trie = _trie(answers)
    assert plan.edge_child.shape == (plan.E,) and plan.edge_child.dtype == np.int32
    assert plan.max_degree == max(int(plan.node_edge_off[n + 1] - plan.node_edge_off[n]) for n in range(plan.N))
    assert ((plan.edge_token == EOS) == (plan.edge_child == -1)).all()              # every EOS edge, and only those, leads nowhere
    assert plan.edge_child.max(initial=-1) < plan.N
    seen = set()
    for c, a in enumerate(answers):                                                 # walk every answer from the root by edge_child
        node, prefix = 0, [BOS]
        path = plan.path_edge[plan.path_off[c]:plan.path_off[c + 1]]
        for t, tok in enumerate(list(a) + [EOS]):
            lo, hi = int(plan.node_edge_off[node]), int(plan.node_edge_off[node + 1])
            toks = plan.edge_token[lo:hi].tolist()
            assert sorted(toks) == sorted(trie.get_next_layer(prefix)), (c, t)      # the node's edges are the trie's next layer
            e = lo + toks.index(tok)
            assert e == int(path[t]) and int(plan.edge_node[e]) == node             # consistent with path_edge
            seen.add(e)
            node = int(plan.edge_child[e])
            prefix.append(tok)
            if tok != EOS:
                assert node == plan.node_of(c, t + 1)
        assert node == -1 and trie.get_next_layer(prefix) == []                     # past EOS nothing is allowed
    assert len(seen) == plan.E                                                      # every edge lies on some answer's walk


def test_edge_child_and_max_degree_match_trie_walks():
    from ofasys_amd import TraversePlan
    plan = TraversePlan(ANSWERS, BOS, EOS, PAD)
    _check_children(plan, ANSWERS)
    assert plan.max_degree == 6 and plan.Tmax == 5                                  # the root: 17, 40, 61, 90, 134, 188
    rng = np.random.default_rng(4711)
    for _ in range(100):
        answers = random_answers(rng, int(rng.integers(1, 40)))
        _check_children(TraversePlan(answers, BOS, EOS, PAD), answers)


def test_to_device_carries_the_new_arrays():
    from ofasys_amd import TraversePlan
    d = TraversePlan(ANSWERS, BOS, EOS, PAD).to_device("cpu")
    assert d["max_degree"] == 6 and d["edge_child"].dtype == torch.int32 and d["edge_child"].numel() == d["E"]
    for k in ("node_edge_off", "edge_token", "edge_node", "rep_ans", "rep_pos", "path_off", "path_edge", "items", "prev_output_tokens"):
        assert k in d                                                               # nothing existing changed


# ------------------------------------------------------------------------------------------------ the C ABI
ENTRY_POINTS = ("ofa_trie_beam_splits", "ofa_trie_beam_topk", "ofa_trie_beam_advance")


def test_header_declares_and_library_exports_trie_beam_entry_points():
    import ctypes
    from ofasys_amd import kernels as K
    from ofasys_amd import lib as L
    protos = L.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos
        getattr(ctypes.CDLL(L.LIB_PATH), name)
    assert all(hasattr(K, n) for n in ("trie_beam_splits", "trie_beam_topk", "trie_beam_advance"))
    h = L.lib()
    # 256 edges per workgroup while the parts fit the sentence pass's layout (ceil(V / 4096) parts), more edges each beyond that
    assert h.cdll.ofa_trie_beam_splits(6, 204) == 1 and h.cdll.ofa_trie_beam_splits(256, 59457) == 1
    assert h.cdll.ofa_trie_beam_splits(257, 59457) == 2 and h.cdll.ofa_trie_beam_splits(3129, 51265) == 13
    assert h.cdll.ofa_trie_beam_splits(3329, 51265) == 7 and h.cdll.ofa_trie_beam_splits(200, 204) == 1
    assert h.cdll.ofa_trie_beam_splits(0, 204) == 0 and h.cdll.ofa_trie_beam_splits(300, 204) == 0
    for V in (204, 4097, 51265, 59457):
        for deg in (1, 255, 256, 257, 1000, 4096, V):
            if deg <= V:
                assert 1 <= h.cdll.ofa_trie_beam_splits(deg, V) <= (V + 4095) // 4096


def test_status_codes_before_any_launch():
    """Argument validation returns status codes before a kernel is launched, so it is observable without a GPU (the pointers are
    never dereferenced)."""
    from ofasys_amd import lib as L
    h = L.lib()
    import ctypes
    from ofasys_amd import kernels as Kn
    p = 4096                                                                        # a 16-byte aligned stand-in for a pointer

    def split(kw, struct, defaults):
        """A descriptor from its defaults and the keywords that name its fields; the other keywords are the call's own."""
        fields = dict(defaults, **{k: kw.pop(k) for k in list(kw) if k in defaults})
        return struct(**fields)

    def topk(**kw):
        pol = split(kw, Kn._GenPolicy, dict(temperature=1.0, cstart=-1, cend=-1, step=0, min_len=1, max_len=10, pad=1, unk=3, eos=2,
                                            unk_penalty=0.0, ngram=0, tokens=None, tok_ld=0, done=None))
        a = dict(h=p, ld_h=64, dtype=L.F32, W=p, ld_w=64, bias=None, D=64, V=204, rows=10, K=5, node=p, off=p, tok=p, N=7, E=20,
                 max_degree=6, pol=ctypes.byref(pol), ws=p, stream=None)
        a.update(kw)
        h.call("ofa_trie_beam_topk", *a.values())

    def advance(**kw):
        # the fin_* fields stay NULL: the advance pass does not read them
        st = split(kw, Kn._GenState, dict(tokens=p, tok_ld=11, tok_cap=11, scores=p, score_ld=11, ignore=p, reorder=p, done=p, nfin=p))
        a = dict(node=p, off=p, tok=p, child=p, N=7, E=20, st=ctypes.byref(st), bsz=2, K=5, step=0, stream=None)
        a.update(kw)
        h.call("ofa_trie_beam_advance", *a.values())

    for bad, match in ((dict(h=None), "null pointer"), (dict(node=None), "null pointer"), (dict(dtype=7), "dtype"),
                       (dict(K=17), "beam size"), (dict(K=0), "beam size"), (dict(rows=11), "multiple of the beam size"),
                       (dict(V=1 << 23), "2\\^24"), (dict(max_degree=0), "max_degree"), (dict(max_degree=205), "max_degree"),
                       (dict(max_degree=21), "max_degree"), (dict(temperature=0.0), "temperature"),
                       (dict(ngram=2), "token history"), (dict(ngram=2, tokens=p, tok_ld=400, step=300), "n-gram bans beyond"),
                       (dict(D=66), "16-byte"), (dict(ld_w=60), "16-byte"), (dict(h=p + 4), "16-byte"),
                       (dict(dtype=L.BF16, D=68, ld_h=68, ld_w=68), "16-byte"), (dict(D=16384, ld_h=16384, ld_w=16384), "LDS"),
                       (dict(N=0), "N=0"), (dict(step=-1), "step=-1"), (dict(pol=None), "null pointer"),
                       (dict(cstart=4, cend=100), "status 1.*constraint range")):     # the trie is the only constraint
        with pytest.raises(L.OfaError, match=match):
            topk(**bad)
    for bad, match in ((dict(child=None), "null pointer"), (dict(nfin=None), "null pointer"), (dict(st=None), "null pointer"),
                       (dict(K=17), "beam size"),
                       (dict(bsz=0), "bsz=0"), (dict(step=11), "too short"), (dict(score_ld=0), "too short"),
                       (dict(tok_ld=5), "too short"), (dict(N=1 << 24), "N=")):
        with pytest.raises(L.OfaError, match=match):
            advance(**bad)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_trie_beam_kernels_compile_without_spills(tmp_path):
    out = tmp_path / "trie_beam.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "ofasys_amd", "csrc", "trie_beam.hip"), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    # the row pass keeps all its LDS in the dynamic region: no static scratch in front of it shifts the base of the staged hidden
    # row off the 16-byte alignment its reads need
    assert all(m.pop("group_segment_fixed_size") == 0 or "advance" in k for k, m in meta.items())
    assert len([k for k in meta if "trie_beam_topk_kernel" in k]) == 3 and len([k for k in meta if "trie_beam_advance_kernel" in k]) == 1
    assert len(meta) == 4, sorted(meta)
    for k, m in meta.items():
        assert m == {"vgpr_spill_count": 0, "sgpr_spill_count": 0, "private_segment_fixed_size": 0}, (k, m)


# ------------------------------------------------------------------------------------------------ options
def _dict():
    from ofasys_amd import Dictionary
    d = Dictionary()
    for i in range(200):
        d.add_symbol(f"<text>_{i}")
    return d


def _plan():
    from ofasys_amd import TraversePlan
    return TraversePlan(ANSWERS, BOS, EOS, PAD)


def test_trie_beam_generator_options():
    from ofasys_amd.generator import SequenceGenerator, TrieBeamGenerator
    d, plan = _dict(), _plan()
    g, s = TrieBeamGenerator(d, plan), SequenceGenerator(d)
    assert isinstance(g, SequenceGenerator) and g.plan is plan
    for name in ("beam_size", "return_n_best", "max_len_a", "max_len_b", "max_len", "min_len", "normalize_scores", "len_penalty",
                 "unk_penalty", "temperature", "no_repeat_ngram_size", "use_graph"):
        assert getattr(g, name) == getattr(s, name), name                           # the same defaults
    g = TrieBeamGenerator(d, plan, beam_size=7, return_n_best=3, max_len=12, normalize_scores=False, unk_penalty=0.5)
    assert (g.beam_size, g.return_n_best, g.max_len, g.normalize_scores, g.unk_penalty) == (7, 3, 12, False, 0.5)
    assert TrieBeamGenerator(d, plan, 4).beam_size == 4                             # positional, as SequenceGenerator
    for kwargs in ({"search_strategy": object()}, {"lm_model": object()}, {"constraint_trie": object()}, {"match_source_len": True},
                   {"beam_size": 17}):
        with pytest.raises(NotImplementedError):                                    # the same refusals
            TrieBeamGenerator(d, plan, **kwargs)
    with pytest.raises(ValueError, match="temperature"):
        TrieBeamGenerator(d, plan, temperature=0.0)
    with pytest.raises(ValueError, match="constraint_range"):                       # sequence_generator.py:730
        TrieBeamGenerator(d, plan, constraint_range="(4, 100)")
    from ofasys_amd import TraversePlan
    with pytest.raises(ValueError, match="BOS / EOS / PAD"):
        TrieBeamGenerator(d, TraversePlan(ANSWERS, BOS, 5, PAD))
    gen = TrieBeamGenerator(d, plan, beam_size=2)
    with pytest.raises(NotImplementedError, match="prefix"):
        gen.generate(None, {"net_input": {"slots": []}, "prefix_tokens": torch.zeros(1, 1, dtype=torch.long)})
    with pytest.raises(NotImplementedError, match="constraints"):
        gen.generate(None, {"net_input": {"slots": []}}, constraints=torch.zeros(1, 1))
    assert gen.check_sample({"net_input": {"slots": []}, "prefix_tokens": torch.zeros(2, 0, dtype=torch.long)}) is True


def test_step_decoder_features_option_defaults_off():
    from ofasys_amd.generator import StepDecoder
    assert StepDecoder(None, 4).features_only is False and StepDecoder(None, 4, features_only=True).features_only is True


def _task(**kw):
    from ofasys_amd import Dictionary, TraverseTask
    t = TraverseTask(name="vqa", instruction="[TEXT:src] what is it? -> [TEXT:tgt]", **kw)
    return t, Dictionary()


def test_traverse_task_search_options():
    from ofasys_amd.generator import TrieBeamGenerator
    t, d = _task()
    assert (t.search, t.beam, t.max_rows) == ("all", 5, 2048)                        # the defaults: today's behaviour
    t2, _ = _task(search="beam", beam=3, max_rows=64)
    assert (t2.search, t2.beam, t2.max_rows) == ("beam", 3, 64)
    with pytest.raises(ValueError, match="search"):
        _task(search="greedy")
    with pytest.raises(ValueError, match="beam"):
        _task(beam=0)
    with pytest.raises(ValueError, match="initialize"):
        t.trie_generator()
    t.initialize(d, closed_set=[tuple(a) for a in ANSWERS])
    with pytest.raises(ValueError, match="search"):                                  # checked before the model is touched
        t.inference(None, {"net_input": {"slots": []}}, search="greedy")
    g = t.trie_generator(beam=t.beam, return_n_best=1)
    assert isinstance(g, TrieBeamGenerator) and g.plan is t.plan
    # build_generator's defaults (task/base.py:475-486): unnormalised scores, one hypothesis
    assert (g.beam_size, g.return_n_best, g.normalize_scores, g.max_len, g.min_len, g.len_penalty) == (5, 1, False, 256, 1, 1)
    assert t.trie_generator(beam=5, return_n_best=1) is g                            # kept: its step graphs are reused
    g2 = t.trie_generator(beam=16, return_n_best=16, unkpen=0.5, lenpen=2, normalize_scores=True, no_repeat_ngram_size=2)
    assert g2 is not g and (g2.beam_size, g2.unk_penalty, g2.len_penalty, g2.normalize_scores, g2.no_repeat_ngram_size) == (16, 0.5, 2, True, 2)
    with pytest.raises(NotImplementedError):
        t.trie_generator(sampling=True)
    assert t._seq2label[(40, 8)] == 2 and len(t._seq2label) == len(distinct(ANSWERS))   # duplicates go to the lowest label
    t.build_plan()
    assert t.trie_generator(beam=5, return_n_best=1) is not g                        # a new plan drops the generators
    with pytest.raises(NotImplementedError, match="constraint_trie"):                # the pinned refusal stays
        t.generator


def test_generator_kwargs_is_what_build_generator_passes():
    from ofasys_amd import Dictionary, Task
    t = Task(name="t2t", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    t.initialize(Dictionary())
    kw = t.generator_kwargs(beam=3, lenpen=2, unkpen=0.25, use_graph=False)
    assert kw == dict(beam_size=3, return_n_best=1, max_len_a=0, max_len_b=200, max_len=256, min_len=1, normalize_scores=False,
                      len_penalty=2, unk_penalty=0.25, temperature=1.0, no_repeat_ngram_size=0, use_graph=False)
    g = t.build_generator(beam=3, lenpen=2, unkpen=0.25)
    assert (g.beam_size, g.len_penalty, g.unk_penalty) == (3, 2, 0.25)


# ------------------------------------------------------------------------------------------------ the golden
def test_golden_is_self_consistent():
    g = load_golden("trie_beam")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(CONFIGS))
    assert json.loads(str(g["closed_sets"])) == json.loads(json.dumps(CLOSED_SETS))
    assert CLOSED_SETS["main"] == ANSWERS
    trav = load_golden("traverse")["scores"]
    min_gap = np.inf
    for name, cfg in CONFIGS.items():
        answers = CLOSED_SETS[cfg["set"]]
        args = generator_args(cfg)
        K, n_best, max_len = args["beam"], args.get("return_n_best", 1), args["max_len"]
        toks, lens, scores, pos = g[f"{name}.tokens"], g[f"{name}.lens"], g[f"{name}.scores"], g[f"{name}.pos"]
        assert toks.shape == (2, n_best, WIDTH)
        # the answers that survive the length limit (EOS at step len <= max_len) and, with n = 2, repeat no bigram
        eligible = [a for a in distinct(answers) if len(a) <= max_len]
        if args.get("no_repeat_ngram_size", 0) == 2:
            eligible = [a for a in eligible if len({(x, y) for x, y in zip([BOS] + a, a)}) == len(a)]
        for b in range(2):
            n_hyp = int((lens[b] > 0).sum())
            assert (lens[b, :n_hyp] > 0).all()
            assert n_hyp == min(n_best, len(eligible)) if K >= len(eligible) else 1 <= n_hyp <= n_best, (name, b, n_hyp)
            seen = []
            for i in range(n_hyp):
                n = int(lens[b, i])
                seq = toks[b, i, :n - 1].tolist()
                assert toks[b, i, n - 1] == EOS and seq in eligible and seq not in seen, (name, b, i)   # a closed-set answer + EOS, once
                seen.append(seq)
                raw = pos[b, i, :n].astype(np.float64).sum()
                if not args.get("normalize_scores", False):
                    # unnormalised, no temperature, no unk in it: the exact route's score of the same answer
                    if args.get("temperature", 1.0) == 1.0 and cfg["set"] == "main":
                        assert abs(raw - float(trav[b, label_of(answers, seq)])) < 1e-4, (name, b, i)
                else:
                    raw /= n ** args.get("lenpen", 1)
                assert abs(raw - float(scores[b, i])) < 1e-4, (name, b, i)
            s = scores[b, :n_hyp].astype(np.float64)
            assert np.all(np.diff(s) < 0), (name, b)                                # best first
            if n_hyp > 1:
                min_gap = min(min_gap, float(-np.diff(s).max()))
            assert int(g[f"{name}.best"][b]) == label_of(answers, toks[b, 0, :int(lens[b, 0]) - 1].tolist())
    assert min_gap >= 1e-2, min_gap                                                 # exact token comparisons are meaningful
    # what the fixture pins: fewer hypotheses than the beam, a strict prefix returned next to its extension, max_len cutting the two
    # 4-token answers, beam 1 missing the exact arg-max, the reference running all max_len + 1 steps when the beam cannot fill
    assert (g["beam16.lens"] > 0).sum(1).tolist() == [13, 13] and (g["beam16_max_len3.lens"] > 0).sum(1).tolist() == [11, 11]
    full = [g["beam16.tokens"][0, i, :int(n) - 1].tolist() for i, n in enumerate(g["beam16.lens"][0]) if n > 0]
    assert [17, 23] in full and [17, 23, 99] in full and [17, 23, 99, 5] in full
    assert g["beam16.best"].tolist() == np.argmax(trav, 1).tolist() != g["beam1.best"].tolist()
    assert int(g["beam16.ref_steps"]) == 11 and int(g["beam5_long.ref_steps"]) <= 5
