"""CPU: diverse decoding without a GPU -- the C ABI of csrc/diverse_beam.hip and its register allocation, the option surface
(DiverseBeamSearch, DiverseSiblingsSearch, SequenceGenerator, Task.diverse_generator, the SCST route and the refusals that stay),
the torch restatement of the two steps (tests/diverse_oracle.py) against what the reference's steps returned, and the
reference-recorded generate() golden's consistency."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import diverse_case as dc
from tests import diverse_oracle as do
from tests.golden_util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EOS = do.EOS


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_diverse_entry_points():
    from ofasys_amd import lib as L
    protos = L.parse_header()
    for name in ("ofa_diverse_group_select", "ofa_diverse_sibling_select"):
        assert name in protos
        getattr(ctypes.CDLL(L.LIB_PATH), name)


def test_diverse_entry_points_validate_before_any_launch():
    """Made-up addresses: refused calls return before anything is launched or read."""
    from ofasys_amd import kernels as Kn
    from ofasys_amd import lib as L
    h = L.lib()
    INVALID, UNSUPPORTED = 1, 2
    p = 0x1000

    def state(cap=8, **fields):
        st = Kn._GenState(p, cap, cap, p, cap, p, p, p, p, p, p, cap, p, p, p)
        for name, value in fields.items():
            setattr(st, name, value)
        return ctypes.byref(st)

    def groups(K=4, G=2, strength=0.5, V=204, step=2, ws=p, **fields):
        return h.cdll.ofa_diverse_group_select(ws, state(**fields), 2, K, V, step, 10, 2, 3, ctypes.c_float(0.0), 0, ctypes.c_float(1.0),
                                               G, ctypes.c_float(strength), None)

    def siblings(K=4, rate=0.5, V=204, step=2, ws=p, **fields):
        return h.cdll.ofa_diverse_sibling_select(ws, state(**fields), 2, K, V, step, 10, 2, 3, ctypes.c_float(0.0), 0,
                                                 ctypes.c_float(1.0), ctypes.c_float(rate), None)

    for call, code, what in [
            (lambda: groups(K=5, G=2), INVALID, b"not divisible"), (lambda: groups(K=4, G=8), INVALID, b"not divisible"),
            (lambda: groups(G=0), INVALID, b"0 groups"), (lambda: groups(strength=-0.5), INVALID, b"strength"),
            (lambda: groups(strength=float("inf")), INVALID, b"strength"), (lambda: groups(strength=float("nan")), INVALID, b"strength"),
            (lambda: groups(K=17, G=1), UNSUPPORTED, b"beam size 17 outside"), (lambda: siblings(K=17), UNSUPPORTED, b"beam size 17 outside"),
            (lambda: siblings(K=4, V=8), INVALID, b"must exceed 2 * beam"), (lambda: siblings(rate=float("nan")), INVALID, b"rate"),
            (lambda: groups(ws=None), INVALID, b"null pointer"), (lambda: siblings(fin_cnt=None), INVALID, b"null pointer"),
            (lambda: groups(step=8), INVALID, b"history buffers too short for step 8"), (lambda: siblings(step=11), INVALID, b"step=11"),
            (lambda: groups(K=16, G=2, V=70000), UNSUPPORTED, b"candidates a row")]:
        rc = call()
        assert rc == code and what in h.cdll.ofa_last_error(), (rc, h.cdll.ofa_last_error())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_diverse_kernels_compile_without_spills(tmp_path):
    out = tmp_path / "diverse_beam.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "ofasys_amd", "csrc", "diverse_beam.hip"), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "wavefront_size")}
    assert len(meta) == 2 and all("diverse_select_kernel" in k for k in meta), sorted(meta)      # groups, siblings
    for k, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (k, m)
        assert m["wavefront_size"] == 64, (k, m)


# ------------------------------------------------------------------------------------------------ options
def _dict(n=40):
    from ofasys_amd import Dictionary
    d = Dictionary()
    for i in range(n):
        d.add_symbol(f"<text>_{i}")
    return d


def _task(scst_args=None):
    from ofasys_amd import Dictionary, Task, TaskConfig
    cfg = TaskConfig()
    if scst_args is not None:
        cfg.scst, cfg.scst_args = True, scst_args
    t = Task(cfg, name="t2t", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    t.initialize(Dictionary())
    return t


def test_sequence_generator_accepts_the_two_holders_and_still_refuses_others():
    import ofasys_amd
    from ofasys_amd import DiverseBeamSearch, DiverseSiblingsSearch
    from ofasys_amd.generator import SequenceGenerator
    assert {"DiverseBeamSearch", "DiverseSiblingsSearch"} <= set(ofasys_amd.__all__)
    d = _dict()
    g = DiverseBeamSearch(d, 2, 0.5)
    assert (g.num_groups, g.diversity_strength) == (2, 0.5)
    gen = SequenceGenerator(d, search_strategy=g, beam_size=4)
    assert gen.diverse is g and gen.sampling is None and gen.beam_size == 4
    s = DiverseSiblingsSearch(d, 0.25)
    gen = SequenceGenerator(d, search_strategy=s, beam_size=3)
    assert gen.diverse is s and gen.sampling is None and s.diversity_rate == 0.25
    assert SequenceGenerator(d).diverse is None
    with pytest.raises(NotImplementedError):
        SequenceGenerator(d, search_strategy=object())
    for refused in ({"lm_model": object()}, {"constraint_trie": object()}, {"match_source_len": True}):
        with pytest.raises(NotImplementedError):
            SequenceGenerator(d, search_strategy=g, beam_size=4, **refused)


def test_diverse_refusals():
    from ofasys_amd import DiverseBeamSearch, DiverseSiblingsSearch
    from ofasys_amd.generator import SequenceGenerator, TrieBeamGenerator
    d = _dict()
    with pytest.raises(ValueError, match="DiverseBeamSearch requires --beam to be divisible by the number of groups"):
        SequenceGenerator(d, search_strategy=DiverseBeamSearch(d, 2, 0.5), beam_size=5)
    with pytest.raises(ValueError, match="strength"):
        DiverseBeamSearch(d, 2, -0.5)
    with pytest.raises(ValueError):
        DiverseBeamSearch(d, 0, 0.5)
    with pytest.raises(ValueError):
        DiverseSiblingsSearch(d, float("nan"))
    with pytest.raises(ValueError, match="top 2"):
        SequenceGenerator(_dict(2), search_strategy=DiverseSiblingsSearch(d, 0.5), beam_size=3)
    prefix = {"net_input": {"slots": []}, "prefix_tokens": torch.full((1, 2), 7, dtype=torch.long)}
    for strategy in (DiverseBeamSearch(d, 2, 0.5), DiverseSiblingsSearch(d, 0.5)):
        gen = SequenceGenerator(d, search_strategy=strategy, beam_size=4)
        with pytest.raises(NotImplementedError, match="prefix_tokens under a diverse search strategy"):
            gen.generate(None, prefix)
        assert gen.check_sample({"prefix_tokens": torch.zeros(2, 0, dtype=torch.long)}) is True      # the collator's empty prefix
        with pytest.raises(NotImplementedError, match="uniforms together with a diverse search strategy"):
            gen.generate(None, {"net_input": {"slots": []}}, uniforms=torch.zeros(3, 4))
        with pytest.raises(NotImplementedError, match="diverse search strategy over the answer trie"):
            TrieBeamGenerator(d, None, search_strategy=strategy)


def test_task_diverse_generator_defaults_selection_and_caching():
    from ofasys_amd import DiverseBeamSearch, DiverseSiblingsSearch
    t = _task()
    g = t.diverse_generator(diverse_beam_groups=2, beam=4)
    assert isinstance(g.diverse, DiverseBeamSearch) and (g.diverse.num_groups, g.diverse.diversity_strength) == (2, 0.5)
    assert (g.beam_size, g.return_n_best, g.normalize_scores, g.max_len) == (4, 1, False, 256)       # the reference's other defaults
    # groups win over a rate that selects siblings but is not "set" (<= 0); both set is the reference's ValueError
    both = t.diverse_generator(diverse_beam_groups=2, diversity_rate=0.0, beam=4)
    assert isinstance(both.diverse, DiverseBeamSearch)
    s = t.diverse_generator(diversity_rate=0.0, beam=3, max_len=9, lenpen=0.5, unkpen=0.25, temperature=0.7, no_repeat_ngram_size=2)
    assert isinstance(s.diverse, DiverseSiblingsSearch) and s.diverse.diversity_rate == 0.0            # rate > -1 selects it
    assert (s.beam_size, s.max_len, s.len_penalty, s.unk_penalty, s.temperature, s.no_repeat_ngram_size) == (3, 9, 0.5, 0.25, 0.7, 2)
    assert isinstance(t.diverse_generator(diverse_beam_groups=0, diversity_rate=0.5).diverse, DiverseSiblingsSearch)
    # one generator per option set
    same = dict(diverse_beam_groups=2, diverse_beam_strength=1.5, beam=4, max_len=12)
    a = t.diverse_generator(**same)
    assert t.diverse_generator(**same) is a
    assert t.diverse_generator(**dict(same, diverse_beam_strength=2.0)) is not a
    assert t.diverse_generator(**dict(same, max_len=11)) is not a
    # the reference's errors, and this method's own
    with pytest.raises(ValueError, match="mutually exclusive"):
        t.diverse_generator(diverse_beam_groups=2, diversity_rate=0.5, beam=4)
    with pytest.raises(ValueError, match="mutually exclusive"):
        t.diverse_generator(diverse_beam_groups=2, sampling=True, beam=4)
    with pytest.raises(ValueError, match="mutually exclusive"):
        t.diverse_generator(diversity_rate=0.5, match_source_len=True)
    with pytest.raises(ValueError, match="DiverseBeamSearch requires --beam to be divisible by the number of groups"):
        t.diverse_generator(diverse_beam_groups=2, beam=5)
    with pytest.raises(ValueError, match="neither"):
        t.diverse_generator(beam=4)
    with pytest.raises(NotImplementedError):
        t.diverse_generator(diverse_beam_groups=2, beam=4, constrained=True)
    t.generator = g
    assert t.generator is g


def test_build_generator_still_refuses_the_diverse_keys_and_says_where_to_go():
    t = _task()
    with pytest.raises(NotImplementedError, match=r"Task\.diverse_generator\(\.\.\.\)"):
        t.build_generator(diverse_beam_groups=2)
    with pytest.raises(NotImplementedError, match=r"Task\.diverse_generator\(\.\.\.\)"):
        t.build_generator(diversity_rate=0.5)


def test_scst_generator_routes_diverse_args():
    from ofasys_amd import DiverseBeamSearch, DiverseSiblingsSearch
    g = _task('{"beam": 4, "diverse_beam_groups": 2}').scst_generator
    assert isinstance(g.diverse, DiverseBeamSearch) and (g.diverse.num_groups, g.beam_size, g.return_n_best) == (2, 4, 4)
    s = _task('{"beam": 3, "diversity_rate": 0.5, "max_len": 6}').scst_generator
    assert isinstance(s.diverse, DiverseSiblingsSearch) and (s.beam_size, s.return_n_best, s.max_len) == (3, 3, 6)
    assert _task('{"beam": 3}').scst_generator.diverse is None


# ------------------------------------------------------------------------------------------------ (a) the restated steps
def test_restated_steps_reproduce_the_reference_recorded_steps():
    """tests/diverse_oracle.py on the inputs the reference's steps were given: tokens and beams equal, scores bit for bit -- and no
    selection so close that the tie rule (the reference's is torch.topk's) could have decided it."""
    g = load_golden("diverse_search_steps")
    cases = [("groups", K, G, s) for K, G, s in dc.STEP_GROUPS] + [("siblings", K, None, r) for K, r in dc.STEP_SIBLINGS]
    gaps, n = [], 0
    for kind, K, G, amount in cases:
        for step in dc.STEP_STEPS:
            key = dc.step_key(kind, K, G, amount, step)
            lprobs, scores = torch.from_numpy(g[f"{key}.lprobs"]), torch.from_numpy(g[f"{key}.scores"])
            assert lprobs.shape == (dc.STEP_BSZ, K, dc.STEP_V)
            if kind == "groups":
                sc, idx, beams = do.group_step(step, lprobs, scores, G, amount, gaps)
                assert sc.shape == (dc.STEP_BSZ, 2 * K if step > 0 else min(2 * (K // G), dc.STEP_V - 1) * G)
            else:
                sc, idx, beams = do.sibling_step(step, lprobs, scores, amount, gaps)
            assert torch.equal(idx, torch.from_numpy(g[f"{key}.out_indices"])), key
            assert torch.equal(beams, torch.from_numpy(g[f"{key}.out_beams"])), key
            assert torch.equal(sc, torch.from_numpy(g[f"{key}.out_scores"])), key
            n += 1
    assert n == 28 and min(gaps) >= dc.MIN_GAP and abs(min(gaps) - float(g["min_gap"])) < 1e-9, min(gaps)


def test_group_step_at_step_zero_reads_the_groups_own_row():
    """The inner BeamSearch.step keeps the group's first row: group g reads row g and reports beam g (rows are equal in generate)."""
    lprobs, scores = dc.step_inputs(4, 0, 7)
    _, idx, beams = do.group_step(0, lprobs, scores, 2, 0.5)
    assert beams.view(dc.STEP_BSZ, -1, 2)[:, :, 0].eq(0).all() and beams.view(dc.STEP_BSZ, -1, 2)[:, :, 1].eq(1).all()
    assert idx[0, 0] == lprobs[0, 0].argmax()


# ------------------------------------------------------------------------------------------------ (b) the generate() golden
def test_diverse_golden_is_self_consistent():
    g = load_golden("diverse_beam")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(dc.CONFIGS))
    gaps = json.loads(str(g["gaps"]))
    assert set(gaps) == set(dc.CONFIGS) and min(gaps.values()) >= dc.MIN_GAP
    steps, distinct = set(), 0
    for name, cfg in dc.CONFIGS.items():
        gen = cfg["gen"]
        toks, lens, scores, pos = g[f"{name}.tokens"], g[f"{name}.lens"], g[f"{name}.scores"], g[f"{name}.pos"]
        assert toks.shape[:2] == (2, gen["return_n_best"])
        for b in range(toks.shape[0]):
            for i in range(toks.shape[1]):
                n = int(lens[b, i])
                if n == 0:
                    continue
                steps.add(n - 1)
                assert toks[b, i, n - 1] == EOS and n <= gen["max_len"] + 1
                raw = pos[b, i, :n].astype(np.float64).sum()
                if gen.get("normalize_scores", True):
                    raw /= n ** gen.get("len_penalty", 1.0)
                assert abs(raw - float(scores[b, i])) < 1e-4, (name, b, i)
            s = scores[b][lens[b] > 0]
            assert np.all(np.diff(s) <= 0), (name, b)           # sorted best first
            distinct = max(distinct, len({tuple(toks[b, i, :int(lens[b, i])]) for i in range(toks.shape[1]) if lens[b, i] > 0}))
    assert len(steps) >= 3 and distinct >= 3
