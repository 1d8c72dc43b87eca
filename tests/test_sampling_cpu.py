"""CPU: sampling generation without a GPU -- the C ABI of csrc/sample.hip and its register allocation, the option surface
(Sampling, SequenceGenerator, Task.sampling_generator and the refusals that stay), the reference-recorded golden's coverage and
margins, and the torch restatement of a step (tests/sampling_case.py) against what the reference's Sampling.step saw and returned."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import sampling_case as sc
from tests.golden_util import load_golden
from tests.sampling_case import CONFIGS, EOS, RUNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_sampling_entry_points():
    from ofasys_amd import lib as L
    protos = L.parse_header()
    for name in ("ofa_sample_ws_bytes", "ofa_sample_draw", "ofa_sample_select"):
        assert name in protos
        getattr(ctypes.CDLL(L.LIB_PATH), name)
    h = L.lib()
    assert h.cdll.ofa_sample_ws_bytes(160, 59457, 5) == 160 * 8          # (lprob fp32, token int32) per row
    assert h.cdll.ofa_sample_ws_bytes(6, 204, 3) == 48
    assert h.cdll.ofa_sample_ws_bytes(0, 204, 5) == 0


def _draw(h, rows=10, V=204, K=5, temperature=1.0, step=0, ngram=0, tokens=None, tok_ld=0, topp=-1.0, logits=0x1000, ld=None):
    """ofa_sample_draw with made-up addresses: refused calls return before anything is launched or read."""
    from ofasys_amd import kernels as Kn
    pol = Kn._GenPolicy(temperature=temperature, cstart=-1, cend=-1, step=step, min_len=1, max_len=10, pad=1, unk=3, eos=2,
                        unk_penalty=0.0, ngram=ngram, tokens=tokens, tok_ld=tok_ld, done=None)
    return h.cdll.ofa_sample_draw(logits, V if ld is None else ld, rows, V, K, ctypes.byref(pol), -1, topp, 0x2000, 0x3000, 0, None)


def test_sampling_entry_points_validate_before_any_launch():
    from ofasys_amd import lib as L
    h = L.lib()
    INVALID, UNSUPPORTED = 1, 2
    assert (L.lib().cdll.ofa_last_error.restype, INVALID, UNSUPPORTED) == (ctypes.c_char_p, 1, 2)
    for kwargs, code, what in [
            (dict(rows=7), INVALID, b"not a multiple"), (dict(K=17, rows=17), UNSUPPORTED, b"beam size"),
            (dict(K=0), UNSUPPORTED, b"beam size"), (dict(temperature=0.0), INVALID, b"temperature"),
            (dict(temperature=-1.0), INVALID, b"temperature"), (dict(ngram=2, step=3), INVALID, b"n-gram"),
            (dict(ngram=2, step=3, tokens=0x4000, tok_ld=3), INVALID, b"n-gram"), (dict(logits=None), INVALID, b"null"),
            (dict(V=70000), UNSUPPORTED, b"vocabulary"), (dict(ld=100), INVALID, b"ld="), (dict(topp=1.5), INVALID, b"top-p")]:
        rc = _draw(h, **kwargs)
        assert rc == code and what in h.cdll.ofa_last_error(), (kwargs, rc, h.cdll.ofa_last_error())
    # the sentence pass: K outside [1, 16], a null buffer, histories too short for the step
    from ofasys_amd import kernels as Kn
    p = 0x1000

    def sel(K=3, step=2, cap=8, ws=p, **fields):
        st = Kn._GenState(p, cap, cap, p, cap, p, p, p, p, p, p, cap, p, p, p)
        for name, value in fields.items():
            setattr(st, name, value)
        return h.cdll.ofa_sample_select(ws, ctypes.byref(st), 2, K, step, 10, 2, 0, 1.0, None)

    assert sel(K=17) == UNSUPPORTED and b"beam size 17 outside" in h.cdll.ofa_last_error()
    assert sel(K=0) == UNSUPPORTED
    assert sel(ws=None) == INVALID and b"null pointer" in h.cdll.ofa_last_error()
    assert sel(fin_cnt=None) == INVALID and b"null pointer" in h.cdll.ofa_last_error()
    assert sel(step=8, cap=8) == INVALID and b"history buffers too short for step 8" in h.cdll.ofa_last_error()
    assert sel(step=11) == INVALID
    assert h.cdll.ofa_sample_select(p, None, 2, 3, 2, 10, 2, 0, 1.0, None) == INVALID and b"null pointer" in h.cdll.ofa_last_error()

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sampling_kernels_compile_without_spills(tmp_path):
    out = tmp_path / "sample.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "ofasys_amd", "csrc", "sample.hip"), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "wavefront_size")}
    drawk = [k for k in meta if "sample_draw_kernel" in k]
    sel = [k for k in meta if "sample_select_kernel" in k]
    assert len(drawk) == 3 and len(sel) == 1 and len(meta) == 4, sorted(meta)
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


def _task():
    from ofasys_amd import Dictionary, Task
    t = Task(name="t2t", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    t.initialize(Dictionary())
    return t


def test_sequence_generator_accepts_sampling_and_nothing_else():
    import ofasys_amd
    from ofasys_amd import Sampling
    from ofasys_amd.generator import SequenceGenerator
    assert "Sampling" in ofasys_amd.__all__
    d = _dict()
    s = Sampling(d, sampling_topk=5)
    assert (s.sampling_topk, s.sampling_topp) == (5, -1.0)
    assert (Sampling(d).sampling_topk, Sampling(d).sampling_topp) == (-1, -1.0)
    gen = SequenceGenerator(d, search_strategy=s, beam_size=3, seed=11)
    assert gen.sampling is s and gen.beam_size == 3 and gen.seed == 11 and gen.return_n_best == 3
    assert SequenceGenerator(d).sampling is None
    with pytest.raises(NotImplementedError):
        SequenceGenerator(d, search_strategy=object())
    with pytest.raises(NotImplementedError):
        SequenceGenerator(d, search_strategy=s, beam_size=SequenceGenerator.MAX_BEAM + 1)
    for refused in ({"lm_model": object()}, {"constraint_trie": object()}, {"match_source_len": True}):
        with pytest.raises(NotImplementedError):
            SequenceGenerator(d, search_strategy=s, **refused)
    with pytest.raises(ValueError):
        Sampling(d, sampling_topp=1.5)


def test_sampling_refuses_a_prefix_with_columns_constraints_and_stray_uniforms():
    from ofasys_amd import Sampling
    from ofasys_amd.generator import SequenceGenerator
    d = _dict()
    gen = SequenceGenerator(d, search_strategy=Sampling(d, sampling_topp=0.9), beam_size=2)
    with pytest.raises(NotImplementedError, match="prefix_tokens under sampling"):
        gen.generate(None, {"net_input": {"slots": []}, "prefix_tokens": torch.full((1, 2), 7, dtype=torch.long)})
    with pytest.raises(NotImplementedError):
        gen.generate(None, {"net_input": {"slots": []}}, constraints=torch.zeros(1, 1))
    assert gen.check_sample({"prefix_tokens": torch.zeros(2, 0, dtype=torch.long)}) is True          # the collator's empty prefix
    with pytest.raises(ValueError, match="uniforms"):
        SequenceGenerator(d, beam_size=2).generate(None, {"net_input": {"slots": []}}, uniforms=torch.zeros(3, 2))


def test_trie_generator_still_refuses_sampling():
    from ofasys_amd import Sampling
    from ofasys_amd.generator import TrieBeamGenerator
    d = _dict()
    with pytest.raises(NotImplementedError):
        TrieBeamGenerator(d, None, search_strategy=Sampling(d))


def test_task_sampling_generator_maps_checks_and_caches():
    t = _task()
    g = t.sampling_generator(sampling=True, sampling_topp=0.9, beam=5, max_len=12, seed=3, lenpen=0.5, unkpen=0.25, temperature=0.7,
                             no_repeat_ngram_size=2, min_len=2, return_n_best=5, normalize_scores=True)
    assert (g.sampling.sampling_topk, g.sampling.sampling_topp, g.seed) == (-1, 0.9, 3)
    assert (g.beam_size, g.return_n_best, g.max_len, g.min_len, g.len_penalty, g.unk_penalty) == (5, 5, 12, 2, 0.5, 0.25)
    assert (g.temperature, g.no_repeat_ngram_size, g.normalize_scores) == (0.7, 2, True)
    # one generator per option set
    same = dict(sampling=True, sampling_topp=0.9, beam=5, max_len=12, seed=3, lenpen=0.5, unkpen=0.25, temperature=0.7,
                no_repeat_ngram_size=2, min_len=2, return_n_best=5, normalize_scores=True)
    assert t.sampling_generator(**same) is g
    assert t.sampling_generator(**dict(same, seed=4)) is not g
    assert t.sampling_generator(**dict(same, sampling_topp=-1.0, sampling_topk=7)) is not g
    d = t.sampling_generator()                                   # `sampling` defaults to True here; the reference's other defaults
    assert (d.sampling.sampling_topk, d.sampling.sampling_topp, d.beam_size, d.return_n_best, d.normalize_scores) == (-1, -1.0, 5, 1, False)
    # the reference's argument checks (task/base.py:498-512)
    with pytest.raises(AssertionError, match="requires --sampling"):
        t.sampling_generator(sampling=False, sampling_topk=5)
    with pytest.raises(AssertionError, match="requires --sampling"):
        t.sampling_generator(sampling=False, sampling_topp=0.5)
    with pytest.raises(ValueError, match="mutually exclusive"):
        t.sampling_generator(sampling=True, diverse_beam_groups=2)
    with pytest.raises(ValueError, match="mutually exclusive"):
        t.sampling_generator(sampling=True, match_source_len=True)
    with pytest.raises(NotImplementedError):
        t.sampling_generator(sampling=True, constrained=True)
    # the door next to it stays shut, and says where to go
    with pytest.raises(NotImplementedError, match="sampling_generator"):
        t.build_generator(sampling=True)
    with pytest.raises(NotImplementedError, match="sampling_generator"):
        t.build_generator(sampling_topk=5)
    t.generator = g
    assert t.generator is g


# ------------------------------------------------------------------------------------------------ the golden
def _runs():
    g = load_golden("sampling")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(CONFIGS))
    return g, [(name, cfg, f"{name}.{i}") for name, cfg in CONFIGS.items() for i in range(RUNS)]


def _step_cfg(cfg):
    g = cfg["gen"]
    return dict(max_len=g["max_len"], normalize=g.get("normalize_scores", True), len_penalty=g.get("len_penalty", 1.0))


def test_sampling_golden_is_self_consistent_and_covers_its_cases():
    g, runs = _runs()
    assert g["margins"].tolist() == [sc.DRAW_MARGIN, sc.TOPP_MARGIN] and float(g["worst_draw_margin"]) >= sc.DRAW_MARGIN
    steps, finish_order, reordered = set(), False, False
    for name, cfg, key in runs:
        gen = cfg["gen"]
        K = gen["beam_size"]
        toks, lens, scores, pos = g[f"{key}.tokens"], g[f"{key}.lens"], g[f"{key}.scores"], g[f"{key}.pos"]
        assert g[f"{key}.uniforms"].shape == (gen["max_len"] + 1, toks.shape[0] * K)
        assert g[f"{key}.uniforms"].dtype == np.float32 and (g[f"{key}.uniforms"] >= 0).all() and (g[f"{key}.uniforms"] < 1).all()
        last = []
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
                assert abs(raw - float(scores[b, i])) < 1e-4, (key, b, i)
            s = scores[b][lens[b] > 0]
            assert np.all(np.diff(s) <= 0), (key, b)
            last.append(int(lens[b].max()))
        # a sentence's last hypothesis ends when the sentence does (K of K returned) -- or it ran to max_len
        if gen.get("return_n_best", -1) in (-1, K) and len(set(last)) > 1:
            finish_order = True
        # a slot ends while a LATER slot of its sentence goes on: the survivors are compacted, the reorder is no identity
        tok = g[f"{key}.step_tok"]
        for t in range(tok.shape[0] - 1):
            for b in range(toks.shape[0]):
                now = tok[t, b * K:(b + 1) * K]
                if tok[t + 1, b * K] >= 0 and (now == EOS).any():
                    first = int(np.argmax(now == EOS))
                    reordered |= bool((now[first + 1:] != EOS).any())
    assert len(steps) >= 3 and finish_order and reordered, (sorted(steps), finish_order, reordered)


def test_restated_step_reproduces_the_reference_recorded_steps():
    """Kept set, draw and sentence pass of tests/sampling_case.py on the lprobs the reference's Sampling.step was given: kept-set
    sizes, kept token ids and drawn tokens exact, values to the step tolerance; the sentence pass, run over the recorded draws,
    ends in the reference's hypotheses."""
    g, runs = _runs()
    for name, cfg, key in runs:
        gen = cfg["gen"]
        K, T = gen["beam_size"], int(g[f"{key}.steps"])
        U, lps = torch.from_numpy(g[f"{key}.uniforms"]), torch.from_numpy(g[f"{key}.step_lprobs"])
        rows = U.shape[1]
        bsz = rows // K
        st = sc.empty_state(bsz, K, gen["max_len"] + 2)
        for t in range(T):
            live = torch.from_numpy(g[f"{key}.step_tok"][t] >= 0)
            done = ~live.view(bsz, K)[:, 0]
            assert torch.equal(done, st["done"].bool()), (key, t)          # the reference dropped exactly the finished sentences
            lp = torch.where(torch.isnan(lps[t]), torch.full_like(lps[t], -math.inf), lps[t])
            tok, lpd, worst, facts = sc.draw_rows(lp, K, t, cfg["topk"], cfg["topp"], U[t], done)
            assert worst >= sc.DRAW_MARGIN, (key, t, worst)
            for r in range(rows):
                if not live[r]:
                    continue
                f = facts[r]
                assert f["kept"] == int(g[f"{key}.step_kept_n"][t, r]), (key, t, r)
                ids = g[f"{key}.step_kept_ids"][t, r]
                kept, _ = sc.kept_set(lp[(r // K) * K if t == 0 else r], cfg["topk"], cfg["topp"])
                if f["kept"] <= ids.shape[0]:
                    assert kept.nonzero().flatten().tolist() == ids[ids >= 0].tolist(), (key, t, r)
                if cfg["topp"] > 0:
                    assert sc.topp_margin_ok(f, cfg["topp"]), (key, t, r, f)
                else:
                    assert sc.topk_margin_ok({k: f[k] for k in ("last", "next") if k in f}), (key, t, r)
            assert torch.equal(tok[live], torch.from_numpy(g[f"{key}.step_tok"][t])[live]), (key, t)
            want_lp = torch.from_numpy(g[f"{key}.step_lp"][t])
            assert torch.allclose(lpd[live], want_lp[live], rtol=1e-5, atol=2e-5), (key, t)
            new = sc.select_step(st, tok, lpd, K, t, _step_cfg(cfg))
            # cumulative scores and parents the reference's step returned, in its (pre-compaction) slot order
            cum = lpd + st["scores"][:, t - 1] if t > 0 else lpd
            assert torch.allclose(cum[live], torch.from_numpy(g[f"{key}.step_score"][t])[live], rtol=1e-5, atol=2e-5), (key, t)
            parent = torch.from_numpy(g[f"{key}.step_beam"][t])
            assert torch.equal(parent[live], (torch.arange(rows) % K)[live] if t > 0 else torch.zeros(rows, dtype=torch.long)[live])
            st = new
        assert bool(st["done"].all()), key
        n_best = gen.get("return_n_best", -1) if gen.get("return_n_best", -1) != -1 else K
        hyps = sc.hypotheses(st, n_best)
        toks, lens, scores, pos = g[f"{key}.tokens"], g[f"{key}.lens"], g[f"{key}.scores"], g[f"{key}.pos"]
        for b, hs in enumerate(hyps):
            assert len(hs) == int((lens[b] > 0).sum()), (key, b)
            for i, (tk, score, ps) in enumerate(hs):
                n = int(lens[b, i])
                assert tk.tolist() == toks[b, i, :n].tolist(), (key, b, i)
                assert abs(score - float(scores[b, i])) <= 2e-5 + 1e-5 * abs(float(scores[b, i])), (key, b, i)
                assert np.allclose(ps.numpy(), pos[b, i, :n], rtol=1e-5, atol=2e-5), (key, b, i)
