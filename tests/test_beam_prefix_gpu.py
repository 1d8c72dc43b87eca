"""GPU: beam search under a forced target prefix (csrc/beam_search.hip: ofa_beam_prefix_topk / _fill / _select,
ofasys_amd.generator.SequenceGenerator with sample["prefix_tokens"], Task.inference).

1. One step of the kernels against the torch restatement of tests/beam_prefix_case.py (the reference's prefix step taken
   literally, ties by the project's rule): prefix steps, the first free step after them, and the single cases.
2. generate() on the fp32 `tiny_text` model against tests/golden/beam_prefix.npz (the reference's own generate on the CPU).
3. Generator behaviour: graphs == eager, one generator across prefix widths, width 0 == no prefix, Task.inference, refusals.
"""
import json

import numpy as np
import pytest
import torch

from oracle import recipe
from oracle.cases import CASES
from tests.beam_prefix_case import BOS, CONFIGS, EOS, PAD, UNK, ref_prefix_step
from tests.golden_util import load_golden
from tests.model_util import build_model
from tests.test_beam_search_gpu import _flat, _model, _sample, compare, make_state

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ one step of the kernels
def run_kernels(logits, st, K, step, cfg, prefix, plen):
    """The launches generator.SequenceGenerator._prefix_step_kernels records, on copies of the state."""
    from ofasys_amd import kernels as Kn
    rows, V = logits.shape
    d = {k: v.to(DEV) for k, v in st.items()}
    ws = torch.empty((Kn.beam_ws_bytes(rows, V, K) + 3) // 4, device=DEV)
    forced = step < prefix.shape[1] and step < cfg["max_len"]
    pre, pl = prefix.to(DEV), plen.to(torch.int32).to(DEV)
    glogit = torch.full((rows,), float("nan"), device=DEV)
    policy = dict(tokens=d["tokens"], done=d["done"], pad=PAD, unk=UNK, unk_penalty=cfg["unk_penalty"], ngram=cfg["ngram"])
    Kn.beam_prefix_topk(logits, K, step, ws, pl, prefix=pre if forced else None, glogit=glogit, temperature=cfg["temperature"],
                        constraint_range=cfg.get("constraint_range"), min_len=cfg["min_len"], max_len=cfg["max_len"], eos=EOS,
                        **policy)
    sel = dict(eos=EOS, unk=UNK, unk_penalty=cfg["unk_penalty"], normalize=cfg["normalize"], len_penalty=cfg["len_penalty"])
    if forced:
        Kn.beam_prefix_fill(ws, rows, V, K, step, pre, pl, glogit, **policy)
        Kn.beam_prefix_select(ws, d, K, V, step, cfg["max_len"], pre, pad=PAD, **sel)
    else:
        Kn.beam_select(ws, d, K, V, step, cfg["max_len"], **sel)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def base_cfg(**over):
    return dict(dict(temperature=0.8, min_len=2, max_len=6, unk_penalty=0.3, ngram=3, normalize=True, len_penalty=1.2,
                     constraint_range=None), **over)


def make_case(K, V, step, ftok, dtype, seed, width=3, ngram_rows=()):
    """bsz 3: sentence 0 forced onto `ftok`, sentence 1 free (<pad> in this column: its prefix ended), sentence 2 done -- with
    by far the smallest lprob at its own prefix token, so a minimum that forgets the done flags shows."""
    bsz, cap = 3, 8
    g = torch.Generator().manual_seed(seed)
    rows = bsz * K
    buf = torch.randn(rows, V + 24, generator=g) * 3               # padded row stride
    other = 9 if ftok != 9 else 10
    buf[2 * K:, other] = -60.0
    buf[K:2 * K, EOS] += 6.0                                         # sentence 1: more EOS candidates than open slots
    st = make_state(bsz, K, step, cap, V, g, ngram_rows)
    st["done"][2] = 1
    prefix = torch.full((bsz, width), PAD, dtype=torch.long)
    prefix[0] = torch.randint(4, V, (width,), generator=g)
    prefix[2] = torch.randint(4, V, (width,), generator=g)
    if step < width:
        prefix[0, step], prefix[2, step] = ftok, other
    prefix[1, :min(step, 1)] = 77                                    # a prefix of one token (none at step 0)
    plen = (prefix != PAD).sum(1)
    dev_logits = buf.to(DEV).to(dtype)[:, :V]
    return dev_logits, st, prefix, plen


PLACES = [(204, 57), (59457, 4), (59457, 4095), (59457, 4096), (59457, 59456)]     # first after the specials, chunk seam, last
STEPS = {"first": 0, "inside": 1, "last_prefix": 2, "first_free": 3}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("V,ftok", PLACES)
@pytest.mark.parametrize("when", list(STEPS))
def test_prefix_kernels_match_reference_step(dtype, K, V, ftok, when):
    step = STEPS[when]
    cfg = base_cfg(constraint_range=(4, V - 7) if K == 2 and ftok < V - 7 else None)
    if when == "first_free":
        # n = 2, the prefix lengths on both sides of step + n - 1 = 4: rows 0 (plen 3) are banned their best token, rows of
        # sentence 1 (plen 5, a prefix that max_len cut) keep it
        cfg["ngram"] = 2
        hist = [(r, [50, ftok if ftok != 50 else 51, 11, 50]) for r in range(2 * K)]
        logits, st, prefix, plen = make_case(K, V, step, ftok, dtype, 7 * K + V % 997 + step, ngram_rows=hist)
        plen[1] = 5
        st["ignore"][1].zero_()
        logits[:2 * K, hist[0][1][1]] += 30.0                        # (well above the EOS boost of sentence 1)
    else:
        logits, st, prefix, plen = make_case(K, V, step, ftok, dtype, 7 * K + V % 997 + step)
    want = ref_prefix_step(logits.cpu(), st, K, step, cfg, prefix, plen)
    got = run_kernels(logits, st, K, step, cfg, prefix, plen)
    compare(got, want)
    if step < 3:                                                     # the forced sentence follows its prefix in its first beam
        assert int(st["ignore"][0, 0]) or int(want["tokens"][0, step + 1]) == ftok
    else:
        banned = hist[0][1][1]
        assert banned not in want["tokens"][:K, step + 1].tolist() and banned in want["tokens"][K:2 * K, step + 1].tolist()


def test_ngram_one_at_step_equal_to_prefix_length():
    """n = 1 bans every token of the history -- except for rows whose prefix has just ended (plen = step: not < step + 0)."""
    K, V, step = 2, 204, 3
    cfg = base_cfg(ngram=1)
    logits, st, prefix, plen = make_case(K, V, step, 57, torch.float32, 11)
    plen[0], plen[1] = 3, 1
    st["ignore"].zero_()
    for r in range(2 * K):
        logits[r, int(st["tokens"][r, 2])] += 12.0                   # every row's best token is in its history
    want = ref_prefix_step(logits.cpu(), st, K, step, cfg, prefix, plen)
    compare(run_kernels(logits, st, K, step, cfg, prefix, plen), want)
    assert int(want["tokens"][0, step + 1]) == int(want["tokens"][0, 2])        # plen 3 = step: not banned
    assert int(want["tokens"][K, step + 1]) not in want["tokens"][K, :step + 1].tolist()


@pytest.mark.parametrize("K", [1, 5])
def test_forced_token_is_unk(K):
    cfg = base_cfg(unk_penalty=0.5)
    logits, st, prefix, plen = make_case(K, 204, 1, UNK, torch.float32, 21 + K)
    want = ref_prefix_step(logits.cpu(), st, K, 1, cfg, prefix, plen)
    compare(run_kernels(logits, st, K, 1, cfg, prefix, plen), want)
    assert int(st["ignore"][0, 0]) or int(want["tokens"][0, 2]) == UNK


@pytest.mark.parametrize("K", [1, 5])
def test_forced_token_banned_by_ngrams(K):
    """n = 3 at step 4 of a width-5 prefix (plen 5 < 4 + 3 - 1): the history ... a b a b bans a, the forced token."""
    a, b, step = 40, 41, 4
    cfg = base_cfg(ngram=3, max_len=7)
    hist = [(r, [a, b, a, b]) for r in range(K)]
    logits, st, prefix, plen = make_case(K, 204, step, a, torch.float32, 31 + K, width=5, ngram_rows=hist)
    assert int(plen[0]) == 5
    want = ref_prefix_step(logits.cpu(), st, K, step, cfg, prefix, plen)
    compare(run_kernels(logits, st, K, step, cfg, prefix, plen), want)
    assert a not in want["tokens"][:K, step + 1].tolist()


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("V", [204, 59457])
def test_forced_token_outside_constraint_range(K, V):
    """g = -inf for the forced rows, so f = -inf: every value of the step's forced rows ends as -inf."""
    cfg = base_cfg(constraint_range=(4, 100))
    logits, st, prefix, plen = make_case(K, V, 1, 150, torch.float32, 41 + K)
    want = ref_prefix_step(logits.cpu(), st, K, 1, cfg, prefix, plen)
    compare(run_kernels(logits, st, K, 1, cfg, prefix, plen), want)
    assert torch.isinf(want["scores"][:K, 1]).all()


def test_min_len_is_off_during_prefix_steps():
    """min_len = 4, EOS the best token of the free sentence at step 1 < width: it finalises."""
    K = 2
    cfg = base_cfg(min_len=4)
    logits, st, prefix, plen = make_case(K, 204, 1, 57, torch.float32, 51)
    logits[K:2 * K, EOS] += 20.0
    st["ignore"].zero_()
    st["fin_cnt"].zero_()
    want = ref_prefix_step(logits.cpu(), st, K, 1, cfg, prefix, plen)
    compare(run_kernels(logits, st, K, 1, cfg, prefix, plen), want)
    assert int(want["fin_cnt"][1]) > 0 and int(want["fin_len"][1, 0]) == 2


# ------------------------------------------------------------------------------------------------ generate() against the reference
def _prefixed(V, prefix, src=None):
    s = _sample(V, src)
    s["prefix_tokens"] = torch.as_tensor(prefix, dtype=torch.long).to(DEV)
    return s


def test_generate_matches_reference_golden():
    from ofasys_amd.generator import SequenceGenerator
    g = load_golden("beam_prefix")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(CONFIGS))
    model, d = _model(torch.float32)
    for name, c in CONFIGS.items():
        assert bool(g[f"{name}.hyps_follow_prefix"]) and bool(g[f"{name}.active_follow_prefix"]) and bool(g[f"{name}.tie_order_free"])
        gen = SequenceGenerator(d, **c["gen"])
        res = _flat(gen.generate(model, _prefixed(len(d), c["prefix"])))
        toks, lens, scores, pos = g[f"{name}.tokens"], g[f"{name}.lens"], g[f"{name}.scores"], g[f"{name}.pos"]
        for b, hyps in enumerate(res):                               # ALL returned hypotheses
            assert len(hyps) == int((lens[b] > 0).sum()), (name, b)
            for i, h in enumerate(hyps):
                n = int(lens[b, i])
                assert h.tokens.tolist() == toks[b, i, :n].tolist(), (name, b, i)
                assert abs(float(h.score) - float(scores[b, i])) < 1e-4, (name, b, i)
                assert np.abs(h.positional_scores.numpy() - pos[b, i, :n]).max() < 1e-4, (name, b, i)


# ------------------------------------------------------------------------------------------------ generator behaviour
def _same(a, b):
    assert len(a) == len(b)
    for ha, hb in zip(a, b):
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            assert torch.equal(x.tokens, y.tokens) and torch.equal(x.score, y.score)
            assert torch.equal(x.positional_scores, y.positional_scores)


GEN = dict(beam_size=4, max_len=8, no_repeat_ngram_size=2, return_n_best=4, normalize_scores=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_graph_replay_equals_eager(dtype):
    from ofasys_amd.generator import SequenceGenerator
    model, d = _model(dtype)
    V = len(d)
    eager, graph = SequenceGenerator(d, use_graph=False, **GEN), SequenceGenerator(d, use_graph=True, **GEN)
    for seed in range(3):                                            # graph generator: eager warm-up, capture, replay
        src = recipe.tokens(f"input.beam_src{seed}", (2, 16), V, [16, 11 + seed])
        prefix = [[17 + seed, 60, 9], [33, PAD, PAD]]
        _same(_flat(eager.generate(model, _prefixed(V, prefix, src))), _flat(graph.generate(model, _prefixed(V, prefix, src))))
    assert any(isinstance(k, tuple) and k[1] == "prefix" for k in graph._dec._graphs)


def test_one_generator_across_prefix_widths():
    """No prefix, width 3, width 1 on the same sources: the step graphs of one width are not replayed for another."""
    from ofasys_amd.generator import SequenceGenerator
    model, d = _model(torch.float32)
    V = len(d)
    src = recipe.tokens("input.beam_src0", (2, 16), V, [16, 11])
    samples = [lambda: _sample(V, src), lambda: _prefixed(V, [[17, 60, 9], [33, 8, PAD]], src), lambda: _prefixed(V, [[17], [33]], src)]
    one = SequenceGenerator(d, **GEN)
    for rounds in range(3):                                          # eager warm-up, capture, replay -- of every variant
        got = [_flat(one.generate(model, s())) for s in samples]
    for s, res in zip(samples, got):
        _same(res, _flat(SequenceGenerator(d, use_graph=False, **GEN).generate(model, s())))
    keys = set(one._dec._graphs)
    assert {0, 1, (0, "prefix"), (1, "prefix"), (1, "free after a prefix")} <= keys


def test_width_zero_prefix_is_todays_path():
    from ofasys_amd.generator import SequenceGenerator
    model, d = _model(torch.float32)
    V = len(d)
    gen = SequenceGenerator(d, **GEN)
    plain = _flat(gen.generate(model, _sample(V)))
    empty = _flat(gen.generate(model, _prefixed(V, torch.zeros(2, 0, dtype=torch.long))))
    _same(plain, empty)


def test_task_inference_with_a_no_loss_target_prefix():
    from ofasys_amd import Task
    from ofasys_amd.preprocessor import to_device
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    task = Task(name="t2t", instruction="[TEXT:src] what is it? -> [TEXT:hint,no_loss] [TEXT:tgt]", micro_batch_size=2)
    task.initialize(d)
    task.cfg.evaluation.generator_args = '{"beam": 1, "max_len": 8, "no_repeat_ngram_size": 2}'
    task.add_dataset([{"src": "a small cat sits on the mat", "hint": "the answer is", "tgt": "a cat"},
                      {"src": "two dogs run in the park", "hint": "it", "tgt": "dogs run"}], "valid")
    batch = to_device(task.get_sample("valid"), DEV)
    prefix = batch["prefix_tokens"]
    assert prefix.shape[1] > 1 and bool((prefix[1] == d.pad()).any()) and not bool((prefix[0] == d.pad()).any())
    gen = task.generator
    raw = gen.generate(model, batch)
    out = task.inference(model, batch)
    assert len(out) == 2
    for b, (o, r) in enumerate(zip(out, raw)):
        n = int((prefix[b] != d.pad()).sum())
        assert r.tokens[:n].tolist() == prefix[b, :n].tolist()       # (one beam: it is forced along the prefix)
        assert o.tokens.tolist() == r.tokens[n:].tolist() and o.tokens[-1] == d.eos()
        assert o.positional_scores.numel() == r.tokens.numel()
        assert isinstance(o.text, str) and o.text == task.general_preprocess.name2pre["text"].decode(o.tokens)
    task.generator = task.build_generator(beam=3, max_len=8)
    assert all(isinstance(o.text, str) for o in task.inference(model, batch))


def test_prefix_with_eos_raises():
    from ofasys_amd.generator import SequenceGenerator
    model, d = _model(torch.float32)
    with pytest.raises(NotImplementedError, match="<eos>"):
        SequenceGenerator(d, beam_size=2, max_len=6).generate(model, _prefixed(len(d), [[17, EOS], [33, 8]]))


def test_trie_generator_refuses_a_prefix():
    from ofasys_amd.generator import TrieBeamGenerator
    from ofasys_amd.traverse import TraversePlan
    model, d = _model(torch.float32)
    plan = TraversePlan([[5, 6], [5, 7, 8]], d.bos(), d.eos(), d.pad())
    with pytest.raises(NotImplementedError, match="prefix"):
        TrieBeamGenerator(d, plan, beam_size=2, max_len=6).generate(model, _prefixed(len(d), [[17], [33]]))
