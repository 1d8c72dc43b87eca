"""GPU: diverse decoding (csrc/diverse_beam.hip, SequenceGenerator(search_strategy=DiverseBeamSearch | DiverseSiblingsSearch)).

1. One step -- the plain row pass, then the diverse sentence pass -- against tests/diverse_oracle.py, the full-vocabulary torch
   restatement: the whole state equal, scores to the plain beam test's tolerance (the arithmetic is the same plus one add).
2. The top-2K argument at its bound: a group pushed to the last two entries of its row's list, and a count of 2 deciding a pick.
3. generate() on the fp32 HIP `tiny_text` model against tests/golden/diverse_beam.npz (the reference's generator on the CPU).
4. Generation through the captured per-step graphs is bit-identical to eager stepping; Task.inference; one SCST step.
5. The entry points' host checks return errors without launching.
"""
import numpy as np
import pytest
import torch

from oracle import recipe
from oracle.cases import CASES
from tests import diverse_case as dc
from tests import diverse_oracle as do
from tests.golden_util import case_inputs, load_golden
from tests.model_util import build_model, make_slots
from tests.test_beam_search_gpu import _flat, _model, _sample, compare, make_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, UNK, BOS, EOS = do.PAD, do.UNK, do.BOS, do.EOS
STEPS = {"first": 0, "min_len": 2, "mid": 5, "max_len": 6}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


# ------------------------------------------------------------------------------------------------ one step against the oracle
def run_kernels(logits, st, K, step, cfg, strategy):
    from ofasys_amd import kernels as Kn
    rows, V = logits.shape
    d = {k: v.to(DEV) for k, v in st.items()}
    ws = torch.empty((Kn.beam_ws_bytes(rows, V, K) + 3) // 4, device=DEV)
    Kn.beam_topk(logits, K, step, ws, tokens=d["tokens"], done=d["done"], temperature=cfg["temperature"],
                 constraint_range=cfg.get("constraint_range"), min_len=cfg["min_len"], max_len=cfg["max_len"], pad=PAD, unk=UNK,
                 eos=EOS, unk_penalty=cfg["unk_penalty"], ngram=cfg["ngram"])
    kw = dict(eos=EOS, unk=UNK, unk_penalty=cfg["unk_penalty"], normalize=cfg["normalize"], len_penalty=cfg["len_penalty"])
    if strategy[0] == "groups":
        Kn.diverse_group_select(ws, d, K, V, step, cfg["max_len"], strategy[1], strategy[2], **kw)
    else:
        Kn.diverse_sibling_select(ws, d, K, V, step, cfg["max_len"], strategy[1], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def check_step(strategy, K, V, dtype, when, crange, seed):
    """The plain beam test's stressors: EOS boosted in sentence 1, a NaN row in sentence 2, random `ignore` and `fin_cnt`, the unk
    penalty, a crafted n-gram ban, a padded row stride, and constraint_range on some cases."""
    step = STEPS[when]
    bsz, cap = 3, 8
    g = torch.Generator().manual_seed(seed)
    rows = bsz * K
    buf = torch.randn(rows, V + 24, generator=g) * 3
    logits = buf[:, :V]
    cfg = dict(temperature=0.8, min_len=2, max_len=6, unk_penalty=0.3, ngram=3, normalize=True, len_penalty=1.2,
               constraint_range=(10, V - 7) if crange else None)
    logits[K:2 * K, EOS] += 6.0
    if K > 1:
        logits[2 * K + 1, 7] = float("nan")
    ngram_rows = [(0, [50, 60, 70, 11, 50, 60])] if step >= 5 else []
    if ngram_rows:
        logits[0, 70] += 12.0
    st = make_state(bsz, K, step, cap, V, g, ngram_rows)
    dev_logits = buf.to(DEV).to(dtype)[:, :V]
    gaps = []
    want = do.ref_step(dev_logits.cpu(), st, K, step, cfg, strategy, gaps)
    # an exact tie is decided by the tie rule on both sides; anything closer than fp32 rounding would make the case a coin toss
    assert all(x == 0.0 or x >= 1e-5 for x in gaps), sorted(gaps)[:3]
    compare(run_kernels(dev_logits, st, K, step, cfg, strategy), want)
    return want


# every (K, G), every V, every dtype and every step at least once; strengths with inexact products among them
GROUP_CASES = [(2, 2, 0.5, 204, F32, "first", False), (4, 2, 2.0, 4099, BF16, "min_len", True), (6, 3, 0.5, 59457, F16, "mid", False),
               (8, 4, 1.5, 204, BF16, "max_len", False), (16, 16, 0.7, 59457, F32, "mid", True), (16, 2, 0.5, 4099, F16, "first", False),
               (4, 2, 0.5, 59457, F32, "max_len", False), (8, 4, 0.3, 4099, F32, "min_len", False), (6, 3, 0.0, 204, F32, "mid", True)]
SIBLING_CASES = [(1, 0.5, 204, F32, "first", False), (2, 3.0, 4099, BF16, "mid", True), (5, 0.5, 59457, F16, "min_len", False),
                 (16, 0.25, 59457, F32, "mid", False), (5, 0.0, 204, F32, "max_len", True), (16, 1.0, 4099, BF16, "first", False),
                 (2, 0.3, 204, F16, "max_len", False), (1, 2.0, 59457, BF16, "min_len", False), (5, -0.5, 4099, F32, "mid", False)]


def _id(case):
    return "-".join(str(x).replace("torch.", "") for x in case)


@pytest.mark.parametrize("case", GROUP_CASES, ids=_id)
def test_group_select_matches_the_oracle(case):
    K, G, strength, V, dtype, when, crange = case
    check_step(("groups", G, strength), K, V, dtype, when, crange, seed=K * 1000 + G * 37 + V % 997 + STEPS[when])


@pytest.mark.parametrize("case", SIBLING_CASES, ids=_id)
def test_sibling_select_matches_the_oracle(case):
    K, rate, V, dtype, when, crange = case
    check_step(("siblings", rate), K, V, dtype, when, crange, seed=K * 1000 + V % 997 + STEPS[when] + 5)


def test_axes_are_covered():
    for cases, first in ((GROUP_CASES, {(2, 2), (4, 2), (6, 3), (8, 4), (16, 16), (16, 2)}), (SIBLING_CASES, {1, 2, 5, 16})):
        key = (lambda c: (c[0], c[1])) if len(cases[0]) == 7 else (lambda c: c[0])
        assert {key(c) for c in cases} == first
        assert {c[-4] for c in cases} == {204, 4099, 59457} and {c[-3] for c in cases} == {F32, BF16, F16}
        assert {c[-2] for c in cases} == set(STEPS) and {c[-1] for c in cases} == {False, True}


# ------------------------------------------------------------------------------------------------ the bound
PLAIN = dict(temperature=1.0, min_len=0, max_len=6, unk_penalty=0.0, ngram=0, normalize=False, len_penalty=1.0)


def _quiet_state(bsz, K, step, V, seed):
    g = torch.Generator().manual_seed(seed)
    st = make_state(bsz, K, step, 8, V, g)
    st["ignore"].zero_()
    st["fin_cnt"].zero_()
    st["scores"][:, :step] = -torch.arange(1, step + 1, dtype=torch.float32)      # equal cumulative scores: the logits decide
    return st, g


def test_group_select_reaches_the_last_two_entries_of_a_rows_list():
    """K = G = 4 (m = 1, two picks a group), strength 50: rows 0..2 take six distinct tokens that are also row 3's six best, so
    group 3 ends on entries 2K - 1 and 2K of row 3's list -- the bound of the top-2K argument.  Sentence 0 shows every group's
    first pick (the K active candidates), sentence 1 -- all first K candidates ignored -- every group's second pick."""
    K, G, V, step, strength = 4, 4, 204, 3, 50.0
    st, g = _quiet_state(2, K, step, V, 11)
    st["ignore"][1] = 1
    logits = torch.randn(2 * K, V, generator=g) * 0.1
    for s in range(2):
        for r in range(3):
            logits[s * K + r, 10 + 2 * r] += 10.0
            logits[s * K + r, 11 + 2 * r] += 9.0
        for i, tok in enumerate([10, 11, 12, 13, 14, 15, 20, 21]):
            logits[s * K + 3, tok] += [10.0, 9.5, 9.0, 8.5, 8.0, 7.5, 4.0, 3.0][i]
    row3 = torch.sort(logits[3], descending=True).indices[:2 * K].tolist()
    assert row3 == [10, 11, 12, 13, 14, 15, 20, 21]                                 # entries 7 and 8 of the row's list: 20, 21
    dev = logits.to(DEV)
    want = do.ref_step(logits, st, K, step, PLAIN, ("groups", G, strength))
    got = run_kernels(dev, st, K, step, PLAIN, ("groups", G, strength))
    compare(got, want)
    assert got["tokens"][:K, step + 1].tolist() == [10, 12, 14, 20] and got["reorder"][:K].tolist() == [0, 1, 2, 3]
    assert got["tokens"][K:, step + 1].tolist() == [11, 13, 15, 21] and got["reorder"][K:].tolist() == [4, 5, 6, 7]
    # group 3's scores carry the penalty of no earlier pick: its two tokens were taken by nobody
    lp = torch.log_softmax(logits[3], -1)
    assert abs(float(got["scores"][3, step]) - (float(lp[20]) - step)) < 1e-4


def test_group_select_counts_a_token_twice():
    """Groups 0 and 1 both take token A; row 2 holds A at +3.0 and B at +1.5 over the rest: with strength 1 group 2 puts B first
    only if A's count is 2 (3 - 2 < 1.5 < 3 - 1)."""
    K, G, V, step, A, B = 4, 4, 204, 3, 30, 40
    st, g = _quiet_state(1, K, step, V, 12)
    logits = torch.randn(K, V, generator=g) * 0.1
    logits[0, A] += 5.0
    logits[0, 50] += 2.0
    logits[1, A] += 5.0
    logits[1, 51] += 2.0
    logits[2, A] += 3.0
    logits[2, B] += 1.5
    logits[3, 60] += 4.0
    want = do.ref_step(logits, st, K, step, PLAIN, ("groups", G, 1.0))
    got = run_kernels(logits.to(DEV), st, K, step, PLAIN, ("groups", G, 1.0))
    compare(got, want)
    assert got["tokens"][:, step + 1].tolist() == [A, A, B, 60]
    once = do.ref_step(logits, st, K, step, PLAIN, ("groups", G, 0.5))              # 3 - 1 > 1.5: a count of 2 at half the strength
    assert once["tokens"][:, step + 1].tolist() == [A, A, A, 60]


# ------------------------------------------------------------------------------------------------ generate() against the reference
def _generator(d, cfg, **kw):
    from ofasys_amd import DiverseBeamSearch, DiverseSiblingsSearch
    from ofasys_amd.generator import SequenceGenerator
    return SequenceGenerator(d, search_strategy=dc.strategy_of(cfg, d, DiverseBeamSearch, DiverseSiblingsSearch), **dict(cfg["gen"], **kw))


def test_generate_matches_reference_golden():
    g = load_golden("diverse_beam")
    model, d = _model(torch.float32)
    for name, cfg in dc.CONFIGS.items():
        res = _flat(_generator(d, cfg).generate(model, _sample(len(d))))
        toks, lens, scores, pos = g[f"{name}.tokens"], g[f"{name}.lens"], g[f"{name}.scores"], g[f"{name}.pos"]
        for b, hyps in enumerate(res):
            assert len(hyps) == int((lens[b] > 0).sum()), (name, b)
            for i, h in enumerate(hyps):
                n = int(lens[b, i])
                assert h.tokens.tolist() == toks[b, i, :n].tolist(), (name, b, i)
                assert abs(float(h.score) - float(scores[b, i])) < 1e-4, (name, b, i)
                assert np.abs(h.positional_scores.numpy() - pos[b, i, :n]).max() < 1e-4, (name, b, i)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_graph_replay_equals_eager(dtype):
    model, d = _model(dtype)
    V = len(d)
    for name in ("groups2_ngram", "siblings_two"):
        cfg = dc.CONFIGS[name]
        eager, graph = _generator(d, cfg, use_graph=False), _generator(d, cfg, use_graph=True)
        for seed in range(3):                             # graph generator: eager warm-up, capture, replay
            src = recipe.tokens(f"input.beam_src{seed}", (2, 16), V, [16, 11 + seed])
            a, b = _flat(eager.generate(model, _sample(V, src))), _flat(graph.generate(model, _sample(V, src)))
            for ha, hb in zip(a, b):
                assert len(ha) == len(hb)
                for x, y in zip(ha, hb):
                    assert torch.equal(x.tokens, y.tokens) and torch.equal(x.score, y.score)
                    assert torch.equal(x.positional_scores, y.positional_scores)
        assert len(graph._dec._graphs) > 0


def test_task_inference_with_a_diverse_generator_decodes_text():
    from ofasys_amd import DiverseBeamSearch, Task
    case = CASES["tiny_text"]
    model, d = build_model(case, DEV, torch.float32)
    task = Task(name="t2t", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    task.initialize(d)
    task.generator = task.diverse_generator(beam=4, diverse_beam_groups=2, max_len=6, return_n_best=4)
    assert isinstance(task.generator.diverse, DiverseBeamSearch)
    vals, _ = case_inputs(case)
    out = task.inference(model, {"net_input": {"slots": make_slots(vals, DEV)}})
    assert len(out) == 2
    for hyps in out:
        assert 1 <= len(hyps) <= 4 and all(isinstance(h.text, str) and h.tokens[-1] == d.eos() for h in hyps)


def test_one_scst_step_with_a_diverse_generator_trains():
    from ofasys_amd import DiverseBeamSearch, Task, TaskConfig
    from ofasys_amd.scst import ScstRewardCriterion
    from ofasys_amd.trainer import TrainStep
    case = CASES["tiny_text"]
    model, d = _model(torch.float32)
    cfg = TaskConfig()
    cfg.scst, cfg.scst_args = True, '{"beam": 4, "diverse_beam_groups": 2, "max_len": 6}'
    task = Task(cfg, name="caption", instruction="[TEXT:src] what does it describe? -> [TEXT:caption]")
    task.initialize(d)
    assert isinstance(task.scst_generator.diverse, DiverseBeamSearch)
    vals, target = case_inputs(case)
    sample = {"net_input": {"slots": make_slots(vals, DEV)}, "target": target.to(DEV)}
    mb, log = ScstRewardCriterion(task, task.cfg.criterion)(model, sample)
    assert mb["reward"].shape == (8,) and mb["target"].shape[0] == 8 and np.isfinite(log["score"])
    assert bool(torch.isfinite(mb["reward"]).all())
    # (random weights against the case's targets score ~0 everywhere: fixed rewards make the update move the weights for certain)
    mb["reward"] = torch.tensor([1.25, -0.5, -0.75, 0.0, 2.0, -2.0, 0.5, -0.5], dtype=torch.float32, device=DEV)
    model.train()
    tr = TrainStep(model, lr=1e-2, clip_norm=1.0, use_graph=False)
    before = tr.master.clone()
    stats = tr.train_step([mb])["stats"]
    torch.cuda.synchronize()
    assert np.isfinite(float(stats[1])) and not torch.equal(before, tr.master)


# ------------------------------------------------------------------------------------------------ host checks
def test_entry_points_refuse_before_launching():
    from ofasys_amd import kernels as Kn
    from ofasys_amd.lib import OfaError

    def state(K, V=204):
        st = {k: v.to(DEV) for k, v in make_state(2, K, 2, 8, V, torch.Generator().manual_seed(1)).items()}
        return st, {k: v.clone() for k, v in st.items()}, torch.zeros(1 << 16, device=DEV)

    st, keep, ws = state(4)
    with pytest.raises(OfaError, match="not divisible"):
        Kn.diverse_group_select(ws, st, 4, 204, 2, 6, 3, 0.5)
    with pytest.raises(OfaError, match="strength"):
        Kn.diverse_group_select(ws, st, 4, 204, 2, 6, 2, -0.5)
    with pytest.raises(OfaError, match="must exceed 2 \\* beam"):
        Kn.diverse_sibling_select(ws, st, 4, 8, 2, 6, 0.5)
    torch.cuda.synchronize()
    assert all(torch.equal(st[k], keep[k]) for k in keep)           # nothing ran
    st17, _, ws17 = state(17)
    with pytest.raises(OfaError, match="beam size 17"):
        Kn.diverse_group_select(ws17, st17, 17, 204, 2, 6, 1, 0.5)
    with pytest.raises(OfaError, match="beam size 17"):
        Kn.diverse_sibling_select(ws17, st17, 17, 204, 2, 6, 0.5)
