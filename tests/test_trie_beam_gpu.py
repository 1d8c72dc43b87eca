"""GPU: trie-constrained beam search (csrc/trie_beam.hip, ofasys_amd.generator.TrieBeamGenerator, TraverseTask(search="beam")).

1. One step of the three launches (trie row pass, the unchanged sentence pass, node advance) against a torch restatement of the
   reference step written here: logits masked to the children of each row's trie node (generator/sequence_generator.py:729-741),
   log_softmax, the masks, topk, finalisation, active selection (:296-492), on the same, already rounded inputs.
2. generate() on the fp32 HIP `tiny_text` model against tests/golden/trie_beam.npz (the reference's generator with its Trie, CPU).
3. Consistency with the exact route (TraverseTask.score) in fp32; structure only in bf16 / fp16.
4. What the design claims: the step count, no output projection, graphs == eager, no allocation on a second batch, and plain
   generation / a captured TrainStep unaffected by a trie generator in between.
"""
import json
import math

import numpy as np
import pytest
import torch

from oracle import recipe
from oracle.cases import CASES, VOCAB_EXTRA, make_value
from tests.golden_util import case_inputs, load_golden
from tests.model_util import build_model, make_slots
from tests.traverse_case import ANSWERS, random_answers, score_err
from tests.trie_beam_case import CLOSED_SETS, CONFIGS, SCORE_TOL, distinct, generator_args, label_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, UNK, BOS, EOS = 1, 3, 0, 2
V_OFA, D_OFA = 59457, 768
V_TINY = VOCAB_EXTRA + 4
KERNEL_TOL = 1e-4             # max |d| / max(|ref|, 1): fp32 accumulation on the same rounded inputs, only the summation order differs
MIN_GAP = 1e-3                # adjacent candidate scores of the restatement: exact comparisons of the choices are meaningful
_CACHE = {}


# ------------------------------------------------------------------------------------------------ torch restatement of one step
def ref_trie_step(logits, node, children, st, K, step, cfg):
    """The reference's step on CPU tensors: `logits` fp32 [rows, V] (projection of the rounded inputs), masked here to the
    children of node[row] (a dead row: nothing allowed).  Returns the new state (with "node") and the smallest gap between
    adjacent finite candidate scores among each sentence's first 2K + 1.  Sentences with done = 1 are skipped."""
    st = {k: v.clone() for k, v in st.items()}
    rows, V = logits.shape
    bsz = rows // K
    x = logits.float() / cfg["temperature"]
    mask = torch.zeros(rows, V, dtype=torch.bool)
    for r in range(rows):
        if node[r] >= 0:
            mask[r, list(children[int(node[r])].keys())] = True
    x = x.masked_fill(~mask, -math.inf)
    lp = torch.log_softmax(x, -1)
    if step < cfg["min_len"]:
        lp[:, EOS] = -math.inf
    lp[lp != lp] = -math.inf
    lp[:, PAD] = -math.inf
    lp[:, UNK] -= cfg["unk_penalty"]
    if step >= cfg["max_len"]:
        lp[:, :EOS] = -math.inf
        lp[:, EOS + 1:] = -math.inf
    n = cfg["ngram"]
    if n > 0 and step + 2 - n >= 0:
        for r in range(rows):
            h = st["tokens"][r, :step + 1].tolist()
            key = h[step + 2 - n:step + 1]
            for i in range(0, step + 2 - n):
                if h[i:i + n - 1] == key:
                    lp[r, h[i + n - 1]] = -math.inf
    new_node = node.clone()
    gap = math.inf
    for s in range(bsz):
        if st["done"][s]:
            continue
        r0 = s * K
        lps = lp[r0:r0 + K]
        cand = lps[:1] if step == 0 else lps + st["scores"][r0:r0 + K, step - 1].unsqueeze(-1)
        flat = cand.reshape(-1)
        k = min(2 * K, flat.numel() - 1)
        order = torch.sort(flat, descending=True, stable=True).indices          # ties (all at -inf) to the lower flat index
        head = flat[order[:k + 1]].double()
        head = head[torch.isfinite(head)]
        if head.numel() > 1:
            gap = min(gap, float((head[:-1] - head[1:]).min()))
        order = order[:k]
        csc = flat[order]
        cidx, cbeam = order % V, order // V
        eos_mask = (cidx == EOS) & (csc != -math.inf)
        ign = st["ignore"][s].bool()
        eos_mask[:K][ign[:min(K, k)]] = False
        cnt = int(st["fin_cnt"][s])
        for j in range(min(K, k)):
            if eos_mask[j] and cnt < K:
                row = r0 + int(cbeam[j])
                toks = st["tokens"][row, 1:step + 2].clone()
                toks[step] = EOS
                pos = st["scores"][row, :step + 1].clone()
                pos[step] = csc[j]
                pos[1:] = pos[1:] - pos[:-1]
                score = csc[j].clone()
                if cfg["normalize"]:
                    score /= (step + 1) ** cfg["len_penalty"]
                st["fin_tok"][s, cnt, :step + 1] = toks
                st["fin_pos"][s, cnt, :step + 1] = pos
                st["fin_score"][s, cnt] = score
                st["fin_len"][s, cnt] = step + 1
                cnt += 1
        st["fin_cnt"][s] = cnt
        if cnt == K or step >= cfg["max_len"]:
            st["done"][s] = 1
            st["nfin"][0] += 1
            st["reorder"][r0:r0 + K] = torch.arange(r0, r0 + K)
            continue
        em = eos_mask.clone()
        em[:K] = ign[:min(K, k)] | eos_mask[:K]
        active_mask = em.long() * (2 * K) + torch.arange(k)
        new_ign, active = torch.topk(active_mask, k=K, largest=False)
        st["ignore"][s] = new_ign.ge(2 * K).int()
        src = r0 + cbeam[active]
        st["tokens"][r0:r0 + K, :step + 1] = st["tokens"][src, :step + 1]
        st["tokens"][r0:r0 + K, step + 1] = cidx[active]
        if step > 0:
            st["scores"][r0:r0 + K, :step] = st["scores"][src, :step]
        st["scores"][r0:r0 + K, step] = csc[active]
        st["reorder"][r0:r0 + K] = src
        # every row's node follows its parent through the chosen token; dead: dead parent, -inf, EOS edge
        alive = False
        for b in range(K):
            pn, sc, tok = int(node[int(src[b])]), float(csc[active][b]), int(cidx[active][b])
            child = -1
            if pn >= 0 and sc != -math.inf:
                child = children[pn].get(tok, -1)
            new_node[r0 + b] = child
            alive = alive or (sc != -math.inf and not bool(st["ignore"][s, b]))
        if not alive:                                                            # nothing more can be finalised (:361)
            st["done"][s] = 1
            st["nfin"][0] += 1
    st["node"] = new_node
    return st, gap


def _plan(which):
    """A closed set over the OFA vocabulary whose root has ~1300 (A) / ~3100 (B) edges, <unk> as an answer and inside answers."""
    if which not in _CACHE:
        from ofasys_amd import TraversePlan
        C = {"A": 1500, "B": 3600}[which]
        rng = np.random.default_rng(C)
        answers = random_answers(rng, C, V=V_OFA, p_dup=0.02, p_ext=0.15) + [[UNK], [UNK, 9], [4, UNK]]
        plan = TraversePlan(answers, BOS, EOS, PAD)
        children = [dict(zip(plan.edge_token[plan.node_edge_off[n]:plan.node_edge_off[n + 1]].tolist(),
                             plan.edge_child[plan.node_edge_off[n]:plan.node_edge_off[n + 1]].tolist())) for n in range(plan.N)]
        deg = np.diff(plan.node_edge_off)
        eos_edge = np.zeros(plan.N, bool)
        eos_edge[plan.edge_node[plan.edge_token == EOS]] = True
        kinds = {"root": [0], "eos_only": np.nonzero(eos_edge & (deg == 1))[0].tolist(),
                 "eos_and_tokens": np.nonzero(eos_edge & (deg > 1))[0].tolist(),
                 "small": np.nonzero(~eos_edge & (deg >= 1) & (deg < 8))[0].tolist()}
        assert all(len(v) > 0 for v in kinds.values()) and int(deg[0]) == plan.max_degree
        _CACHE[which] = (plan, children, kinds, plan.to_device(DEV))
    return _CACHE[which]


def _proj(dtype):
    if ("W", dtype) not in _CACHE:
        g = torch.Generator().manual_seed(11)
        _CACHE[("W", dtype)] = ((torch.randn(V_OFA, D_OFA, generator=g) * 0.05).to(DEV).to(dtype),
                                torch.randn(V_OFA, generator=g).to(DEV).to(dtype))
    return _CACHE[("W", dtype)]


def _scenario(seed, plan, kinds, K, step, cap, dtype):
    """State, nodes and hidden rows of 4 sentences (the last one already done) at `step`."""
    g = torch.Generator().manual_seed(seed)
    bsz = 4
    rows = bsz * K
    tokens = torch.full((rows, cap), PAD, dtype=torch.long)
    tokens[:, 0] = BOS
    scores = torch.zeros(rows, cap)
    node = torch.zeros(rows, dtype=torch.int32)
    if step > 0:
        tokens[:, 1:step + 1] = torch.randint(4, V_OFA, (rows, step), generator=g)
        scores[:, :step] = -torch.rand(rows, step, generator=g).cumsum(1) * 2
        order = ["root", "small", "eos_and_tokens", "dead", "eos_only", "small"]
        for r in range(rows):
            kind = order[(r + seed) % len(order)]
            if kind == "dead":
                node[r] = -1
                if r % 2 == 0:
                    scores[r, step - 1] = -math.inf
            else:
                pool = kinds[kind]
                node[r] = pool[int(torch.randint(len(pool), (1,), generator=g))]
        if step >= 3:                                        # n = 2: ... 7 c 7 bans c, a child of the row's node
            for r in range(rows):
                if node[r] > 0:
                    lo = int(plan.node_edge_off[int(node[r])])
                    tokens[r, step - 2], tokens[r, step - 1], tokens[r, step] = 7, int(plan.edge_token[lo]), 7
                    break
    i32 = torch.int32
    st = {"tokens": tokens, "scores": scores,
          "ignore": (torch.rand(bsz, K, generator=g) < 0.25).to(i32) if step > 0 else torch.zeros(bsz, K, dtype=i32),
          "done": torch.tensor([0, 0, 0, 1], dtype=i32), "nfin": torch.ones(1, dtype=i32),
          "reorder": torch.arange(rows, dtype=torch.long),
          "fin_tok": torch.zeros(bsz, K, cap, dtype=torch.long), "fin_pos": torch.zeros(bsz, K, cap),
          "fin_score": torch.zeros(bsz, K), "fin_len": torch.zeros(bsz, K, dtype=i32),
          "fin_cnt": torch.randint(0, K, (bsz,), generator=g).to(i32)}
    h = (torch.randn(rows, D_OFA + 8, generator=g) * 2).to(DEV).to(dtype)[:, :D_OFA]          # a padded row stride
    return st, node, h


STEPS = {"first": 0, "min_len": 1, "mid": 3, "max_len": 6}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [1, 2, 5, 8, 16])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("when", list(STEPS))
def test_trie_beam_kernels_match_reference_step(dtype, K, with_bias, when):
    """Bound on the scores: 1e-4 relative (floor absolute), the closed-set kernels' bound for the same arithmetic.  Everything
    else -- tokens and beams of finite candidates, reorder, ignore, the nodes, the finalised set -- is exact; the seed of a case is
    the first for which the RESTATEMENT's adjacent candidate scores are more than 1e-3 apart.  Measured maximum on an MI355X over
    the 120 cases: 8.5e-6 (fp32), 3.5e-6 (bf16), 5.1e-6 (fp16) (profiles/trie_beam_parity.txt)."""
    from ofasys_amd import kernels as Kn
    step, cap = STEPS[when], 8
    plan, children, kinds, dev = _plan("B" if with_bias else "A")
    assert Kn.trie_beam_splits(plan.max_degree, V_OFA) > 1 and plan.max_degree > 1000
    W, bias = _proj(dtype)
    bias = bias if with_bias else None
    cfg = dict(temperature=0.8, min_len=2, max_len=6, unk_penalty=0.3, ngram=2, normalize=True, len_penalty=1.2)
    base = K * 1000 + step * 10 + int(with_bias)
    for seed in range(base, base + 50):
        st, node, h = _scenario(seed, plan, kinds, K, step, cap, dtype)
        logits = h.float() @ W.float().t()
        if bias is not None:
            logits += bias.float()
        want, gap = ref_trie_step(logits.cpu(), node, children, st, K, step, cfg)
        if gap > MIN_GAP:
            break
    assert gap > MIN_GAP, gap                                # asserted on the restatement itself; no case is skipped
    rows = 4 * K
    d = {k: v.to(DEV) for k, v in st.items()}
    d["node"] = node.to(DEV)
    ws = torch.full(((Kn.beam_ws_bytes(rows, V_OFA, K) + 3) // 4,), 12345.0, device=DEV)      # nothing relies on what was there
    Kn.trie_beam_topk(h, W, bias, dev, d["node"], K, step, ws, tokens=d["tokens"], done=d["done"], temperature=cfg["temperature"],
                      min_len=cfg["min_len"], max_len=cfg["max_len"], pad=PAD, unk=UNK, eos=EOS, unk_penalty=cfg["unk_penalty"],
                      ngram=cfg["ngram"])
    Kn.beam_select(ws, d, K, V_OFA, step, cfg["max_len"], eos=EOS, unk=UNK, unk_penalty=cfg["unk_penalty"],
                   normalize=cfg["normalize"], len_penalty=cfg["len_penalty"])
    Kn.trie_beam_advance(dev, d["node"], d, K, step)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in d.items()}
    for name in ("reorder", "ignore", "done", "nfin", "fin_cnt", "fin_len", "fin_tok", "node"):
        assert torch.equal(got[name], want[name]), (name, got[name], want[name])
    assert torch.equal(got["tokens"][:, :step + 1], want["tokens"][:, :step + 1])
    live = torch.isfinite(want["scores"][:, step]) & (want["done"].repeat_interleave(K) == 0)
    assert torch.equal(got["tokens"][live, step + 1], want["tokens"][live, step + 1])          # (not the tokens of -inf beams)
    worst = 0.0
    for name in ("scores", "fin_score", "fin_pos"):
        a, b = got[name], want[name]
        assert torch.equal(torch.isinf(a), torch.isinf(b)) and not torch.isnan(a).any(), name
        fin = torch.isfinite(b)
        if fin.any():
            worst = max(worst, score_err(a[fin].numpy(), b[fin].numpy()))
    print(f"trie beam kernels {dtype} K={K} bias={with_bias} {when}: seed {seed} gap {gap:.2e} root {plan.max_degree} edges, "
          f"{int(want['fin_cnt'].sum() - st['fin_cnt'].sum())} finalised, {int(live.sum())} live rows, max score err {worst:.2e}")
    assert worst <= KERNEL_TOL, worst
    if when == "mid":
        assert int(live.sum()) > 0 and int((want["node"] >= 0).sum()) > 0


def test_trie_beam_kernels_reject_mismatched_inputs():
    from ofasys_amd import kernels as Kn
    from ofasys_amd.lib import OfaError
    plan, _, _, dev = _plan("A")
    W = torch.zeros(V_OFA, 64, device=DEV)
    ws = torch.empty(1 << 20, device=DEV)
    node = torch.zeros(10, dtype=torch.int32, device=DEV)
    with pytest.raises(OfaError, match="dtype"):
        Kn.trie_beam_topk(torch.zeros(10, 64, device=DEV, dtype=torch.bfloat16), W, None, dev, node, 5, 0, ws)
    with pytest.raises(OfaError, match="node"):
        Kn.trie_beam_topk(torch.zeros(10, 64, device=DEV), W, None, dev, node[:5], 5, 0, ws)
    with pytest.raises(OfaError, match="beam size"):
        Kn.trie_beam_topk(torch.zeros(17, 64, device=DEV), W, None, dev, torch.zeros(17, dtype=torch.int32, device=DEV), 17, 0, ws)


# ------------------------------------------------------------------------------------------------ generate() against the reference
def _task(d, which="main", **kw):
    from ofasys_amd import TraverseTask
    task = TraverseTask(name="vqa", instruction="[TEXT:src] what is it? -> [TEXT:tgt]", **kw)
    task.initialize(d, closed_set=[tuple(a) for a in CLOSED_SETS[which]])
    return task


def _sample(V=V_TINY, src=None):
    from ofasys_amd import ModalityType, Slot
    case = CASES["tiny_text"]
    slots = [Slot(ModalityType[m], True, (src if src is not None else make_value(spec, V)).to(DEV), attributes=a)
             for m, s, spec, a in case["slots"] if s]
    return {"net_input": {"slots": slots}}


def _flat(result):
    return [r if isinstance(r, list) else [r] for r in result]


def _search_args(cfg):
    a = generator_args(cfg)
    return dict(beam=a.pop("beam"), n_best=a.pop("return_n_best", 1), **a)


def test_generate_matches_reference_golden():
    """Tokens and lengths exact; scores and positional scores within the standing fp32 bound against the reference, 1e-3 relative
    with a floor of 1e-3 absolute.  Measured maximum on an MI355X: 2.0e-6 (profiles/trie_beam_parity.txt)."""
    g = load_golden("trie_beam")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(CONFIGS))
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    tasks = {which: _task(d, which) for which in CLOSED_SETS}
    worst = 0.0
    for name, cfg in CONFIGS.items():
        task = tasks[cfg["set"]]
        args = _search_args(cfg)
        res = _flat(task.beam_search(model, _sample(), **args))
        toks, lens, scores, pos = g[f"{name}.tokens"], g[f"{name}.lens"], g[f"{name}.scores"], g[f"{name}.pos"]
        pre = task.general_preprocess.name2pre["text"]
        for b, hyps in enumerate(res):
            assert len(hyps) == int((lens[b] > 0).sum()), (name, b, len(hyps))
            for i, h in enumerate(hyps):
                n = int(lens[b, i])
                assert h.tokens.tolist() == toks[b, i, :n].tolist(), (name, b, i)
                worst = max(worst, score_err(float(h.score), float(scores[b, i])), score_err(h.positional_scores.numpy(), pos[b, i, :n]))
                assert h.attention.numel() == 0 and h.text == pre.decode(h.tokens)
        gen = task.trie_generator(beam=args["beam"], return_n_best=args["n_best"], **{k: v for k, v in args.items() if k not in ("beam", "n_best")})
        assert gen.steps_run <= min(args["max_len"], task.plan.Tmax) + 1
        best = task.inference(model, _sample(), search="beam", **{k: v for k, v in args.items() if k != "n_best"})
        assert best == [task.index2ans[int(i)] for i in g[f"{name}.best"]], (name, best)
        print(f"trie beam parity {name}: steps run {gen.steps_run} (reference {int(g[f'{name}.ref_steps'])})")
    print(f"trie beam parity (tiny_text, fp32): max |score - reference| / max(|reference|, 1) = {worst:.3e}")
    assert worst <= SCORE_TOL, worst
    assert not model.training


def test_no_hypothesis_raises_and_names_the_sentence():
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    task = _task(d, "small")
    with pytest.raises(ValueError, match="sentence 0"):                      # min_len 5: EOS is masked wherever the trie allows it
        task.inference(model, _sample(), search="beam", min_len=5, max_len=10)
    assert task.beam_search(model, _sample(), n_best=5, min_len=5, max_len=10) == [[], []]


# ------------------------------------------------------------------------------------------------ consistency with the exact route
def test_fp32_scores_equal_the_exact_route():
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    task = _task(d)
    exact = task.score(model, _sample()).numpy()
    worst = 0.0
    for beam in (1, 3, 5, 16):
        res = _flat(task.beam_search(model, _sample(), beam=beam, n_best=beam, max_len=10))
        for b, hyps in enumerate(res):
            for h in hyps:
                worst = max(worst, score_err(float(h.score), float(exact[b, label_of(ANSWERS, h.tokens[:-1].tolist())])))
        if beam == 16:                                                        # the whole closed set comes back
            assert all(sorted(h.tokens[:-1].tolist() for h in hyps) == sorted(distinct(ANSWERS)) for hyps in res)
    print(f"trie beam vs TraverseTask.score (fp32): max |d| / max(|score|, 1) = {worst:.3e}")
    assert worst <= 1e-3, worst
    assert task.inference(model, _sample(), search="beam", beam=16, max_len=10) == task.inference(model, _sample(), search="all")
    assert task.inference(model, _sample()) == task.inference(model, _sample(), search="all")   # the default is unchanged
    beam_task = _task(d, search="beam", beam=16)
    assert beam_task.inference(model, _sample()) == task.inference(model, _sample())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_low_precision_structure(dtype):
    """bf16 / fp16: only the structure is asserted (closed-set answers, descending, finite); the gap to TraverseTask.score of the
    same dtype is printed (profiles/trie_beam_parity.txt) -- the two routes run the decoder at different row counts and lengths,
    and nothing in the project yields a bound for that.  Measured on an MI355X: 2.2e-2 (bf16), 1.3e-3 (fp16)."""
    model, d = build_model(CASES["tiny_text"], DEV, dtype)
    task = _task(d)
    exact = task.score(model, _sample()).numpy()
    res = _flat(task.beam_search(model, _sample(), beam=16, n_best=16, max_len=10))
    worst = 0.0
    for b, hyps in enumerate(res):
        assert len(hyps) >= 1
        seqs = [h.tokens[:-1].tolist() for h in hyps]
        assert all(h.tokens[-1] == EOS for h in hyps) and all(s in distinct(ANSWERS) for s in seqs)
        assert len({tuple(s) for s in seqs}) == len(seqs)
        sc = [float(h.score) for h in hyps]
        assert all(math.isfinite(x) for x in sc) and all(x >= y for x, y in zip(sc, sc[1:]))
        for h, s in zip(hyps, seqs):
            worst = max(worst, score_err(float(h.score), float(exact[b, label_of(ANSWERS, s)])))
    print(f"trie beam vs TraverseTask.score ({dtype}): {[len(h) for h in res]} hypotheses, max |d| / max(|score|, 1) = {worst:.3e}")


# ------------------------------------------------------------------------------------------------ the claims
def _same(a, b):
    assert len(a) == len(b)
    for ha, hb in zip(a, b):
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            assert torch.equal(x.tokens, y.tokens) and torch.equal(x.score, y.score)
            assert torch.equal(x.positional_scores, y.positional_scores)


def test_step_count_and_no_output_projection():
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    task = _task(d)
    ga = model.decoder.adaptor
    original = ga.forward_output

    def refuse(*a, **k):
        raise AssertionError("the output projection ran in trie mode")
    ga.forward_output = refuse
    try:
        for _ in range(3):                                                    # eager warm-up, capture, replay
            res = _flat(task.beam_search(model, _sample(), beam=5, n_best=5, max_len=256))
    finally:
        ga.forward_output = original
    gen = task.trie_generator(beam=5, return_n_best=5, max_len=256)
    assert gen.steps_run <= min(256, task.plan.Tmax) + 1 == 6
    assert gen._dec.max_len == task.plan.Tmax + 1 and gen._dec.tokens.shape[1] == task.plan.Tmax + 1      # not 257
    assert len(gen._dec._graphs) > 0 and all(len(h) == 5 for h in res)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graph_replay_equals_eager(dtype):
    from ofasys_amd.generator import TrieBeamGenerator
    model, d = build_model(CASES["tiny_text"], DEV, dtype)
    task = _task(d)
    cfg = dict(beam_size=4, max_len=8, no_repeat_ngram_size=2, return_n_best=4, normalize_scores=True)
    eager, graph = TrieBeamGenerator(d, task.plan, use_graph=False, **cfg), TrieBeamGenerator(d, task.plan, use_graph=True, **cfg)
    for seed in range(3):
        src = recipe.tokens(f"input.beam_src{seed}", (2, 16), V_TINY, [16, 11 + seed])
        _same(_flat(eager.generate(model, _sample(V_TINY, src))), _flat(graph.generate(model, _sample(V_TINY, src))))
    assert len(graph._dec._graphs) > 0 and len(eager._dec._graphs) == 0


def test_second_generate_allocates_nothing():
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    task = _task(d)
    for seed in range(3):                                                     # eager warm-up, capture, replay
        src = recipe.tokens(f"input.beam_src{seed}", (2, 16), V_TINY, [16, 12])
        task.inference(model, _sample(V_TINY, src), search="beam")
    gen = task.trie_generator(beam=5)                                         # the generator inference(search="beam") used
    assert gen._state is not None and len(task._trie_gens) == 1
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in gen._state.items() if torch.is_tensor(v)}
    plan_ptrs = {k: v.data_ptr() for dev in gen._dev.values() for k, v in dev.items() if torch.is_tensor(v)}
    graphs = dict(gen._dec._graphs)
    before = torch.cuda.memory_allocated()
    out = task.inference(model, _sample(V_TINY, recipe.tokens("input.beam_src1", (2, 16), V_TINY, [16, 12])), search="beam")
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert {k: v.data_ptr() for k, v in gen._state.items() if torch.is_tensor(v)} == ptrs
    assert {k: v.data_ptr() for dev in gen._dev.values() for k, v in dev.items() if torch.is_tensor(v)} == plan_ptrs
    assert gen._dec._graphs == graphs and len(task._trie_gens) == 1 and len(out) == 2 and not model.training


def _generation_and_training(with_trie):
    """Plain beam search, [the trie generator], a captured TrainStep (lr = 0), [the trie generator], plain beam search, a train
    step: what the plain generator and the trainer return."""
    from ofasys_amd import ops
    from ofasys_amd.generator import SequenceGenerator
    from ofasys_amd.trainer import TrainStep
    ops.manual_seed(1234)
    case = CASES["tiny_text"]
    model, d = build_model(case, DEV, torch.float32)
    plain = SequenceGenerator(d, beam_size=3, max_len=6, return_n_best=3)
    task = _task(d)
    out = {"plain": [], "stats": [], "trie": []}
    for _ in range(3):
        out["plain"].append(_flat(plain.generate(model, _sample())))
    if with_trie:
        for _ in range(3):
            out["trie"].append(_flat(task.beam_search(model, _sample(), beam=5, n_best=5)))
    vals, target = case_inputs(case)
    model.train()
    tr = TrainStep(model, lr=0.0, clip_norm=0.0, use_graph=True, graph_warmup=1)
    for _ in range(3):
        out["stats"].append(tr.train_step([{"slots": make_slots(vals, DEV), "target": target.to(DEV)}])["stats"].clone())
    assert tr.captured_graphs() >= 1
    if with_trie:
        for _ in range(3):                                                    # the weights now live in the trainer's arenas
            out["trie"].append(_flat(task.beam_search(model, _sample(), beam=5, n_best=5)))
    out["plain"].append(_flat(plain.generate(model, _sample())))
    model.train()
    out["stats"].append(tr.train_step([{"slots": make_slots(vals, DEV), "target": target.to(DEV)}])["stats"].clone())
    torch.cuda.synchronize()
    return out


def test_trie_generator_between_generation_and_a_captured_train_step():
    """the trie generator's graphs and scratch live in its own StepDecoder; plain generation and a captured
    TrainStep before and after it give exactly what they give without it."""
    without, with_ = _generation_and_training(False), _generation_and_training(True)
    for a, b in zip(without["plain"], with_["plain"]):
        _same(a, b)
    for a, b in zip(without["stats"], with_["stats"]):
        assert torch.equal(a, b) and torch.isfinite(a.float()).all()
    for r in with_["trie"][1:]:                                               # lr = 0: the same weights before and after the trainer
        _same(with_["trie"][0], r)
