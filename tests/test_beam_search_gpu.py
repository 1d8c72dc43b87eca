"""GPU: beam search (csrc/beam_search.hip, ofasys_amd.generator.SequenceGenerator, Task.inference).

1. One step of the two beam kernels against a torch restatement of the reference step written here
   (generator/sequence_generator.py:283-492, finalize_hypos :530-627, utils/search.py:107-142, utils/ngram_repeat_block.py).
2. generate() on the fp32 HIP `tiny_text` model against tests/golden/beam_search.npz (the reference's generator on the CPU).
3. Generation through the captured per-step graphs is bit-identical to eager stepping (fp32, bf16, three batches).
4. Task.inference returns decoded strings, and training still works afterwards.
"""
import json
import math

import numpy as np
import pytest
import torch

from oracle import recipe
from oracle.cases import CASES, VOCAB_EXTRA, make_value
from tests.beam_case import CONFIGS, boost_eos
from tests.golden_util import case_inputs, load_golden
from tests.model_util import build_model, make_slots

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, UNK, BOS, EOS = 1, 3, 0, 2


# ------------------------------------------------------------------------------------------------ torch restatement of one step
def ref_step(logits, st, K, step, cfg):
    """The reference's step on CPU tensors (float32): returns the new state dict.  Sentences with done = 1 are skipped (the
    reference removes them from the batch; rows are independent)."""
    st = {k: v.clone() for k, v in st.items()}
    rows, V = logits.shape
    bsz = rows // K
    x = logits.float() / cfg["temperature"]
    if cfg.get("constraint_range") is not None:
        cs, ce = cfg["constraint_range"]
        x[:, 4:cs] = -math.inf
        x[:, ce:] = -math.inf
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
    for s in range(bsz):
        if st["done"][s]:
            continue
        r0 = s * K
        lps = lp[r0:r0 + K]
        if step == 0:
            cand = lps[:1]
        else:
            cand = lps + st["scores"][r0:r0 + K, step - 1].unsqueeze(-1)
        flat = cand.reshape(-1)
        k = min(2 * K, flat.numel() - 1)
        # topk with ties to the lower flat index (the kernels' order; tests avoid finite ties)
        order = torch.sort(flat, descending=True, stable=True).indices[:k]
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
    return st


def make_state(bsz, K, step, cap, V, g, ngram_rows=()):
    rows = bsz * K
    tokens = torch.full((rows, cap), PAD, dtype=torch.long)
    tokens[:, 0] = BOS
    if step > 0:
        tokens[:, 1:step + 1] = torch.randint(4, V, (rows, step), generator=g)
    for r, pattern in ngram_rows:
        m = min(len(pattern), step + 1)
        tokens[r, step + 1 - m:step + 1] = torch.tensor(pattern[-m:])
    scores = torch.zeros(rows, cap, dtype=torch.float32)
    if step > 0:
        scores[:, :step] = -torch.rand(rows, step, generator=g).cumsum(1) * 2
    i32 = torch.int32
    return {"tokens": tokens, "scores": scores,
            "ignore": (torch.rand(bsz, K, generator=g) < 0.25).to(i32) if step > 0 else torch.zeros(bsz, K, dtype=i32),
            "done": torch.zeros(bsz, dtype=i32), "nfin": torch.zeros(1, dtype=i32),
            "reorder": torch.arange(rows, dtype=torch.long),
            "fin_tok": torch.zeros(bsz, K, cap, dtype=torch.long), "fin_pos": torch.zeros(bsz, K, cap),
            "fin_score": torch.zeros(bsz, K), "fin_len": torch.zeros(bsz, K, dtype=i32),
            "fin_cnt": torch.randint(0, K, (bsz,), generator=g).to(i32)}


def run_kernels(logits, st, K, step, cfg):
    from ofasys_amd import kernels as Kn
    rows, V = logits.shape
    d = {k: v.to(DEV) for k, v in st.items()}
    ws = torch.empty((Kn.beam_ws_bytes(rows, V, K) + 3) // 4, device=DEV)
    Kn.beam_topk(logits, K, step, ws, tokens=d["tokens"], done=d["done"], temperature=cfg["temperature"],
                 constraint_range=cfg.get("constraint_range"), min_len=cfg["min_len"], max_len=cfg["max_len"], pad=PAD, unk=UNK,
                 eos=EOS, unk_penalty=cfg["unk_penalty"], ngram=cfg["ngram"])
    Kn.beam_select(ws, d, K, V, step, cfg["max_len"], eos=EOS, unk=UNK, unk_penalty=cfg["unk_penalty"],
                   normalize=cfg["normalize"], len_penalty=cfg["len_penalty"])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def compare(got, want):
    for name in ("tokens", "reorder", "ignore", "done", "nfin", "fin_cnt", "fin_len", "fin_tok"):
        assert torch.equal(got[name], want[name]), (name, got[name], want[name])
    for name in ("scores", "fin_score", "fin_pos"):
        a, b = got[name], want[name]
        assert torch.equal(torch.isinf(a), torch.isinf(b)), name
        fin = torch.isfinite(b)
        assert torch.allclose(a[fin], b[fin], rtol=1e-5, atol=2e-5), (name, float((a[fin] - b[fin]).abs().max()))


STEPS = {"first": 0, "min_len": 2, "mid": 5, "max_len": 6}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [1, 2, 4, 5, 8])
@pytest.mark.parametrize("V", [204, 59457])
@pytest.mark.parametrize("when", list(STEPS))
def test_beam_kernels_match_reference_step(dtype, K, V, when):
    step = STEPS[when]
    bsz, cap = 3, 8
    g = torch.Generator().manual_seed(K * 1000 + V % 997 + step)
    rows = bsz * K
    ld = V + 24                                                      # padded row stride
    buf = torch.randn(rows, ld, generator=g) * 3
    logits = buf[:, :V]
    cfg = dict(temperature=0.8, min_len=2, max_len=6, unk_penalty=0.3, ngram=3, normalize=True, len_penalty=1.2,
               constraint_range=(10, V - 7) if K in (2, 5) else None)
    # EOS high in sentence 1 (more EOS candidates than open slots: fin_cnt and cands_to_ignore take part)
    logits[K:2 * K, EOS] += 6.0
    # a NaN in one row of sentence 2 (not beam 0 at step 0: a whole -inf row keeps the index-order ties)
    if K > 1:
        logits[2 * K + 1, 7] = float("nan")
    # a crafted n-gram history in row 0: ... 50 60 70 ... 50 60 -> 70 banned, and 70 is that row's best token
    ngram_rows = [(0, [50, 60, 70, 11, 50, 60])] if step >= 5 else []
    if ngram_rows:
        logits[0, 70] += 12.0
    st = make_state(bsz, K, step, cap, V, g, ngram_rows)
    dev_logits = buf.to(DEV).to(dtype)[:, :V]
    want = ref_step(dev_logits.cpu(), st, K, step, cfg)
    got = run_kernels(dev_logits, st, K, step, cfg)
    compare(got, want)
    if ngram_rows:
        assert int(want["tokens"][0, step + 1]) != 70 or int(want["reorder"][0]) != 0


def test_beam_kernels_reject_large_beam():
    from ofasys_amd import kernels as Kn
    from ofasys_amd.lib import OfaError
    logits = torch.zeros(17, 204, device=DEV)
    ws = torch.empty(1 << 20, device=DEV)
    with pytest.raises(OfaError, match="beam size"):
        Kn.beam_topk(logits, 17, 0, ws)


# ------------------------------------------------------------------------------------------------ generate() against the reference
def _model(dtype):
    model, d = build_model(CASES["tiny_text"], DEV, dtype)
    with torch.no_grad():
        boost_eos(model.state_dict()["decoder.adaptor.embed_tokens.weight"], d.eos())
    model.eval()
    return model, d


def _sample(V, src=None):
    from ofasys_amd import ModalityType, Slot
    case = CASES["tiny_text"]
    slots = [Slot(ModalityType[m], True, (src if src is not None else make_value(spec, V)).to(DEV), attributes=a)
             for m, s, spec, a in case["slots"] if s]
    slots.append(Slot(ModalityType.TEXT, False, torch.zeros(slots[0].value.shape[0], 1, dtype=torch.long, device=DEV)))
    return {"net_input": {"slots": slots}}


def _flat(result):
    return [r if isinstance(r, list) else [r] for r in result]


def test_generate_matches_reference_golden():
    from ofasys_amd.generator import SequenceGenerator
    g = load_golden("beam_search")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(CONFIGS))
    model, d = _model(torch.float32)
    for name, cfg in CONFIGS.items():
        gen = SequenceGenerator(d, **cfg)
        res = _flat(gen.generate(model, _sample(len(d))))
        toks, lens, scores, pos = g[f"{name}.tokens"], g[f"{name}.lens"], g[f"{name}.scores"], g[f"{name}.pos"]
        for b, hyps in enumerate(res):
            assert len(hyps) == int((lens[b] > 0).sum()), (name, b)
            for i, h in enumerate(hyps):
                n = int(lens[b, i])
                assert h.tokens.tolist() == toks[b, i, :n].tolist(), (name, b, i)
                assert abs(float(h.score) - float(scores[b, i])) < 1e-4, (name, b, i)
                assert np.abs(h.positional_scores.numpy() - pos[b, i, :n]).max() < 1e-4, (name, b, i)
                assert h.attention.numel() == 0


def test_generate_max_len_quirk_ignores_source_length():
    """sequence_generator.py:180-182: the text-slot filter never matches, so max_len_a / max_len_b do not shorten the output."""
    from ofasys_amd.generator import SequenceGenerator
    model, d = _model(torch.float32)
    gen = SequenceGenerator(d, beam_size=2, max_len=6, max_len_a=0, max_len_b=1, min_len=6)
    res = _flat(gen.generate(model, _sample(len(d))))
    assert all(h.tokens.numel() == 7 for hyps in res for h in hyps)


# ------------------------------------------------------------------------------------------------ graphs == eager
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_graph_replay_equals_eager(dtype):
    from ofasys_amd.generator import SequenceGenerator
    model, d = _model(dtype)
    V = len(d)
    cfg = dict(beam_size=4, max_len=8, no_repeat_ngram_size=2, return_n_best=4, normalize_scores=True)
    eager, graph = SequenceGenerator(d, use_graph=False, **cfg), SequenceGenerator(d, use_graph=True, **cfg)
    for seed in range(3):                                 # graph generator: eager warm-up, capture, replay
        src = recipe.tokens(f"input.beam_src{seed}", (2, 16), V, [16, 11 + seed])
        a, b = _flat(eager.generate(model, _sample(V, src))), _flat(graph.generate(model, _sample(V, src)))
        for ha, hb in zip(a, b):
            assert len(ha) == len(hb)
            for x, y in zip(ha, hb):
                assert torch.equal(x.tokens, y.tokens) and torch.equal(x.score, y.score)
                assert torch.equal(x.positional_scores, y.positional_scores)
    assert len(graph._dec._graphs) > 0


# ------------------------------------------------------------------------------------------------ Task.inference
def test_task_inference_decodes_text_and_training_continues():
    from ofasys_amd import Task
    from ofasys_amd.trainer import TrainStep
    case = CASES["tiny_text"]
    model, d = build_model(case, DEV, torch.float32)
    task = Task(name="t2t", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    task.initialize(d)
    task.cfg.evaluation.generator_args = '{"beam": 3, "max_len": 6, "no_repeat_ngram_size": 2}'
    vals, target = case_inputs(case)
    sample = {"net_input": {"slots": make_slots(vals, DEV)}}
    out = task.inference(model, sample)
    assert len(out) == 2 and all(isinstance(o.text, str) for o in out)
    assert all(o.tokens[-1] == d.eos() for o in out)
    model.train()
    tr = TrainStep(model, lr=1e-3, clip_norm=1.0)
    stats = tr.train_step([{"slots": make_slots(vals, DEV), "target": target.to(DEV)}])["stats"]
    assert np.isfinite(float(stats[1]))


def test_task_inference_on_the_tasks_own_collated_batch():
    """A batch from task.get_sample(): the collater always adds `prefix_tokens`, [bsz, 0] for a plain target, which the reference
    reads as no prefix -- generation must run on it."""
    from ofasys_amd import Task
    from ofasys_amd.preprocessor import to_device
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    task = Task(name="t2t", instruction="[TEXT:src] what is it? -> [TEXT:tgt]", micro_batch_size=2)
    task.initialize(d)
    task.cfg.evaluation.generator_args = '{"beam": 3, "max_len": 6, "no_repeat_ngram_size": 2}'
    task.add_dataset([{"src": "a small cat sits on the mat", "tgt": "a cat"},
                      {"src": "two dogs run in the park", "tgt": "dogs run"}], "valid")
    batch = to_device(task.get_sample("valid"), DEV)
    assert batch["prefix_tokens"].shape == (2, 0)
    out = task.inference(model, batch)
    assert len(out) == 2
    for o in out:
        assert isinstance(o.text, str) and o.tokens[-1] == d.eos() and 2 <= o.tokens.numel() <= 7
        assert o.text == task.general_preprocess.name2pre["text"].decode(o.tokens)
