"""GPU: sampling generation (csrc/sample.hip, SequenceGenerator(search_strategy=Sampling(...)), Task.sampling_generator).

1. The row pass (ofa_sample_draw) against the torch restatement of tests/sampling_case.py: token exact, lprob to the step
   tolerance of test_beam_search_gpu.py.  Uniforms are built, not drawn blind: midpoints of chosen tokens' CDF intervals plus
   random ones that keep the draw margin in float64; the top-p / top-k margin conditions are asserted on the inputs first.
2. The sentence pass (ofa_sample_select) over scripted draws against the restated bookkeeping.
3. generate(uniforms=U) on the fp32 HIP `tiny_text` model against tests/golden/sampling.npz (the reference's generator on the CPU
   with the same draw rule), eagerly and through the captured step graphs; seeds; Task.inference.
"""
import json
import math

import numpy as np
import pytest
import torch

from oracle.cases import CASES, make_value
from tests import sampling_case as sc
from tests.golden_util import case_inputs, load_golden
from tests.model_util import build_model, make_slots
from tests.sampling_case import BOS, CONFIGS, EOS, PAD, RUNS, boost_eos

DEV = "cuda"
RTOL, ATOL = 1e-5, 2e-5                                     # the step tolerance of test_beam_search_gpu.py

# ------------------------------------------------------------------------------------------------ inputs of the row pass
# A row is a few heavy tokens over a light tail, so that every threshold the modes look for falls between heavy tokens and a
# chosen token's CDF interval is wide enough for the draw margin.  Probabilities (before the masks) of the heavy tokens:
HEAVY = (0.34, 0.24, 0.17, 0.09, 0.10, 0.025)               # dealt to ids 5, ~4095, ~4096, V - 1, 100, 70
P_EOS, P_PAD, P_TAIL = 0.015, 0.01, 0.01
TEMPERATURE = 0.8
LADDER = 260                                                # the tail's largest values are distinct in every dtype: no top-k 256 tie
MODES = [("plain", -1, -1.0), ("topk1", 1, -1.0), ("topk5", 5, -1.0), ("topk256", 256, -1.0), ("topkV3", None, -1.0),
         ("topp_one", -1, 0.2), ("topp09", -1, 0.9), ("topp1", -1, 1.0)]
WHENS = ("first", "mid", "max_len", "nan_done")


def heavy_ids(V):
    return [5, min(4095, V - 3), min(4096, V - 2), V - 1, 100, 70]


def make_logits(V, rows, g, ban_row0):
    """fp32 [rows, V]: logits whose softmax at TEMPERATURE is the heavy / tail split above.  Row 0 of a `mid` step holds 0.09 at
    token 70, which its history bans; elsewhere 70 is the light one and the rest is dealt at random, so rows differ."""
    x = torch.empty(rows, V)
    ids = heavy_ids(V)
    for r in range(rows):
        tail = -0.1 - torch.randn(V, generator=g).abs()
        n = min(LADDER, V - 16)
        at = torch.randperm(V, generator=g)[:n]
        tail[at] = 4.0 - torch.arange(n) / 64.0             # multiples of 1/64 up to 4: exact in bf16 and fp16
        mask = torch.ones(V, dtype=torch.bool)
        mask[ids + [EOS, PAD]] = False
        lse_tail = torch.logsumexp(tail[mask].double(), 0)
        perm = torch.randperm(5, generator=g).tolist()
        frac = [HEAVY[i] for i in perm] + [HEAVY[5]]
        if ban_row0 and r == 0:
            j = frac.index(0.09)
            frac[j], frac[5] = frac[5], frac[j]
        row = tail.clone()
        for i, f in zip(ids + [EOS, PAD], frac + [P_EOS, P_PAD]):
            row[i] = float(lse_tail + math.log(f / P_TAIL))
        x[r] = row * TEMPERATURE
    return x


def build_case(V, K, when, dtype, seed):
    """(logits in dtype on the CPU with ld > V, tokens, done, step, cfg, lprobs restated from the rounded logits)."""
    g = torch.Generator().manual_seed(seed)
    bsz, rows, cap = 2, 2 * K, 8
    step = {"first": 0, "mid": 5, "max_len": 6, "nan_done": 5}[when]
    cfg = dict(temperature=TEMPERATURE, min_len=6, max_len=6, unk_penalty=0.3, ngram=3, constraint_range=None)
    buf = torch.zeros(rows, V + 24)
    buf[:, :V] = make_logits(V, rows, g, ban_row0=when == "mid")
    tokens = torch.full((rows, cap), PAD, dtype=torch.long)
    tokens[:, 0] = BOS
    if step > 0:
        tokens[:, 1:step + 1] = torch.randint(110, 140, (rows, step), generator=g)     # (no heavy token in a history)
    if when == "mid":
        tokens[0, :step + 1] = torch.tensor([50, 60, 70, 11, 50, 60])                 # ... 50 60 -> 70 banned in row 0
    done = torch.zeros(bsz, dtype=torch.int32)
    if when == "nan_done":
        buf[K - 1, 9] = float("nan")
        done[1] = 1
    logits = buf.to(dtype)
    lp = sc.step_lprobs(logits[:, :V].float(), tokens, step, cfg)
    return logits, tokens, done, step, cfg, lp


def build_uniforms(lp, K, step, topk, topp, done, g):
    """One uniform per row: midpoints of the first / last heavy kept token and of ids 4095 / 4096 / V - 1 when kept, in turn, then
    random numbers that keep the draw margin.  Also asserts the mode's margin conditions on the rows."""
    rows, V = lp.shape
    u = torch.zeros(rows)
    for r in range(rows):
        if done[r // K]:
            continue
        row = lp[(r // K) * K if step == 0 else r]
        kept, facts = sc.kept_set(row, topk, topp)
        if topp > 0:
            assert sc.topp_margin_ok(facts, topp), (r, facts)
        else:
            assert sc.topk_margin_ok(facts), (r, facts)
        w = torch.where(kept, row.double().exp(), torch.zeros((), dtype=torch.float64))
        W = float(w.sum())
        if not W > 0:
            continue                                         # no weight: the top-ranked token whatever u
        wide = (w >= 2.5 * sc.DRAW_MARGIN * W).nonzero().flatten().tolist()
        targets = [wide[0], wide[-1]] + [c for c in (min(4095, V - 3), min(4096, V - 2), V - 1) if c in wide]
        choice = r + step
        if choice % 8 < len(targets):
            u[r] = sc.uniform_for(row, kept, targets[choice % 8])
            assert sc.draw(row, kept, float(u[r]))[0] == targets[choice % 8]
        else:
            for _ in range(64):
                u[r] = torch.rand((), generator=g)
                if sc.draw(row, kept, float(u[r]))[1] >= sc.DRAW_MARGIN:
                    break
        assert sc.draw(row, kept, float(u[r]))[1] >= sc.DRAW_MARGIN, (r, float(u[r]))
    return u


def run_draw(logits, V, K, step, cfg, tokens, done, u, topk, topp):
    from ofasys_amd import kernels as Kn
    rows = logits.shape[0]
    ws = torch.full((Kn.sample_ws_bytes(rows, V, K) // 4,), -7.0, device=DEV)
    dev = logits.to(DEV)[:, :V]
    assert dev.stride(0) > V
    Kn.sample_draw(dev, K, step, ws, u.to(DEV), topk=topk, topp=topp, tokens=tokens.to(DEV), done=done.to(DEV),
                   temperature=cfg["temperature"], constraint_range=cfg["constraint_range"], min_len=cfg["min_len"],
                   max_len=cfg["max_len"], pad=PAD, unk=sc.UNK, eos=EOS, unk_penalty=cfg["unk_penalty"], ngram=cfg["ngram"])
    torch.cuda.synchronize()
    return ws.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("V", [204, 4097, 59457])
def test_row_pass_matches_restatement(dtype, K, V):
    rows = 2 * K
    for wi, when in enumerate(WHENS):
        logits, tokens, done, step, cfg, lp = build_case(V, K, when, dtype, seed=V * 31 + K * 7 + wi)
        g = torch.Generator().manual_seed(wi + 99)
        for name, topk, topp in MODES:
            topk = V + 3 if topk is None else topk
            u = build_uniforms(lp, K, step, topk, topp, done, g)
            tok, lpd, worst, _ = sc.draw_rows(lp, K, step, topk, topp, u, done)
            ws = run_draw(logits, V, K, step, cfg, tokens, done, u, topk, topp)
            again = run_draw(logits, V, K, step, cfg, tokens, done, u, topk, topp)
            assert torch.equal(ws.view(torch.int32), again.view(torch.int32)), (when, name)          # identical bytes
            got_lp, got_tok = ws[:rows], ws[rows:].view(torch.int32).long()
            live = ~done.bool().repeat_interleave(K)
            assert torch.equal(got_tok[live], tok[live]), (when, name, got_tok, tok, u)
            assert torch.equal(torch.isinf(got_lp[live]), torch.isinf(lpd[live])), (when, name)
            fin = live & torch.isfinite(lpd)
            assert torch.allclose(got_lp[fin], lpd[fin], rtol=RTOL, atol=ATOL), (when, name, got_lp, lpd)
            # a finished sentence's entries are left alone
            assert bool((ws[:rows][~live] == -7.0).all()) and bool((ws[rows:][~live] == -7.0).all()), (when, name)
            if when == "max_len":
                assert bool((got_tok == EOS).all())
            if when == "mid" and name in ("plain", "topp09", "topp1"):
                assert int(sc.kept_set(lp[0], topk, topp)[0].sum()) == V and lp[0, 70] == -math.inf      # the ban opened the set
            if name == "topk1":                                      # the arg-max whatever u says
                for uu in (0.0, 0.5, 0.99999994):
                    w1 = run_draw(logits, V, K, step, cfg, tokens, done, torch.full((rows,), uu), 1, -1.0)
                    src = lp if step > 0 else lp[(torch.arange(rows) // K) * K]
                    assert torch.equal(w1[rows:].view(torch.int32).long()[live], src.argmax(-1)[live]), (when, uu)


@pytest.mark.gpu
def test_row_pass_constraint_range_and_unk_penalty():
    """constraint_range changes the normaliser; the unk penalty is part of the weight and of the score."""
    V, K, step = 4097, 3, 2
    g = torch.Generator().manual_seed(5)
    logits, tokens, done, _, cfg, _ = build_case(V, K, "mid", torch.float32, seed=77)
    logits[:, sc.UNK] = logits[:, 5]                                      # unk as heavy as token 5
    cfg = dict(cfg, constraint_range=(10, 4096), min_len=0, ngram=0, unk_penalty=0.7)
    lp = sc.step_lprobs(logits[:, :V].float(), tokens, step, cfg)
    assert bool(torch.isinf(lp[:, 4:10]).all()) and bool(torch.isinf(lp[:, 4096]).all()) and bool(torch.isfinite(lp[:, sc.UNK]).all())
    u = torch.zeros(2 * K)
    for r in range(2 * K):
        kept, _ = sc.kept_set(lp[r], 8, -1.0)
        assert bool(kept[sc.UNK])
        u[r] = sc.uniform_for(lp[r], kept, sc.UNK if r % 2 == 0 else int(kept.nonzero()[-1]))
    tok, lpd, worst, _ = sc.draw_rows(lp, K, step, 8, -1.0, u)
    assert worst >= sc.DRAW_MARGIN and bool((tok[::2] == sc.UNK).all())
    ws = run_draw(logits, V, K, step, cfg, tokens, done, u, 8, -1.0)
    assert torch.equal(ws[2 * K:].view(torch.int32).long(), tok)
    assert torch.allclose(ws[:2 * K], lpd, rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["topk", "topp"])
def test_row_pass_breaks_a_boundary_tie_towards_the_lower_token(mode):
    """The ranking is (lprob descending, token ascending): of two tokens with the same logit at the boundary of the kept set the
    lower id is kept.  The 5th-ranked token of every row gets a twin at id 3000 -- above some rows' token, below others'."""
    V, K, twin = 4097, 3, 3000
    logits, tokens, done, step, cfg, lp = build_case(V, K, "first", torch.float32, seed=7)
    rows = 2 * K
    fifth = torch.sort(lp, descending=True, stable=True).indices[:, 4]
    for r in range(rows):
        logits[r, twin] = logits[r, fifth[r]]
    lp = sc.step_lprobs(logits[:, :V].float(), tokens, step, cfg)
    assert bool((lp[torch.arange(rows), fifth] == lp[:, twin]).all())
    assert int(fifth[0]) > twin > int(fifth[K])                       # (step 0 reads rows 0 and K: one case each)
    u, want = torch.zeros(rows), []
    topk, topp = (5, -1.0) if mode == "topk" else (-1, None)
    for r in range(rows):
        row = lp[(r // K) * K]
        low = min(int(fifth[(r // K) * K]), twin)
        if mode == "topp":                                           # p halfway into the first twin's weight: the second is dropped
            order = torch.sort(row, descending=True, stable=True).indices
            ahead = float(row.double().exp()[order[:4]].sum())
            topp = float(torch.tensor(ahead + 0.5 * float(row[low].double().exp()), dtype=torch.float32))
        kept, facts = sc.kept_set(row, topk, topp)
        assert int(kept.sum()) == 5 and bool(kept[low]) and not bool(kept[max(int(fifth[(r // K) * K]), twin)])
        if mode == "topp":
            assert sc.topp_margin_ok(facts, topp)
        u[r] = sc.uniform_for(row, kept, low)
        assert sc.draw(row, kept, float(u[r])) == (low, sc.draw(row, kept, float(u[r]))[1]) and sc.draw(row, kept, float(u[r]))[1] >= sc.DRAW_MARGIN
        want.append(low)
        if mode == "topp":                                           # (p differs per sentence: one call per row's p)
            ws = run_draw(logits, V, K, step, cfg, tokens, done, u, topk, topp)
            assert int(ws[rows:].view(torch.int32)[r]) == low, (r, ws[rows:].view(torch.int32), low)
    if mode == "topk":
        ws = run_draw(logits, V, K, step, cfg, tokens, done, u, topk, topp)
        assert ws[rows:].view(torch.int32).tolist() == want
        assert torch.allclose(ws[:rows], lp[(torch.arange(rows) // K) * K, torch.tensor(want)], rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------------ the sentence pass
def compare_state(got, want, where):
    for name in ("tokens", "reorder", "ignore", "done", "nfin", "fin_cnt", "fin_len", "fin_tok"):
        assert torch.equal(got[name], want[name]), (where, name, got[name], want[name])
    for name in ("scores", "fin_score", "fin_pos"):
        a, b = got[name], want[name]
        assert torch.equal(torch.isinf(a), torch.isinf(b)), (where, name)
        fin = torch.isfinite(b)
        assert torch.allclose(a[fin], b[fin], rtol=RTOL, atol=ATOL), (where, name, float((a[fin] - b[fin]).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [False, True])
def test_sentence_pass_matches_restated_bookkeeping(normalize):
    """Scripted draws, K = 3, four sentences, max_len 4: slots ending at different steps (compaction, non-identity reorder), an
    ignored slot that draws EOS, all K ending in one step, an EOS at -inf, and sentences that run into max_len."""
    from ofasys_amd import kernels as Kn
    K, bsz, max_len = 3, 4, 4
    E = EOS
    script = [   # per step: tokens [bsz][K] in the slot order of that step
        [[7, E, 9], [10, 11, 12], [20, 21, 22], [E, 30, E]],
        [[E, 13, E], [E, E, E], [23, 24, 25], [31, E, 32]],
        [[14, E, 15], [1, 1, 1], [26, E, 27], [33, 34, E]],
        [[16, 17, E], [1, 1, 1], [28, 29, 40], [E, 35, 36]],
        [[E, E, E], [1, 1, 1], [E, E, 41], [1, 1, 1]],
    ]
    g = torch.Generator().manual_seed(3)
    cfg = dict(max_len=max_len, normalize=normalize, len_penalty=1.3)
    want = sc.empty_state(bsz, K, max_len + 2)
    dev = {k: v.to(DEV) for k, v in want.items()}
    seen_reorder = False
    for step, toks in enumerate(script):
        tok = torch.tensor(toks).view(-1)
        lp = -torch.rand(bsz * K, generator=g) * 3 - 0.01
        if step == 4:
            lp[2 * K] = -math.inf                                          # an EOS at -inf is not finalised
        ws = torch.cat([lp, tok.to(torch.int32).view(torch.float32)]).to(DEV)
        Kn.sample_select(ws, dev, K, step, max_len, eos=EOS, normalize=normalize, len_penalty=cfg["len_penalty"])
        torch.cuda.synchronize()
        want = sc.select_step(want, tok, lp, K, step, cfg)
        compare_state({k: v.cpu() for k, v in dev.items()}, want, step)
        seen_reorder |= not torch.equal(want["reorder"], torch.arange(bsz * K))
    assert seen_reorder and bool(want["done"].all()) and int(want["nfin"]) == bsz
    assert want["fin_cnt"].tolist() == [3, 3, 2, 3] and bool(want["ignore"][0].any())


@pytest.mark.gpu
def test_beam_and_sampling_sentence_passes_share_their_bookkeeping():
    """The same K (score, beam, token) candidates through sample_select (scripted draws) and through beam_select (a hand-built
    workspace, V = 8: one normaliser part per row) leave the same state, bit for bit: bsz 2, K 3, max_len 3, steps 0 .. 3.
    Step 0 reads beam 0 only (the beam workspace lists the K candidates in row 0's list, sampling gives every slot parent 0);
    sentence 0 finalises an EOS at step 0, so one of its slots is ignored from step 1 on -- where it draws an EOS that must not be
    finalised -- and at step 2 its first slot ends, so the reorder is no identity; sentence 1 draws an EOS at -inf at step 1, which
    is not finalised and goes on at -inf; step 3 = max_len finishes both.  Every candidate list descends in slot order, as the
    beam pass's merge sorts it; the values are multiples of 1/8 and every row's normaliser is exactly 2 (max 2, sum 1), so both
    routes hold identical floats before the shared bookkeeping starts."""
    from ofasys_amd import kernels as Kn
    K, bsz, V, max_len, E, NI = 3, 2, 8, 3, EOS, -math.inf
    rows, K2, LSE = bsz * K, 2 * K, 2.0
    script = [   # per step: (tokens, lprobs) [bsz][K] in the slot order of that step
        ([[5, E, 6], [7, 4, 6]], [[-0.25, -0.5, -1.0], [-0.125, -0.375, -0.75]]),
        ([[4, 5, E], [5, 6, E]], [[-0.25, -0.5, -2.0], [-0.25, -0.25, NI]]),
        ([[E, 7, 4], [4, 5, 6]], [[-0.25, -0.25, -0.5], [-0.5, -0.5, -0.5]]),
        ([[E, E, E], [E, E, E]], [[-0.125, -1.5, -0.5], [-0.125, -0.125, -0.125]]),
    ]
    cfg = dict(max_len=max_len, normalize=True, len_penalty=1.3)
    want = sc.empty_state(bsz, K, max_len + 2)
    samp = {k: v.to(DEV) for k, v in want.items()}
    beam = {k: v.to(DEV) for k, v in want.items()}
    assert Kn.beam_ws_bytes(rows, V, K) == rows * (2 + 2 * K2) * 4
    for step, (toks, lps) in enumerate(script):
        tok, lp = torch.tensor(toks).view(-1), torch.tensor(lps).view(-1)
        cum = lp + want["scores"][:, step - 1] if step > 0 else lp
        assert bool((cum.view(bsz, K)[:, :-1] >= cum.view(bsz, K)[:, 1:]).all()), step      # the order the beam merge would give
        # ---- sampling: the draws as sample_draw leaves them
        sws = torch.cat([lp, tok.to(torch.int32).view(torch.float32)]).to(DEV)
        Kn.sample_select(sws, samp, K, step, max_len, eos=E, normalize=True, len_penalty=cfg["len_penalty"])
        # ---- beam: stats [rows, 1, 2], values [rows, 1, 2K], tokens [rows, 1, 2K] (-1: none); value = lprob + normaliser
        stats = torch.tensor([LSE, 1.0]).repeat(rows, 1)
        cval, ctok = torch.full((rows, K2), NI), torch.full((rows, K2), -1, dtype=torch.int32)
        if step == 0:                                          # one row is read: its list holds the sentence's K candidates
            cval.view(bsz, K, K2)[:, 0, :K], ctok.view(bsz, K, K2)[:, 0, :K] = (lp + LSE).view(bsz, K), tok.to(torch.int32).view(bsz, K)
        else:                                                  # one candidate per row: beam j continues as slot j
            cval[:, 0], ctok[:, 0] = lp + LSE, tok.to(torch.int32)
        bws = torch.cat([stats.view(-1), cval.view(-1), ctok.view(-1).view(torch.float32)]).to(DEV)
        Kn.beam_select(bws, beam, K, V, step, max_len, eos=E, unk=sc.UNK, unk_penalty=0.0, normalize=True, len_penalty=cfg["len_penalty"])
        torch.cuda.synchronize()
        for name in want:
            a, b = samp[name].cpu(), beam[name].cpu()
            same = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
            assert same, (step, name, a, b)
        want = sc.select_step(want, tok, lp, K, step, cfg)
        compare_state({k: v.cpu() for k, v in samp.items()}, want, step)
        if step == 0:
            assert want["ignore"].tolist() == [[0, 0, 1], [0, 0, 0]] and want["fin_cnt"].tolist() == [1, 0]
            assert want["reorder"].tolist() == [0, 0, 0, 3, 3, 3]                            # every slot continues beam 0
        if step == 1:                                          # neither the ignored slot's EOS nor the EOS at -inf is finalised
            assert want["fin_cnt"].tolist() == [1, 0] and want["scores"][5, 1] == NI and want["tokens"][5, 2] == E
        if step == 2:
            assert want["reorder"].tolist() == [1, 0, 2, 3, 4, 5] and want["ignore"].tolist() == [[0, 1, 1], [0, 0, 0]]
    assert want["done"].tolist() == [1, 1] and int(want["nfin"]) == 2 and want["fin_cnt"].tolist() == [3, 2]


# ------------------------------------------------------------------------------------------------ generate() against the reference
def _model(dtype=torch.float32):
    model, d = build_model(CASES["tiny_text"], DEV, dtype)
    with torch.no_grad():
        boost_eos(model.state_dict()["decoder.adaptor.embed_tokens.weight"], d.eos())
    model.eval()
    return model, d


def _sample(V):
    from ofasys_amd import ModalityType, Slot
    case = CASES["tiny_text"]
    slots = [Slot(ModalityType[m], True, make_value(spec, V).to(DEV), attributes=a) for m, s, spec, a in case["slots"] if s]
    slots.append(Slot(ModalityType.TEXT, False, torch.zeros(slots[0].value.shape[0], 1, dtype=torch.long, device=DEV)))
    return {"net_input": {"slots": slots}}


def _flat(result):
    return [r if isinstance(r, list) else [r] for r in result]


def _check_golden(res, g, key):
    toks, lens, scores, pos = g[f"{key}.tokens"], g[f"{key}.lens"], g[f"{key}.scores"], g[f"{key}.pos"]
    for b, hyps in enumerate(_flat(res)):
        assert len(hyps) == int((lens[b] > 0).sum()), (key, b)
        for i, h in enumerate(hyps):
            n = int(lens[b, i])
            assert h.tokens.tolist() == toks[b, i, :n].tolist(), (key, b, i)
            assert abs(float(h.score) - float(scores[b, i])) < 1e-4, (key, b, i)
            assert np.abs(h.positional_scores.numpy() - pos[b, i, :n]).max() < 1e-4, (key, b, i)


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_generate_matches_reference_golden(use_graph):
    from ofasys_amd import Sampling
    from ofasys_amd.generator import SequenceGenerator
    g = load_golden("sampling")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(CONFIGS)) and RUNS == 2
    model, d = _model()
    for name, cfg in CONFIGS.items():
        gen = SequenceGenerator(d, search_strategy=Sampling(d, cfg["topk"], cfg["topp"]), use_graph=use_graph, **cfg["gen"])
        # graphed: an eager warm-up, the capture, then replays -- every table read from the same fixed address
        for run in (0, 1, 0, 1):
            U = torch.from_numpy(g[f"{name}.{run}.uniforms"]).to(DEV)
            _check_golden(gen.generate(model, _sample(len(d)), uniforms=U), g, f"{name}.{run}")
        assert (len(gen._dec._graphs) > 0) == use_graph


@pytest.mark.gpu
def test_seeds_repeat_and_differ():
    from ofasys_amd import Sampling
    from ofasys_amd.generator import SequenceGenerator
    model, d = _model()
    cfg = dict(beam_size=4, max_len=8, min_len=3, normalize_scores=False)

    def tokens_of(seed):
        gen = SequenceGenerator(d, search_strategy=Sampling(d), seed=seed, **cfg)
        first = [[h.tokens.tolist() for h in hyps] for hyps in _flat(gen.generate(model, _sample(len(d))))]
        second = [[h.tokens.tolist() for h in hyps] for hyps in _flat(gen.generate(model, _sample(len(d))))]
        return first, second
    a, a2 = tokens_of(5)
    b, _ = tokens_of(5)
    c, _ = tokens_of(6)
    assert a == b and a != c
    assert a != a2                                             # one generator draws on from call to call
    assert all(len(hyps) == 4 for hyps in a)


@pytest.mark.gpu
def test_task_inference_samples_through_sampling_generator():
    from ofasys_amd import Task
    case = CASES["tiny_text"]
    model, d = build_model(case, DEV, torch.float32)
    task = Task(name="t2t", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    task.initialize(d)
    task.generator = task.sampling_generator(sampling=True, sampling_topp=0.9, beam=5, return_n_best=5, max_len=6, seed=1)
    vals, _ = case_inputs(case)
    out = task.inference(model, {"net_input": {"slots": make_slots(vals, DEV)}})
    assert len(out) == 2
    for hyps in out:
        assert len(hyps) == 5
        for h in hyps:
            assert isinstance(h.text, str) and h.tokens[-1] == d.eos() and 1 <= h.tokens.numel() <= 7
            assert abs(float(h.positional_scores.sum()) - float(h.score)) < 1e-4
    again = task.sampling_generator(sampling=True, sampling_topp=0.9, beam=5, return_n_best=5, max_len=6, seed=1)
    assert again is task.generator
