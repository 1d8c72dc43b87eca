"""The sampling golden scenario shared by tools/gen_sampling_golden.py (reference, CPU) and tests/test_sampling_*.py: generator
configurations, and the torch restatement of one sampling step -- kept set, draw, sentence pass -- that both the reference's
recorded steps and the HIP kernels are compared with.  TEST INFRASTRUCTURE.

The draw rule (the project's own): with weights w_c = exp(lprob_c), the kept set S and the row's uniform u in
[0, 1), the draw is the kept token with the smallest id c* such that sum_{c in S, c <= c*} w_c > u * W, W = sum_{c in S} w_c;
if rounding leaves none, the last kept token with non-zero weight; if no kept token has weight, the top-ranked token.
"""
import math

import torch

from tests.beam_case import boost_eos  # noqa: F401  (the same EOS boost as the beam golden)

PAD, UNK, BOS, EOS = 1, 3, 0, 2
DRAW_MARGIN = 1e-3          # u * W stays this far (in units of W) from both ends of the drawn token's CDF interval
TOPP_MARGIN = 1e-4          # the weight ahead of the last kept / first dropped token stays this far from p
RUNS = 2                    # recorded uniform tables per configuration

# "gen": SequenceGenerator keywords; topk / topp: Sampling's
CONFIGS = {
    "plain1": dict(gen=dict(beam_size=1, max_len=10, normalize_scores=False), topk=-1, topp=-1.0),
    "topk5": dict(gen=dict(beam_size=3, max_len=10, no_repeat_ngram_size=2, unk_penalty=0.5, normalize_scores=True, len_penalty=1.0),
                  topk=5, topp=-1.0),
    "topp08": dict(gen=dict(beam_size=4, max_len=10, temperature=0.7, min_len=2, return_n_best=4, normalize_scores=False),
                   topk=-1, topp=0.8),
    "topk8_range": dict(gen=dict(beam_size=3, max_len=9, constraint_range="(4, 120)", return_n_best=3, normalize_scores=False),
                        topk=8, topp=-1.0),
}


# ------------------------------------------------------------------------------------------------ lprobs of a step
def step_lprobs(logits, tokens, step, cfg):
    """The reference's lprobs of a step on CPU tensors (sequence_generator.py:283-343): fp32 log-softmax of x / T under
    constraint_range, then its masks in its order.  cfg: temperature, min_len, max_len, unk_penalty, ngram, constraint_range."""
    rows, V = logits.shape
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
            h = tokens[r, :step + 1].tolist()
            key = h[step + 2 - n:step + 1]
            for i in range(0, step + 2 - n):
                if h[i:i + n - 1] == key:
                    lp[r, h[i + n - 1]] = -math.inf
    return lp


# ------------------------------------------------------------------------------------------------ kept set and draw of one row
def kept_set(lp, topk, topp):
    """lp fp32 [V] -> (kept bool [V], facts).  Ranking: lprob descending, token ascending.  facts: for top-p the weight ahead of
    the last kept and of the first dropped token and the row's total (float64); for top-k the lprobs at the boundary."""
    V = lp.numel()
    w = lp.double().exp()
    order = torch.sort(lp, descending=True, stable=True).indices
    kept = torch.zeros(V, dtype=torch.bool)
    facts = {}
    if topp > 0:
        ws = w[order]
        ahead = ws.cumsum(0) - ws
        n = int((ahead < topp).sum())
        kept[order[:n]] = True
        facts = dict(ahead_last=float(ahead[n - 1]), ahead_next=float(ahead[n]) if n < V else None, total=float(ws.sum()))
    elif 0 < topk < V:
        kept[order[:topk]] = True
        facts = dict(last=float(lp[order[topk - 1]]), next=float(lp[order[topk]]))
    else:
        kept[:] = True
    return kept, facts


def topp_margin_ok(facts, topp, margin=TOPP_MARGIN):
    """The top-p boundary is decided by more than `margin`: the whole row is below p, or the weights ahead of the last kept and of
    the first dropped token lie on their sides of p by it."""
    if facts["total"] < topp - margin:
        return True
    return (facts["ahead_last"] < topp - margin and facts["ahead_next"] is not None and facts["ahead_next"] >= topp + margin)


def topk_margin_ok(facts):
    """No tie at the top-k boundary (equal -inf on both sides weighs nothing and is no tie that matters)."""
    return not facts or facts["last"] != facts["next"] or facts["last"] == -math.inf


def draw(lp, kept, u):
    """-> (token, margin): the draw of the rule above in float64, and how far u * W is from the nearer end of the drawn token's
    CDF interval, in units of W (inf when the row has no weight: the top-ranked token is drawn whatever u)."""
    w = torch.where(kept, lp.double().exp(), torch.zeros((), dtype=torch.float64))
    W = float(w.sum())
    if not W > 0:
        return int(torch.sort(lp, descending=True, stable=True).indices[0]), math.inf
    cdf = w.cumsum(0)
    t = float(u) * W
    hit = ((cdf > t) & (w > 0)).nonzero()
    c = int(hit[0]) if hit.numel() else int((w > 0).nonzero()[-1])
    lo, hi = float(cdf[c] - w[c]), float(cdf[c])
    return c, min(t - lo, hi - t) / W


def draw_rows(lp, K, step, topk, topp, uniforms, done=None):
    """The row pass restated: lp [rows, V], uniforms [rows] -> (tok int64 [rows], lprob fp32 [rows], worst draw margin, facts per
    row).  At step 0 every row reads its sentence's first row.  Rows of done sentences: token -1, lprob NaN."""
    rows = lp.shape[0]
    tok = torch.full((rows,), -1, dtype=torch.long)
    out = torch.full((rows,), math.nan)
    worst, facts = math.inf, []
    for r in range(rows):
        if done is not None and done[r // K]:
            facts.append(None)
            continue
        row = lp[(r // K) * K if step == 0 else r]
        kept, f = kept_set(row, topk, topp)
        c, m = draw(row, kept, float(uniforms[r]))
        tok[r], out[r] = c, row[c]
        worst = min(worst, m)
        facts.append(dict(f, kept=int(kept.sum())))
    return tok, out, worst, facts


def uniform_for(lp, kept, c):
    """The midpoint of token c's CDF interval, as a float32 uniform (c kept, with weight)."""
    w = torch.where(kept, lp.double().exp(), torch.zeros((), dtype=torch.float64))
    cdf = w.cumsum(0)
    return float(torch.tensor((float(cdf[c]) - 0.5 * float(w[c])) / float(w.sum()), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ sentence pass
def select_step(st, tok, lprob, K, step, cfg):
    """The generator's bookkeeping for a K-wide candidate list (sequence_generator.py:345-492, finalize_hypos :530-627): slot j's
    candidate is its own draw (parent 0 at step 0).  st: tokens, scores, ignore [bsz, K], done, nfin, reorder, fin_tok, fin_pos,
    fin_score, fin_len, fin_cnt (CPU tensors); cfg: max_len, normalize, len_penalty.  Returns the new state."""
    st = {k: v.clone() for k, v in st.items()}
    bsz = st["done"].numel()
    for s in range(bsz):
        if st["done"][s]:
            continue
        r0 = s * K
        lp = lprob[r0:r0 + K].float()
        csc = lp + st["scores"][r0:r0 + K, step - 1] if step > 0 else lp.clone()
        cidx = tok[r0:r0 + K]
        cbeam = torch.zeros(K, dtype=torch.long) if step == 0 else torch.arange(K)
        ign = st["ignore"][s].bool()
        eos_mask = (cidx == EOS) & (csc != -math.inf) & ~ign
        cnt = int(st["fin_cnt"][s])
        for j in range(K):
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
        em = ign | eos_mask
        active_mask = em.long() * (2 * K) + torch.arange(K)
        new_ign, active = torch.sort(active_mask, stable=True)          # (= topk(k=K, largest=False) of K distinct values)
        st["ignore"][s] = new_ign.ge(2 * K).int()
        src = r0 + cbeam[active]
        st["tokens"][r0:r0 + K, :step + 1] = st["tokens"][src, :step + 1]
        st["tokens"][r0:r0 + K, step + 1] = cidx[active]
        if step > 0:
            st["scores"][r0:r0 + K, :step] = st["scores"][src, :step]
        st["scores"][r0:r0 + K, step] = csc[active]
        st["reorder"][r0:r0 + K] = src
    return st


def empty_state(bsz, K, cap):
    rows = bsz * K
    tokens = torch.full((rows, cap), PAD, dtype=torch.long)
    tokens[:, 0] = BOS
    i32 = torch.int32
    return {"tokens": tokens, "scores": torch.zeros(rows, cap), "ignore": torch.zeros(bsz, K, dtype=i32),
            "done": torch.zeros(bsz, dtype=i32), "nfin": torch.zeros(1, dtype=i32), "reorder": torch.arange(rows),
            "fin_tok": torch.zeros(bsz, K, cap, dtype=torch.long), "fin_pos": torch.zeros(bsz, K, cap),
            "fin_score": torch.zeros(bsz, K), "fin_len": torch.zeros(bsz, K, dtype=i32), "fin_cnt": torch.zeros(bsz, dtype=i32)}


def hypotheses(st, n_best):
    """The generator's output order from a final state: per sentence the finalised hypotheses, best score first (stable)."""
    out = []
    for s in range(st["done"].numel()):
        n = int(st["fin_cnt"][s])
        order = torch.sort(st["fin_score"][s, :n], descending=True).indices[:n_best]
        out.append([(st["fin_tok"][s, i, :int(st["fin_len"][s, i])], float(st["fin_score"][s, i]),
                     st["fin_pos"][s, i, :int(st["fin_len"][s, i])]) for i in order.tolist()])
    return out
