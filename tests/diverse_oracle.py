"""A plain-torch restatement of diverse decoding, written for this project's tests.  TEST INFRASTRUCTURE.

`group_step` / `sibling_step` restate utils/search.py:549-593 / :738-787 as FULL-VOCABULARY steps: the penalties are applied to
[K, V] lprobs and every selection is a sort of everything under this project's tie rule (value descending, then
beam * V + token ascending) -- no use of the top-2K shortcut the kernels rely on.  `ref_step` puts either in front of the
bookkeeping of one generator step (generator/sequence_generator.py:283-492, finalize_hypos :530-627) on a state dict, as
tests/test_beam_search_gpu.py does for plain beam search.

gaps: if a list is passed, every selection appends the smallest difference between neighbouring FINITE scores among its picks and
the first candidate it left out -- the margin by which fp32 rounding could change the outcome.
"""
import math

import torch

PAD, UNK, BOS, EOS = 1, 3, 0, 2


def _topk(flat, key, k, gaps=None):
    """Indices of the k best of `flat` [n]: score descending, ties to the lower `key` (int64 [n], unique)."""
    by_key = torch.sort(key, stable=True).indices
    order = by_key[torch.sort(flat[by_key], descending=True, stable=True).indices]
    if gaps is not None:
        s = flat[order[:k + 1]]
        s = s[torch.isfinite(s)].double()
        if s.numel() > 1:
            gaps.append(float((s[:-1] - s[1:]).min()))
    return order[:k]


def beam_step(step, lprobs, scores, gaps=None):
    """BeamSearch.step for one sentence: lprobs [R, V], scores [R, >= step] -> (scores, tokens, rows) of the top min(2R, n - 1)."""
    R, V = lprobs.shape
    lp = lprobs[:1] if step == 0 else lprobs + scores[:, step - 1].unsqueeze(-1)
    flat = lp.reshape(-1)
    idx = _topk(flat, torch.arange(flat.numel()), min(2 * R, flat.numel() - 1), gaps)
    return flat[idx], idx % V, idx // V


def group_step(step, lprobs, scores, G, strength, gaps=None):
    """DiverseBeamSearch.step: lprobs [bsz, K, V], scores [bsz, K, >= step] -> (scores, tokens, beams) [bsz, G * k], interleaved."""
    bsz, K, V = lprobs.shape
    if K % G != 0:
        raise ValueError("DiverseBeamSearch requires --beam to be divisible by the number of groups")
    out = []
    for b in range(bsz):
        count = torch.zeros(V)
        sc_g, tok_g, beam_g = [], [], []
        for g in range(G):
            lp = lprobs[b, g::G]
            if g > 0:
                lp = lp + (count * -float(strength)).unsqueeze(0)
            s, t, r = beam_step(step, lp, scores[b, g::G] if step > 0 else None, gaps)
            sc_g.append(s)
            tok_g.append(t)
            beam_g.append(r * G + g)
            count.scatter_add_(0, t, torch.ones(t.numel()))
        out.append([torch.stack(x, 1).reshape(-1) for x in (sc_g, tok_g, beam_g)])
    return tuple(torch.stack([o[i] for o in out]) for i in range(3))


def sibling_step(step, lprobs, scores, rate, gaps=None):
    """DiverseSiblingsSearch.step: lprobs [bsz, K, V], scores [bsz, K, >= step] -> (scores, tokens, beams) [bsz, k]."""
    bsz, K, V = lprobs.shape
    k = min(2 * K, K * V - 1)
    out = []
    for b in range(bsz):
        if step == 0:
            out.append(beam_step(0, lprobs[b], None, gaps))
            continue
        lp = lprobs[b] + scores[b, :, step - 1].unsqueeze(-1)
        penalty = torch.arange(1, k + 1).to(lp) * float(rate)
        s_all, key_all, tok_all = [], [], []
        for i in range(K):
            idx = _topk(lp[i], torch.arange(V), k)          # (needs V >= k: the reference's per-beam topk raises otherwise)
            s_all.append(lp[i][idx] - penalty)
            tok_all.append(idx)
            key_all.append(i * V + idx)
        s_all, key_all, tok_all = torch.cat(s_all), torch.cat(key_all), torch.cat(tok_all)
        pick = _topk(s_all, key_all, k, gaps)
        out.append((s_all[pick], tok_all[pick], key_all[pick] // V))
    return tuple(torch.stack([o[i] for o in out]) for i in range(3))


def masked_lprobs(logits, tokens, step, cfg):
    """What the generator hands its search strategy: log-softmax of logits / T under constraint_range, then the masks in the
    reference's order (sequence_generator.py:296-343).  logits [rows, V] fp32; tokens [rows, >= step + 1] the history."""
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


def sentence_step(st, s, csc, cidx, cbeam, K, step, cfg):
    """The bookkeeping of one step for sentence s over its candidate list (scores, tokens, beams; any order the strategy gives):
    in place on the state dict."""
    r0, k = s * K, csc.numel()
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
        return
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


def ref_step(logits, st, K, step, cfg, strategy, gaps=None):
    """One generator step on CPU tensors under strategy = ("groups", G, strength) or ("siblings", rate): the new state dict.
    Sentences with done = 1 are skipped (the reference removes them from the batch; rows are independent)."""
    st = {k: v.clone() for k, v in st.items()}
    rows, V = logits.shape
    bsz = rows // K
    lp = masked_lprobs(logits, st["tokens"], step, cfg).view(bsz, K, V)
    sc = st["scores"].view(bsz, K, -1)
    for s in range(bsz):
        if st["done"][s]:
            continue
        if strategy[0] == "groups":
            csc, cidx, cbeam = group_step(step, lp[s:s + 1], sc[s:s + 1], strategy[1], strategy[2], gaps)
        else:
            csc, cidx, cbeam = sibling_step(step, lp[s:s + 1], sc[s:s + 1], strategy[1], gaps)
        sentence_step(st, s, csc[0], cidx[0], cbeam[0], K, step, cfg)
    return st
