"""Beam search under a forced target prefix: the torch restatement of one step of the reference (generator/sequence_generator.py
:283-492 with `_prefix_tokens` :497-523, finalize_hypos :530-627, utils/search.py:107-142) taken literally, except that ties are
broken by the project's rule (value descending, then beam * V + token ascending) where torch.topk leaves them open; and the
golden scenario shared by tools/gen_beam_prefix_golden.py (reference, CPU) and tests/test_beam_prefix_*.py.  TEST INFRASTRUCTURE."""
import math

import torch

PAD, UNK, BOS, EOS = 1, 3, 0, 2

# generator configurations and the forced prefixes (token ids of the tiny_text dictionary, <pad> where a sentence's prefix has ended)
# Beam 5 under the tie rule: at step 0 only the first beam counts, so K - 1 of the active beams are tie tokens at f, and <eos>
# (id 2) at f is among the first K candidates -- a hypothesis of <eos> alone takes one of the K finalised slots.
# The beam-5 configurations therefore flatten the distribution (the beams off the prefix, >= 1 below, die at the first free
# step), keep the free steps from finalising early (min_len) and return fewer than K hypotheses, so that what is returned does
# not depend on the order of ties: tools/gen_beam_prefix_golden.py asserts it by running the reference under both orders.
CONFIGS = {
    "beam1_w1": dict(gen=dict(beam_size=1, max_len=8, normalize_scores=False), prefix=[[17], [33]]),
    "beam1_w3": dict(gen=dict(beam_size=1, max_len=8, temperature=4.0, normalize_scores=False), prefix=[[17, 60, 9], [33, 8, 121]]),
    "beam5_w1": dict(gen=dict(beam_size=5, max_len=8, min_len=6, temperature=4.0, return_n_best=4, normalize_scores=True),
                     prefix=[[17], [33]]),
    "beam5_w3": dict(gen=dict(beam_size=5, max_len=8, min_len=8, temperature=8.0, return_n_best=2, normalize_scores=True),
                     prefix=[[17, 60, 9], [33, 8, 121]]),
    "beam5_ragged": dict(gen=dict(beam_size=5, max_len=8, min_len=8, temperature=8.0, return_n_best=2, normalize_scores=True),
                         prefix=[[17, 60, 9], [33, PAD, PAD]]),
    "beam5_ngram": dict(gen=dict(beam_size=5, max_len=8, min_len=8, temperature=8.0, no_repeat_ngram_size=2, unk_penalty=0.5,
                                 return_n_best=2, normalize_scores=True), prefix=[[17, 60, 17], [33, PAD, PAD]]),
}
LPROBS_OF = "beam1_w1"            # the configuration whose step-0 lprobs (after log_softmax) the fixture records


def prefix_lprobs(logits, st, K, step, cfg, prefix_col=None, plen=None):
    """The lprobs the reference hands to search.step.  prefix_col [bsz] long: column `step` of prefix_tokens when this is a prefix
    step (step < width and step < max_len), else None; plen [bsz]: prefix lengths (None: the sample has no prefix_tokens)."""
    x = logits.float() / cfg["temperature"]
    if cfg.get("constraint_range") is not None:
        cs, ce = cfg["constraint_range"]
        x[:, 4:cs] = -math.inf
        x[:, ce:] = -math.inf
    return mask_lprobs(torch.log_softmax(x, -1), st, K, step, cfg, prefix_col, plen)


def mask_lprobs(lp, st, K, step, cfg, prefix_col=None, plen=None):
    """sequence_generator.py:296-343 on the log-softmax output `lp` (changed in place and returned)."""
    rows = lp.shape[0]
    live = (st["done"] == 0).repeat_interleave(K)             # the reference has removed the finished sentences
    if prefix_col is not None:
        tok = prefix_col.repeat_interleave(K)
        g = lp.gather(1, tok.unsqueeze(1)).squeeze(1)
        f = torch.min(g[live]) - 1                            # (NaN wins in torch.min)
        for r in range(rows):
            if live[r] and tok[r] != PAD:
                lp[r] = f
                lp[r, tok[r]] = g[r]
    elif step < cfg["min_len"]:
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
            if plen is not None and not int(plen[r // K]) < step + n - 1:
                continue
            h = st["tokens"][r, :step + 1].tolist()
            key = h[step + 2 - n:step + 1]
            for i in range(0, step + 2 - n):
                if h[i:i + n - 1] == key:
                    lp[r, h[i + n - 1]] = -math.inf
    return lp


def select(lp, st, K, step, cfg):
    """search.step and the bookkeeping of one step on the masked lprobs: returns the new state dict."""
    st = {k: v.clone() for k, v in st.items()}
    rows, V = lp.shape
    for s in range(rows // K):
        if st["done"][s]:
            continue
        r0 = s * K
        lps = lp[r0:r0 + K]
        cand = lps[:1] if step == 0 else lps + st["scores"][r0:r0 + K, step - 1].unsqueeze(-1)
        flat = cand.reshape(-1)
        k = min(2 * K, flat.numel() - 1)
        order = torch.sort(flat, descending=True, stable=True).indices[:k]      # value descending, flat index ascending
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


def ref_prefix_step(logits, st, K, step, cfg, prefix=None, plen=None):
    """One step on CPU tensors.  prefix [bsz, W] long or None; the step is a prefix step when step < W and step < max_len."""
    forced = prefix is not None and step < prefix.shape[1] and step < cfg["max_len"]
    lp = prefix_lprobs(logits, st, K, step, cfg, prefix[:, step] if forced else None, plen)
    return select(lp, st, K, step, cfg)
