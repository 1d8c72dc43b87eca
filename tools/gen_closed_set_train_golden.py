"""Generate tests/golden/closed_set_train.npz by RUNNING THE REFERENCE's label_smoothed_nll_loss on the CPU (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_closed_set_train_golden.py
The closed set is tests/traverse_case.ANSWERS over the 204-symbol test dictionary.  Every answer is one target row [a_1 .. a_n, eos,
<pad> ...] of Tmax = 5 positions; the logits [14, 5, 204] are recipe values.  The constraint masks come from the reference's own Trie
(get_next_layer of the prefix, as preprocessor/default/text.py builds sample["constraint_masks"]) and are prepared exactly as the
criterion's get_constraint_masks / get_lprobs_and_target / compute_loss do (label_smoothed_cross_entropy.py:147-191): AND with the
constraint range, masked_fill(-inf), fp32 log_softmax, rows with target == <pad> removed; then the reference's label_smoothed_nll_loss
and autograd.  Settings: eps 0 and 0.1, without and with a constraint range [4, 100) that removes children of several nodes (134 and
188 at the root, 120 and 150 deeper); with the range, the targets it would remove are set to <pad>, so no live target leaves the
allowed set.  Only data is stored: logits, nodes (the project's numbering: traverse.TraversePlan.walk, each node's children checked
here against the reference Trie's next layer), and per setting target, loss, nll_loss, ntokens and the fp32 logits gradient.
Every recorded loss is asserted finite.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import recipe  # noqa: E402
from oracle.ref_import import install  # noqa: E402
from tests.traverse_case import ANSWERS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "closed_set_train.npz")
V, BOS, PAD, EOS = 204, 0, 1, 2
RANGE = (4, 100)
SETTINGS = [("eps0", 0.0, None), ("eps01", 0.1, None), ("eps0_range", 0.0, RANGE), ("eps01_range", 0.1, RANGE)]


def main():
    install()
    from ofasys.engine.criterion.label_smoothed_cross_entropy import label_smoothed_nll_loss
    from ofasys.utils.trie import Trie
    from ofasys_amd.traverse import TraversePlan
    trie = Trie(EOS)
    for a in ANSWERS:
        trie.insert([BOS] + list(a) + [EOS])
    plan = TraversePlan(ANSWERS, BOS, EOS, PAD)
    C, T = len(ANSWERS), max(len(a) for a in ANSWERS) + 1
    target = torch.full((C, T), PAD, dtype=torch.int64)
    nodes = np.full((C, T), -1, np.int32)
    masks = torch.ones(C, T, V, dtype=torch.bool)            # (<pad> positions: collate_tokens pads the mask rows with pad_idx = 1)
    for c, a in enumerate(ANSWERS):
        target[c, :len(a) + 1] = torch.tensor(list(a) + [EOS])
        walk = plan.walk(a)
        for i in range(len(a) + 1):
            allowed = trie.get_next_layer([BOS] + list(a[:i]))
            masks[c, i] = False
            masks[c, i, allowed] = True
            n = int(walk[i])
            assert sorted(plan.edge_token[plan.node_edge_off[n]:plan.node_edge_off[n + 1]].tolist()) == sorted(allowed), (c, i)
            nodes[c, i] = n
    logits = recipe.floats("closed_set_train.logits", (C, T, V), 2.0)
    out = {"logits": logits.numpy(), "nodes": nodes, "pad": np.array([PAD]), "answers_rows": np.array([C, T])}
    for name, eps, crange in SETTINGS:
        tg = target.clone()
        cm = masks.clone()
        if crange is not None:
            inside = (tg < 4) | ((tg >= crange[0]) & (tg < crange[1]))
            tg = torch.where(inside, tg, torch.full_like(tg, PAD))
            rm = torch.ones(C, T, V, dtype=torch.bool)       # get_constraint_masks (:147-156)
            rm[..., 4:crange[0]] = 0
            rm[..., crange[1]:] = 0
            cm = torch.logical_and(cm, rm)
            cut = (masks & ~rm)[tg != PAD].any(-1)
            assert int(cut.sum()) >= 3, "the range must remove children of live rows"
        x = logits.clone().requires_grad_(True)
        xin = x.masked_fill(~cm, -math.inf)                  # get_lprobs_and_target (:158-173)
        lprobs = torch.log_softmax(xin.float(), dim=-1).view(-1, V)
        t1, cm1 = tg.view(-1), cm.reshape(-1, V)
        keep = t1 != PAD                                     # compute_loss (:175-191)
        loss, nll, ntok = label_smoothed_nll_loss(lprobs[keep], t1[keep], eps, update_num=0, constraint_masks=cm1[keep])
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(nll)), (name, loss, nll)
        loss.backward()
        assert bool(torch.isfinite(x.grad).all()), name
        assert 0 < int((~keep).sum()) and int(ntok) == int(keep.sum())
        out.update({f"{name}.target": tg.numpy(), f"{name}.loss": loss.detach().numpy().reshape(1),
                    f"{name}.nll_loss": nll.detach().numpy().reshape(1), f"{name}.ntokens": np.array([ntok]),
                    f"{name}.dlogits": x.grad.numpy(),
                    f"{name}.cfg": np.array([eps, -1 if crange is None else crange[0], -1 if crange is None else crange[1]])})
        print(name, "loss", float(loss.detach()), "nll", float(nll.detach()), "ntokens", ntok, "pad positions", int((~keep).sum()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
