"""Generate tests/golden/traverse.npz by RUNNING THE REFERENCE's TraverseTask.inference on the CPU (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_traverse_golden.py
The reference GeneralistModel (`tiny_text` case, recipe weights, eval mode) scores the answer set of tests/traverse_case.py for the
case's two source sentences.  The reference's TraverseTask cannot be initialised here (its text preprocessor downloads the
tokenizer files), so the object is made without __init__ and given exactly what traverse_task.py:26-61 builds -- from token-id
answers, with the reference's own Trie and collate_tokens and valid_batch_size = 5 -- and then the class's own `inference` runs.
`inference` returns only the winning answers; the per-answer scores are recorded by repeating its calls (traverse_task.py:74-107)
on the same modules, and the script asserts that their arg-max is what `inference` returned.  Only data is stored: the answers,
scores [2, C], arg-max, the padded decoder inputs / targets and the allowed-token set of every (answer, position).
It also asserts what the tests rely on: for both sentences best minus second-best score (duplicates counted once) exceeds
10 x the score tolerance, and >= 3 distinct answer lengths occur.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import recipe  # noqa: E402
from oracle.cases import CASES, VOCAB_EXTRA, make_value  # noqa: E402
from oracle.ref_import import build_reference_model, install  # noqa: E402
from tests.traverse_case import ANSWERS, SCORE_TOL, VALID_BATCH_SIZE  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "traverse.npz")


def build_task(d):
    """A reference TraverseTask holding what its initialize() builds (traverse_task.py:26-61), from token-id answers."""
    from ofasys.preprocessor.utils import collate_tokens
    from ofasys.task.traverse_task import TraverseTask
    from ofasys.utils.trie import Trie
    task = TraverseTask.__new__(TraverseTask)
    task.global_dict = d
    trie = Trie(d.eos())
    for a in ANSWERS:
        trie.insert([d.bos()] + list(a) + [d.eos()])
    task.constraint_trie = trie
    task.valid_batch_size = VALID_BATCH_SIZE
    tgt_list, prev_output_list, task.index2ans = [], [], {}
    for i, a in enumerate(ANSWERS):
        item = torch.LongTensor(list(a))
        tgt_list += [torch.cat([item, torch.LongTensor([d.eos()])])]
        prev_output_list += [torch.cat([torch.LongTensor([d.bos()]), item])]
        task.index2ans[i] = i
    mask_list, allowed = [], []
    for prev in prev_output_list:
        mask = torch.zeros((len(prev), len(d))).bool()
        row = []
        for i in range(len(prev)):
            nodes = trie.get_next_layer(prev[: i + 1].tolist())
            mask[i][nodes] = True
            row.append(sorted(nodes))
        mask_list.append(mask)
        allowed.append(row)
    eos, pad = d.eos(), d.pad()
    task.val_tgt_l, task.val_prev_output_l, task.val_cons_masks_l = [], [], []
    for i in range(0, len(tgt_list), VALID_BATCH_SIZE):
        task.val_tgt_l.append(collate_tokens(tgt_list[i:i + VALID_BATCH_SIZE], pad_idx=pad, eos_idx=eos, left_pad=False))
        task.val_prev_output_l.append(collate_tokens(prev_output_list[i:i + VALID_BATCH_SIZE], pad_idx=pad, eos_idx=eos, left_pad=False))
        task.val_cons_masks_l.append(collate_tokens(mask_list[i:i + VALID_BATCH_SIZE], pad_idx=pad, left_pad=False))
    whole = (collate_tokens(prev_output_list, pad_idx=pad, eos_idx=eos, left_pad=False),
             collate_tokens(tgt_list, pad_idx=pad, eos_idx=eos, left_pad=False))
    return task, allowed, whole


def scores_of(task, model, sample):
    """The calls of TraverseTask.inference (traverse_task.py:64-107), keeping the scores it reduces to an arg-max."""
    from ofasys import ModalityType
    from ofasys.preprocessor.instruction import Slot
    model.eval()
    with torch.no_grad():
        slots = sample["net_input"]["slots"]
        src_tokens = [s.value for s in slots if s.modality == ModalityType.TEXT and s.is_src][-1]
        bsz = src_tokens.size(0)
        encoder_out = model.encoder(list(filter(lambda x: x.is_src, slots)))
        result = []
        for val_tgt, val_prev, val_masks in zip(task.val_tgt_l, task.val_prev_output_l, task.val_cons_masks_l):
            n = val_tgt.size(0)
            val_tgt, val_prev, val_masks = val_tgt.repeat(bsz, 1), val_prev.repeat(bsz, 1), val_masks.repeat(bsz, 1, 1)
            enc = {"encoder_out": [encoder_out["encoder_out"][0].repeat_interleave(n, dim=1)],
                   "encoder_padding_mask": [encoder_out["encoder_padding_mask"][0].repeat_interleave(n, dim=0)],
                   "position_embeddings": [encoder_out["position_embeddings"][0].repeat_interleave(n, dim=0)]}
            out = model.decoder([Slot(modality=ModalityType.TEXT, is_src=False, value=val_prev, split="valid")], encoder_out=enc)
            out[0].masked_fill_(~val_masks, -math.inf)
            lprobs = model.get_normalized_probs(out, log_probs=True)
            sc = lprobs.gather(dim=-1, index=val_tgt.unsqueeze(-1)).squeeze(-1)
            sc = sc.masked_fill(val_tgt.eq(task.target_dictionary.pad()), 0).sum(1)
            result.append(sc.view(-1, n))
        return torch.cat(result, dim=-1)


def main():
    install()
    import ofasys  # noqa: F401
    from ofasys import ModalityType
    from ofasys.preprocessor import Slot
    case = CASES["tiny_text"]
    model, d = build_reference_model(case["arch"], VOCAB_EXTRA, case["active"], case["overrides"], case["adaptor_overrides"])
    recipe.fill_state(model.state_dict())
    model.eval()
    V = len(d)
    src = [Slot(ModalityType[m], True, make_value(spec, V), attributes=a) for m, s, spec, a in case["slots"] if s]
    sample = {"net_input": {"slots": src}}
    task, allowed, (prev, tgt) = build_task(d)
    hyps = task.inference(model, sample)                                   # the reference's own method
    scores = scores_of(task, model, sample)
    best = scores.argmax(1).tolist()
    assert hyps == best, (hyps, best)
    # margins: best minus second best, duplicate answers counted once
    first = [ANSWERS.index(a) for a in ANSWERS]
    uniq = sorted(set(first))
    margins = []
    for b in range(scores.shape[0]):
        s = np.sort(scores[b, uniq].numpy().astype(np.float64))[::-1]
        margins.append(float(s[0] - s[1]))
    assert min(margins) > 10 * SCORE_TOL, f"margins {margins}: change the answer set, not the tolerance"
    lengths = sorted(set(len(a) for a in ANSWERS))
    assert len(lengths) >= 3, lengths
    Tmax = prev.shape[1]
    allowed_arr = np.full((len(ANSWERS), Tmax, max(len(r) for row in allowed for r in row)), -1, np.int64)
    for c, row in enumerate(allowed):
        for t, toks in enumerate(row):
            allowed_arr[c, t, :len(toks)] = toks
    answers = np.full((len(ANSWERS), max(lengths)), -1, np.int64)
    for c, a in enumerate(ANSWERS):
        answers[c, :len(a)] = a
    np.savez_compressed(OUT, answers=answers, scores=scores.numpy().astype(np.float32), argmax=np.array(best, np.int64),
                        prev_output_tokens=prev.numpy(), target=tgt.numpy(), allowed=allowed_arr,
                        margins=np.array(margins, np.float64), valid_batch_size=np.array(VALID_BATCH_SIZE))
    print("wrote", OUT, os.path.getsize(OUT), "bytes; argmax", best, "margins", margins, "answer lengths", lengths)
    print("scores", scores.numpy().round(3).tolist())


if __name__ == "__main__":
    main()
