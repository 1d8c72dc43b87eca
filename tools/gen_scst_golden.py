"""Generate tests/golden/scst.npz by RUNNING THE REFERENCE's SCST criterion pieces on the CPU (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_scst_golden.py
What runs is the reference's own code, on toy inputs:
  * metric/pyciderevalcap/ciderD `CiderD` with a pickled toy document-frequency table (its pickle layout: ref_len, document_frequency),
    and once more in "corpus" mode;
  * ScstRewardCriterion.get_reward_and_scores (through _calculate_eval_scores / _wrap_sentence) -> scores and rewards;
  * ScstRewardCriterion.get_net_output -> the repeated source slot and the prev_output_tokens / target collation of the hypotheses;
  * get_lprobs_and_target + scst_loss on one [6, 5, V] fp32 logits tensor with a constraint range -> loss, ntokens and, by autograd,
    d loss / d logits; and the same with ignore_prefix_size = 1.
The criterion object is made without its constructor (which downloads the COCO table); its task and model are stand-ins that hold
only what these methods read.  Only data is stored: strings, token lists, numbers.
"""
import json
import os
import pickle
import string
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import install  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "scst.npz")
PAD, BOS, EOS = 1, 0, 2
B, K, V = 2, 3, 100
CRANGE = (10, 90)

# hypotheses (token ids incl. EOS) per sentence, and references, in the stand-in tokenizer's '<id>' words
HYP_TOKENS = [[14, 15, 16, 17, EOS], [14, 15, 33, EOS], [40, 41, EOS],
              [50, 51, 52, 53, EOS], [50, 51, 60, 61, EOS], [70, EOS]]
REFS = [["<14> <15> <16> <17> .", "<14> <15> <33> <17> <18>"], ["<50> <51> <52> <53>", "<50> , <51> <60> <53> .", "<80> <81>"]]


def words(tokens):
    return " ".join(f"<{t}>" for t in tokens if t not in (BOS, EOS))


def toy_df():
    """Document frequencies over a made-up corpus of 40 documents: every n-gram of the references and of some hypotheses gets a count
    below ref_len; the rest stay absent (document frequency 0)."""
    from ofasys.metric.pyciderevalcap.ciderD.ciderD_scorer import precook
    trans = str.maketrans({k: None for k in string.punctuation})
    df = {}
    rng = np.random.default_rng(7)
    sents = [r for rs in REFS for r in rs] + [words(HYP_TOKENS[0]), words(HYP_TOKENS[4])]
    for s in sents:
        for ngram in precook(s.translate(trans) + " <eos>"):
            df[ngram] = float(rng.integers(1, 30))
    return {"ref_len": 40, "document_frequency": df}


def main():
    install()
    from ofasys.engine.criterion import scst_loss as ref
    from ofasys.metric.pyciderevalcap.ciderD.ciderD import CiderD

    table = toy_df()
    # (the reference looks absent n-grams up with [], so the table it reads must be a defaultdict; the fixture stores the plain entries)
    import collections
    with tempfile.NamedTemporaryFile(suffix=".p", delete=False) as f:
        pickle.dump({"ref_len": table["ref_len"],
                     "document_frequency": collections.defaultdict(float, table["document_frequency"])}, f)
        path = f.name

    crit = object.__new__(ref.ScstRewardCriterion)
    crit.transtab = str.maketrans({key: None for key in string.punctuation})
    crit.padding_idx = PAD
    crit.constraint_start, crit.constraint_end = CRANGE
    crit.ignore_prefix_size = 0
    crit.task = types.SimpleNamespace(tgt_dict=types.SimpleNamespace(eos=lambda: EOS, bos=lambda: BOS, pad=lambda: PAD))
    gen_res = [words(t) for t in HYP_TOKENS]

    out = {}
    for mode, df in (("table", path), ("corpus", "corpus")):
        crit.scst_cider_scorer = CiderD(df=df)
        reward, scores = crit.get_reward_and_scores(gen_res, REFS, device="cpu")
        out[f"{mode}.scores"] = np.asarray(scores, dtype=np.float64)
        out[f"{mode}.reward"] = reward.numpy().astype(np.float64)
    os.unlink(path)

    # collation of the hypotheses (get_net_output), with a stand-in model that records what it is called with
    src = torch.arange(B * 4).view(B, 4) + 4
    slots = [types.SimpleNamespace(is_src=True, value=src.clone(), modality=types.SimpleNamespace(value=1)),
             types.SimpleNamespace(is_src=False, value=torch.zeros(B, 1, dtype=torch.long), modality=types.SimpleNamespace(value=1))]
    sample = {"target": torch.full((B, 3), 5), "net_input": {"slots": slots}}
    seen = {}

    class Model:
        def train(self):
            pass

        def __call__(self, slots):
            seen["src"], seen["prev"] = slots[0].value.clone(), slots[1].value.clone()
            return ("net_output",)

    gen_target = [torch.tensor(t, dtype=torch.int32) for t in HYP_TOKENS]
    _, target = crit.get_net_output(Model(), sample, gen_target)
    out["src"], out["src_repeated"] = src.numpy(), seen["src"].numpy()
    out["prev"], out["target"] = seen["prev"].numpy(), target.numpy()

    # the loss on one logits tensor, rewards of the table mode
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(B * K, target.shape[1], V, generator=g) * 2).float()
    reward = torch.from_numpy(out["table.reward"])

    def get_normalized_probs(net, log_probs):             # model/ofa.py:287-299: fp32 log-softmax, tagged batch-first
        lp = torch.log_softmax(net[0].float(), dim=-1)
        lp.batch_first = True
        return lp
    model = types.SimpleNamespace(get_normalized_probs=get_normalized_probs)
    out["logits"] = logits.numpy()
    for prefix in (0, 1):
        crit.ignore_prefix_size = prefix
        x = logits.clone().requires_grad_(True)
        net = [x * 1.0]                                   # (the reference writes -inf into the output in place)
        lprobs, tgt = crit.get_lprobs_and_target(model, net, target.clone())
        loss, ntokens = ref.scst_loss(lprobs, tgt, reward, ignore_index=PAD, reduce=True)
        loss.backward()
        out[f"loss.{prefix}"] = np.float64(loss.item())
        out[f"ntokens.{prefix}"] = np.int64(int(ntokens))
        out[f"dlogits.{prefix}"] = x.grad.numpy().astype(np.float32)
    out["meta"] = np.array(json.dumps({
        "pad": PAD, "bos": BOS, "eos": EOS, "B": B, "K": K, "V": V, "crange": list(CRANGE), "hyp_tokens": HYP_TOKENS,
        "gen_res": gen_res, "refs": REFS, "ref_len": table["ref_len"],
        "document_frequency": [[list(k), v] for k, v in table["document_frequency"].items()]}))
    assert table["ref_len"] > max(table["document_frequency"].values())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; scores {out['table.scores']}, loss {out['loss.0']}, ntokens {out['ntokens.0']}")


if __name__ == "__main__":
    main()
