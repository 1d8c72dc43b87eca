"""Self-critical sequence training (SCST, https://arxiv.org/abs/1612.00563): the second stage of caption training, which optimises the
CIDEr-D of the model's OWN captions (reference: engine/criterion/scst_loss.py, metric/pyciderevalcap/ciderD, task/base.py:170-174,
249-253).

    criterion = ScstRewardCriterion(task, task.cfg.criterion)
    micro_batch, log = criterion(model, sample)          # sample: one collated batch on the device
    TrainStep.train_step([micro_batch])                  # a micro-batch with "reward" takes ops.scst_loss

Per batch of B sentences: the task's `scst_generator` produces K hypotheses each (beam search, or K independent samples); hypotheses
and references are decoded to text and scored on the host (`CiderD`); a hypothesis's reward is its score minus the mean score of the
sentence's other K - 1; and the training batch is the B*K hypotheses themselves -- sources repeated K times, the generated tokens as
decoder input and target -- whose token log-probabilities the step weights by the reward (csrc/loss_optim.hip, scst_fwd_grad_kernel).
The scorer stays on the host: it works on strings and dictionaries of n-grams.
"""
import copy
import math
import pickle
import string
from collections import defaultdict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .preprocessor.collate import collate_tokens


# ---------------------------------------------------------------------------------------------------------------- CIDEr-D
def ngram_counts(sentence: str, n: int = 4) -> Dict[Tuple[str, ...], int]:
    """Counts of the 1- to n-grams of the whitespace-split sentence."""
    words = sentence.split()
    counts: Dict[Tuple[str, ...], int] = defaultdict(int)
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            counts[tuple(words[i:i + k])] += 1
    return counts


class CiderD:
    """CIDEr-D (Vedantam et al., https://arxiv.org/abs/1411.5726) as the reference computes it (ciderD_scorer.py:137-216): per n in 1..4
    the tf-idf vectors of hypothesis and reference, their cosine with the hypothesis's weights CLIPPED to the reference's, a Gaussian
    penalty exp(-(delta length)^2 / (2 sigma^2)) with sigma = 6; the mean over n, the mean over the references, times 10.

    df: where the document frequencies come from --
        a path: a pickle of {"ref_len": number of documents, "document_frequency": {n-gram tuple: count}} (the reference's layout),
        a dict of the same two keys, or
        "corpus": counted over the references handed to each `compute_score` call (one document per hypothesis, as the reference).
    An n-gram the table does not hold has document frequency 0, which counts as 1 (idf = log ref_len).

    One quirk of the reference is kept, since its scores are the yardstick: the "length" that enters the penalty is the number of
    BIGRAMS of the sentence (words - 1), not of words -- the difference of two lengths is the same either way, except against a
    one-word sentence."""

    def __init__(self, n: int = 4, sigma: float = 6.0, df="corpus"):
        self.n, self.sigma = n, sigma
        self.corpus = isinstance(df, str) and df == "corpus"
        self.log_ref_len, self.document_frequency = None, None
        if not self.corpus:
            if isinstance(df, dict):
                table = df
            else:
                with open(df, "rb") as f:
                    table = pickle.load(f, encoding="latin1")
            self.log_ref_len = float(np.log(float(table["ref_len"])))
            self.document_frequency = table["document_frequency"]

    def _vector(self, counts, df, log_ref_len):
        vec = [dict() for _ in range(self.n)]
        norm = [0.0] * self.n
        length = 0
        for ngram, tf in counts.items():
            k = len(ngram) - 1
            w = float(tf) * (log_ref_len - float(np.log(max(1.0, df.get(ngram, 0.0)))))
            vec[k][ngram] = w
            norm[k] += w * w
            if k == 1:
                length += tf
        return vec, [float(np.sqrt(x)) for x in norm], length

    def _similarity(self, hyp, ref):
        (vh, nh, lh), (vr, nr, lr) = hyp, ref
        penalty = math.e ** (-(float(lh - lr) ** 2) / (2 * self.sigma ** 2))
        val = np.zeros(self.n)
        for k in range(self.n):
            for ngram, w in vh[k].items():
                r = vr[k].get(ngram, 0.0)
                val[k] += min(w, r) * r
            if nh[k] != 0 and nr[k] != 0:
                val[k] /= nh[k] * nr[k]
            val[k] *= penalty
        return val

    def score_pairs(self, pairs: Sequence[Tuple[str, Sequence[str]]]) -> np.ndarray:
        """pairs: (hypothesis, its references) -> float64 scores, one per pair."""
        cooked = [(ngram_counts(h, self.n), [ngram_counts(r, self.n) for r in refs]) for h, refs in pairs]
        if self.corpus:
            df: Dict = defaultdict(float)
            for _, refs in cooked:
                for ngram in set(g for ref in refs for g in ref):
                    df[ngram] += 1
            log_ref_len = float(np.log(float(len(cooked))))
        else:
            df, log_ref_len = self.document_frequency, self.log_ref_len
        scores = []
        for hyp, refs in cooked:
            assert len(refs) > 0, "CiderD: a hypothesis without a reference"
            h = self._vector(hyp, df, log_ref_len)
            total = np.zeros(self.n)
            for ref in refs:
                total += self._similarity(h, self._vector(ref, df, log_ref_len))
            scores.append(float(np.mean(total)) / len(refs) * 10.0)
        return np.array(scores, dtype=np.float64)

    def compute_score(self, gts, res):
        """The reference's call (ciderD.py:33-58): gts {id: [reference, ...]}, res [{"image_id": id, "caption": [hypothesis]}]
        -> (mean score, scores in the order of res)."""
        pairs = []
        for r in res:
            hypo, refs = r["caption"], gts[r["image_id"]]
            assert isinstance(hypo, list) and len(hypo) == 1 and isinstance(refs, list) and len(refs) > 0
            pairs.append((hypo[0], refs))
        scores = self.score_pairs(pairs)
        return float(np.mean(scores)), scores

    def method(self):
        return "CIDEr-D"


# ---------------------------------------------------------------------------------------------------------------- reward and batch
def self_critical_reward(scores, k: int) -> np.ndarray:
    """scores [B*K], the K hypotheses of a sentence adjacent -> score minus the mean of the sentence's OTHER K - 1 scores
    (scst_loss.py:166-181)."""
    sc = np.asarray(scores, dtype=np.float64).reshape(-1, k)
    baseline = (sc.sum(1, keepdims=True) - sc) / (k - 1)
    return (sc - baseline).reshape(-1)


def hypothesis_batch(hyps: Sequence[torch.Tensor], pad: int, bos: int, pad_to_multiple: int = 1, ignore_prefix_size: int = 0):
    """Generated token lists (each ending in EOS) -> (prev_output_tokens, target), int64 [len(hyps), T]: the target is the hypothesis,
    the decoder input the same tokens moved right behind BOS (scst_loss.py:183-212); both padded to a multiple of `pad_to_multiple`.
    The first `ignore_prefix_size` targets become pad: the loss and its token count then equal the reference's slice (:219-225)."""
    toks = [torch.as_tensor(h).long().reshape(-1).cpu() for h in hyps]
    prev = collate_tokens(toks, pad_idx=pad, eos_idx=bos, left_pad=False, move_eos_to_beginning=True, pad_to_multiple=pad_to_multiple)
    target = collate_tokens(toks, pad_idx=pad, left_pad=False, pad_to_multiple=pad_to_multiple)
    if ignore_prefix_size > 0:
        target[:, :ignore_prefix_size] = pad
    return prev, target


def repeat_sources(slots, k: int, prev: torch.Tensor):
    """The slots of the training batch: every source slot's value repeated K times along the batch (`repeat_interleave`, tensors inside
    dict-valued slots included), the target slot -- there must be exactly one, of TEXT modality -- holding `prev`."""
    def rep(v):
        if torch.is_tensor(v):
            return torch.repeat_interleave(v, k, dim=0)
        if isinstance(v, dict):
            return {key: rep(x) for key, x in v.items()}
        if isinstance(v, (list, tuple)):
            return type(v)(rep(x) for x in v)
        return v
    out, targets = [], 0
    for slot in slots:
        s = copy.copy(slot)
        if slot.is_src:
            s.value = rep(slot.value)
        else:
            if getattr(slot.modality, "name", str(slot.modality)) != "TEXT":
                raise NotImplementedError(f"SCST trains TEXT targets only, got a {slot.modality} target slot")
            s.value = prev
            targets += 1
        out.append(s)
    if targets != 1:
        raise ValueError(f"SCST needs exactly one target slot, the instruction has {targets}")
    return out


class ScstRewardCriterion:
    """The reference's ScstRewardCriterion (engine/criterion/scst_loss.py:59-236) up to the loss itself: `criterion(model, sample)`
    generates, scores, and returns the micro-batch {"slots", "target", "reward": fp32 [B*K], "task"} the step engine trains on, plus
    {"score": summed CIDEr-D, "nsentences", "ntokens"} for logging.  cfg: a task.CriterionConfig -- scst_cider_cached_tokens,
    sentence_avg, ignore_prefix_size, constraint_range ("start,end")."""

    CIDER_REWARD_WEIGHT = 1

    def __init__(self, task, cfg):
        self.task, self.cfg = task, cfg
        self.scorer = CiderD(df=cfg.scst_cider_cached_tokens)
        self.sentence_avg, self.ignore_prefix_size = bool(cfg.sentence_avg), int(cfg.ignore_prefix_size)
        self.transtab = str.maketrans({key: None for key in string.punctuation})
        self.constraint_range: Optional[Tuple[int, int]] = None
        if cfg.constraint_range is not None:
            start, end = str(cfg.constraint_range).strip("()[] ").split(",")
            self.constraint_range = (int(start), int(end))

    # ------------------------------------------------------------------ text
    @property
    def text(self):
        return self.task.general_preprocess.name2pre["text"]

    @staticmethod
    def _wrap_sentence(s: str) -> str:
        """The sentence ends in ' <eos>', as the cached document frequencies were counted (scst_loss.py:130-138)."""
        r = s.strip()
        if r.endswith("."):
            r = r[:-1]
        return r + " <eos>"

    def clean(self, s: str) -> str:
        return self._wrap_sentence(s.strip().translate(self.transtab))

    def references(self, sample) -> List[List[str]]:
        """Per sentence its reference captions: the decoded target, split on '&&' (scst_loss.py:162).  Override to read them from
        elsewhere."""
        pad = self.task.global_dict.pad()
        out = []
        for row in sample["target"].cpu():
            out.append(self.text.decode(row[row.ne(pad)]).strip().split("&&"))
        return out

    def scores(self, gen_res: Sequence[str], gt_res: Sequence[Sequence[str]], k: int) -> np.ndarray:
        """CIDEr-D of every hypothesis against its sentence's references (hypothesis i belongs to sentence i // k)."""
        refs = [[self.clean(r) for r in rs] for rs in gt_res]
        pairs = [(self.clean(h), refs[i // k]) for i, h in enumerate(gen_res)]
        return self.CIDER_REWARD_WEIGHT * self.scorer.score_pairs(pairs)

    # ------------------------------------------------------------------ the batch
    def generate(self, model, sample):
        """-> (K, hypothesis token tensors [B*K], hypothesis strings [B*K]).  The model is left in eval mode (the step engine sets
        train mode itself)."""
        model.eval()
        with torch.no_grad():
            out = self.task.scst_generator.generate(model, sample)
        out = [h if isinstance(h, list) else [h] for h in out]
        k = len(out[0]) if out else 0
        if k < 2 or any(len(h) != k for h in out):
            raise ValueError(f"SCST needs the same number K >= 2 of hypotheses for every sentence, the generator returned "
                             f"{[len(h) for h in out]} (scst_args: a beam of at least 2 with every hypothesis returned; under beam "
                             "search a sentence can finish fewer than `beam` hypotheses within max_len)")
        toks = [h.tokens for hyps in out for h in hyps]
        return k, toks, [self.text.decode(t).strip() for t in toks]

    def __call__(self, model, sample):
        d = self.task.global_dict
        k, toks, gen_res = self.generate(model, sample)
        scores = self.scores(gen_res, self.references(sample), k)
        reward = self_critical_reward(scores, k)
        prev, target = hypothesis_batch(toks, d.pad(), d.bos(), int(getattr(self.task.cfg.text, "pad_to_multiple", 1) or 1),
                                        self.ignore_prefix_size)
        device = sample["target"].device
        mb = {"slots": repeat_sources(sample["net_input"]["slots"], k, prev.to(device)), "target": target.to(device),
              "reward": torch.as_tensor(reward, dtype=torch.float32).to(device), "task": self.task.name}
        if self.sentence_avg:
            mb["sentence_avg"] = True
        if self.constraint_range is not None:
            mb["constraint_range"] = "%d,%d" % self.constraint_range
        log = {"score": float(scores.sum()), "nsentences": len(toks), "ntokens": int(target.ne(d.pad()).sum())}
        return mb, log
