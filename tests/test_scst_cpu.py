"""CPU: self-critical sequence training off the device -- the CIDEr-D scorer, the reward and the hypothesis batch against what the
reference's own code produced (tests/golden/scst.npz, written by tools/gen_scst_golden.py); the criterion's host logic with a stand-in
generator; the surface (TaskConfig / CriterionConfig / Task.scst_generator); the argument checks of ofa_scst_loss_fwd_grad through its
status codes; and the float64 oracle of the kernels (tests/scst_oracle.py): sound, able to see the mutations it exists for, and in
agreement with the reference's loss and autograd gradient on the golden logits."""
import json
import pickle
import types

import numpy as np
import pytest
import torch

from tests import criterion_oracle as co
from tests import scst_oracle as so
from tests.golden_util import load_golden


@pytest.fixture(scope="module")
def G():
    g = load_golden("scst")
    g["meta"] = json.loads(str(g["meta"]))
    return g


def _table(meta):
    return {"ref_len": meta["ref_len"], "document_frequency": {tuple(k): v for k, v in meta["document_frequency"]}}


def _criterion(meta, df, **cfg):
    from ofasys_amd import Dictionary, Task
    from ofasys_amd.scst import ScstRewardCriterion
    from ofasys_amd.task import CriterionConfig
    task = Task(name="caption", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    task.initialize(Dictionary())
    return ScstRewardCriterion(task, CriterionConfig(name="scst_reward_criterion", scst_cider_cached_tokens=df, **cfg)), task


# ------------------------------------------------------------------------------------------------ scorer, reward, batch
def test_cider_d_matches_the_reference_scores(G, tmp_path):
    """Both sides are float64 and the scores lie in 0..10: only the order of a few sums can differ -- 1e-9 absolute."""
    from ofasys_amd.scst import CiderD
    meta = G["meta"]
    path = tmp_path / "df.p"
    with open(path, "wb") as f:
        pickle.dump(_table(meta), f)
    for df, key in ((_table(meta), "table"), (str(path), "table"), ("corpus", "corpus")):
        crit, _ = _criterion(meta, df)
        got = crit.scores(meta["gen_res"], meta["refs"], meta["K"])
        assert got.dtype == np.float64 and np.abs(got - G[f"{key}.scores"]).max() <= 1e-9, (key, got, G[f"{key}.scores"])
    # the reference's own call shape
    scorer = CiderD(df=_table(meta))
    gts = {i: [crit.clean(r) for r in meta["refs"][i // meta["K"]]] for i in range(len(meta["gen_res"]))}
    res = [{"image_id": i, "caption": [crit.clean(h)]} for i, h in enumerate(meta["gen_res"])]
    mean, scores = scorer.compute_score(gts, res)
    assert np.abs(scores - G["table.scores"]).max() <= 1e-9 and abs(mean - G["table.scores"].mean()) <= 1e-9
    assert scores.max() > 3 and scores.min() < 1 and scorer.method() == "CIDEr-D"          # the fixture spans good and bad captions


def test_reward_is_score_minus_the_mean_of_the_others(G):
    from ofasys_amd.scst import self_critical_reward
    for key in ("table", "corpus"):
        got = self_critical_reward(G[f"{key}.scores"], G["meta"]["K"])
        assert np.abs(got - G[f"{key}.reward"]).max() <= 1e-9
        assert np.abs(got.reshape(-1, G["meta"]["K"]).sum(1)).max() < 1e-9                 # a sentence's rewards sum to zero


def test_hypothesis_batch_and_repeated_slots_are_bit_exact(G):
    from ofasys_amd import ModalityType, Slot
    from ofasys_amd.scst import hypothesis_batch, repeat_sources
    meta = G["meta"]
    hyps = [torch.tensor(t) for t in meta["hyp_tokens"]]
    prev, target = hypothesis_batch(hyps, meta["pad"], meta["bos"])
    assert prev.dtype == target.dtype == torch.int64
    assert np.array_equal(prev.numpy(), G["prev"]) and np.array_equal(target.numpy(), G["target"])
    slots = [Slot(ModalityType.TEXT, True, torch.from_numpy(G["src"])),
             Slot(ModalityType.TEXT, False, torch.zeros(meta["B"], 1, dtype=torch.long))]
    out = repeat_sources(slots, meta["K"], prev)
    assert np.array_equal(out[0].value.numpy(), G["src_repeated"]) and out[1].value is prev
    assert slots[0].value.shape[0] == meta["B"]                                             # the sample's own slots are left alone
    # padded to a multiple, and the ignored prefix
    prev8, target8 = hypothesis_batch(hyps, meta["pad"], meta["bos"], pad_to_multiple=8, ignore_prefix_size=1)
    assert prev8.shape == target8.shape == (6, 8) and bool((target8[:, 0] == meta["pad"]).all())
    assert torch.equal(prev8[:, :5], prev) and torch.equal(target8[:, 1:5], target[:, 1:]) and bool((target8[:, 5:] == meta["pad"]).all())
    with pytest.raises(ValueError, match="one target slot"):
        repeat_sources(slots[:1], 3, prev)
    with pytest.raises(NotImplementedError, match="TEXT"):
        repeat_sources([slots[0], Slot(ModalityType.IMAGE, False, torch.zeros(2, 3))], 3, prev)


class _FakeGenerator:
    def __init__(self, hyps, k):
        self.hyps, self.k = hyps, k

    def generate(self, model, sample):
        return [[types.SimpleNamespace(tokens=torch.tensor(t)) for t in self.hyps[b * self.k:(b + 1) * self.k]]
                for b in range(len(self.hyps) // self.k)]


def test_criterion_builds_the_micro_batch(G):
    """Generation replaced by the golden hypotheses: the micro-batch holds the repeated sources, the hypotheses as decoder input and
    target, and the rewards of the decoded strings (the stand-in tokenizer renders token i as '<i - 4>': a consistent renaming of the
    fixture's words, so corpus-mode scores are the fixture's)."""
    from ofasys_amd import ModalityType, Slot
    meta = G["meta"]
    crit, task = _criterion(meta, "corpus", sentence_avg=True, constraint_range="10,90")
    task.cfg.text.pad_to_multiple = 4
    import re
    from ofasys_amd.scst import ScstRewardCriterion
    assert task.global_dict.get_start_end_idx("<text>")[0] == 4
    refs = [[re.sub(r"<(\d+)>", lambda m: f"<{int(m.group(1)) - 4}>", r) for r in rs] for rs in meta["refs"]]

    class Crit(ScstRewardCriterion):
        def references(self, sample):
            return refs
    crit.__class__ = Crit
    model = types.SimpleNamespace(eval=lambda: None)
    sample = {"net_input": {"slots": [Slot(ModalityType.TEXT, True, torch.from_numpy(G["src"])),
                                      Slot(ModalityType.TEXT, False, torch.zeros(2, 1, dtype=torch.long))]},
              "target": torch.full((2, 3), 7)}
    task._scst_generator = _FakeGenerator(meta["hyp_tokens"], meta["K"])
    mb, log = crit(model, sample)
    assert set(mb) == {"slots", "target", "reward", "task", "sentence_avg", "constraint_range"} and mb["constraint_range"] == "10,90"
    assert mb["reward"].dtype == torch.float32 and mb["reward"].shape == (6,) and mb["task"] == "caption"
    assert np.abs(mb["reward"].double().numpy() - G["corpus.reward"]).max() < 1e-6 and abs(log["score"] - G["corpus.scores"].sum()) < 1e-9
    assert mb["target"].shape == (6, 8) and torch.equal(mb["target"][:, :5], torch.from_numpy(G["target"]))
    assert torch.equal(mb["slots"][1].value[:, :5], torch.from_numpy(G["prev"])) and mb["slots"][0].value.shape == (6, 4)
    assert log["nsentences"] == 6 and log["ntokens"] == int(G["ntokens.0"])
    # the references of the default method: the decoded target, split on '&&'
    assert ScstRewardCriterion.references(crit, {"target": torch.tensor([[14, 15, 2, 1]])}) == [["<10> <11>"]]
    # K must be the same for every sentence, and at least 2
    task._scst_generator = _FakeGenerator(meta["hyp_tokens"][:5], 3)
    task._scst_generator.generate = lambda m, s: [[types.SimpleNamespace(tokens=torch.tensor([5, 2]))] * 3,
                                                  [types.SimpleNamespace(tokens=torch.tensor([5, 2]))] * 2]
    with pytest.raises(ValueError, match="K >= 2"):
        crit(model, sample)
    task._scst_generator.generate = lambda m, s: [types.SimpleNamespace(tokens=torch.tensor([5, 2]))] * 2
    with pytest.raises(ValueError, match="K >= 2"):
        crit(model, sample)


def test_surface_options():
    from ofasys_amd import CiderD, Dictionary, ScstRewardCriterion, Task, TaskConfig  # noqa: F401
    from ofasys_amd.task import CriterionConfig
    c = CriterionConfig()
    assert (c.name, c.label_smoothing, c.drop_worst_ratio) == ("label_smoothed_cross_entropy", 0.0, 0.0)        # defaults unchanged
    assert (c.sentence_avg, c.ignore_prefix_size, c.constraint_range) == (False, 0, None) and c.scst_cider_cached_tokens == "corpus"
    cfg = TaskConfig()
    assert cfg.scst is False and cfg.scst_args == "{}"
    cfg.scst, cfg.scst_args = True, '{"beam": 3, "max_len": 6, "min_len": 1}'
    task = Task(cfg, name="caption", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    task.initialize(Dictionary())
    gen = task.scst_generator
    assert gen.beam_size == 3 and gen.return_n_best == 3 and gen.sampling is None and task.scst_generator is gen
    cfg2 = TaskConfig()
    cfg2.scst_args = '{"sampling": true, "sampling_topk": 5, "beam": 4, "max_len": 6, "seed": 3}'
    task2 = Task(cfg2, name="caption", instruction="[TEXT:src] what is it? -> [TEXT:tgt]")
    task2.initialize(Dictionary())
    gen2 = task2.scst_generator
    assert gen2.sampling is not None and gen2.sampling.sampling_topk == 5 and gen2.return_n_best == 4 and gen2.seed == 3


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_refuses_bad_arguments():
    from ofasys_amd import lib as L
    h = L.lib()
    assert "ofa_scst_loss_fwd_grad" in h.protos
    #        logits target reward row_seq rps gs lse row_loss dlogits rows nseq V ld ignore cs ce dtype stream
    good = [1, 1, 1, None, 3, None, 1, 1, 1, 12, 4, 204, 208, 1, -1, -1, L.BF16, None]

    def refused(match, **change):
        names = ["logits", "target", "reward", "row_seq", "rps", "gs", "lse", "row_loss", "dlogits", "rows", "nseq", "V", "ld", "ignore",
                 "cs", "ce", "dtype", "stream"]
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        with pytest.raises(L.OfaError, match=match):
            h.call("ofa_scst_loss_fwd_grad", *args)
    refused("dtype", dtype=7)
    refused("vector width", ld=204)                       # 16-bit: a multiple of 8
    refused("vector width", ld=206, dtype=L.F32)          # fp32: a multiple of 4
    refused("bad argument", ld=200)                       # ld < V
    refused("constraint range", cs=3, ce=100)             # a range may not start inside [0, 4)
    refused("constraint range", cs=50, ce=50)
    refused("constraint range", cs=50, ce=205)            # past V
    for name in ("logits", "target", "reward", "lse", "row_loss", "dlogits"):
        refused("bad argument", **{name: None})
    refused("rows_per_seq", rps=0)
    refused("bad argument", nseq=0)
    refused("bad argument", rows=-1)
    args = list(good)
    args[9] = 0
    h.call("ofa_scst_loss_fwd_grad", *args)               # rows == 0: nothing to do, status 0


# ------------------------------------------------------------------------------------------------ the kernels' oracle
def _outputs_differ(got, ref, bd, dtype, g, reward, seq):
    """Does any of the three outputs miss the tolerance the GPU test holds the kernels to?"""
    e = co.excess(got["d"], ref["d"], bd, co.EPS.get(dtype, 1.0), co.floor_of(dtype, g * max(abs(r) for r in so.REWARDS)))
    if e > (co.G32_TOL if dtype == torch.float32 else co.TOL):
        return True
    if float((got["lse"].double() - ref["lse"]).abs().max()) > co.LSE_TOL:
        return True
    fin = torch.isfinite(ref["row_loss"])
    w = reward.double()[seq].abs().clamp_min(1.0)
    if not torch.equal(torch.isfinite(got["row_loss"]), fin):
        return True
    return bool((((got["row_loss"].double() - ref["row_loss"])[fin]).abs() > co.ROW_TOL * w[fin]).any())


SMALL = [c for c in so.CASES16 if c.V <= 8200]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_oracle_emulation_sits_inside_the_ceiling(dtype):
    """The fp32 emulation of either form against the float64 reference: 16-bit gradients within CEILING eps of the bound (one rounding),
    lse and row_loss within an eighth of their tolerances -- the tolerances' own derivation (criterion_oracle.py), which must hold on
    this table too.  fp32 gradients: G32_TOL / 8 is the cross-entropy emulation's measured error, (p - onehot) g; this one multiplies
    by the rounded product w g instead of g, two more roundings of at most 2^-24 each relative to the bound: G32_TOL / 8 + 2^-23."""
    cases = so.CASES32 if dtype == torch.float32 else SMALL + so.CASES16[-2:] + so.CASES_STREAM16[:2]
    worst = 0.0
    for case in cases:
        b = so.build(case, dtype)
        g = 1.0 if b["g"] is None else b["g"]
        ref, bd = so.scst_reference(b["x"], b["t"], b["reward"], b["seq"], g, case.crange)
        got = so.scst_emulate(b["x"], b["t"], b["reward"], b["seq"], g, dtype, so.registers_form(dtype, case.ld), case.crange)
        e = co.excess(got["d"], ref["d"], bd, co.EPS.get(dtype, 1.0), co.floor_of(dtype, g * 1.5))
        worst = max(worst, e)
        assert e <= (co.G32_TOL / 8 + 2.0 ** -23 if dtype == torch.float32 else co.CEILING), (case, e)
        assert float((got["lse"].double() - ref["lse"]).abs().max()) <= co.LSE_TOL / 8, case
        assert float(got["row_loss"][so.IGNORED_ROW]) == 0.0 and float(ref["row_loss"][so.IGNORED_ROW]) == 0.0
        assert not _outputs_differ(got, ref, bd, dtype, g, b["reward"], b["seq"]), case
        # rows of reward 0 and the ignored row: an all-zero bound
        zero_rows = [r for r in range(so.ROWS) if so.REWARDS[int(b["seq"][r])] == 0.0 or r == so.IGNORED_ROW]
        assert len(zero_rows) == 4 and float(bd[zero_rows].abs().max()) == 0.0 and float(bd[:, case.V:].abs().max()) == 0.0
    print(f"\nscst emulation vs float64, worst excess: {worst:.3g}")


@pytest.mark.parametrize("mutation", so.MUTATIONS)
def test_oracle_sees_the_mutation(mutation):
    """Every named fault of a kernel -- the reward of the neighbouring sentence, a disallowed column (either side of the range) leaking
    into lse, a lost reward sign, ... -- moves at least one output past the tolerance the kernels are held to, in both forms."""
    for dtype, cases in ((torch.bfloat16, SMALL), (torch.float32, so.CASES32)):
        seen = 0
        for case in cases:
            if mutation.startswith("leak") and case.crange is None:
                continue
            b = so.build(case, dtype)
            g = 1.0 if b["g"] is None else b["g"]
            ref, bd = so.scst_reference(b["x"], b["t"], b["reward"], b["seq"], g, case.crange)
            got = so.scst_emulate(b["x"], b["t"], b["reward"], b["seq"], g, dtype, so.registers_form(dtype, case.ld), case.crange, mutation)
            seen += _outputs_differ(got, ref, bd, dtype, g, b["reward"], b["seq"])
        assert seen > 0, (mutation, dtype)


def test_planted_seams_cover_both_sides_of_the_range():
    for case in so.CASES16 + so.CASES_STREAM16 + so.CASES32:
        if case.crange is None:
            continue
        dtype = torch.float32 if case in so.CASES32 else torch.bfloat16
        per, t = so.layout(case, dtype)
        flat = {c for cols in per for c in cols}
        cs, ce = case.crange
        assert {cs - 1, cs, ce - 1, ce} <= flat | {co.IGNORE} and {0, 3, 4, case.V - 1} <= flat, case
        A = so.allowed(case.V, case.crange, "cpu")
        assert all(bool(A[c]) for r, c in enumerate(t) if r != so.IGNORED_ROW), case
    assert any(c.crange and c.crange[0] >= 8192 for c in so.CASES16)                        # a range that starts inside the second slab
    assert {(c.perm, c.g) for c in so.CASES16} == {(p, g) for p in (False, True) for g in so.GS}


def test_oracle_reproduces_the_reference_loss_and_gradient(G):
    """The float64 oracle on the golden logits against the reference's own (fp32) loss and autograd gradient, with the constraint range
    and with ignore_prefix_size = 1: gradient error / bound within G32_TOL, the loss within G32_TOL of its magnitude."""
    meta = G["meta"]
    x = torch.from_numpy(G["logits"]).reshape(-1, meta["V"])
    reward = torch.from_numpy(G["table.reward"])
    seq = torch.arange(x.shape[0]) // torch.from_numpy(G["target"]).shape[1]
    for prefix in (0, 1):
        t = torch.from_numpy(G["target"]).clone()
        t[:, :prefix] = meta["pad"]
        ref, bd = so.scst_reference(x, t.reshape(-1), reward, seq, 1.0, tuple(meta["crange"]), ignore=meta["pad"])
        want = torch.from_numpy(G[f"dlogits.{prefix}"]).reshape(-1, meta["V"])
        assert co.excess(want, ref["d"], bd, 1.0, co.FLT_MIN) <= co.G32_TOL
        assert float(want[:, 4:meta["crange"][0]].abs().max()) == 0.0 and float(want[:, meta["crange"][1]:].abs().max()) == 0.0
        mag = float(ref["row_loss"].abs().sum())
        assert abs(float(ref["row_loss"].sum()) - float(G[f"loss.{prefix}"])) <= co.G32_TOL * mag
        assert int((t != meta["pad"]).sum()) == int(G[f"ntokens.{prefix}"])
