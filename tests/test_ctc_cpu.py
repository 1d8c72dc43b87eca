"""CPU: the CTC oracle (tests/ctc_oracle.py) is pinned against torch.nn.functional.ctc_loss in float64 on every case of the list the
GPU tests run, the library exports the CTC entry points the header declares, and the host-side pieces (edit distance, the wrappers'
refusals that need no device) behave.  torch is the reference here; the oracle is the yardstick of tests/test_ctc_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ctc_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ofa_ctc_rows", "ofa_ctc_alpha_beta", "ofa_ctc_grad", "ofa_ctc_greedy_decode", "ofa_ctc_max_classes", "ofa_ctc_max_target")


@pytest.mark.parametrize("zero_infinity", [False, True])
@pytest.mark.parametrize("case", co.CASES, ids=[c.name for c in co.CASES])
def test_oracle_equals_torch_float64(case, zero_infinity):
    d = co.build(case)
    assert [co.labels_of(r) for r in d["target"]] == d["labels"]          # the target rows (interior <eos>, trailing <pad>) hold the labels
    ref = co.ctc_reference(d["x"], d["lengths"], d["labels"], zero_infinity)
    tl, tn, tg = co.torch_reference(torch.from_numpy(d["x"]), d["lengths"], d["labels"], zero_infinity, torch.float64)
    assert np.isfinite(ref["loss"]) == (case.feasible or zero_infinity)
    fin_s = np.isfinite(ref["nll"])
    assert (np.isfinite(tn) == fin_s).all() and (np.isposinf(tn) == np.isposinf(ref["nll"])).all()
    if fin_s.any():
        assert np.abs(tn[fin_s] - ref["nll"][fin_s]).max() <= 1e-10 * max(1.0, np.abs(ref["nll"][fin_s]).max())
    if fin_s.all():
        assert abs(tl - ref["loss"]) <= 1e-10 * max(1.0, abs(ref["loss"]))
    else:
        assert tl == float("inf") and ref["loss"] == float("inf")
    # gradient: NaN exactly where torch's is (the live rows of an infeasible sentence without zero_infinity), 1e-10 of the largest
    # element elsewhere, exact zeros past every length
    fin = np.isfinite(ref["grad"])
    assert (np.isnan(tg) == ~fin).all() and (np.isnan(ref["grad"]) == ~fin).all()
    if fin.any():
        assert np.abs(tg[fin] - ref["grad"][fin]).max() <= 1e-10 * max(1.0, np.abs(tg[fin]).max())
    for b in range(d["B"]):
        assert (ref["grad"][int(d["lengths"][b]):, b] == 0).all() and (tg[int(d["lengths"][b]):, b] == 0).all()


def test_case_list_covers_the_state_counts_and_class_counts_the_kernels_branch_on():
    S = {2 * len(l) + 1 for c in co.CASES for _, l in c.sents}
    assert {63, 65, 127, 129, 255, 257, 767, 769} <= S                    # a wave, two waves, the workgroup, three states per thread
    assert {2, 5, 64, 65, 300} <= {c.C for c in co.CASES}
    sharp = co.CASE["sharp"]
    assert sharp.scale == 20.0 and sharp.sents[0][0] == 600 and len(sharp.sents[0][1]) == 40
    assert np.isfinite(co.ctc_reference(co.build(sharp)["x"], [600], [sharp.sents[0][1]], False)["loss"])
    for c in co.CASES:                                                    # a tight case's target width is its label count
        if c.tight:
            assert co.build(c)["target"].shape[1] == len(c.sents[0][1])


def test_greedy_reference_collapses_then_drops_blanks_and_takes_the_lowest_of_equals():
    x = np.full((6, 4), -1.0)
    for t, c in enumerate([2, 2, 0, 2, 3, 3]):
        x[t, c] = 1.0
    assert co.greedy_reference(x) == [2, 2, 3]
    x[4, 1] = 1.0                                                         # classes 1 and 3 tie in row 4: the lower one
    assert co.greedy_reference(x) == [2, 2, 1, 3]
    assert co.greedy_reference(np.zeros((0, 4))) == []


def test_library_exports_the_ctc_entry_points_and_the_header_declares_them():
    from ofasys_amd.lib import HEADER, LIB_PATH, parse_header
    protos = parse_header()
    src = open(HEADER).read()
    cdll = ctypes.CDLL(LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in protos and re.search(r"\b%s\s*\(" % name, src), name
        assert getattr(cdll, name) is not None
    assert "ctc.hip" in open(os.path.join(ROOT, "ofasys_amd", "csrc", "Makefile")).read()


def test_limits_and_host_refusals():
    from ofasys_amd import kernels as K, ops
    cmax, lmax = K.ctc_limits()
    assert cmax == 8192 and 2 * lmax + 1 <= 9 * 256 < 2 * (lmax + 1) + 1
    with pytest.raises(ValueError, match="rows"):
        ops.encoder_ctc_logits(torch.zeros(2, 1, 4), torch.zeros(10, 4), 6, 12)
    # no CPU fallback: a CPU tensor is refused, not computed by torch
    lay = ops.CtcLayout(torch.tensor([[0, 2]], dtype=torch.int32), 1, 2)
    with pytest.raises(Exception, match="GPU|fallback"):
        ops.ctc_loss(torch.zeros(2, 1, 4), lay, torch.ones(1, 3, dtype=torch.int64), 10, 1, 2, True)
    with pytest.raises(ValueError, match="encoder_target"):
        ops.ctc_loss(torch.zeros(2, 1, 4), lay, torch.ones(2, 3, dtype=torch.int64), 10, 1, 2, True)


def test_padded_layout_table():
    from ofasys_amd import ops
    lay = ops.CtcLayout.padded(torch.tensor([5, 3, 7]), 7)
    assert lay.seg.dtype == torch.int32 and lay.seg.tolist() == [[0, 5], [1, 3], [2, 7]] and (lay.row_stride, lay.tmax) == (3, 7)


def test_edit_distance_on_hand_worked_pairs():
    from ofasys_amd import ops
    for a, b, want in co.levenshtein_pairs():
        assert ops.edit_distance(a, b) == want and ops.edit_distance(b, a) == want, (a, b)
    assert ops.edit_distance("kitten", "sitting") == 3


# ------------------------------------------------------------------ the configuration surface (Task / Trainer), host only
def _asr_task(phone=("a", "b", "c", "d"), **crit):
    from ofasys_amd import Task
    t = Task(name="asr", instruction='what is said in " [TEXT:hint] "? -> [TEXT:text]', micro_batch_size=2)
    t.cfg.criterion.name = "speech_to_text_loss"
    for k, v in crit.items():
        setattr(t.cfg.criterion, k, v)
    t.cfg.text.phone_dict = list(phone) if phone is not None else None
    t.add_dataset([{"hint": f"clip {i}", "text": f"the words of clip number {i}"} for i in range(4)], "train")
    return t


def test_criterion_config_builds_with_the_references_defaults():
    from ofasys_amd.task import CriterionConfig
    c = CriterionConfig(name="speech_to_text_loss")
    assert (c.ce_weight, c.ctc_weight, c.zero_infinity, c.sentence_avg) == (1.0, 0.0, False, False)
    c = CriterionConfig(name="speech_to_text_loss", ce_weight=0.5, ctc_weight=0.5, zero_infinity=True)
    assert (c.ce_weight, c.ctc_weight, c.zero_infinity) == (0.5, 0.5, True)
    assert CriterionConfig().name == "label_smoothed_cross_entropy"


def test_collator_emits_encoder_target_and_the_phone_rows_are_registered():
    from ofasys_amd import Dictionary, Task
    d = Dictionary()
    t = _asr_task()
    t.initialize(d)
    ds, de = d.index("<phone>_dict_begin"), d.index("<phone>_dict_end")
    assert de - ds == 5 and [d[i] for i in range(ds + 1, de)] == ["<phone>_a", "<phone>_b", "<phone>_c", "<phone>_d"]
    s = t.get_sample("train")
    assert torch.equal(s["encoder_target"], s["target"]) and s["encoder_target"].dtype == torch.int64
    # a task without a phone dictionary collates what it always did
    plain = Task(name="plain", instruction="[TEXT:hint] -> [TEXT:text]", micro_batch_size=2)
    plain.add_dataset([{"hint": "a b", "text": "c d"}] * 2, "train")
    plain.initialize(Dictionary())
    assert "encoder_target" not in plain.get_sample("train")


def test_use_t2p_is_refused_with_its_reason():
    from ofasys_amd import Dictionary
    t = _asr_task()
    t.cfg.text.use_t2p = True
    with pytest.raises(NotImplementedError, match="g2p"):
        t.initialize(Dictionary())


def test_plain_micro_batch_carries_the_ctc_fields_only_for_such_tasks():
    from ofasys_amd import Dictionary, Task, Trainer
    d = Dictionary()
    asr = _asr_task(ce_weight=0.7, ctc_weight=0.3, zero_infinity=True)
    plain = Task(name="plain", instruction="[TEXT:hint] -> [TEXT:text]", micro_batch_size=2)
    plain.add_dataset([{"hint": "a b", "text": "c d"}] * 2, "train")
    for t in (asr, plain):
        t.initialize(d)
    tr = Trainer()
    mb = tr._plain_micro_batch(asr, asr.get_sample("train"))
    ds, de = d.index("<phone>_dict_begin"), d.index("<phone>_dict_end")
    assert mb["ctc_range"] == f"{ds},{de}" and (mb["ce_weight"], mb["ctc_weight"], mb["zero_infinity"], mb["sentence_avg"]) == (0.7, 0.3, True, False)
    assert torch.equal(mb["encoder_target"], mb["target"])
    own = asr.get_sample("train")
    own["encoder_target"] = torch.full((2, 3), ds + 1)                      # a sample's own labels pass through unchanged
    assert tr._plain_micro_batch(asr, own)["encoder_target"] is own["encoder_target"]
    mp = tr._plain_micro_batch(plain, plain.get_sample("train"))
    assert set(mp) == {"slots", "target", "task"}
    # the criterion without the phone rows in the dictionary is refused by name
    bare = _asr_task(phone=None)
    bare.initialize(Dictionary())
    with pytest.raises(ValueError, match="phone"):
        tr._plain_micro_batch(bare, bare.get_sample("train"))
