"""CPU: closed-set targets as trie node ids (TextPreprocessConfig.closed_set_nodes) -- TraversePlan.walk and the node-mode collation
against what the REFERENCE recorded (tests/golden/traverse.npz: its Trie's next layer for every (answer, position);
tests/golden/collate.npz: its constraint masks for the `closed_set` collation case), the refusals, the switch, and the C ABI of the
node-form criterion (csrc/trie_loss.hip)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle.collate_cases import CASES, N_TEXT, make_samples
from ofasys_amd import lib as L
from ofasys_amd.preprocessor import (DefaultBoxPreprocess, DefaultTextPreprocess, Dictionary, GeneralPreprocess, Instruction,
                                     ModalityType, Slot, TensorPreprocess, to_device)
from ofasys_amd.preprocessor.collate import BoxPreprocessConfig, PreprocessConfig, TextPreprocessConfig
from ofasys_amd.traverse import TraversePlan
from tests.closed_set_train_case import nodes_to_masks
from tests.traverse_case import ANSWERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT = dict(np.load(os.path.join(ROOT, "tests", "golden", "traverse.npz"), allow_pickle=False))
GC = dict(np.load(os.path.join(ROOT, "tests", "golden", "collate.npz"), allow_pickle=False))
BOS, PAD, EOS = 0, 1, 2


def _children(plan, n):
    return sorted(plan.edge_token[plan.node_edge_off[n]:plan.node_edge_off[n + 1]].tolist())


def test_walk_matches_the_reference_trie():
    """For every answer (duplicates and answers that are prefixes of others included) the children of walk()'s node i are the tokens
    the reference's Trie allows at position i; entry 0 is the root and the last entry's node has the EOS edge."""
    plan = TraversePlan(ANSWERS, BOS, EOS, PAD)
    for c, a in enumerate(ANSWERS):
        nodes = plan.walk(a)
        assert nodes.dtype == np.int32 and nodes.shape == (len(a) + 1,) and nodes[0] == 0
        for i, n in enumerate(nodes):
            want = sorted(int(t) for t in GT["allowed"][c, i] if t >= 0)
            assert _children(plan, int(n)) == want, (c, i)
            assert int(n) == plan.node_of(c, i)
        assert EOS in _children(plan, int(nodes[-1]))


def test_walk_refuses_answers_outside_the_closed_set():
    plan = TraversePlan(ANSWERS, BOS, EOS, PAD)
    with pytest.raises(ValueError, match=r"position 1 .*outside the closed set"):
        plan.walk([17, 24])
    with pytest.raises(ValueError, match=r"position 0 .*outside the closed set"):
        plan.walk([5])
    with pytest.raises(ValueError, match="outside the closed set"):
        plan.walk([40])                                       # a strict prefix of [40, 8]: no EOS edge at its node
    with pytest.raises(ValueError, match="outside the closed set"):
        plan.walk([17, EOS])                                  # EOS in the middle: no child node to go on from


def _dictionary():
    d = Dictionary()
    for i in range(N_TEXT):
        d.add_symbol(f"<text>_{i}")
    d.add_symbol("<mask>")
    return d


def _general(case, nodes):
    d = _dictionary()
    cfg = TextPreprocessConfig(pad_to_multiple=case.get("pad_to_multiple", 1), max_src_length=case.get("max_src_length", 1024),
                               max_tgt_length=case.get("max_tgt_length", 1024))
    if nodes is not None:
        cfg.closed_set_nodes = nodes
    closed = [[4 + t for t in ans] for ans in case["closed_set"]]
    pres = {"text": DefaultTextPreprocess(d, cfg, closed_set=closed), "box": DefaultBoxPreprocess(d, BoxPreprocessConfig()),
            "image": TensorPreprocess(d, PreprocessConfig(), ModalityType.IMAGE)}
    return GeneralPreprocess(d, pres)


def _run(case, nodes, raws=None):
    gp = _general(case, nodes)
    samples = []
    for raw in (make_samples(case) if raws is None else raws):
        slots = [Slot(ModalityType[m], is_src, v, global_position=i, attributes=attrs, split=case.get("split", "train"),
                      is_plaintext=plain) for i, (m, is_src, v, attrs, plain) in enumerate(raw)]
        samples.append(gp(Instruction(slots, case["template"], {"uid": len(samples)})))
    return gp, samples


def _same_tree(a, b, path=""):
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), path
    elif isinstance(a, dict):
        assert list(a) == list(b), (path, list(a), list(b))
        for k in a:
            _same_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, f"{path}/{i}")
    elif isinstance(a, Slot):
        assert (a.modality, a.is_src, a.attributes) == (b.modality, b.is_src, b.attributes), path
        _same_tree(a.value, b.value, path + "/value")
    else:
        assert a == b, (path, a, b)


def test_node_collation_matches_the_reference_masks():
    """The `closed_set` collation case in node mode: the nodes expand to the reference's recorded constraint masks at every position
    whose target is not <pad>, they are -1 at every other position, constraint_masks is absent and every other field is the
    mask-mode run's."""
    case = CASES["closed_set"]
    gp, samples = _run(case, True)
    plan = gp.name2pre["text"].constraint_plan
    assert isinstance(plan, TraversePlan) and plan.C == len(case["closed_set"])
    res = gp.collate(samples)
    gm, sm = _run(case, False)
    ref = gm.collate(sm)
    assert "constraint_masks" not in res and "constraint_nodes" not in ref
    nodes, target = res["constraint_nodes"], res["target"]
    assert nodes.dtype == torch.int32 and nodes.shape == target.shape
    want = torch.from_numpy(GC["closed_set.extra.constraint_masks"])
    assert torch.equal(want, ref["constraint_masks"])
    got = nodes_to_masks(nodes, plan.node_edge_off, plan.edge_token, want.shape[-1])
    live = target.ne(gp.pad)
    assert bool(live.any()) and bool((~live).any())
    assert torch.equal(got[live], want[live])
    assert bool((nodes[~live] == -1).all()) and bool((nodes[live] >= 0).all())
    assert set(ref) - set(res) == {"constraint_masks"} and set(res) - set(ref) == {"constraint_nodes"}
    for k in ref:
        if k != "constraint_masks":
            _same_tree(res[k], ref[k], k)
    # the int32 field survives the one-buffer device packing, -1 included
    out = to_device(gp.collate(_run(case, True)[1]), "cpu")
    assert out["constraint_nodes"].dtype == torch.int32 and torch.equal(out["constraint_nodes"], nodes)


def test_switch_off_leaves_the_sample_as_it_was():
    """closed_set_nodes unset and closed_set_nodes=False: the grouped slot values and the collated sample are today's, key for key (the
    recorded reference masks included), and the preprocessor builds no plan."""
    case = CASES["closed_set"]
    g0, s0 = _run(case, None)
    g1, s1 = _run(case, False)
    assert g0.name2pre["text"].constraint_plan is None and g1.name2pre["text"].constraint_plan is None
    for a, b in zip(s0, s1):
        for x, y in zip(a.slots, b.slots):
            assert "constraint_nodes" not in x.value and list(x.value) == ["inputs", "target", "constraint_masks", "raw_tokens",
                                                                           "prefix_tokens"]
            _same_tree(x.value, y.value)
    r0, r1 = g0.collate(s0), g1.collate(s1)
    _same_tree(r0, r1)
    assert "constraint_nodes" not in r0
    assert np.array_equal(r0["constraint_masks"].numpy(), GC["closed_set.extra.constraint_masks"])


def test_collation_refuses_what_the_reference_cannot_score():
    case = CASES["closed_set"]
    raws = make_samples(case)
    # an answer outside the closed set
    bad = [list(r) for r in raws]
    m, is_src, v, attrs, plain = bad[0][-1]
    assert "closed_set" in attrs
    bad[0][-1] = (m, is_src, np.asarray([10, 13], dtype=np.int64), attrs, plain)     # [10, 13]: 13 is no child of the node of [10]
    with pytest.raises(ValueError, match="outside the closed set"):
        _run(case, True, bad)
    # a live target on a -1 node: the slot in front of the answer carries loss but no closed set
    bad = [list(r) for r in raws]
    for r in bad:
        m, is_src, v, attrs, plain = r[1]
        assert attrs == ["no_loss"]
        r[1] = (m, is_src, v, None, plain)
    gp, samples = _run(case, True, bad)
    with pytest.raises(ValueError, match="no trie node"):
        gp.collate(samples)


def test_traverse_task_shares_the_preprocessors_plan():
    from ofasys_amd.task import TaskConfig
    from ofasys_amd.traverse import TraverseTask
    d = _dictionary()
    cfg = TaskConfig()
    cfg.text.closed_set_nodes = True
    t = TraverseTask(cfg)
    t.initialize(d, closed_set=[tuple(a) for a in ANSWERS])
    pre = t.general_preprocess.name2pre["text"]
    assert t.plan is pre.constraint_plan and t.plan.C == len(ANSWERS)
    trie = t.constraint_trie_on("cpu")
    assert trie is t.constraint_trie_on("cpu") and trie["N"] == t.plan.N and trie["E"] == t.plan.E
    assert trie["node_edge_off"].dtype == torch.int32 and trie["edge_token"].dtype == torch.int32
    assert np.array_equal(trie["edge_token"].numpy(), t.plan.edge_token)
    t2 = TraverseTask(TaskConfig())                           # off: its own plan, and no trie to hand out
    t2.initialize(_dictionary(), closed_set=[tuple(a) for a in ANSWERS])
    assert t2.general_preprocess.name2pre["text"].constraint_plan is None and t2.plan is not None
    with pytest.raises(ValueError, match="closed_set_nodes"):
        t2.constraint_trie_on("cpu")


def test_header_declares_and_library_exports_the_trie_criterion():
    protos = L.parse_header()
    cdll = ctypes.CDLL(L.LIB_PATH)
    for name in ("ofa_trie_ls_cross_entropy_fwd", "ofa_trie_ls_cross_entropy_bwd"):
        assert name in protos and len(protos[name][1]) == 22 - (name.endswith("bwd")), name
        getattr(cdll, name)
    h = L.lib()
    P = 4096                                                  # a fake, aligned device address: every call below is refused before a launch
    fwd = [P, P, P, P, P, 3, 5, None, P, P, P, P, P, 4, 204, 208, 1, 0.1, -1, -1, L.BF16, None]
    h.call("ofa_trie_ls_cross_entropy_fwd", *(fwd[:13] + [0] + fwd[14:]))                      # rows == 0: nothing to do
    for change, match in (({20: 7}, "bad dtype 7"), ({15: 204 + 2}, "multiple of the 16-byte vector"), ({5: 0}, "bad trie"),
                          ({2: None}, "bad argument"), ({12: P + 8}, "16-byte aligned"), ({18: 2, 19: 100}, "constraint range"),
                          ({17: 1.0}, "bad eps"), ({8: None}, "bad argument")):
        args = list(fwd)
        for i, v in change.items():
            args[i] = v
        with pytest.raises(L.OfaError, match=match):
            h.call("ofa_trie_ls_cross_entropy_fwd", *args)
    bwd = [P, P, P, P, P, 3, 5, P, P, None, None, P, 4, 204, 208, 1, 0.1, -1, -1, L.F32, None]
    with pytest.raises(L.OfaError, match="bad argument"):
        h.call("ofa_trie_ls_cross_entropy_bwd", *(bwd[:11] + [None] + bwd[12:]))               # no dlogits
    h.call("ofa_trie_ls_cross_entropy_bwd", *(bwd[:12] + [0] + bwd[13:]))
