"""CPU: closed-set inference without a GPU -- the C ABI of csrc/closed_set_score.hip and its register allocation, the
reference-recorded golden's self-consistency, TraversePlan against the collater's Trie, the algebra the kernels rely on
(edge logit minus node log-sum-exp, summed along the path == masked log_softmax + gather), and the task surface."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.golden_util import load_golden
from tests.traverse_case import ANSWERS, SCORE_TOL, VALID_BATCH_SIZE, random_answers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BOS, PAD, EOS = 0, 1, 2


def test_header_declares_and_library_exports_closed_set_entry_points():
    import ctypes
    from ofasys_amd import lib as L
    protos = L.parse_header()
    for name in ("ofa_closed_set_ws_bytes", "ofa_closed_set_edge_logits", "ofa_closed_set_reduce", "ofa_closed_set_score"):
        assert name in protos
        getattr(ctypes.CDLL(L.LIB_PATH), name)
    h = L.lib()
    assert h.cdll.ofa_closed_set_ws_bytes(32, 8000, 5000) == 32 * 13000 * 4
    assert h.cdll.ofa_closed_set_ws_bytes(0, 10, 10) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_closed_set_kernels_compile_without_spills(tmp_path):
    out = tmp_path / "closed_set_score.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "ofasys_amd", "csrc", "closed_set_score.hip"), "-o", str(out)], check=True,
                   stderr=subprocess.DEVNULL)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in ("vgpr_spill_count", "private_segment_fixed_size")}
    assert len([k for k in meta if "closed_set_edge_kernel" in k]) == 3, sorted(meta)
    assert len([k for k in meta if "closed_set_lse_kernel" in k]) == 1 and len([k for k in meta if "closed_set_path_kernel" in k]) == 1
    assert len(meta) == 5, sorted(meta)
    for k, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (k, m)


def _golden_answers(g):
    return [[int(t) for t in row if t >= 0] for row in g["answers"]]


def test_golden_is_self_consistent():
    g = load_golden("traverse")
    assert _golden_answers(g) == ANSWERS and int(g["valid_batch_size"]) == VALID_BATCH_SIZE
    assert 12 <= len(ANSWERS) <= 16 and all(1 <= len(a) <= 4 for a in ANSWERS)
    assert len(set(len(a) for a in ANSWERS)) >= 3
    assert any(a != b and b[:len(a)] == a for a in ANSWERS for b in ANSWERS)          # a strict prefix of another answer
    assert len(set(map(tuple, ANSWERS))) == len(ANSWERS) - 1                           # one duplicate
    scores = g["scores"]
    assert scores.shape == (2, len(ANSWERS)) and np.isfinite(scores).all() and (scores <= 0).all()
    assert g["argmax"].tolist() == np.argmax(scores, axis=1).tolist()
    uniq = sorted(set(ANSWERS.index(a) for a in ANSWERS))
    for b in range(2):
        s = np.sort(scores[b, uniq].astype(np.float64))[::-1]
        assert s[0] - s[1] > 10 * SCORE_TOL
        assert abs((s[0] - s[1]) - float(g["margins"][b])) < 1e-6
    dup = [i for i, a in enumerate(ANSWERS) if ANSWERS.index(a) != i]
    for i in dup:
        assert np.array_equal(scores[:, i], scores[:, ANSWERS.index(ANSWERS[i])])


def _check_plan(plan, answers, trie):
    C = len(answers)
    assert plan.C == C and plan.node_edge_off[0] == 0 and plan.node_edge_off[-1] == plan.E == len(plan.edge_token)
    assert plan.rep_ans[0] == 0 and plan.rep_pos[0] == 0
    lowest = {}
    for c, a in enumerate(answers):
        prev = [BOS] + list(a)
        assert plan.prev_output_tokens[c, :len(prev)].tolist() == prev and (plan.prev_output_tokens[c, len(prev):] == PAD).all()
        assert plan.target[c, :len(prev)].tolist() == list(a) + [EOS] and (plan.target[c, len(prev):] == PAD).all()
        path = plan.path_edge[plan.path_off[c]:plan.path_off[c + 1]]
        assert len(path) == len(a) + 1
        assert plan.edge_token[path].tolist() == list(a) + [EOS]                 # the path spells the target and ends in EOS
        for t in range(len(prev)):
            allowed = plan.allowed(c, t)
            assert len(set(allowed)) == len(allowed)
            assert set(allowed) == set(trie.get_next_layer(prev[:t + 1])), (c, t)
            n = plan.node_of(c, t)
            assert plan.edge_node[path[t]] == n
            lowest.setdefault(n, (c, t))
    assert len(lowest) == plan.N                                                 # every node lies on some path
    for n, (c, t) in lowest.items():                                             # representatives: the lowest answer index
        assert (int(plan.rep_ans[n]), int(plan.rep_pos[n])) == (c, t)
    assert np.all(np.diff(plan.rep_ans) >= 0)
    # work items: a partition of the edges, each inside one node, at most ITEM_EDGES long
    covered = np.zeros(plan.E, np.int32)
    for n, e0, e1 in plan.items.tolist():
        assert plan.node_edge_off[n] <= e0 < e1 <= plan.node_edge_off[n + 1] and e1 - e0 <= plan.ITEM_EDGES
        covered[e0:e1] += 1
    assert (covered == 1).all()
    # chunks: the items of [c0, c1) are exactly those whose node's representative lies there
    for per in (1, 5, C):
        seen = 0
        for c0 in range(0, C, per):
            c1 = min(C, c0 + per)
            i0, i1, T = plan.chunk_items(c0, c1)
            assert i0 == seen and T == max(len(a) for a in answers[c0:c1]) + 1
            assert all(c0 <= plan.rep_ans[n] < c1 and plan.rep_pos[n] < T for n in plan.items[i0:i1, 0])
            seen = i1
        assert seen == len(plan.items)


def _trie(answers):
    from ofasys_amd.preprocessor.collate import Trie
    trie = Trie(EOS)
    for a in answers:
        trie.insert([BOS] + list(a) + [EOS])
    return trie


def test_plan_matches_trie_and_golden_on_the_fixture_set():
    from ofasys_amd import TraversePlan
    g = load_golden("traverse")
    plan = TraversePlan(ANSWERS, BOS, EOS, PAD)
    _check_plan(plan, ANSWERS, _trie(ANSWERS))
    assert np.array_equal(plan.prev_output_tokens, g["prev_output_tokens"]) and np.array_equal(plan.target, g["target"])
    for c, a in enumerate(ANSWERS):                              # the reference's recorded masks
        for t in range(len(a) + 1):
            assert sorted(plan.allowed(c, t)) == [int(x) for x in g["allowed"][c, t] if x >= 0], (c, t)


def test_plan_matches_trie_on_random_answer_sets():
    from ofasys_amd import TraversePlan
    rng = np.random.default_rng(20240)
    for i in range(200):
        answers = random_answers(rng, int(rng.integers(1, 40)))
        _check_plan(TraversePlan(answers, BOS, EOS, PAD), answers, _trie(answers))


def test_edge_minus_node_lse_along_the_path_equals_masked_log_softmax():
    """The algebra of the kernels, in float64: the dense formulation of traverse_task.py:99-104 (project onto V, mask to the
    trie's next layer, log_softmax, gather the target, zero the padding, sum) equals sum over path(c) of (z[e] - lse[node(e)])."""
    from ofasys_amd import TraversePlan
    rng = np.random.default_rng(7)
    V, D, bsz = 204, 16, 3
    for answers in (ANSWERS, random_answers(rng, 30), random_answers(rng, 1)):
        plan = TraversePlan(answers, BOS, EOS, PAD)
        trie = _trie(answers)
        C, T = plan.C, plan.Tmax
        h = rng.standard_normal((bsz, C, T, D))
        for c, a in enumerate(answers):                          # causal decoder: answers sharing a prefix share the hidden state
            for t in range(len(a) + 1):
                n = plan.node_of(c, t)
                h[:, c, t] = h[:, plan.rep_ans[n], plan.rep_pos[n]]
        W, bias = rng.standard_normal((V, D)), rng.standard_normal(V)
        # dense
        logits = h @ W.T + bias
        dense = np.zeros((bsz, C))
        for c, a in enumerate(answers):
            for t in range(len(a) + 1):
                mask = np.full(V, -math.inf)
                mask[trie.get_next_layer(plan.prev_output_tokens[c, :t + 1].tolist())] = 0.0
                x = logits[:, c, t] + mask
                m = x.max(-1, keepdims=True)
                lp = x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))
                dense[:, c] += lp[:, plan.target[c, t]]
        # edges / nodes / paths
        rows = h[:, plan.rep_ans[plan.edge_node], plan.rep_pos[plan.edge_node]]               # [bsz, E, D]
        z = np.einsum("bed,ed->be", rows, W[plan.edge_token]) + bias[plan.edge_token]
        lse = np.zeros((bsz, plan.N))
        for n in range(plan.N):
            zn = z[:, plan.node_edge_off[n]:plan.node_edge_off[n + 1]]
            m = zn.max(-1)
            lse[:, n] = m + np.log(np.exp(zn - m[:, None]).sum(-1))
        sparse = np.zeros((bsz, C))
        for c in range(C):
            for e in plan.path_edge[plan.path_off[c]:plan.path_off[c + 1]]:
                sparse[:, c] += z[:, e] - lse[:, plan.edge_node[e]]
        assert np.abs(sparse - dense).max() <= 1e-6, float(np.abs(sparse - dense).max())


def _task(**kw):
    from ofasys_amd import Dictionary, TraverseTask
    return TraverseTask(name="vqa", instruction="[TEXT:src] what is it? -> [TEXT:tgt]", **kw), Dictionary()


def test_initialize_without_a_closed_set_raises():
    t, d = _task()
    with pytest.raises(ValueError, match="closed set"):
        t.initialize(d)


def test_closed_set_sources_and_index2ans():
    from ofasys_amd import Task
    t, d = _task()
    t.initialize(d, closed_set=["yes", "no", "yes sir"])
    assert t.index2ans == {0: "yes", 1: "no", 2: "yes sir"} and t.plan.C == 3
    pre = t.general_preprocess.name2pre["text"]
    assert pre.ans2label_dict == ["yes", "no", "yes sir"]
    assert t.plan.prev_output_tokens[2, 1:].tolist() == pre.encode("yes sir").tolist()
    # cfg.text.ans2label: the JSON string of preprocessor/default/text.py:37-40
    t2, d2 = _task()
    t2.cfg.text.ans2label = '{"yes": 0, "no": 1}'
    t2.initialize(d2)
    assert t2.index2ans == {0: "yes", 1: "no"} and t2.general_preprocess.name2pre["text"].ans2label_dict == {"yes": 0, "no": 1}
    # set through the text preprocessor's prepare_for_generation, then initialised again
    t3, d3 = _task()
    with pytest.raises(ValueError):
        t3.initialize(d3)
    t3.general_preprocess.name2pre["text"].prepare_for_generation({"a cat": 0, "a dog": 1})
    t3.initialize(d3)
    assert t3.index2ans == {0: "a cat", 1: "a dog"}
    # token-id answers; a plain Task's preprocessor remembers the closed set too and still builds the same trie
    t4, d4 = _task()
    Task.initialize(t4, d4)
    t4.initialize(d4, closed_set=[tuple(a) for a in ANSWERS])
    assert t4.plan.C == len(ANSWERS) and t4.index2ans[1] == tuple(ANSWERS[1])
    assert t4.general_preprocess.name2pre["text"].constraint_trie.root == _trie(ANSWERS).root
    with pytest.raises(ValueError, match="outside the dictionary"):
        _task()[0].initialize(d4, closed_set=[[10 ** 6]])


def test_generator_still_refuses_the_trie():
    t, d = _task()
    t.initialize(d, closed_set=["yes", "no"])
    with pytest.raises(NotImplementedError, match="constraint_trie"):
        t.generator


def test_max_rows_is_validated():
    with pytest.raises(ValueError):
        _task(max_rows=0)
