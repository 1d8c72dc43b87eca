"""CPU: the trie-edge head's oracle, plan and surface (no GPU).

* tests/closed_set_head_case.head_reference / dx_reference / dw_reference equal float64 torch autograd through x @ W^T, the masks
  nodes_to_masks gives and the masked label-smoothed loss -- loss, dX, dW (and dbias) on every case.
* TraversePlan's inverse CSR by token equals a brute-force inversion, on traverse_case.ANSWERS and on every trie_layout (node 0's list
  holds junk tokens).
* The header declares and the library exports the three entry points, and every host precondition is refused with its status code
  before any launch.
* ops.trie_head_cross_entropy / ops.trie_head_eval and TrainStep(closed_set_edge_head=) have the agreed defaults and errors.
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from ofasys_amd import lib as L
from tests import closed_set_head_case as hc
from tests import closed_set_train_case as cst
from tests.traverse_case import ANSWERS

F64 = torch.float64


def _rel(a, b):
    """max |a - b| against max(1, max |b|): the planted rows' losses and gradients are differences of O(10) logits that nearly cancel"""
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1.0)


def _check_oracle(b, tag):
    ref = hc.head_reference(b)
    total, dx, dw, db, rows = hc.dense_autograd(b)
    good = ref["good"]
    w = b["row_w"].to(F64)
    mine = float((ref["row_loss"] * w * good.to(F64)).sum() * b["gs"])
    assert abs(mine - float(total)) <= 1e-11 * max(1.0, abs(float(total))), (tag, mine, float(total))
    assert _rel(ref["row_loss"][good], rows[good]) <= 1e-11, tag
    odx, _ = hc.dx_reference(b, ref["g"], ref["tok"], ref["A"])
    odw, _, n, odb, _ = hc.dw_reference(b, ref["g"], ref["tok"], ref["A"])
    assert _rel(odx, dx) <= 1e-10, (tag, "dX", _rel(odx, dx))
    assert _rel(odw, dw) <= 1e-10, (tag, "dW", _rel(odw, dw))
    assert bool((odx[~good] == 0).all()) and bool((dx[~good] == 0).all()), (tag, "rows outside the oracle")
    assert bool((odw[n == 0] == 0).all()) and bool((dw[n == 0].abs() <= 1e-300).all()), (tag, "tokens nobody touches")
    if db is not None:
        assert _rel(odb, db) <= 1e-10, (tag, "dbias")
    return ref


@pytest.mark.parametrize("case", hc.HEAD_CASES, ids=[f"c{c.idx}-D{c.D}" for c in hc.HEAD_CASES])
def test_oracle_equals_dense_autograd(case):
    b = hc.build_head_case(case, torch.bfloat16 if case.idx % 2 else torch.float32)
    ref = _check_oracle(b, case)
    kinds = b["kinds"]
    assert [k in ("dead_node", "not_child", "cut_target") for k in kinds] == ref["dead"].tolist()
    assert ref["row_cnt"][:len(case.trie.degrees)].tolist() == [float(d) for d in case.trie.degrees] or case.trie.crange is not None


def test_oracle_on_the_shared_node_case():
    b = hc.build_dw_case(torch.float32)
    ref = _check_oracle(b, "dw")
    _, _, n, _, _ = hc.dw_reference(b, ref["g"], ref["tok"], ref["A"])
    assert n[9] == 5 and n[5] == 3 and n[20] == 2            # token 9: three rows of node 0 and two of node 1
    assert all(n[u] == 0 for u in hc.DW_UNTOUCHED) and n[31] == 1      # (row 7 has row_w = 0: node 2 is left with row 6)
    # the twins: bit-identical rows, the lowest token is the arg-max
    assert ref["hit"].tolist()[6:] == [1, 0] and float(ref["z"][6, 0]) == float(ref["z"][6, 1])


def _brute_ok(plan_arrays, edge_token):
    head, off, edges = plan_arrays
    bh, bo, be = hc.invert_brute(edge_token)
    assert head.dtype == off.dtype == edges.dtype == np.int32
    assert np.array_equal(head, bh) and np.array_equal(off, bo) and np.array_equal(edges, be)
    assert np.all(np.diff(head) > 0) and off[0] == 0 and off[-1] == len(edge_token) == len(edges)
    for u, t in enumerate(head):
        es = edges[off[u]:off[u + 1]]
        assert len(es) >= 1 and np.all(np.diff(es) > 0) and np.all(np.asarray(edge_token)[es] == t)


def test_inverse_csr_by_token():
    from ofasys_amd.traverse import TraversePlan
    plan = TraversePlan(ANSWERS, 0, 2, 1)
    _brute_ok((plan.head_tokens, plan.tok_edge_off, plan.tok_edge), plan.edge_token)
    assert plan.U == len(plan.head_tokens) == len(set(plan.edge_token.tolist()))
    assert np.max(np.diff(plan.tok_edge_off)) > 1             # EOS hangs under many nodes
    dev = plan.to_device("cpu")
    arrays = plan.head_arrays("cpu")
    for k in ("head_tokens", "tok_edge_off", "tok_edge"):
        assert torch.equal(dev[k], torch.from_numpy(getattr(plan, k))) and torch.equal(arrays[k], dev[k]) and dev[k].dtype == torch.int32
    assert dev["max_degree"] == arrays["max_degree"] == plan.max_degree and dev["U"] == arrays["U"] == plan.U
    assert torch.equal(arrays["node_ids"], torch.arange(plan.N + 1, dtype=torch.int32))
    assert torch.equal(arrays["edge_node"], torch.from_numpy(plan.edge_node))
    for case in cst.TRIE_CASES:                               # node 0's list holds junk tokens: values like any other
        lay = cst.trie_layout(case)
        _brute_ok(TraversePlan.invert_edges(lay["edge_token"]), lay["edge_token"])
        assert -7 in TraversePlan.invert_edges(lay["edge_token"])[0]


def test_task_hands_out_the_same_head_arrays():
    from ofasys_amd.task import TaskConfig
    from ofasys_amd.traverse import TraverseTask
    from tests.test_closed_set_nodes_cpu import _dictionary
    cfg = TaskConfig()
    cfg.text.closed_set_nodes = True
    t = TraverseTask(cfg)
    t.initialize(_dictionary(), closed_set=[tuple(a) for a in ANSWERS])
    trie = t.constraint_trie_on("cpu")
    assert trie is t.constraint_trie_on("cpu")
    for k in ("node_edge_off", "edge_token", "edge_node", "head_tokens", "tok_edge_off", "tok_edge", "node_ids"):
        assert torch.is_tensor(trie[k]) and trie[k].dtype == torch.int32, k
    assert (trie["N"], trie["E"], trie["U"], trie["max_degree"]) == (t.plan.N, t.plan.E, t.plan.U, t.plan.max_degree)


# ---------------------------------------------------------------------------------------------------------------- the C ABI
P = 4096                                                      # a fake, aligned device address: every call below is refused before a launch


def _fwd(**kw):
    a = dict(feats=P, ld_x=16, W=P, ld_w=16, bias=None, D=16, V=204, target=P, node=P, off=P, tok=P, N=3, E=5, Cmax=4, z=P, lse=P,
             row_loss=P, row_nll=P, row_cnt=P, g=P, row_hit=None, rows=4, ignore=1, eps=0.1, cs=-1, ce=-1, dtype=L.BF16, stream=None)
    a.update(kw)
    return list(a.values())


def _dx(**kw):
    a = dict(g=P, W=P, ld_w=16, D=16, V=204, target=P, node=P, off=P, tok=P, N=3, E=5, Cmax=4, row_w=None, gs=None, dx=P, ld_dx=16,
             rows=4, ignore=1, cs=-1, ce=-1, dtype=L.BF16, stream=None)
    a.update(kw)
    return list(a.values())


def _dw(**kw):
    a = dict(g=P, feats=P, ld_x=16, D=16, V=204, off=P, edge_node=P, N=3, E=5, Cmax=4, head=P, toff=P, tedge=P, U=4, brows=P, boff=P,
             row_w=None, gs=None, dW=P, ld_dw=16, dbias=None, rows=4, cs=-1, ce=-1, dtype=L.BF16, stream=None)
    a.update(kw)
    return list(a.values())


REFUSALS = [
    ("ofa_trie_head_fwd", _fwd, [
        (dict(feats=None), 1), (dict(W=None), 1), (dict(target=None), 1), (dict(node=None), 1), (dict(off=None), 1), (dict(tok=None), 1),
        (dict(z=None), 1), (dict(lse=None), 1), (dict(row_loss=None), 1), (dict(row_nll=None), 1), (dict(row_cnt=None), 1),
        (dict(g=None), 1),                                    # (neither g nor row_hit: nothing to compute)
        (dict(dtype=7), 1), (dict(Cmax=0), 1), (dict(N=0), 1), (dict(E=-1), 1), (dict(V=1), 1), (dict(rows=-1), 1),
        (dict(eps=1.0), 1), (dict(eps=-0.1), 1), (dict(cs=2, ce=9), 1), (dict(cs=8, ce=8), 1), (dict(cs=8, ce=205), 1),
        (dict(D=12), 2), (dict(D=20, ld_x=20, ld_w=20, dtype=L.BF16), 2), (dict(ld_x=12), 2), (dict(ld_w=8), 2),
        (dict(feats=P + 8), 2), (dict(W=P + 2), 2), (dict(D=40000, ld_x=40000, ld_w=40000), 2),
    ]),
    ("ofa_trie_head_bwd_dx", _dx, [
        (dict(g=None), 1), (dict(W=None), 1), (dict(dx=None), 1), (dict(target=None), 1), (dict(node=None), 1), (dict(off=None), 1),
        (dict(tok=None), 1), (dict(dtype=-1), 1), (dict(Cmax=0), 1), (dict(cs=3, ce=9), 1), (dict(cs=8, ce=300), 1),
        (dict(D=12), 2), (dict(ld_dx=12), 2), (dict(dx=P + 4), 2), (dict(W=P + 8), 2),
    ]),
    ("ofa_trie_head_bwd_dw", _dw, [
        (dict(g=None), 1), (dict(feats=None), 1), (dict(dW=None), 1), (dict(off=None), 1), (dict(edge_node=None), 1), (dict(head=None), 1),
        (dict(toff=None), 1), (dict(tedge=None), 1), (dict(brows=None), 1), (dict(boff=None), 1), (dict(dtype=3), 1), (dict(Cmax=0), 1),
        (dict(U=6), 1), (dict(U=-1), 1), (dict(N=0), 1), (dict(cs=1, ce=9), 1),
        (dict(D=12), 2), (dict(ld_dw=12), 2), (dict(dW=P + 8), 2), (dict(feats=P + 2), 2),
    ]),
]


def test_header_declares_and_library_exports_the_head():
    protos = L.parse_header()
    cdll = ctypes.CDLL(L.LIB_PATH)
    for name, nargs in (("ofa_trie_head_fwd", 28), ("ofa_trie_head_bwd_dx", 22), ("ofa_trie_head_bwd_dw", 26)):
        assert name in protos and len(protos[name][1]) == nargs, name
        getattr(cdll, name)


@pytest.mark.parametrize("name,make,cases", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_precondition_is_refused_with_its_status(name, make, cases):
    h = L.lib()
    h.call(name, *make(rows=0))                               # nothing to do -- and nothing launched
    h.call(name, *make(rows=0, dtype=L.F32, D=4, **({"ld_x": 4} if name != "ofa_trie_head_bwd_dx" else {"ld_dx": 4})))
    for change, status in cases:
        with pytest.raises(L.OfaError, match=f"status {status}"):
            h.call(name, *make(**change))


# ---------------------------------------------------------------------------------------------------------------- op and step surface
def test_op_and_step_defaults_and_errors():
    from ofasys_amd import kernels as K
    from ofasys_amd import ops
    from ofasys_amd.engine import CommonConfig, Trainer
    from ofasys_amd.trainer import TrainStep
    sig = inspect.signature(ops.trie_head_cross_entropy)
    assert list(sig.parameters) == ["feats", "weight", "bias", "target", "nodes", "trie", "ignore_index", "eps", "constraint_range",
                                    "drop_worst_ratio"]
    assert sig.parameters["constraint_range"].default is None and sig.parameters["drop_worst_ratio"].default == 0.0
    ev = inspect.signature(ops.trie_head_eval)
    assert list(ev.parameters)[:8] == ["feats", "weight", "bias", "target", "nodes", "trie", "pad", "eps"] and ev.parameters["acc"].default is None
    assert inspect.signature(TrainStep.__init__).parameters["closed_set_edge_head"].default is False
    assert CommonConfig().closed_set_edge_head is False and Trainer(closed_set_edge_head=True).cfg.common.closed_set_edge_head is True
    for fn in ("trie_head_fwd", "trie_head_bwd_dx", "trie_head_bwd_dw", "trie_head_buckets"):
        assert callable(getattr(K, fn))
    b = hc.build_dw_case(torch.float32)
    x, W = b["x"].requires_grad_(True), b["W"].requires_grad_(True)
    old = {k: b["trie"][k] for k in ("node_edge_off", "edge_token", "N", "E")}           # the node criterion's dict: no inverse CSR
    with pytest.raises(ValueError, match="edge_node"):
        ops.trie_head_cross_entropy(x, W, None, b["t"], b["nodes"], old, 1, 0.1)
    with pytest.raises(ValueError, match="max_degree"):
        ops.trie_head_eval(x, W, None, b["t"], b["nodes"], old, 1, 0.1)
    with pytest.raises(ValueError, match="drop_worst_ratio"):
        ops.trie_head_cross_entropy(x, W, None, b["t"], b["nodes"], b["trie"], 1, 0.1, drop_worst_ratio=1.0)
    with pytest.raises(ValueError, match="nodes"):
        ops.trie_head_cross_entropy(x, W, None, b["t"], b["nodes"][:3], b["trie"], 1, 0.1)
    with pytest.raises(ValueError, match="projection is"):
        ops.trie_head_cross_entropy(x, W.detach().to(torch.bfloat16), None, b["t"], b["nodes"], b["trie"], 1, 0.1)
