"""GPU: closed-set training by trie node ids -- the node-form label-smoothed criterion (csrc/trie_loss.hip:
ofa_trie_ls_cross_entropy_fwd / _bwd), its autograd op and the train step that takes "constraint_nodes".

The kernel against float64: tests/criterion_oracle.lsce_reference fed the masks the nodes stand for (closed_set_train_case.
nodes_to_masks), in the manner of tests/test_criterion_edges_gpu.py -- every element of [rows, ld], output buffers NaN-poisoned, exactly
0 where the bound is 0, the project's tolerances (co.TOL, co.G32_TOL, co.LSE_TOL, co.LSROW_TOL; row_cnt exact).  The +inf rows (a live
target on node -1, a target that is no allowed child) and the rows without any allowed column are checked for their values and a zero
gradient row outside excess().  Against the REFERENCE: tests/golden/closed_set_train.npz (tools/gen_closed_set_train_golden.py) within
traverse_case.SCORE_TOL.  Measured on an MI355X (printed with -s): see DESIGN.md 5q."""
import os

import numpy as np
import pytest
import torch

from tests import closed_set_train_case as cs
from tests import criterion_oracle as co
from tests.traverse_case import ANSWERS, SCORE_TOL, score_err

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
NAN = float("nan")
INF = float("inf")
F32 = torch.float32
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "closed_set_train.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def plan():
    from ofasys_amd.traverse import TraversePlan
    return TraversePlan(ANSWERS, 0, 2, 1)


def _trie_on(plan, device=DEV):
    return {"node_edge_off": torch.from_numpy(plan.node_edge_off).to(device), "edge_token": torch.from_numpy(plan.edge_token).to(device),
            "N": plan.N, "E": plan.E}


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _poison(*specs):
    """NaN-filled tensors of exactly the sizes the wrapper is about to torch.empty, freed again: the caching allocator hands those
    blocks straight back, so an element the kernel leaves unwritten reads NaN."""
    keep = [_nan(shape, dtype) for shape, dtype in specs]
    torch.cuda.synchronize()
    del keep


def _gs(g):
    return torch.tensor([g], dtype=F32, device=DEV)


def _note(name, dtype, value):
    key = (name, NAMES[dtype])
    WORST[key] = max(WORST.get(key, 0.0), value)


def _grad_excess(name, got, ref, bd, dtype, g, tag):
    assert got.shape == ref.shape and got.dtype == dtype, (tag, got.shape, ref.shape, got.dtype)
    assert bool(torch.isfinite(got).all()), (tag, name, "not finite (an element that was not written reads NaN)")
    e = co.excess(got, ref, bd, co.EPS.get(dtype, 1.0), co.floor_of(dtype, g))
    limit = co.G32_TOL if dtype == F32 else co.TOL
    _note(name, dtype, e)
    assert e <= limit, (tag, name, e, limit)


def _f32_close(name, got, ref, tol, dtype, tag):
    assert got.dtype == F32 and bool(torch.isfinite(got).all()), (tag, name, "not finite")
    e = float((got.double() - ref).abs().max())
    _note(name, dtype, e / tol)
    assert e <= tol, (tag, name, e, tol)


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _check_rows(got, b, dtype, tag, row_w, name):
    """got: dict(lse, row_loss, row_nll, row_cnt or None each, d [R, stride])."""
    x, t, A, good, dead = b["x"], b["t"], b["A"], b["good"], b["dead"]
    stride = x.stride(0)
    xs = b["store"][good][:, :x.shape[1]]                    # the oracle's rows: the same row stride, so its gradients are [n, stride]
    assert xs.stride(0) == stride and int(good.sum()) > 1
    ref, bd = co.lsce_reference(xs, t[good], b["g"], b["eps"], crange=b["crange"], cmask=A[good],
                                row_w=None if row_w is None else row_w[good])
    d = got["d"]
    assert d.shape == (x.shape[0], stride) and d.dtype == dtype
    _grad_excess(f"{name} d", d[good], ref["d"], bd, dtype, b["g"], tag)
    rest = ~good
    assert bool(torch.isfinite(d).all()) and float(d[rest].float().abs().max()) == 0.0, (tag, "gradient rows of dead / empty rows")
    if got["lse"] is None:
        return
    C = A.sum(1).float()
    assert torch.equal(got["row_cnt"], C), (tag, "row_cnt", got["row_cnt"], C)
    _f32_close("lse", got["lse"][good], ref["lse"], co.LSE_TOL, dtype, tag)
    _f32_close("row_loss", got["row_loss"][good], ref["row_loss"], co.LSROW_TOL, dtype, tag)
    _f32_close("row_nll", got["row_nll"][good], ref["row_nll"], co.LSROW_TOL, dtype, tag)
    ignored = t == co.IGNORE
    assert bool((got["row_loss"][ignored] == 0).all()) and bool((got["row_nll"][ignored] == 0).all()), (tag, "ignored rows")
    assert int(dead.sum()) >= 2
    assert bool((got["row_loss"][dead] == INF).all()) and bool((got["row_nll"][dead] == INF).all()), (tag, "+inf rows", got["row_loss"])
    empty = ~A.any(1)
    assert int(empty.sum()) >= 2 and bool((got["lse"][empty] == -INF).all()), (tag, "lse of rows without an allowed column")
    some = rest & ~empty                                     # a dead row on a node that has allowed children: its lse is the node's
    if bool(some.any()):
        want = torch.logsumexp(x[some].double().masked_fill(~A[some], -INF), 1)
        _f32_close("lse", got["lse"][some], want, co.LSE_TOL, dtype, tag)


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=[NAMES[d] for d in co.DTYPES3])
def test_trie_kernel_against_float64(K, dtype):
    """Every case of closed_set_train_case.TRIE_CASES through the forward-with-gradient launch, the forward alone and the backward
    entry (row weights 1, 0, 0.5)."""
    for case in cs.TRIE_CASES:
        b = cs.build_trie_case(case, dtype, DEV)
        x, t = b["x"], b["t"]
        R, V = x.shape
        stride = x.stride(0)
        cs_, ce_ = case.crange if case.crange is not None else (-1, -1)
        tag = f"{NAMES[dtype]} {tuple(case)}"
        _poison(*[((R,), F32)] * 4, ((R, stride), dtype))
        lse, row_loss, row_nll, row_cnt, d = K.trie_ls_cross_entropy_fwd(x, t, b["nodes"], b["trie"], V, co.IGNORE, case.eps, cs_, ce_,
                                                                         grad_scale=_gs(case.g), want_grad=True)
        torch.cuda.synchronize()
        fwd = dict(lse=lse, row_loss=row_loss, row_nll=row_nll, row_cnt=row_cnt, d=d)
        _check_rows(fwd, b, dtype, tag + " fwd+grad", None, "fwd")
        _poison(*[((R,), F32)] * 4)
        alone = K.trie_ls_cross_entropy_fwd(x, t, b["nodes"], b["trie"], V, co.IGNORE, case.eps, cs_, ce_)
        torch.cuda.synchronize()
        assert alone[4] is None
        for a, w in zip(alone[:4], (lse, row_loss, row_nll, row_cnt)):
            assert torch.equal(a, w), (tag, "the forward alone")
        d2 = K.trie_ls_cross_entropy_bwd(x, t, b["nodes"], b["trie"], lse, row_cnt, b["row_w"], _gs(case.g), V, co.IGNORE, case.eps, cs_,
                                         ce_, dlogits=_nan((R, stride), dtype))
        torch.cuda.synchronize()
        _check_rows(dict(lse=None, d=d2), b, dtype, tag + " bwd", b["row_w"], "bwd")
        d3 = K.trie_ls_cross_entropy_bwd(x, t, b["nodes"], b["trie"], lse, row_cnt, None, _gs(case.g), V, co.IGNORE, case.eps, cs_, ce_,
                                         dlogits=_nan((R, stride), dtype))
        torch.cuda.synchronize()
        _check_rows(dict(lse=None, d=d3), b, dtype, tag + " bwd, no row_w", None, "bwd")
    print(f"\ntrie criterion {NAMES[dtype]}: " + ", ".join(f"{n} {v:.3g}" for (n, dn), v in sorted(WORST.items()) if dn == NAMES[dtype]),
          f"(gradients: excess in eps against {co.TOL} / error over bound against {co.G32_TOL:.3g}; fp32 outputs: share of tolerance)")


def test_fp32_path_against_the_reference(golden, plan):
    """ops.trie_label_smoothed_cross_entropy on fp32 logits against the reference's own label_smoothed_nll_loss and autograd: loss, nll
    and every element of the logits gradient within the project's standing bound (relative, floor absolute); ntokens exact."""
    from ofasys_amd import ops
    trie = _trie_on(plan)
    nodes = torch.from_numpy(golden["nodes"]).to(DEV)
    worst = 0.0
    for name in ("eps0", "eps01", "eps0_range", "eps01_range"):
        eps, c0, c1 = (float(v) for v in golden[f"{name}.cfg"])
        crange = None if c0 < 0 else (int(c0), int(c1))
        x = torch.from_numpy(golden["logits"]).to(DEV).requires_grad_(True)
        t = torch.from_numpy(golden[f"{name}.target"]).to(DEV)
        assert bool((t == 1).any())
        loss, nll, ntok = ops.trie_label_smoothed_cross_entropy(x, t, nodes, trie, 1, eps, crange)
        loss.backward()
        torch.cuda.synchronize()
        errs = (score_err(float(loss.detach()), golden[f"{name}.loss"][0]), score_err(float(nll.detach()), golden[f"{name}.nll_loss"][0]),
                score_err(x.grad.cpu(), golden[f"{name}.dlogits"]))
        print(name, "loss / nll / gradient error against the reference:", " ".join(f"{e:.2e}" for e in errs), "of", SCORE_TOL)
        worst = max(worst, *errs)
        assert int(ntok) == int(golden[f"{name}.ntokens"][0])
        assert max(errs) <= SCORE_TOL, (name, errs)
        assert bool((x.grad[t == 1] == 0).all())
    print(f"worst {worst:.2e}")


# ------------------------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("ratio", [0.0, 0.85])
def test_op_equals_the_mask_op(golden, plan, dtype, ratio):
    """Loss, nll and ntokens equal ops.label_smoothed_cross_entropy fed the expanded masks on the same logits: both are fp32 sums of
    rows that each sit within LSROW_TOL of float64."""
    from ofasys_amd import ops
    trie = _trie_on(plan)
    nodes = torch.from_numpy(golden["nodes"]).to(DEV)
    t = torch.from_numpy(golden["eps01.target"]).to(DEV)
    x = torch.from_numpy(golden["logits"]).to(DEV).to(dtype)
    V = x.shape[-1]
    masks = cs.nodes_to_masks(nodes, plan.node_edge_off, plan.edge_token, V).to(DEV)
    rows = t.numel()
    for crange in (None, (4, 100)):
        if crange is not None:
            t = torch.from_numpy(golden["eps01_range.target"]).to(DEV)
        a = ops.trie_label_smoothed_cross_entropy(x, t, nodes, trie, 1, 0.1, crange, ratio)
        m = ops.label_smoothed_cross_entropy(x, t, 1, 0.1, crange, masks, ratio)
        torch.cuda.synchronize()
        tol = 2 * co.LSROW_TOL * rows
        print(NAMES[dtype], ratio, crange, "loss", float(a[0]), float(m[0]), "nll", float(a[1]), float(m[1]), "ntokens", int(a[2]), "tol", tol)
        assert int(a[2]) == int(m[2]) and (ratio == 0 or int(a[2]) < int((t != 1).sum()))
        assert abs(float(a[0]) - float(m[0])) <= tol and abs(float(a[1]) - float(m[1])) <= tol
        assert not a[2].requires_grad


def _neighbours(a, b, dtype):
    """equal, or adjacent values of dtype (one rounding of two fp32 results a few ulps apart); exactly equal where one is 0"""
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= 2 * co.EPS[dtype] * torch.maximum(a.abs(), b.abs())).all())


def test_seeded_backward(K, golden, plan):
    """The gradient the forward launch wrote at the seed's scale is handed out once, to the backward seeded with that very tensor; a
    second backward, another tensor and a seed written to since all recompute through the backward entry.  Each meets float64."""
    from ofasys_amd import ops
    dtype = torch.bfloat16
    trie = _trie_on(plan)
    nodes = torch.from_numpy(golden["nodes"]).to(DEV).reshape(-1)
    t = torch.from_numpy(golden["eps01.target"]).to(DEV).reshape(-1)
    x = torch.from_numpy(golden["logits"]).to(DEV).to(dtype).reshape(t.numel(), -1)
    R, V = x.shape
    ld = (V + 7) // 8 * 8
    logits = x.clone().requires_grad_(True)                  # dense [70, 204]: the op pads the rows to 208 itself
    padded = torch.zeros(R, ld, dtype=dtype, device=DEV)
    padded[:, :V] = x
    A = cs.nodes_to_masks(nodes, plan.node_edge_off, plan.edge_token, V).to(DEV)
    live = t != 1

    def meets_reference(d, g, tag):
        assert d.shape == (R, V) and d.dtype == dtype
        ref, bd = co.lsce_reference(padded[live][:, :V], t[live], g, 0.1, cmask=A[live])
        _grad_excess("op d", torch.nn.functional.pad(d, (0, ld - V))[live], ref["d"], bd, dtype, g, tag)
        assert bool((d[~live] == 0).all())

    seed = torch.ones((), dtype=F32, device=DEV)
    loss, _, _ = ops.trie_label_smoothed_cross_entropy(logits, t, nodes, trie, 1, 0.1, seed=seed)
    want = K.trie_ls_cross_entropy_fwd(padded[:, :V], t, nodes, trie, V, 1, 0.1, grad_scale=seed.reshape(1), want_grad=True)[4][:, :V]
    first, = torch.autograd.grad(loss, logits, seed, retain_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(first, want) and float(first.float().abs().max()) > 0, "the first backward returns the forward launch's gradient"
    meets_reference(first, 1.0, "first")
    kept = first.clone()
    _poison(((R, ld), dtype))
    again, = torch.autograd.grad(loss, logits, seed, retain_graph=True)                                  # a second time: recomputed
    assert again.data_ptr() != first.data_ptr() and torch.equal(first, kept) and _neighbours(again, first, dtype)
    meets_reference(again, 1.0, "again")
    _poison(((R, ld), dtype))
    other, = torch.autograd.grad(loss, logits, torch.ones((), device=DEV), retain_graph=True)            # another tensor: recomputed
    assert other.data_ptr() != first.data_ptr() and torch.equal(first, kept) and _neighbours(other, first, dtype)
    meets_reference(other, 1.0, "other")
    seed2 = torch.ones((), dtype=F32, device=DEV)                                                        # a seed written to since
    loss2, _, _ = ops.trie_label_smoothed_cross_entropy(logits, t, nodes, trie, 1, 0.1, seed=seed2)
    seed2.mul_(2.0)
    changed, = torch.autograd.grad(loss2, logits, seed2)
    torch.cuda.synchronize()
    print("elements that differ from the first gradient: again", int((again != first).sum()), "other", int((other != first).sum()),
          "changed", int((changed.float() != first.float() * 2).sum()), "of", first.numel())
    assert _neighbours(changed.float(), first.float() * 2, dtype)
    meets_reference(changed, 2.0, "changed")
    # with drop_worst the forward is not seeded: the backward entry runs with the row weights
    loss3, _, ntok = ops.trie_label_smoothed_cross_entropy(logits, t, nodes, trie, 1, 0.1, drop_worst_ratio=0.5, seed=seed)
    dropped, = torch.autograd.grad(loss3, logits, seed)
    nonzero = int((dropped.float().abs().sum(1) > 0).sum())  # (a kept row on an EOS-only node has a zero gradient of its own)
    assert 0 < nonzero <= int(ntok) < int(live.sum())


# ------------------------------------------------------------------------------------------------------------------ the step
CASE = {"arch": "tiny", "active": {"text"}, "overrides": {"use_self_attn_bias": False, "entangle_position_embedding": True, "dropout": 0.0},
        "adaptor_overrides": {"text": {"entangle_position_embedding": True}}}
SRC_LEN = [23, 9, 17, 12]


def _sample(which, plan, trie, form, V, pack=False):
    from oracle import recipe
    from ofasys_amd.packing import build_pack_plan
    from tests.model_util import make_slots
    b = cs.step_batch(which, plan, V)
    src = recipe.tokens("closed_set_train.src", (4, 23), V, SRC_LEN)
    s = {"slots": make_slots([("TEXT", True, src, None), ("TEXT", False, b["prev"], None)], DEV, torch.bfloat16),
         "target": b["target"].to(DEV)}
    if form in ("masks", "both"):
        s["constraint_masks"] = b["masks"].to(DEV)
    if form in ("nodes", "both"):
        s["constraint_nodes"] = b["nodes"].to(DEV)
        s["constraint_trie"] = trie
    if pack:
        s["pack"] = build_pack_plan(src.eq(1), b["prev"].eq(1), bucket=64).to(DEV)
    return s


def _step(**kw):
    from ofasys_amd.trainer import TrainStep
    from tests.model_util import build_model
    model, d = build_model(CASE, DEV, torch.bfloat16)
    return TrainStep(model, lr=1e-3, clip_norm=1.0, label_smoothing=0.1, **kw), len(d)


def test_train_step_on_nodes(plan):
    """One TrainStep.train_step, dropout off, the same weights: nodes padded == masks padded within the two criterion kernels' row
    error (the logits are the same bits); nodes with a pack plan run and land within the packed-vs-padded bound of
    tests/test_packing_gpu.py."""
    trie = _trie_on(plan)
    loss = {}
    for form, pack in (("masks", False), ("nodes", False), ("nodes", True)):
        tr, V = _step()
        stats = tr.train_step([_sample(0, plan, trie, form, V, pack)], eager=True)["stats"]
        torch.cuda.synchronize()
        loss[form, pack] = float(stats[1])
        assert float(stats[2]) == 15                         # 11 answer tokens + 4 EOS
    rows = 20
    print("step loss: masks padded", loss["masks", False], "nodes padded", loss["nodes", False], "nodes packed", loss["nodes", True])
    assert abs(loss["nodes", False] - loss["masks", False]) <= 2 * co.LSROW_TOL * rows
    assert abs(loss["nodes", True] - loss["nodes", False]) <= 2e-3 * abs(loss["nodes", False])
    assert np.isfinite(loss["nodes", True]) and loss["nodes", False] > 0


def test_train_step_on_nodes_replays_a_captured_graph(plan):
    """Packed nodes samples under graph capture: warm-up, capture, then replays with the other batch's nodes copied into the static
    inputs -- bit for bit the eager run; the trie's arrays are the same tensors in every sample and are not copied."""
    trie = _trie_on(plan)
    before = {k: v.clone() for k, v in trie.items() if torch.is_tensor(v)}
    runs = {}
    for mode in ("eager", "graph"):
        tr, V = _step(use_graph=mode == "graph", graph_warmup=1)
        losses = []
        for step in range(6):
            losses.append(float(tr.train_step([_sample(step % 2, plan, trie, "nodes", V, True)])["stats"][1]))
        torch.cuda.synchronize()
        runs[mode] = (losses, tr)
    le, lg = runs["eager"][0], runs["graph"][0]
    print("eager", le, "graph", lg)
    assert le == lg                                          # replays == eager, bit for bit
    assert le[0] != le[1]                                    # (the two batches do differ)
    tr = runs["graph"][1]
    assert sum(1 for e in tr._graphs.values() if "graphs" in e) == 1
    for k, v in before.items():
        assert torch.equal(trie[k], v)


def test_train_step_refusals(plan):
    trie = _trie_on(plan)
    tr, V = _step()
    with pytest.raises(ValueError, match="not both"):
        tr.train_step([_sample(0, plan, trie, "both", V)], eager=True)
    s = _sample(0, plan, trie, "nodes", V)
    s["reward"] = torch.ones(4, dtype=F32, device=DEV)
    with pytest.raises(NotImplementedError, match="constraint_nodes"):
        tr.train_step([s], eager=True)
    s = _sample(0, plan, trie, "nodes", V)
    del s["constraint_trie"]
    with pytest.raises(ValueError, match="constraint_trie"):
        tr.train_step([s], eager=True)
    with pytest.raises(NotImplementedError, match="pack plan"):           # the refusal that stays: masks are laid out by padded position
        tr.train_step([_sample(0, plan, trie, "masks", V, pack=True)], eager=True)
