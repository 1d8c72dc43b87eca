"""GPU: the trie-edge head -- csrc/trie_head.hip (ofa_trie_head_fwd / _bwd_dx / _bwd_dw), ops.trie_head_cross_entropy /
ops.trie_head_eval and TrainStep(closed_set_edge_head=True).

The kernels against tests/closed_set_head_case's float64 oracle, every tolerance an a-priori bound (u = 2^-24, u_T the unit roundoff
of the output dtype):
  z                          the oracle                                D u sum_d |x_d w_d| (+ u |z| with a bias)
  lse, row_loss, row_nll     the oracle fed the kernel's own z         criterion_oracle.LSE_TOL / LSROW_TOL
  g                          the oracle fed the kernel's own z         G32_TOL x its magnitude bound
  row_cnt, row_hit           the oracle                                exact
  dX                         the oracle fed the kernel's own g         (u_T + C u) sum_j |g_j W[tok_j, d]|
  dW (dbias)                 the oracle fed the kernel's own g         (u_T + n u) sum |g x| + u_T |prior|, n = contributing (row, edge) pairs
(fp16 outputs: plus half a subnormal spacing, 2^-25, see UNDERFLOW.)  Where a bound is 0 the element is exactly 0.  Output buffers are NaN-poisoned, the dW destination holds a known prior and the rows
nobody touches keep its bits.  The worst shares are printed with -s (DESIGN.md 5s records them)."""
import numpy as np
import pytest
import torch

from tests import closed_set_head_case as hc
from tests import closed_set_train_case as cst
from tests import criterion_oracle as co
from tests.traverse_case import ANSWERS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
F32, F64 = torch.float32, torch.float64
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
WORST = {}


@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def plan():
    from ofasys_amd.traverse import TraversePlan
    return TraversePlan(ANSWERS, 0, 2, 1)


def _poison(*specs):
    """NaN-filled tensors of exactly the sizes the wrapper is about to torch.empty, freed again: the caching allocator hands those
    blocks straight back, so an element the kernel leaves unwritten reads NaN."""
    keep = [torch.full(shape, NAN, dtype=dtype, device=DEV) if dtype.is_floating_point else
            torch.full(shape, -77, dtype=dtype, device=DEV) for shape, dtype in specs]
    torch.cuda.synchronize()
    del keep


def _note(name, dtype, value):
    key = (name, NAMES[dtype])
    WORST[key] = max(WORST.get(key, 0.0), value)


# fp16 outputs underflow gradually: below 2^-14 the spacing is 2^-24 whatever the value, so a correctly rounded result is off by up to
# half of it where u_T |value| is smaller (a dX element of a planted row; a dW element whose prior is below 2^-14).  The relative bounds
# above hold for normal numbers; this is the absolute term of the standard rounding model for the one format that needs it.
UNDERFLOW = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}


def _share(name, got, ref, bound, dtype, tag, floor=0.0):
    """max (|got - ref| - floor) / bound over bound > 0 (must be <= 1); exactly 0 where bound == 0; everything finite."""
    e = co.excess(got.detach().cpu(), ref, bound, 1.0, floor)
    _note(name, dtype, e)
    assert e <= 1.0, (tag, name, e)


def _gs(b):
    return torch.tensor([b["gs"]], dtype=F32, device=DEV)


def _range(b):
    return b["crange"] if b["crange"] is not None else (-1, -1)


def _forward(K, b, want_hit=True):
    R, Cmax = b["x"].shape[0], b["trie"]["max_degree"]
    _poison(((R, Cmax), F32), ((R, Cmax), F32), ((R,), F32), ((R,), F32), ((R,), F32), ((R,), F32), ((R,), torch.int32))
    return K.trie_head_fwd(b["x"], b["W"], b["bias"], b["t"], b["nodes"], b["trie"], co.IGNORE, b["eps"], *_range(b), want_grad=True,
                           want_hit=want_hit)


def _check_kernels(K, b, dtype, tag, prior_seed=7):
    """The three launches on one case -> dict of every output (for the determinism test)."""
    R, D = b["x"].shape
    V, Cmax = b["V"], b["trie"]["max_degree"]
    out = _forward(K, b)
    torch.cuda.synchronize()
    ref0 = hc.head_reference(b)
    tok, A, deg = ref0["tok"], ref0["A"], ref0["deg"]
    inside = torch.arange(Cmax)[None, :] < deg[:, None]
    z, g = out["z"].cpu(), out["g"].cpu()
    assert out["z"].dtype == out["g"].dtype == F32 and bool(torch.isfinite(z[inside]).all()) and bool(torch.isfinite(g[inside]).all()), \
        (tag, "a slot inside the degree was not written")
    # z against the oracle
    _share("z", z.masked_fill(~A, 0.0), ref0["z"], ref0["zbound"], dtype, tag)
    # the row core against the oracle fed the kernel's own z
    ref = hc.head_reference(b, z=z)
    good, dead, ignored = ref["good"], ref["dead"], ref["ignored"]
    assert torch.equal(out["row_cnt"].cpu().double(), ref["row_cnt"]), (tag, "row_cnt")
    assert torch.equal(out["row_hit"].cpu(), ref["hit"]), (tag, "row_hit", out["row_hit"], ref["hit"])
    for name, tol in (("lse", co.LSE_TOL), ("row_loss", co.LSROW_TOL), ("row_nll", co.LSROW_TOL)):
        got = out[name].cpu()
        e = float((got[good].double() - ref[name][good]).abs().max())
        _note(name, dtype, e / tol)
        assert bool(torch.isfinite(got[good]).all()) and e <= tol, (tag, name, e, tol)
    rl, rn, lse = out["row_loss"].cpu(), out["row_nll"].cpu(), out["lse"].cpu()
    assert bool((rl[ignored] == 0).all()) and bool((rn[ignored] == 0).all()), (tag, "ignored rows")
    assert bool((rl[dead] == INF).all()) and bool((rn[dead] == INF).all()), (tag, "+inf rows", rl)
    assert bool((lse[~A.any(1)] == -INF).all()), (tag, "lse of rows without an allowed child")
    e = co.excess(g.masked_fill(~inside, 0.0), ref["g"], ref["gbound"], 1.0, co.floor_of(F32, 1.0))
    _note("g", dtype, e / co.G32_TOL)
    assert e <= co.G32_TOL, (tag, "g", e)
    assert float(g.masked_fill(~inside, 0.0)[~good | ignored].abs().max()) == 0.0, (tag, "g of ignored / filler / dead rows")
    # dX against the oracle fed the kernel's own g
    _poison(((R, D), dtype))
    dx = K.trie_head_bwd_dx(out["g"], b["W"], b["t"], b["nodes"], b["trie"], b["row_w"], _gs(b), co.IGNORE, *_range(b))
    torch.cuda.synchronize()
    assert dx.dtype == dtype and dx.shape == (R, D)
    rx, mx = hc.dx_reference(b, g, tok, A)
    C = ref["row_cnt"]
    _share("dX", dx, rx, (hc.U_T[dtype] + C * hc.U32)[:, None] * mx, dtype, tag, UNDERFLOW[dtype])
    # dW (and dbias) against the oracle fed the kernel's own g, onto a known prior
    gen = torch.Generator(device="cpu").manual_seed(prior_seed)
    prior = torch.randn(V, D, generator=gen).to(dtype)
    prior_b = torch.randn(V, generator=gen).to(dtype) if b["bias"] is not None else None
    dW = prior.to(DEV)
    db = prior_b.to(DEV) if prior_b is not None else None
    buckets = K.trie_head_buckets(b["nodes"], b["trie"])
    K.trie_head_bwd_dw(out["g"], b["x"], b["trie"], buckets, b["row_w"], _gs(b), dW, db, *_range(b))
    torch.cuda.synchronize()
    rw, mw, n, rb, mb = hc.dw_reference(b, g, tok, A)
    un = n == 0
    assert torch.equal(dW.cpu()[un].view(torch.int16 if dtype != F32 else torch.int32),
                       prior[un].view(torch.int16 if dtype != F32 else torch.int32)), (tag, "a row of dW nobody touches changed")
    u_t = hc.U_T[dtype]
    bound = (u_t + n * hc.U32)[:, None] * mw + u_t * prior.double().abs()
    err = ((dW.cpu().double() - (prior.double() + rw)).abs() - UNDERFLOW[dtype]).clamp_min(0)
    assert bool(torch.isfinite(dW).all())
    share = float((err[~un] / bound[~un]).max()) if bool((~un).any()) else 0.0
    _note("dW", dtype, share)
    assert share <= 1.0, (tag, "dW", share)
    if db is not None:
        assert torch.equal(db.cpu()[un], prior_b[un]), (tag, "dbias of a token nobody touches")
        bb = (u_t + n * hc.U32) * mb + u_t * prior_b.double().abs()
        eb = ((db.cpu().double() - (prior_b.double() + rb)).abs() - UNDERFLOW[dtype]).clamp_min(0)
        share = float((eb[~un] / bb[~un]).max()) if bool((~un).any()) else 0.0
        _note("dbias", dtype, share)
        assert share <= 1.0, (tag, "dbias", share)
    return dict(out, dx=dx, dW=dW, db=db, buckets=buckets)


CASE_IDS = [f"c{c.idx}-V{c.trie.V}-D{c.D}" for c in hc.HEAD_CASES]


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=[NAMES[d] for d in co.DTYPES3])
@pytest.mark.parametrize("case", hc.HEAD_CASES, ids=CASE_IDS)
def test_head_kernels_against_the_float64_oracle(K, case, dtype):
    b = hc.build_head_case(case, dtype, DEV)
    assert "dead_node" in b["kinds"] and "ignored" in b["kinds"] and "filler" in b["kinds"] and "not_child" in b["kinds"]
    _check_kernels(K, b, dtype, (case, NAMES[dtype]))


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=[NAMES[d] for d in co.DTYPES3])
def test_rows_that_share_nodes_and_tokens(K, dtype):
    """Three rows on one node, two on another, token 9 under both (a target here, a non-target child there), a node whose only row
    is ignored, tokens no row touches, a dropped row -- and the hit tie of two bit-identical weight rows: the lowest token wins."""
    b = hc.build_dw_case(dtype, device=DEV)
    out = _check_kernels(K, b, dtype, ("dw", NAMES[dtype]))
    z = out["z"].cpu()
    assert float(z[6, 0]) == float(z[6, 1]) and float(z[7, 0]) == float(z[7, 1])      # the twins' logits: the same bits in either row
    assert out["row_hit"].cpu().tolist()[6:] == [1, 0]
    # a validation launch (no g) gives the same rows
    ev = K.trie_head_fwd(b["x"], b["W"], b["bias"], b["t"], b["nodes"], b["trie"], co.IGNORE, b["eps"], want_grad=False, want_hit=True)
    assert ev["g"] is None
    for k in ("lse", "row_loss", "row_nll", "row_cnt", "row_hit"):
        assert torch.equal(ev[k], out[k]), k


def test_worst_shares_are_reported():
    for key in sorted(WORST):
        print(f"  worst share {key[0]:9s} {key[1]}: {WORST[key]:.3f}")


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=["bf16", "fp32"])
def test_two_calls_give_identical_bits(K, dtype):
    for b in (hc.build_dw_case(dtype, device=DEV), hc.build_head_case(hc.HEAD_CASES[11], dtype, DEV)):
        runs = []
        for _ in range(2):
            out = _forward(K, b)
            dx = K.trie_head_bwd_dx(out["g"], b["W"], b["t"], b["nodes"], b["trie"], b["row_w"], _gs(b), co.IGNORE, *_range(b))
            dW = torch.zeros_like(b["W"])
            db = torch.zeros(b["V"], dtype=dtype, device=DEV)
            bk = K.trie_head_buckets(b["nodes"], b["trie"])
            K.trie_head_bwd_dw(out["g"], b["x"], b["trie"], bk, b["row_w"], _gs(b), dW, db, *_range(b))
            inside = torch.arange(out["z"].shape[1], device=DEV)[None, :] < hc.slots_of(b)[2].to(DEV)[:, None]
            runs.append([out["z"].masked_fill(~inside, 0), out["g"].masked_fill(~inside, 0), out["lse"], out["row_loss"], out["row_nll"],
                         out["row_cnt"], out["row_hit"], dx, dW, db, bk[0], bk[1]])
        torch.cuda.synchronize()
        for i, (p, q) in enumerate(zip(*runs)):
            assert torch.equal(p, q) or (p.dtype.is_floating_point and torch.equal(p.isnan(), q.isnan()) and
                                         torch.equal(p.nan_to_num(0), q.nan_to_num(0))), i


def test_row_buckets(K):
    b = hc.build_dw_case(torch.float32, device=DEV)
    rows, off = K.trie_head_buckets(b["nodes"], b["trie"])
    assert rows.dtype == off.dtype == torch.int32
    assert rows.cpu().tolist() == [0, 1, 2, 3, 4, 6, 7, 5] and off.cpu().tolist() == [0, 3, 5, 7, 7, 8]
    nodes = torch.tensor([2, -1, 0, 99, 2, 0], dtype=torch.int32, device=DEV)         # nodes outside [0, N) sort past every bucket
    rows, off = K.trie_head_buckets(nodes, b["trie"])
    assert rows.cpu().tolist() == [2, 5, 0, 4, 1, 3] and off.cpu().tolist() == [0, 2, 2, 4, 4, 4]


# ------------------------------------------------------------------------------------------------------------------ the gradient sinks
@pytest.mark.parametrize("order", ("alone", "after_dense", "before_dense"))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=["bf16", "fp32"])
def test_partial_writer_composes_with_first_touch(K, dtype, order):
    """weight._ofa_grad a view of an arena pre-filled with 3.0, between grad_begin and grad_end: the head's weight gradient alone,
    after a dense full writer of the same view and before one -- each equals the same sequence on a zero-filled arena, bit for bit
    (the technique of tests/test_grad_first_touch_gpu.py)."""
    from ofasys_amd import ops
    b = hc.build_dw_case(dtype, device=DEV)
    V, D = b["V"], b["D"]
    gen = torch.Generator(device="cpu").manual_seed(11)
    dy = (torch.randn(16, V, generator=gen) * 0.1).to(dtype).to(DEV)
    x2 = torch.randn(16, D, generator=gen).to(dtype).to(DEV)
    got, fired = {}, {}
    for fill in (3.0, 0.0):
        arena = torch.full((64 + V * D + V + 200,), fill, dtype=dtype, device=DEV)
        weight = b["W"].clone().requires_grad_(True)
        bias = b["bias"].clone().requires_grad_(True)
        weight._ofa_grad = arena[64:64 + V * D].view(V, D)
        bias._ofa_grad = arena[64 + V * D:64 + V * D + V]
        count = [0]
        weight._ofa_grad_ready = lambda: count.__setitem__(0, count[0] + 1)
        feats = b["x"].clone().requires_grad_(True)
        ops.grad_begin(arena)
        try:
            if order == "after_dense":
                K.gemm(dy, x2, True, False, out=weight._ofa_grad, accumulate=True)
            loss, _, _ = ops.trie_head_cross_entropy(feats, weight, bias, b["t"], b["nodes"], b["trie"], co.IGNORE, b["eps"])
            loss.backward(torch.tensor(b["gs"], dtype=F32, device=DEV))
            if order == "before_dense":
                K.gemm(dy, x2, True, False, out=weight._ofa_grad, accumulate=True)
            demand, unused = ops.grad_end()
        except BaseException:
            ops.grad_abort()
            raise
        torch.cuda.synchronize()
        assert weight.grad is None and bias.grad is None and feats.grad is not None      # the sinks took both gradients
        got[fill], fired[fill] = (arena.clone(), feats.grad.clone()), count[0]
    assert torch.equal(got[3.0][0], got[0.0][0]) and torch.equal(got[3.0][1], got[0.0][1])
    assert fired[3.0] == fired[0.0] == 1
    gw = got[3.0][0][64:64 + V * D].view(V, D).float()
    assert float(got[3.0][0][:64].abs().max()) == 0.0 and float(gw.abs().max()) > 0        # what nobody wrote is cleared; the rows landed
    if order == "alone":
        assert float(gw[list(hc.DW_UNTOUCHED)].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ the op
def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


def _op_inputs(which, plan):
    if which == "shared":
        b = hc.build_dw_case(F32, device=DEV)
        return b["x"], b["W"], b["bias"], b["t"], b["nodes"], b["trie"]
    V, D = int(plan.edge_token.max()) + 10, 64
    sb = cst.step_batch(0, plan, V)
    gen = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(sb["target"].numel(), D, generator=gen).to(DEV)
    W = (torch.randn(V, D, generator=gen) * (2.0 / D ** 0.5)).to(DEV)
    return x.view(4, -1, D), W, None, sb["target"].to(DEV), sb["nodes"].to(DEV), plan.head_arrays(DEV)


@pytest.mark.parametrize("ratio", (0.0, 0.85))
@pytest.mark.parametrize("which", ("shared", "answers"))
def test_op_against_the_dense_route(plan, which, ratio):
    """fp32: ops.trie_head_cross_entropy against ops.linear + ops.trie_label_smoothed_cross_entropy (the behaviour of the dense head,
    pinned by tests/test_closed_set_train_gpu.py): loss, nll, dfeats, dW (dbias) within the project's fp32 parity, 1e-3 relative;
    ntokens exactly."""
    from ofasys_amd import ops
    x, W, bias, t, nodes, trie = _op_inputs(which, plan)
    res = {}
    for route in ("dense", "head"):
        xx, ww = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
        bb = bias.clone().requires_grad_(True) if bias is not None else None
        if route == "dense":
            loss, nll, ntok = ops.trie_label_smoothed_cross_entropy(ops.linear(xx, ww, bb), t, nodes, trie, co.IGNORE, 0.1,
                                                                    drop_worst_ratio=ratio)
        else:
            loss, nll, ntok = ops.trie_head_cross_entropy(xx, ww, bb, t, nodes, trie, co.IGNORE, 0.1, drop_worst_ratio=ratio)
        loss.backward(torch.tensor(0.5, device=DEV))
        torch.cuda.synchronize()
        res[route] = (loss.detach(), nll.detach(), int(ntok), xx.grad, ww.grad, None if bb is None else bb.grad)
    d, h = res["dense"], res["head"]
    assert d[2] == h[2] and d[2] > 0, (d[2], h[2])
    figures = dict(loss=_rel(h[0], d[0]), nll=_rel(h[1], d[1]), dfeats=_rel(h[3], d[3]), dW=_rel(h[4], d[4]))
    if bias is not None:
        figures["dbias"] = _rel(h[5], d[5])
    print(f"\n{which} drop_worst={ratio}: ntokens {h[2]}, head vs dense {figures}")
    assert h[3].shape == x.shape and h[4].shape == W.shape
    assert all(v <= 1e-3 for v in figures.values()), figures


def test_trie_head_eval_against_criterion_eval(plan):
    from ofasys_amd import ops
    x, W, bias, t, nodes, trie = _op_inputs("shared", plan)
    acc_d, *rows_d = ops.criterion_eval(ops.linear(x, W, bias), t, co.IGNORE, 0.1, nodes=nodes, trie=trie)
    acc_h, *rows_h = ops.trie_head_eval(x, W, bias, t, nodes, trie, co.IGNORE, 0.1)
    torch.cuda.synchronize()
    assert acc_h[0] == acc_d[0] and acc_h[3] == acc_d[3]
    assert _rel(acc_h[1:3], acc_d[1:3]) <= 1e-3 and torch.equal(rows_h[2], rows_d[2])


# ------------------------------------------------------------------------------------------------------------------ the step
SRC_LEN = [23, 9, 17, 12]


def _case(dropout=0.0):
    return {"arch": "tiny", "active": {"text"}, "overrides": {"use_self_attn_bias": False, "entangle_position_embedding": True,
                                                              "dropout": dropout},
            "adaptor_overrides": {"text": {"entangle_position_embedding": True}}}


def _sample(which, plan, trie, V, dtype, pack=False, nodes=True):
    from oracle import recipe
    from ofasys_amd.packing import build_pack_plan
    from tests.model_util import make_slots
    b = cst.step_batch(which, plan, V)
    src = recipe.tokens(f"closed_set_head.src{which}", (4, 23), V, SRC_LEN)
    s = {"slots": make_slots([("TEXT", True, src, None), ("TEXT", False, b["prev"], None)], DEV, dtype), "target": b["target"].to(DEV)}
    if nodes:
        s["constraint_nodes"] = b["nodes"].to(DEV)
        s["constraint_trie"] = trie
    if pack:
        s["pack"] = build_pack_plan(src.eq(1), b["prev"].eq(1), bucket=64).to(DEV)
    return s


def _engine(dtype, head, dropout=0.0, **kw):
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    from tests.model_util import build_model
    model, d = build_model(_case(dropout), DEV, dtype)
    ops.manual_seed(1234)
    return TrainStep(model, lr=1e-3, clip_norm=1.0, label_smoothing=0.1, closed_set_edge_head=head, **kw), len(d)


def _grads(tr):
    names = {id(p): n for n, p in tr.model.named_parameters()}
    return {names.get(id(p), str(i)): tr.fp.grad[o:o + p.numel()].float().clone() for i, (p, o) in enumerate(zip(tr.fp.params, tr.fp.offsets))}


def _worst_tensor(gh, gd):
    """-> (share, name): the largest max |edge - dense| of a gradient tensor as a share of that tensor's max-abs in the dense step.
    The attention KEY biases are the exception: softmax does not see a shift of a query's scores, so their gradient is identically
    zero and what either step holds is the rounding residue of a sum that cancels (1e-8 where the arena's largest entry is O(1); the
    two steps' residues differ by about themselves).  They are held to 1e-3 of the largest entry of the whole arena instead."""
    top = max(float(g.abs().max()) for g in gd.values())
    scale = {n: top if n.endswith("k_proj.bias") else float(gd[n].abs().max()) for n in gd}
    shares = {n: float((gh[n] - gd[n]).abs().max()) / scale[n] for n in gd if float(gd[n].abs().max()) > 0}
    for n in sorted(shares, key=shares.get, reverse=True)[:4]:
        print(f"    {n}: share {shares[n]:.3e}, max-abs {float(gd[n].abs().max()):.3e}")
    n = max(shares, key=shares.get)
    return shares[n], n


def _one_step(dtype, head, plan, pack, samples=None):
    tr, V = _engine(dtype, head)
    trie = plan.head_arrays(DEV)
    batch = samples(plan, trie, V, dtype) if samples is not None else [_sample(0, plan, trie, V, dtype, pack)]
    stats = tr.train_step(batch, eager=True)["stats"].clone()
    torch.cuda.synchronize()
    return stats, _grads(tr), tr.fp.grad.float().clone()


def test_fp32_step_edge_head_against_the_node_step(plan, pack=False):
    """(padded: the project runs packed batches on the fused 16-bit attention kernels alone; the bf16 test below runs both layouts)"""
    sd, gd, _ = _one_step(F32, False, plan, pack)
    sh, gh, _ = _one_step(F32, True, plan, pack)
    assert float(sh[2]) == float(sd[2]) == 15 and float(sh[0]) == float(sd[0])
    rel = abs(float(sh[1]) - float(sd[1])) / abs(float(sd[1]))
    worst, name = _worst_tensor(gh, gd)
    print(f"\nfp32 step pack={pack}: loss {float(sh[1]):.6f} vs {float(sd[1]):.6f} (rel {rel:.2e}); worst gradient tensor {name}: {worst:.2e} of its max-abs")
    assert rel <= 1e-3 and worst <= 1e-3, (rel, worst, name)
    for n in gd:
        if float(gd[n].abs().max()) == 0:
            assert float(gh[n].abs().max()) == 0, n


@pytest.mark.parametrize("pack", (False, True), ids=["padded", "packed"])
def test_bf16_step_gap_is_within_twice_the_dense_routes_own(plan, pack):
    _, _, ref = _one_step(F32, False, plan, False)           # (fp32 runs padded: packed batches need the 16-bit attention kernels)
    _, _, dense = _one_step(torch.bfloat16, False, plan, pack)
    _, _, head = _one_step(torch.bfloat16, True, plan, pack)
    e_d, e_h = float((dense - ref).abs().max()), float((head - ref).abs().max())
    print(f"\nbf16 step pack={pack}: max-abs error over the arena against the fp32 node step: dense {e_d:.3e}, edge head {e_h:.3e}")
    assert np.isfinite(e_h) and e_h <= 2 * e_d


def test_packed_steps_replay_a_captured_graph(plan):
    """Six packed steps alternating the two batches: the replays of ONE captured graph equal the eager run bit for bit."""
    runs = {}
    for mode in ("eager", "graph"):
        tr, V = _engine(torch.bfloat16, True, use_graph=mode == "graph", graph_warmup=1)
        trie = plan.head_arrays(DEV)
        losses = [float(tr.train_step([_sample(step % 2, plan, trie, V, torch.bfloat16, True)])["stats"][1]) for step in range(6)]
        torch.cuda.synchronize()
        runs[mode] = (losses, tr.fp.flat.clone(), tr)
    print("\neager", runs["eager"][0], "graph", runs["graph"][0])
    assert runs["eager"][0] == runs["graph"][0] and torch.equal(runs["eager"][1], runs["graph"][1])
    assert runs["eager"][0][0] != runs["eager"][0][1]
    assert sum(1 for e in runs["graph"][2]._graphs.values() if "graphs" in e) == 1


@pytest.mark.parametrize("first", ("closed", "caption"))
def test_closed_set_and_caption_micro_batches_in_one_step(plan, first):
    """One closed-set micro-batch (edge head: a partial writer of the tied embedding's gradient) and one plain caption micro-batch
    (dense head: a full writer) in either order, against the same step with the dense head for both."""
    def two(plan, trie, V, dtype):
        a, b = _sample(0, plan, trie, V, dtype), _sample(1, plan, trie, V, dtype, nodes=False)
        return [a, b] if first == "closed" else [b, a]
    sd, gd, _ = _one_step(F32, False, plan, False, two)
    sh, gh, _ = _one_step(F32, True, plan, False, two)
    assert float(sh[2]) == float(sd[2]) == 30
    rel = abs(float(sh[1]) - float(sd[1])) / abs(float(sd[1]))
    worst, name = _worst_tensor(gh, gd)
    print(f"\ntwo micro-batches, {first} first: loss rel {rel:.2e}, worst gradient tensor {name}: {worst:.2e}")
    assert rel <= 1e-3 and worst <= 1e-3, (rel, worst, name)


def test_valid_step_with_the_edge_head(plan):
    """fp32, the planted batch (the projection row of every first target raised along its own feature row, so the arg-max is decided
    by a margin): ntokens and n_correct equal the dense valid_step's, loss and nll within 1e-3 relative."""
    accs = {}
    for head in (False, True):
        tr, V = _engine(F32, head)
        trie = plan.head_arrays(DEV)
        s = _sample(0, plan, trie, V, F32)
        with tr._valid_mode(tr.model):
            feats = tr._criterion_inputs(tr.model, s, features=True)[0].reshape(4, -1, tr.model.decoder.adaptor.embed_tokens.weight.shape[1])
        W = tr.output_projection(tr.model)[0]
        with torch.no_grad():
            for r in range(4):
                h = feats[r, 0].float()
                W[int(s["target"][r, 0])] += (12.0 * h / float((h * h).sum())).to(W.dtype)
        tr.valid_begin()
        tr.valid_step([s], eager=True)
        tr.valid_step([_sample(1, plan, trie, V, F32)], eager=True)
        torch.cuda.synchronize()
        accs[head] = tr._valid_acc.clone().cpu()
    d, h = accs[False], accs[True]
    print(f"\nvalid_step: dense {d.tolist()} edge head {h.tolist()}")
    assert h[0] == d[0] == 30 and h[3] == d[3] and d[3] >= 1
    assert abs(float(h[1] - d[1])) <= 1e-3 * abs(float(d[1])) and abs(float(h[2] - d[2])) <= 1e-3 * abs(float(d[2]))


def test_validation_between_train_steps_changes_no_bit(plan):
    runs = {}
    for validated in (False, True):
        tr, V = _engine(torch.bfloat16, True, dropout=0.1, use_graph=True, graph_warmup=1)
        trie = plan.head_arrays(DEV)
        stats = []
        for i in range(4):
            if validated and i == 2:
                tr.valid_begin()
                for w in (1, 0):
                    tr.valid_step([_sample(w, plan, trie, V, torch.bfloat16, True)])
                assert tr.valid_result()["ntokens"] == 30
            out = tr.train_step([_sample(i % 2, plan, trie, V, torch.bfloat16, True)])
            stats.append((out["stats"].clone(), out["gnorm"].clone()))
        torch.cuda.synchronize()
        runs[validated] = ([t.clone() for t in (tr.fp.flat, tr.master, tr.exp_avg, tr.exp_avg_sq, tr._step_t, tr._sched)], stats)
    for x, y in zip(runs[False][0], runs[True][0]):
        assert torch.equal(x, y)
    for (s1, g1), (s2, g2) in zip(runs[False][1], runs[True][1]):
        assert torch.equal(s1, s2) and torch.equal(g1, g2)


def test_step_refusals_stay(plan):
    tr, V = _engine(torch.bfloat16, True)
    trie = plan.head_arrays(DEV)
    s = _sample(0, plan, trie, V, torch.bfloat16)
    s["constraint_masks"] = cst.step_batch(0, plan, V)["masks"].to(DEV)
    with pytest.raises(ValueError, match="not both"):
        tr.train_step([s], eager=True)
    s = _sample(0, plan, trie, V, torch.bfloat16)
    s["reward"] = torch.ones(4, dtype=F32, device=DEV)
    with pytest.raises(NotImplementedError, match="constraint_nodes"):
        tr.train_step([s], eager=True)
    s = _sample(0, plan, trie, V, torch.bfloat16)
    del s["constraint_trie"]
    with pytest.raises(ValueError, match="constraint_trie"):
        tr.train_step([s], eager=True)
