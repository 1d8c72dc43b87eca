"""GPU: first-touch gradient writes.  Every gradient sink, told by the step's touched set (ops.grad_mode) that it is the first full
writer of its view, STORES over an output holding the finite sentinel 3.0 -- and must leave exactly the numbers the same launch leaves
when it ADDS onto zeros (compared with torch.equal: as numbers, a stored -0.0 equals the +0.0 that 0 + -0.0 gives).  Then one tiny
train step, first-touch against the arena-wide fill of before (the debug library's OFA_STEP_TAIL_OLD switch) and eager against replay."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from ofasys_amd import kernels as K
from ofasys_amd import ops
from ofasys_amd.lib import dtype_code, lib, stream

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
SENTINEL = 3.0


class _Arena:
    """A gradient arena of sentinels with a running step around it: views carved from it are asked about as a train step's are."""

    def __init__(self, numel, dtype):
        self.buf = torch.full((numel,), SENTINEL, dtype=dtype, device=DEV)
        self.off = 0

    def view(self, *shape):
        n = 1
        for s in shape:
            n *= s
        v = self.buf[self.off:self.off + n].view(*shape)
        self.off += (n + 7) // 8 * 8
        assert self.off <= self.buf.numel()
        return v

    def __enter__(self):
        ops.grad_begin(self.buf)
        return self

    def __exit__(self, *exc):
        ops.grad_abort()
        return False


def _group(products, dtype, splits):
    """ofa_gemm_group_tn over products [(dy [k, m], x [k, n], out [m, n])] with the K-slice count forced to `splits`: one slice writes
    out directly (the per-item store bit), more go through fp32 slabs and a fold job that takes the mode."""
    arr = (K._GroupItem * len(products))()
    slabs = []
    for it, (dy, x, out) in zip(arr, products):
        it.a, it.b, it.lda, it.ldb = dy.data_ptr(), x.data_ptr(), dy.stride(0), x.stride(0)
        it.m, it.n, it.k, it.splits = dy.shape[1], x.shape[1], dy.shape[0], splits
        if splits == 1:
            it.out, it.ldo, it.out_alpha = out.data_ptr(), out.stride(0), 0.5
            it.store = int(not K._accum(out, True))
            slabs.append(None)
        else:
            sl = torch.empty(splits * it.m * it.n, dtype=torch.float32, device=DEV)
            it.slabs = sl.data_ptr()
            slabs.append(sl)
    lib().call("ofa_gemm_group_tn", ctypes.addressof(arr), len(products), dtype_code(products[0][0]), stream())
    q = K.FoldQueue()
    for it, sl, (dy, x, out) in zip(arr, slabs, products):
        if sl is not None:
            q.add(sl, 0, out, it.m * it.n, it.m * it.n, splits, 0.5, True)
    q.flush()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("k,splits", [(64, 1), (100, 1), (100, 2)], ids=["k64-direct", "k100-direct", "k100-slabs"])
def test_grouped_launch_store_equals_add_onto_zeros(dtype, k, splits):
    """Two items per launch: 256 x 256 (whole tiles) and 320 x 272 (partial tiles); k = 100 takes the zero-source path of a row count
    that is no multiple of the 64-row K tile."""
    torch.manual_seed(k + splits)
    shapes = [(256, 256), (320, 272)]
    ops_ = [(torch.randn(k, m, device=DEV).to(dtype), torch.randn(k, n, device=DEV).to(dtype)) for m, n in shapes]
    zeros = [torch.zeros(m, n, dtype=dtype, device=DEV) for m, n in shapes]
    _group([(dy, x, o) for (dy, x), o in zip(ops_, zeros)], dtype, splits)               # no step running: adds onto the zeros
    with _Arena(sum(m * n for m, n in shapes), dtype) as ar:
        outs = [ar.view(m, n) for m, n in shapes]
        _group([(dy, x, o) for (dy, x), o in zip(ops_, outs)], dtype, splits)            # first writers: store over the sentinels
        second = [o.clone() for o in outs]
        _group([(dy, x, o) for (dy, x), o in zip(ops_, outs)], dtype, splits)            # second writers of the step: add
    torch.cuda.synchronize()
    for (dy, x), z, s, o in zip(ops_, zeros, second, outs):
        assert torch.equal(s, z)
        ref = 0.5 * (dy.float().t() @ x.float())
        assert (z.float() - ref).abs().max() <= 2.0 ** -7 * ref.abs().max()              # (and it is the product: 8 significant bits)
        if splits == 1:                              # direct: the rounded product plus the rounded gradient, rounded
            assert torch.equal(o, (s.float() + z.float()).to(dtype))
        else:                                        # slabs: the fold adds in fp32 and rounds once
            assert not torch.equal(o, s) and (o.float() - 2 * ref).abs().max() <= 2.0 ** -7 * 2 * ref.abs().max()


@pytest.mark.parametrize("accumulate", [True, False], ids=["accum", "plain"])
def test_gemm_store_equals_add_onto_zeros(accumulate):
    torch.manual_seed(1)
    dt = torch.bfloat16
    dy, x = torch.randn(64, 128, device=DEV).to(dt), torch.randn(64, 128, device=DEV).to(dt)
    zero = torch.zeros(128, 128, dtype=dt, device=DEV)
    K.gemm(dy, x, True, False, alpha=0.5, out=zero, accumulate=True)
    with _Arena(128 * 128, dt) as ar:
        out = ar.view(128, 128)
        K.gemm(dy, x, True, False, alpha=0.5, out=out, accumulate=accumulate)
        first = out.clone()
        if accumulate:
            K.gemm(dy, x, True, False, alpha=0.5, out=out, accumulate=True)              # the second writer adds
        _, unused = ops.grad_end()
    assert torch.equal(first, zero)
    assert unused == []                              # a plain store is a writer too: grad_end does not clear what it wrote
    assert torch.equal(out, (zero.float() * 2).to(dt) if accumulate else zero)


@pytest.mark.parametrize("nslots,lanes16", [(3, False), (17, False), (17, True)], ids=["3-rows", "17-rows-8-lanes", "17-rows-16-lanes"])
def test_fold_job_store_equals_add_onto_zeros(nslots, lanes16):
    torch.manual_seed(nslots)
    cols, dt = 200, torch.bfloat16
    part = torch.randn(nslots, cols, device=DEV)
    zero = torch.zeros(cols, dtype=dt, device=DEV)
    q = K.FoldQueue()
    q.add(part, 0, zero, cols, cols, nslots, 0.25, True, lanes16=lanes16)
    q.flush()
    with _Arena(cols, dt) as ar:
        out = ar.view(cols)
        q.add(part, 0, out, cols, cols, nslots, 0.25, True, lanes16=lanes16)
        q.flush()
        first = out.clone()
        q.add(part, 0, out, cols, cols, nslots, 0.25, True, lanes16=lanes16)
        q.flush()
    assert torch.equal(first, zero) and bool((zero != 0).any())
    # the second writer: fp32 (alpha * sum + what is there), rounded once (alpha a power of two: no FMA question)
    assert torch.equal(out, (first.float() + 0.25 * _slot_sum(part, lanes16)).to(dt))


def _slot_sum(part, lanes16):
    """The fold kernel's fp32 sum over the slots, in its own order: a store into an fp32 output."""
    out = torch.zeros(part.shape[1], dtype=torch.float32, device=DEV)
    q = K.FoldQueue()
    q.add(part, 0, out, part.shape[1], part.shape[1], part.shape[0], 1.0, False, lanes16=lanes16)
    q.flush()
    return out


@pytest.mark.parametrize("deferred", [False, True], ids=["immediate", "fold-queue"])
def test_layernorm_reduce_store_equals_add_onto_zeros(deferred):
    torch.manual_seed(2)
    rows, cols, dt = 300, 256, torch.bfloat16
    x, dy = torch.randn(rows, cols, device=DEV).to(dt), torch.randn(rows, cols, device=DEV).to(dt)
    g, b = torch.randn(cols, device=DEV).to(dt), torch.randn(cols, device=DEV).to(dt)
    _, mean, rstd = K.layernorm_fwd(x, g, b)

    def run(dg, db):
        q = K.FoldQueue() if deferred else None
        K.layernorm_bwd(dy, x, g, mean, rstd, dgamma=dg, dbeta=db, fold=q)
        if q is not None:
            q.flush()

    zg, zb = torch.zeros(cols, dtype=dt, device=DEV), torch.zeros(cols, dtype=dt, device=DEV)
    run(zg, zb)
    with _Arena(2 * cols, dt) as ar:
        dg, db = ar.view(cols), ar.view(cols)
        run(dg, db)
        fg, fb = dg.clone(), db.clone()
        run(dg, db)
    assert torch.equal(fg, zg) and torch.equal(fb, zb) and bool((zg != 0).any())
    assert not torch.equal(dg, fg)                   # the second call added


def test_c_attn_grad_and_batch_sum_store_equal_add_onto_zeros():
    torch.manual_seed(3)
    dt = torch.bfloat16
    B, H, T, ld = 3, 2, 5, 8
    delta = torch.randn(B * H, ld, device=DEV)
    c = (torch.rand(H, device=DEV) + 0.5).to(dt)
    xs = torch.randn(3, 40, device=DEV).to(dt)
    zc, zs = torch.zeros(H, dtype=dt, device=DEV), torch.zeros(40, dtype=dt, device=DEV)
    K.c_attn_grad(delta, c, B, H, T, out=zc, accumulate=True)
    K.batch_sum(xs, 3, out=zs, accumulate=True)
    with _Arena(64, dt) as ar:
        oc, os_ = ar.view(H), ar.view(40)
        K.c_attn_grad(delta, c, B, H, T, out=oc, accumulate=True)
        K.batch_sum(xs, 3, out=os_, accumulate=True)
        fc, fs = oc.clone(), os_.clone()
        K.c_attn_grad(delta, c, B, H, T, out=oc, accumulate=True)
        K.batch_sum(xs, 3, out=os_, accumulate=True)
    assert torch.equal(fc, zc) and torch.equal(fs, zs)
    assert torch.equal(oc, (fc.float() * 2).to(dt)) and torch.equal(os_, (fs.float() * 2).to(dt))


def test_partial_writer_clears_on_demand_and_unwritten_views_are_cleared_at_the_end():
    """ofa_embedding_bwd_ids touches the rows of its ids only: what is under it is cleared first (ofa_zero_batched), once; a view nobody
    writes is cleared by grad_end."""
    torch.manual_seed(4)
    dt = torch.bfloat16
    V, D = 37, 16
    ids = torch.tensor([[1, 5, 5, 30]], device=DEV)
    dout = torch.randn(1, 4, D, device=DEV).to(dt)
    want = K.embedding_bwd(dout, ids, V)
    with _Arena(V * D + 64, dt) as ar:
        table, other = ar.view(V, D), ar.view(50)
        K.embedding_bwd(dout, ids, V, dweight=table)
        first = table.clone()
        K.embedding_bwd(dout, ids, V, dweight=table)
        demand, unused = ops.grad_end()
    assert torch.equal(first, want)
    assert demand == [(0, V * D)] and unused == [(V * D, ar.buf.numel())]
    assert torch.equal(other, torch.zeros_like(other)) and torch.equal(first[[0, 2, 36]], torch.zeros(3, D, dtype=dt, device=DEV))
    assert not bool((ar.buf == SENTINEL).any())


def test_train_step_first_touch_equals_the_arena_fill_and_eager_equals_replay():
    """tests/first_touch_step.py under the debug library: gradient arena, gnorm, statistics and master weights of three steps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dbg = os.path.join(root, "ofasys_amd", "libofasys_amd_dbg.so")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "first_touch_step.py")], env=dict(os.environ, OFASYS_AMD_LIB=dbg),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["new"]["finite"] and 0 < out["new"]["nonzero"] < out["new"]["numel"]      # (parameters without a gradient: exact zeros)
    assert out["replay"]["graphs"] == 1
    assert out["old"]["prezero"] == 0                # the old path keeps no list: it fills
    assert out["new"]["prezero"] > 0                 # partial writers were learned and cleared up front (the position tables)
    assert out["new"]["unused"] > out["new"]["gaps"] # parameters nobody wrote, beyond the alignment gaps between views
    assert out["new"]["rng"] == out["old"]["rng"] == out["replay"]["rng"]          # the Philox counter advanced alike
    assert out["new_vs_old"] == [True] * 3, out
    assert out["eager_vs_replay"] == [True] * 3, out


def test_layernorm_reduce_mixed_modes_clear_through_the_touched_set():
    """One accumulate flag over dgamma and dbeta: with dbeta already written in the step the launch adds to both, dgamma is cleared on
    demand first -- through ops, so that the range is learned for the next step's up-front launch."""
    torch.manual_seed(5)
    rows, cols, dt = 300, 256, torch.bfloat16
    x, dy = torch.randn(rows, cols, device=DEV).to(dt), torch.randn(rows, cols, device=DEV).to(dt)
    g, b = torch.randn(cols, device=DEV).to(dt), torch.randn(cols, device=DEV).to(dt)
    _, mean, rstd = K.layernorm_fwd(x, g, b)
    zg, zb = torch.zeros(cols, dtype=dt, device=DEV), torch.zeros(cols, dtype=dt, device=DEV)
    K.layernorm_bwd(dy, x, g, mean, rstd, dgamma=zg, dbeta=zb)
    with _Arena(2 * cols, dt) as ar:
        dg, db = ar.view(cols), ar.view(cols)
        assert ops.grad_mode(db, True) is False      # some other full writer of dbeta came first ...
        db.zero_()                                   # ... (and stored zeros)
        K.layernorm_bwd(dy, x, g, mean, rstd, dgamma=dg, dbeta=db)
        demand, _ = ops.grad_end()
    assert demand == [(0, cols)]
    assert torch.equal(dg, zg) and torch.equal(db, zb)


def _schedule_state(scaled):
    st = {"stats": torch.tensor([37.0, 5.0, 37.0], dtype=torch.float64, device=DEV), "step": torch.zeros(1, dtype=torch.float64, device=DEV),
          "lr": torch.tensor([1e-3], dtype=torch.float64, device=DEV), "sched": torch.zeros(5, device=DEV),
          "gnorm": torch.zeros(1, device=DEV), "gsq": torch.full((1,), 7.0, device=DEV),
          "counter": torch.tensor([11], dtype=torch.int64, device=DEV)}
    if scaled:
        st["ls"] = torch.tensor([128.0, 0, -1, -1, 0, 0, 0, 0], dtype=torch.float64, device=DEV)
    return st


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "loss-scale"])
@pytest.mark.parametrize("n", [1, 255, 256 * 1024 + 3, (1 << 21) + 5])
def test_fused_norm_and_schedule_equal_the_separate_launches(n, scaled):
    """ofa_sumsq_schedule against ofa_sumsq + ofa_step_schedule[_scaled] + the counter add, bit for bit, on two consecutive calls (the
    ticket resets itself; gsq needs no clearing): one block (1, 255 elements), 128 blocks, the full 1024-block grid on its only
    trip (tests/test_stream_edges_gpu.py goes past it, against an integer sum)."""
    torch.manual_seed(n % 1000)
    dt = torch.bfloat16
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    a, b = _schedule_state(scaled), _schedule_state(scaled)
    for call in range(2):
        x = (torch.randn(n, device=DEV) * (3.0 if call else 0.5)).to(dt)
        a["gsq"].zero_()
        K.sumsq(x, a["gsq"])
        if scaled:
            K.step_schedule_scaled(a["gsq"], a["stats"], a["step"], a["lr"], a["sched"], a["gnorm"], a["ls"], 1.0, 0.9, 0.999, 2.0, 4, 0.0, None, 1e-4)
        else:
            K.step_schedule(a["gsq"], a["stats"], a["step"], a["lr"], a["sched"], a["gnorm"], 1.0, 0.9, 0.999)
        a["counter"].add_(5)
        # (both forms write their block partials to the same cached workspace: poison it, or a last block that read stale partials
        #  would find the reference launch's, which are the right ones)
        K.workspace(lib().cdll.ofa_sumsq_ws_floats() * 4, x.device, "sumsq").view(torch.float32).fill_(float("nan"))
        K.sumsq_schedule(x, b["gsq"], ticket, b["stats"], b["step"], b["lr"], b["sched"], b["gnorm"], 1.0, 0.9, 0.999,
                         loss_scaler=b.get("ls"), scale_factor=2.0, scale_window=4, tolerance=0.0, threshold=None, min_loss_scale=1e-4,
                         counter=b["counter"], counter_add=5)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (call, k, a[k], b[k])
        assert int(ticket) == 0 and float(a["gsq"]) > 0 and float(a["step"]) == call + 1


@pytest.mark.parametrize("rows", [1, 5])
def test_fused_criterion_statistics_equal_the_separate_launches(rows):
    """ofa_cross_entropy_fwd_grad_stats against ofa_cross_entropy_fwd_grad + ofa_reduce_sum_f32 + ofa_step_stats_add at V = 520, a pad
    target among the rows, bit for bit on two consecutive calls."""
    torch.manual_seed(rows)
    V, pad, dt = 520, 1, torch.bfloat16
    seed = torch.ones((), dtype=torch.float32, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    sa = torch.tensor([2.0, 0.5, 2.0], dtype=torch.float64, device=DEV)
    sb = sa.clone()
    for call in range(2):
        logits = (torch.randn(rows, V, device=DEV) * 2).to(dt)
        target = torch.randint(4, V, (rows,), device=DEV)
        target[rows // 2] = pad if (rows > 1 or call) else 7
        lse, row_loss, d = K.cross_entropy_fwd_grad(logits, target, seed, V, pad)
        loss = K.sum_f32(row_loss)
        K.step_stats_add(sa, loss, target, pad)
        lse2, row_loss2, d2, loss2 = K.cross_entropy_fwd_grad(logits, target, seed, V, pad, sb, ticket)
        torch.cuda.synchronize()
        assert torch.equal(lse, lse2) and torch.equal(row_loss, row_loss2) and torch.equal(d, d2)
        assert torch.equal(loss, loss2) and torch.equal(sa, sb) and int(ticket) == 0
    assert float(sa[0]) > 2.0
