"""CPU: the exact-integer GEMM cases of tests/gemm_exact.py -- every case builds and meets its regime's precondition, every case (or
its plan twin) is on the route it is there to cover (ofa_gemm_plan, host only: a planner change that moves a case off its kernel fails
here instead of silently un-covering it), and the checker reports every planted fault while passing the unmodified reference."""
import json
import re

import pytest
import torch

from tests import gemm_exact as G
from tests.test_gemm_plan_cpu import describe, plan

PRODUCTS = sorted({n.rsplit(" ", 1)[0] for n in G.CASES})


def _forms(product):
    return [c for n, c in G.CASES.items() if n.rsplit(" ", 1)[0] == product]


@pytest.mark.parametrize("product", PRODUCTS)
def test_case_builds_and_meets_its_precondition(product):
    """build() asserts the regime's precondition on the float64 reference; the reference written into a fresh poisoned output passes
    the checker, and the poison is where the table says: NaN rows after every operand, NaN columns up to the leading dimension (zeros
    only under KPAD_ZERO_TAIL), ldc > N4 unless a named exception says otherwise."""
    for case in _forms(product):
        bt = G.build(case)
        assert bt.expected.shape == (case.nbatch, case.M, case.N) and bool(torch.isfinite(bt.expected).all())
        assert set(case.exceptions) <= {G.KPAD_ZERO_TAIL, G.FOLD_DENSE_OUT, G.HEADS_S_PAD}
        assert (G.KPAD_ZERO_TAIL in case.exceptions) == case.a_kpad_zero and (G.FOLD_DENSE_OUT in case.exceptions) == case.fold
        if case.heads:
            store, geom, want, skip = G.heads_output(bt)
            assert bool(torch.isnan(store[:, case.M:]).all()) and int(skip.sum()) == case.nbatch * case.M * (case.N4 - case.N) * (case.heads[2] == "scores")
            continue
        for x, st in ((bt.a, bt.a_store), (bt.b, bt.b_store)):       # st: the NaN storage [batch, R + 8, ld] behind the view
            assert x.data_ptr() == st.data_ptr() and x.stride(-2) == st.stride(1)
            R, W = x.shape[-2:]
            assert st.shape[1] == R + G.ROW_PAD and st.shape[2] >= W and bool(torch.isnan(st[:, R:]).all())
            tail = st[:, :R, W:]
            if x is bt.a and case.a_kpad_zero:
                assert tail.shape[2] >= G.ceil_to(case.K, 8) - case.K and bool((tail == 0).all())
            else:
                assert bool(torch.isnan(tail).all())
        store, out = G.new_output(bt)
        assert store.shape[1] == case.M + G.ROW_PAD and (store.shape[2] > case.N4 or case.fold)
        with pytest.raises(AssertionError, match="wrong elements"):
            G.check(case, store, bt.expected)                   # (an output nobody wrote: NaN, or the old C, inside [M, N])
        out.copy_(bt.expected)
        G.check(case, store, bt.expected)


def test_route_table():
    """Every case the shipped planner runs: ofa_gemm_plan of the case, or of its plan twin, gives the recorded route."""
    wrong = {}
    for name, case in G.CASES.items():
        if not case.env:
            got = describe(plan(*case.plan_args()))
            if got != G.route_of(case):
                wrong[name] = (got, G.route_of(case))
    assert not wrong, wrong
    # the route families the table is there to cover are all in it
    routes = {G.route_of(c) for c in G.CASES.values()}
    for kernel in ("SIMPLE", "REG 64x64", "LDS_DMA 64x64", "LDS_DMA 64x128", "LDS_DMA 128x128", "RING 64x64", "RING 64x128", "RING 128x128",
                   "BIG 256x256", "BIG 192x256", "PP 256x256", "PP 192x256", "MIXED 256x256"):
        assert any(r.startswith(kernel) for r in routes), kernel
    for kernel in ("LDS_DMA", "RING", "BIG", "PP"):
        assert any(r.startswith(kernel) and "+reduce" in r for r in routes), kernel


@pytest.mark.parametrize("group", sorted(G.forced_groups()))
def test_forced_route_table(group):
    """The forced cases under the debug library's planner overrides (a process of its own: OFA_GEMM_SPLIT_MIN_K is read once)."""
    r = G.run_child("plan", group)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROUTES ")][0][7:])
    names = G.forced_groups()[group]
    assert sorted(got) == sorted(names)
    assert {n: got[n] for n in names} == {n: G.route_of(G.CASES[n]) for n in names}
    if group == "split":      # every forced four-wave tile is split on the ring AND on the double-buffered loop, in TN and in NN
        assert all("splits=" in v and "+reduce" in v for v in got.values()), got
        seen = {(v.split(" waves")[0], re.search(r" (NN|TN) ", n).group(1)) for n, v in got.items()}
        assert seen == {(f"{k} {t}", lay) for k in ("RING", "LDS_DMA") for t in ("64x64", "64x128", "128x128") for lay in ("NN", "TN")}, seen
    if group == "big":        # every shape in every layout on every tile / loop setting
        assert len({n.rsplit(" ", 1)[0] for n in names}) == 2 * 2 * 3 * 3


def test_colstat_route_table():
    """The two gemm_colstat products of the GPU test write their statistics from different epilogues (rows per partial row 32 / 64)."""
    for M, N, K, bias, route in G.COLSTAT:
        assert describe(plan(M, N, K, G.NT, G.BIAS_COL if bias else 0)) == route
    assert {r.split("colstat=")[1] for *_, r in G.COLSTAT} == {"32", "64"} and len({r.split(" ")[0] for *_, r in G.COLSTAT}) == 2


def test_plan_twins():
    """A view names the dense product its launch plans: K rounded up to 64 (a_kpad_zero), N up to 8 (ragged N), M up to 8 (m-major A
    stored with lda = ceil8(M)), every tile count unchanged -- and it needs the twin: planned as a dense product of its own sizes the view
    is a different launch (the exact kernel, or another contraction length)."""
    twins = [c for c in G.CASES.values() if c.twin]
    assert len(twins) >= 60
    for c in twins:
        assert G.plan_twin_ok(c), c.name
        own = describe(plan(c.M, c.N, c.K, c.layout, c.flags, G.DTYPE_CODES[c.dtype], c.nbatch, G.WS))
        assert own != G.route_of(c), (c.name, own)
    for c in G.CASES.values():            # and every ragged size that ofa_gemm_plan cannot see as a dense product has one
        ragged = (c.N % 8 and not c.layout[1]) or c.N % 4 or (c.a_kpad_zero and c.K % 64) or (c.layout[0] and c.M % 8)
        if ragged and not c.unaligned and c.dtype != "f32" and not G.route_of(c).startswith("SIMPLE"):
            assert c.twin, c.name


def test_group_plan_covers_the_direct_and_the_slab_path():
    """ofa_gemm_group_plan (host only) of the grouped test's products: some are one K-slice (direct onto a 16-bit out), some are split."""
    import ctypes
    from ofasys_amd import lib as L
    from ofasys_amd.kernels import _GroupItem
    arr = (_GroupItem * len(G.GROUP))()
    for i, (it, (m, n, k)) in enumerate(zip(arr, G.GROUP)):
        it.a, it.b, it.lda, it.ldb, it.m, it.n, it.k = 4096, 8192, m + 8 * (i % 2), n + 8 * ((i + 1) % 2), m, n, k     # (never dereferenced)
    L.lib().call("ofa_gemm_group_plan", ctypes.addressof(arr), len(G.GROUP), L.BF16)
    assert [it.splits for it in arr] == G.GROUP_SPLITS and 1 in G.GROUP_SPLITS and max(G.GROUP_SPLITS) > 1


# ------------------------------------------------------------------ the checker's sensitivity
def _written(case):
    """(built case, output storage holding exactly the reference, its [batch, M, N] view)."""
    bt = G.build(case)
    store, out = G.new_output(bt)
    out.copy_(bt.expected)
    G.check(case, store, bt.expected)          # the unmodified reference passes
    return bt, store, out


def _must_report(case, store, bt, count, where):
    with pytest.raises(AssertionError) as e:
        G.check(case, store, bt.expected)
    msg = str(e.value)
    assert f": {count} wrong elements" in msg and where in msg, msg
    assert "tile (" in msg and "sub-tile (" in msg and "m % 32 = " in msg and "n % 8 = " in msg, msg


BIAS_CASE = G.CASES["LDS_DMA 600x520x192 NT bf16 bias"]
PLAIN_CASE = G.CASES["view ragged N RING 136x141x256 NT bf16 plain"]
TIE_CASE = G.CASES["RING 200x264x1024 NN bf16 rounding"]


def test_checker_reports_a_dropped_k_term():
    bt, store, out = _written(BIAS_CASE)
    a, b = bt.a.double(), bt.b.double()                      # NT: a [M, K], b [N, K]
    r = 77
    k = int(a[r].nonzero()[-1])                              # the row's last non-zero k-term
    term = a[r, k] * b[:, k] * BIAS_CASE.alpha
    out[0, r] = (bt.expected[0, r] - term).to(out.dtype)
    _must_report(BIAS_CASE, store, bt, int((term != 0).sum()), "[0, 77, ")


def test_checker_reports_two_swapped_rows():
    bt, store, out = _written(PLAIN_CASE)
    r0, r1 = 31, 32
    out[0, [r0, r1]] = out[0, [r1, r0]]
    differ = int((bt.expected[0, r0] != bt.expected[0, r1]).sum())
    assert differ > 100
    _must_report(PLAIN_CASE, store, bt, 2 * differ, "[0, 31, ")


def test_checker_reports_a_bias_skipped_on_the_last_quad():
    bt, store, out = _written(BIAS_CASE)
    N = BIAS_CASE.N
    quad = bt.bias.double()[N - 4:]
    assert int((quad != 0).sum()) >= 1
    out[0, :, N - 4:] = (bt.expected[0, :, N - 4:] - quad * BIAS_CASE.alpha).to(out.dtype)
    _must_report(BIAS_CASE, store, bt, BIAS_CASE.M * int((quad != 0).sum()), "tile (0, 8) of 64x64")


def test_checker_reports_an_element_left_nan():
    bt, store, out = _written(PLAIN_CASE)
    out[0, 135, 140] = G.NAN
    _must_report(PLAIN_CASE, store, bt, 1, "[0, 135, 140] got nan")


def test_checker_reports_a_write_at_column_n4_and_in_row_m():
    c = PLAIN_CASE
    bt, store, out = _written(c)
    store[0, 5, c.N:c.N4] = 7.0                    # [N, N4) is unspecified: the rest of the last quad may be written
    G.check(c, store, bt.expected)
    store[0, 5, c.N4] = 0.0
    _must_report(c, store, bt, 1, f"[0, 5, {c.N4}] got 0.0 want nan (outside [M, N]: must stay NaN)")
    bt, store, out = _written(c)
    store[0, c.M, 3] = 1.0
    _must_report(c, store, bt, 1, f"[0, {c.M}, 3] got 1.0 want nan")


def test_checker_reports_a_tie_rounded_away_from_even():
    bt, store, out = _written(TIE_CASE)
    x = bt.product[0]                                # the float64 value before its one rounding
    r = bt.expected[0]
    other = 2 * x - r                                # a tie: the other neighbour is as far away, and representable
    ties = (x != r) & (other.to(torch.bfloat16).double() == other)
    assert int(ties.sum()) > 1000                    # integers above 256 sit on bf16 ties all the time
    m, n = ties.nonzero()[0].tolist()
    bits = out[0, m, n].view(torch.int16)
    assert int(bits) % 2 == 0                        # the reference took the even significand
    out[0, m, n] = other[m, n].to(out.dtype)
    assert int(out[0, m, n].view(torch.int16)) % 2 == 1
    _must_report(TIE_CASE, store, bt, 1, f"[0, {m}, {n}]")


def test_the_two_accumulation_contracts_differ_in_the_rounding_regime():
    """round-add-round and fp32-once give different bits on the same operands: the table's rounding + accumulate cases tell them apart."""
    tile, once = G.CASES["RING 200x264x1024 NN bf16 round_acc16"], G.CASES["LDS_DMA split 520x520x4100 TN bf16 round_acc16"]
    assert G.contract_of(tile) == "round-add-round" and G.contract_of(once) == "fp32-once"
    assert G.contract_of(G.CASES["SIMPLE 70x77x200 NT bf16 round_acc16"]) == "fp32-once"
    assert G.contract_of(G.CASES["view fold-deferred 392x140x2100 TN bf16 round_acc16"]) == "fp32-once"
    for case in (tile, once):
        bt = G.build(case)
        x = bt.product
        a = G.round_to(G.round_to(x, torch.bfloat16) + bt.old, torch.bfloat16)
        b = G.round_to(x + bt.old, torch.bfloat16)
        assert int((a != b).sum()) > 100
        assert torch.equal(bt.expected, a if case is tile else b)
