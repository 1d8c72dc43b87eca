"""GPU: the streaming kernels of csrc/elementwise.hip and the step tail of csrc/loss_optim.hip below, at and past their grid caps, against
the oracle of tests/stream_oracle.py.  Every element of every output is compared; every output buffer holds NaN (a sentinel for bytes)
before the call and the 64 elements behind it are checked untouched.

What each test pins (the gaps the suite had):
  one small shape, max|a-b| / max|b| at 2e-2 ............... per element against the componentwise bound, one rounding; exactly 0 where it is 0
  the second grid-stride trip never ran .................... threads + 300 vectors (+ a tail): blocks 0 and 1 go round again, block 1 on 44 threads
  rows that straddle the trip seam ......................... 5465 rows of 96 vectors; a masked row, a group boundary, a part seam at the seam
  the dropout mask read off the kernel itself .............. a Philox4x32-10 restatement, bit for bit: offsets, offset_base, a wrapping low word
  movers compared at 231 ids ............................... bit for bit with index arithmetic in torch, clamped / out-of-range ids, pad bytes
  sumsq compared with sumsq only, one trip ................. integers in [-2, 2]: the integer sum, bit for bit, two trips and a tail
  colsum's ninth pass of the strided row loop .............. 8193 and 8200 rows, exact
  Adam: k = 1 quad, second trip, m and v never read ........ ofa_adam_step_grid's max_blocks; m, v and master per element; model copy in bits
Run with -s for the worst figure per kernel and dtype."""
import ctypes

import pytest
import torch

from tests import stream_oracle as so

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
IDS = [so.NAMES[d] for d in so.DTYPES3]
GUARD = 64
NAN = float("nan")
F32 = torch.float32


@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


def out_buf(n, dtype):
    """n elements for the kernel and GUARD behind them, all NaN (bytes: the sentinel)."""
    return torch.full((n + GUARD,), so.SENTINEL if dtype == torch.uint8 else NAN, dtype=dtype, device=DEV)


def taken(buf, n, tag):
    """The n elements the kernel owns, once the guard behind them is seen untouched."""
    g = buf[n:]
    assert g.numel() == GUARD and bool((g == so.SENTINEL).all() if buf.dtype == torch.uint8 else torch.isnan(g).all()), (tag, "wrote past its output")
    return buf[:n]


def run(K, case, b, dtype):
    """One case through its C-ABI entry point into a poisoned, guarded buffer -> {output name: flat tensor}."""
    call, ptr, st, k = K.lib().call, K.ptr, K.stream(), case.kernel
    code = K.dtype_code(torch.empty(0, dtype=dtype))
    n = so.case_numel(case, dtype)
    y = out_buf(n, dtype)
    extra = {}
    if k == "gelu_fwd":
        call("ofa_gelu_fwd", ptr(b["x"]), ptr(y), n, code, st)
    elif k == "gelu_bwd":
        call("ofa_gelu_bwd", ptr(b["dy"]), ptr(b["x"]), ptr(y), n, code, st)
    elif k == "dropout_add":
        base = torch.tensor([b["base"]], dtype=torch.int64, device=DEV) if b["base"] else None
        call("ofa_dropout_add_fwd", ptr(b["x"]), ptr(b["res"]), ptr(y), n, float(b["p"]), so.SEED, b["offset"], ptr(base), code, st)
    elif k == "add_rowvec_mask":
        mask = b["mask"].view(torch.uint8) if b["mask"] is not None else None
        call("ofa_add_rowvec_mask", ptr(b["a"]), ptr(b["b"]), ptr(b["vec"]), ptr(mask), ptr(y), b["rows"], b["D"], b["period"], code, st)
    elif k == "mul":
        call("ofa_mul", ptr(b["a"]), ptr(b["b"]), ptr(y), b["rows"], b["D"], int(b["rowvec"]), code, st)
    elif k == "scale_row_groups":
        call("ofa_scale_row_groups", ptr(b["a"]), ptr(b["scale"]), ptr(y), b["rows"], b["D"], b["group"], code, st)
    elif k == "add_n":
        arr = (ctypes.c_void_p * len(b["ins"]))(*[K.dptr(t) for t in b["ins"]])
        call("ofa_add_n", ctypes.addressof(arr), len(b["ins"]), ptr(y), n, code, st)
    elif k == "batch_sum":
        if b["prev"] is not None:
            y[:n] = b["prev"]
        call("ofa_batch_sum", ptr(b["x"]), ptr(y), b["x"].shape[0], n, int(b["prev"] is not None), code, st)
    elif k == "embedding_fwd":
        pad = b["pad_id"] is not None and b["D"] % so.NVEC[dtype] == 0
        extra["is_pad"] = out_buf(b["rows"], torch.uint8) if pad else None
        call("ofa_embedding_fwd", ptr(b["w"]), ptr(b["ids"]), ptr(y), b["rows"], b["D"], b["w"].shape[0], ptr(extra["is_pad"]),
             int(b["pad_id"]) if pad else 0, code, st)
    elif k == "gather_rows":
        call("ofa_gather_rows", ptr(b["src"]), ptr(b["index"]), ptr(y), b["rows"], b["D"], b["src"].shape[0], code, st)
    elif k == "gather_rows_parts":
        srcs = (ctypes.c_void_p * len(b["parts"]))(*[K.dptr(t) for t in b["parts"]])
        lens = (ctypes.c_int * len(b["parts"]))(*b["lens"])
        call("ofa_gather_rows_parts", ctypes.addressof(srcs), ctypes.addressof(lens), len(b["parts"]), ptr(b["index"]), ptr(y), b["rows"], b["D"],
             b["B"], code, st)
    elif k == "scatter_rows_part":
        call("ofa_scatter_rows_part", ptr(b["src"]), ptr(b["inverse"]), ptr(y), b["B"], b["nk"], b["Ttot"], b["start"], b["D"], b["src"].shape[0],
             code, st)
    elif k == "im2col_patch":
        B, C, H, W = b["img"].shape
        call("ofa_im2col_patch", ptr(b["img"]), ptr(y), B, C, H, W, b["p"], b["Kpad"], b["lead"], code, st)
    else:
        raise KeyError(k)
    torch.cuda.synchronize()
    out = {"out": taken(y, n, case.name)}
    if extra.get("is_pad") is not None:
        out["is_pad"] = taken(extra["is_pad"], b["rows"], case.name)
    return out


def launch_is_as_restated(case, dtype):
    """The precondition of every comparison: the case sits where its name says against the grid the entry point launches."""
    assert so.case_where(case, dtype) == so.case_pos(case, dtype), (case.name, so.case_work(case, dtype), so.case_grid(case, dtype))


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
@pytest.mark.parametrize("kernel", so.ONE_ROUNDING)
def test_one_rounding_kernels(K, kernel, dtype):
    """GELU forward / backward, dropout + residual (the restated mask as an input; a dropped element is the residual's bits),
    add + row vector + row mask, mul, scale_row_groups, add_n, batch_sum: every element within TOL eps of float64 relative to its
    magnitude bound (fp32: error / bound within G32), exactly 0 where the bound is 0."""
    worst = (0.0, None)
    for case in so.cases_of(kernel):
        launch_is_as_restated(case, dtype)
        b = so.build(case, dtype, DEV)
        fig = so.figures(case, b, run(K, case, b, dtype)["out"], dtype)
        bad = {n: v for n, v in fig.items() if not v <= so.limit(kernel, n, dtype)}
        assert not bad, (case.name, so.NAMES[dtype], bad, so.limit(kernel, "y", dtype))
        if fig["y"] > worst[0]:
            worst = (fig["y"], case.name)
    print(f"\n{kernel} {so.NAMES[dtype]}: y {worst[0]:.3g} of {so.limit(kernel, 'y', dtype):.3g} ({worst[1]})")


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
def test_dropout_mask_is_the_restated_philox_stream(K, dtype):
    """The keep decisions of dropout_kernel on ones, element for element against the integer restatement: counter offset + e / 8 with
    offset_base added on the device, halfword e % 8, kept iff >= round(p 65536); the kept values are rnd(1 / (1 - p))."""
    for case in so.cases_of("dropout_add"):
        launch_is_as_restated(case, dtype)
        b = so.build(case, dtype, DEV)
        ones = dict(b, x=torch.ones_like(b["x"]), res=None)
        y = run(K, case, ones, dtype)["out"]
        scale = (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(b["p"], dtype=F32))).to(dtype).to(DEV)
        assert torch.equal(y != 0, b["mask"]), (case.name, int(((y != 0) != b["mask"]).sum()), "mask bits differ")
        assert bool((y[b["mask"]] == scale).all()), case.name
    print(f"\ndropout mask {so.NAMES[dtype]}: {len(so.cases_of('dropout_add'))} cases, every bit as restated")


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
@pytest.mark.parametrize("kernel", so.MOVERS)
def test_movers_bit_for_bit(K, kernel, dtype):
    """embedding_fwd (vector and scalar route, clamped ids, the pad byte per row), gather_rows (-1 and >= src_rows: zero rows),
    gather_rows_parts (1, 3, 8 parts, both sides of every part seam), scatter_rows_part, im2col_patch (both kernels, lead 0 / 1,
    zero padding columns): the bits index arithmetic in torch gives."""
    for case in so.cases_of(kernel):
        launch_is_as_restated(case, dtype)
        b = so.build(case, dtype, DEV)
        want, got = so.mover_expected(case, b), run(K, case, b, dtype)
        assert set(want) == set(got), (case.name, sorted(want), sorted(got))
        for n in want:
            assert so.same_bits(got[n].view_as(want[n]), want[n]), (case.name, so.NAMES[dtype], n, "bits differ")
    print(f"\n{kernel} {so.NAMES[dtype]}: {len(so.cases_of(kernel))} cases, bit for bit")


def test_refused_shapes_raise(K):
    """What the tables leave out because the entry points refuse it: asserted as the exception, nothing launched."""
    from ofasys_amd.lib import OfaError
    for dtype in so.DTYPES3:
        N = so.NVEC[dtype]
        x = torch.ones(2, N + 1, dtype=dtype, device=DEV)
        for fn in (lambda: K.mul(x, x), lambda: K.add_rowvec_mask(x), lambda: K.batch_sum(x, 2),
                   lambda: K.scale_row_groups(x, torch.ones(2, device=DEV), 1),
                   lambda: K.gather_rows(x, torch.zeros(1, dtype=torch.int64, device=DEV))):
            with pytest.raises(OfaError, match="vector"):
                fn()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ exact reductions
def _sched_state():
    st = {"stats": torch.tensor([37.0, 5.0, 37.0], dtype=torch.float64, device=DEV), "step": torch.zeros(1, dtype=torch.float64, device=DEV),
          "lr": torch.tensor([1e-3], dtype=torch.float64, device=DEV), "sched": torch.zeros(5, device=DEV), "gnorm": torch.zeros(1, device=DEV)}
    return st


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
def test_sumsq_is_the_integer_sum(K, dtype):
    """ofa_sumsq below, at and past its 1024-block grid on integers in [-2, 2]: 7 + the integer sum of squares, bit for bit (it adds onto
    out).  ofa_sumsq_schedule writes the same gsq on two consecutive calls with the partials' workspace poisoned, and leaves the
    schedule ofa_step_schedule computes from that gsq."""
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for i, (pos, u, t) in enumerate(so.SUMSQ_SIZES):
        n = so.sumsq_n(u, t, dtype)
        assert so.where(n // so.NVEC[dtype], so.sumsq_grid(n, dtype) * 256) == pos
        x = so.small_ints(n, 100 + i, dtype).to(DEV)
        total = int((x.long() ** 2).sum())
        out = out_buf(1, F32)
        out[0] = 7.0
        K.sumsq(x, out)
        torch.cuda.synchronize()
        assert float(taken(out, 1, pos)[0]) == 7.0 + total, (pos, n, float(out[0]), total)
        a, b2 = _sched_state(), _sched_state()
        for call in range(2):
            gsq = out_buf(1, F32)
            K.workspace(K.lib().cdll.ofa_sumsq_ws_floats() * 4, x.device, "sumsq").fill_(NAN)      # (stale partials of the launch before)
            K.sumsq_schedule(x, gsq, ticket, b2["stats"], b2["step"], b2["lr"], b2["sched"], b2["gnorm"], 1.0, 0.9, 0.999)
            torch.cuda.synchronize()
            assert float(taken(gsq, 1, pos)[0]) == float(total) and int(ticket) == 0, (pos, n, call, float(gsq[0]), total)
            K.step_schedule(torch.tensor([float(total)], device=DEV), a["stats"], a["step"], a["lr"], a["sched"], a["gnorm"], 1.0, 0.9, 0.999)
            torch.cuda.synchronize()
            for name in a:
                assert so.same_bits(a[name], b2[name]), (pos, n, call, name, a[name], b2[name])
    # randn at the past size against float64: c 2^-24 sum|terms| along the longest chain of additions
    n = so.sumsq_n(*so.SUMSQ_SIZES[-1][1:], dtype)
    x = torch.randn(n, generator=so._gen(99)).to(dtype).to(DEV)
    out = torch.full((1,), 3.0, device=DEV)
    K.sumsq(x, out)
    torch.cuda.synchronize()
    terms = torch.cat([x.double() ** 2, torch.tensor([3.0], dtype=torch.float64, device=DEV)])
    err, bound = abs(float(out.double()[0]) - float(terms.sum())), so.reduction_bound(terms, so.sumsq_chain(dtype))
    print(f"\nsumsq {so.NAMES[dtype]}: integer sums exact at {len(so.SUMSQ_SIZES)} sizes; randn error {err / bound:.3g} of its bound")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
def test_colsum_and_reduce_sum_are_the_integer_sums(K, dtype):
    """colsum at 8191, 8192, 8193 and 8200 rows (the last two past the 128 row-group slots: a ninth pass of the strided row loop), N and
    768 columns, fp32 out, accumulate on and off; reduce_sum_f32 at 1, 255, 257 and 70 001 elements."""
    N = so.NVEC[dtype]
    for i, rows in enumerate(so.COLSUM_ROWS):
        assert K.lib().cdll.ofa_colsum_slots(rows) == so.colsum_slots(rows)
        for cols in (N, 768):
            x = so.small_ints(rows * cols, 200 + i, dtype).view(rows, cols).to(DEV)
            want = x.long().sum(0)
            for acc in (False, True):
                out = out_buf(cols, F32)
                if acc:
                    out[:cols] = 3.0
                K.colsum(x, 1.0, out=out[:cols], accumulate=acc)
                torch.cuda.synchronize()
                assert torch.equal(taken(out, cols, rows), (want + (3 if acc else 0)).float()), (rows, cols, acc)
    if dtype == F32:
        for i, n in enumerate(so.REDUCE_N):
            x = so.small_ints(n, 300 + i, F32).to(DEV)
            out = out_buf(1, F32)
            K.lib().call("ofa_reduce_sum_f32", K.ptr(x), K.ptr(out), n, K.stream())
            torch.cuda.synchronize()
            assert float(taken(out, 1, n)[0]) == float(x.long().sum()), n
    rows, cols = 8200, 768
    x = torch.randn(rows, cols, generator=so._gen(98)).to(dtype).to(DEV)
    prev = torch.randn(cols, generator=so._gen(97)).to(DEV)
    out = prev.clone()
    K.colsum(x, 1.0, out=out, accumulate=True)
    torch.cuda.synchronize()
    ref = x.double().sum(0) + prev.double()
    bound = so.COLSUM_CHAIN * so.U32 * (x.double().abs().sum(0) + prev.double().abs())
    fig = float(((out.double() - ref).abs() / bound).max())
    print(f"\ncolsum {so.NAMES[dtype]}: integer sums exact at {len(so.COLSUM_ROWS)} row counts; randn error {fig:.3g} of its bound")
    assert fig <= 1.0, fig


# ------------------------------------------------------------------------------------------------------------------ Adam
def _adam_run(K, b, dtype, max_blocks):
    n = b["p"].numel()
    bufs = {}
    for name in ("p", "m", "v"):
        bufs[name] = out_buf(n, F32)
        bufs[name][:n] = b[name]
    bufs["model"] = out_buf(n, dtype)
    K.adam_step(bufs["p"][:n], bufs["m"][:n], bufs["v"][:n], b["g"], bufs["model"][:n], b["coef"], b["lr"], b["b1"], b["b2"], b["eps"], b["wd"],
                b["step"], max_blocks=max_blocks)
    torch.cuda.synchronize()
    return {name: taken(t, n, name) for name, t in bufs.items()}


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
def test_adam_step_per_element(K, dtype):
    """adam_kernel through ofa_adam_step_grid: m', v' and the master weights per element against float64, the model copy
    round_to_dtype(the kernel's own master) in bits; the default grid at n = 1 ... 1027, max_blocks = 1 (a second quad on 10 threads; a
    second trip) and 2 (a full first trip, a second trip with 100 second quads, a tail); the schedule from the host, with a one-element
    coef and from the device; wd 0 and 0.01; first and second update; gradients of 64 at the first k = 1 quad and the last quad.
    Capped runs equal the default-grid run of the same data in every bit; sched[3] = 1 leaves all five arrays untouched."""
    h, worst, ran = K.lib().cdll, {}, []
    for case in so.ADAM_CASES:
        # the launch the restated arithmetic expects, before anything is compared: a cap that were ignored fails here
        blocks = h.ofa_adam_step_blocks(case.n, case.max_blocks)
        assert blocks == so.adam_grid(case.n, case.max_blocks), (case.name, blocks)
        trips = so.adam_trips(case.n, case.max_blocks)
        if case.max_blocks:
            assert blocks == case.max_blocks < so.cdiv(case.n, 256) and so.where(case.n >> 2, blocks * 256) == "past" and trips[0] > 0, case.name
            ran.append(f"n={case.n} max_blocks={case.max_blocks}: second quads {trips[0]}, second trip {trips[1]} + {trips[2]}")
        else:
            assert trips == (0, 0, 0)
        b = so.build_adam(case, dtype, DEV)
        got = _adam_run(K, b, dtype, case.max_blocks)
        if case.skip:
            for name in ("p", "m", "v"):
                assert so.same_bits(got[name], b[name]), (case.name, name)
            assert bool(torch.isnan(got["model"]).all()) and so.same_bits(b["g"], so.build_adam(case, dtype, DEV)["g"]), case.name
            continue
        fig = so.adam_figures(b, got)
        for name, v in fig.items():
            worst[name] = max(worst.get(name, 0.0), v)
        bad = {name: v for name, v in fig.items() if not v <= so.adam_limit(name)}
        assert not bad, (case.name, so.NAMES[dtype], bad)
        if case.max_blocks:
            full = _adam_run(K, b, dtype, 0)
            for name in got:
                assert so.same_bits(got[name], full[name]), (case.name, name, "differs from the default-grid run")
    print(f"\nadam {so.NAMES[dtype]}: " + ", ".join(f"{n} {v:.3g} of {so.adam_limit(n):.3g}" for n, v in sorted(worst.items())) +
          "\n  " + "\n  ".join(sorted(set(ran))))
