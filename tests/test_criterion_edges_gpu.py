"""GPU: the criterion kernels (csrc/loss_optim.hip: cross entropy by the two-kernel and the fused one-pass route, label-smoothed cross
entropy, the fp32 softmax / log-softmax of get_normalized_probs) at their vector, trip and register-slab seams, against the float64 oracle
of tests/criterion_oracle.py.  Every gradient is compared per element of [rows, ld], padding included: excess(kernel, reference, bound) <=
TOL in units of the 16-bit eps (fp32 gradients: error / bound <= G32_TOL), exactly 0 where the bound is 0; every fp32 output (lse, row
losses, counts, probabilities) against the float64 value within its recorded tolerance.  Every output buffer holds NaN before the call.

What each test pins (the gaps the suite had):
  max|a-b| / max|b| sees the target column only ..... check_grad(): per element against (p + onehot)|g|, no blind columns
  the fused kernel compared with a kernel only ...... test_fused_cross_entropy: against float64, lse against logsumexp
  ce_fwd_grad_kernel<T, 2> never ran ................. ld = 8200, 16384 (and 8256 as a view of wider storage)
  the two-kernel route never saw fp16 or a tail ...... test_two_kernel_cross_entropy: fp32 / bf16 / fp16, targets inside the scalar tail
  softmax and label smoothing thin ................... test_probs (second trip, V = 1), test_label_smoothed_cross_entropy (ranges, masks, row_w)
  random rows cannot show a dropped column ........... the `planted` regime: the row's dominant logit sits on each seam column in turn
  a target outside [0, V) through the fused entry .... test_fused_cross_entropy_survives_targets_outside_the_vocabulary
  a stale or repeated seeded backward ................ test_seeded_backward_of_cross_entropy_sum"""
import pytest
import torch

from tests import criterion_oracle as co

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
NAN = float("nan")
F32 = torch.float32
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
WORST = {}                  # (output, dtype name) -> worst figure seen by this process, printed by every test (-s)


@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _poison(*specs):
    """Allocate and free NaN-filled tensors of exactly the sizes the wrapper is about to torch.empty: the caching allocator hands those
    blocks straight back, so an element the kernels leave unwritten reads NaN instead of the previous call's correct number."""
    keep = [_nan(shape, dtype) for shape, dtype in specs]
    torch.cuda.synchronize()
    del keep


def _note(name, dtype, value):
    key = (name, NAMES[dtype])
    WORST[key] = max(WORST.get(key, 0.0), value)


def _report(title):
    print(f"\n{title}: " + ", ".join(f"{n} {d} {v:.3g}" for (n, d), v in sorted(WORST.items())))


def check_grad(name, got, ref, bd, dtype, g, tag):
    """Every element of [rows, ld]: finite, within TOL eps of the reference relative to the magnitude bound (fp32: error / bound within
    G32_TOL), exactly zero where the bound is zero."""
    assert got.shape == ref.shape and got.dtype == dtype, (tag, got.shape, got.dtype)
    assert bool(torch.isfinite(got).all()), (tag, name, "not finite (an element that was not written reads NaN)")
    e = co.excess(got, ref, bd, co.EPS.get(dtype, 1.0), co.floor_of(dtype, g))
    limit = co.G32_TOL if dtype == F32 else co.TOL
    _note(name, dtype, e)
    print(tag, name, f"{e:.3g}", "of", f"{limit:.3g}")
    assert e <= limit, (tag, name, e, limit)


def check_f32(name, got, ref, tol, dtype, tag):
    assert got.dtype == F32 and bool(torch.isfinite(got).all()), (tag, name, "not finite")
    e = float((got.double() - ref).abs().max())
    _note(name, dtype, e / tol)
    assert e <= tol, (tag, name, e, tol)


def _gs(g):
    return torch.tensor([g], dtype=F32, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ cross entropy
def _check_ce(got, b, dtype, tag, route):
    ref, bd = co.ce_reference(b["x"], b["t"], b["g"])
    check_f32(f"{route} lse", got["lse"], ref["lse"], co.LSE_TOL, dtype, tag)
    check_f32(f"{route} row_loss", got["row_loss"], ref["row_loss"], co.ROW_TOL, dtype, tag)
    assert float(got["row_loss"][b["ignored"]]) == 0.0, (tag, "row_loss of the ignored row")
    check_grad(f"{route} d", got["d"], ref["d"], bd, dtype, b["g"], tag)


def _two_kernel(K, b):
    x, t = b["x"], b["t"]
    R, V = x.shape
    _poison(((R,), F32), ((R,), F32))
    lse, row_loss = K.cross_entropy_fwd(x, t, V, co.IGNORE)
    d = K.cross_entropy_bwd(x, t, lse, _gs(b["g"]), V, co.IGNORE, dlogits=_nan((R, x.stride(0)), x.dtype))
    torch.cuda.synchronize()
    return dict(lse=lse, row_loss=row_loss, d=d)


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=[NAMES[d] for d in co.DTYPES3])
def test_two_kernel_cross_entropy(K, dtype):
    """ce_fwd_kernel + ce_bwd_kernel: no vector at all, exactly one trip of 256 vectors, a second trip, a 5-wide scalar tail with the
    target and the row's dominant logit inside it, one and two whole padding vectors; g = 1, 0.37 and a loss scale of 128."""
    for case in co.CE_TWO_CASES:
        b = co.build_ce(case, dtype, DEV)
        _check_ce(_two_kernel(K, b), b, dtype, str(tuple(case)), "two-kernel")
    _report("two-kernel cross entropy")


FUSED_LDS = co.FUSED_LD + (co.WIDE[1],)


@pytest.mark.parametrize("dtype", co.CE_DTYPES[True], ids=[NAMES[d] for d in co.CE_DTYPES[True]])
@pytest.mark.parametrize("ld", FUSED_LDS)
def test_fused_cross_entropy(K, dtype, ld):
    """ce_fwd_grad_kernel<T, NV> on both sides of every NV boundary, V = ld, ld - 3 (a partial last vector), ld - 11 (a whole padding
    vector behind it), the dominant logit and the target on each side of every slab seam (8192 k), of a wave seam (1536) and of the last
    full vector's edge -- against float64, not against the two-kernel route; the two routes' lse agree within 2 LSE_TOL."""
    cases = [c for c in co.CE_FUSED_CASES if c.ld == ld]
    assert cases
    for i, case in enumerate(cases):
        b = co.build_ce(case, dtype, DEV)
        x, t = b["x"], b["t"]
        R, V = x.shape
        assert x.stride(0) == ld and K.cross_entropy_fwd_grad_ok(x, V)
        _poison(((R,), F32), ((R,), F32), ((R, ld), dtype))
        lse, row_loss, d = K.cross_entropy_fwd_grad(x, t, _gs(case.g), V, co.IGNORE)
        torch.cuda.synchronize()
        _check_ce(dict(lse=lse, row_loss=row_loss, d=d), b, dtype, f"NV={co.nv_of(ld)} {tuple(case)}", "fused")
        if i == 0:
            lse2, _ = K.cross_entropy_fwd(x, t, V, co.IGNORE)
            assert float((lse2 - lse).abs().max()) <= 2 * co.LSE_TOL, (case, "the two routes' lse")
    _report(f"fused cross entropy ld={ld}")


def test_fused_cross_entropy_survives_targets_outside_the_vocabulary(K):
    """A non-ignored target outside [0, V) handed to ofa_cross_entropy_fwd_grad is a caller error the kernel survives as
    ofa_scst_loss_fwd_grad does (test_scst_kernel_gpu.test_disallowed_targets_are_survived): nothing read out of bounds, row_loss = +inf,
    a zero gradient row -- and the other rows meet the float64 reference."""
    from tests import scst_oracle as so
    dtype, V, ld, g = torch.bfloat16, 8193, 8200, 0.37
    b = so.build(so.ScstCase("planted", V, ld, None, g, False, 78, 0), dtype, DEV)
    x, t = b["x"], b["t"].clone()
    R = so.ROWS
    bad = {8: V + 1, 9: -7, 10: 10 ** 12, 11: ld}                        # padding, < 0, huge, one past the storage row
    assert R == 12 and so.IGNORED_ROW < 8
    for r, v in bad.items():
        t[r] = v
    _poison(((R,), F32), ((R,), F32), ((R, ld), dtype))
    lse, row_loss, d = K.cross_entropy_fwd_grad(x, t, _gs(g), V, co.IGNORE)
    torch.cuda.synchronize()
    for r in bad:
        assert float(row_loss[r]) == float("inf") and float(d[r].float().abs().max()) == 0.0, r
    assert bool(torch.isfinite(d).all())
    good = dict(x=x[:8], t=t[:8], g=g, ignored=so.IGNORED_ROW)
    _check_ce(dict(lse=lse[:8], row_loss=row_loss[:8], d=d[:8]), good, dtype, "targets outside [0, V)", "fused")
    check_f32("fused lse", lse[8:], co.ce_reference(x[8:], torch.zeros(4, dtype=torch.int64, device=DEV), g)[0]["lse"], co.LSE_TOL, dtype,
              "lse of the rows with a bad target")


def _bf16_neighbours(a, b):
    """a and b are roundings to bf16 of two fp32 values a few fp32 ulps apart (the same gradient by v_exp_f32 and by expf): equal, or
    adjacent bf16 values -- at most one bf16 ulp, 2^-7 of the larger magnitude, apart; exactly equal where one is 0."""
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs())).all())


def test_seeded_backward_of_cross_entropy_sum(K):
    """ops.cross_entropy_sum with a seed (tests/test_scst_gpu.py::test_seeded_backward for the SCST op): the gradient precomputed at the
    seed's scale is what the backward seeded with that very tensor returns; a second backward (retain_graph), another tensor of the same
    value and a seed written to since the forward all recompute through ce_bwd_kernel -- to equal numbers on these inputs (the two
    kernels' exponentials differ by fp32 ulps, which no element's bf16 rounding sees here), or, within one bf16 rounding, to the new scale.  Each gradient meets the float64 reference at its scale."""
    from ofasys_amd import ops
    dtype, R, V = torch.bfloat16, 6, 257
    x = co.make_case("randn3", R, V, V, None, 640).to(dtype).to(DEV)
    t = torch.randint(0, V, (R,), generator=torch.Generator(device="cpu").manual_seed(641))
    t[2] = co.IGNORE
    t = t.to(DEV)
    logits = x.clone().requires_grad_(True)                  # dense [6, 257]: the op pads the rows to 264 itself
    padded = torch.zeros(R, 264, dtype=dtype, device=DEV)
    padded[:, :V] = x

    def meets_reference(d, g, tag):
        assert d.shape == (R, V) and d.dtype == dtype
        ref, bd = co.ce_reference(padded[:, :V], t, g)
        check_grad("ce op d", torch.nn.functional.pad(d, (0, 264 - V)), ref["d"], bd, dtype, g, tag)

    seed = torch.ones((), dtype=F32, device=DEV)
    _poison(((R,), F32), ((R,), F32), ((R, 264), dtype))
    loss = ops.cross_entropy_sum(logits, t, co.IGNORE, seed=seed)
    want = K.cross_entropy_fwd_grad(padded[:, :V], t, seed.reshape(1), V, co.IGNORE)[2][:, :V]
    first, = torch.autograd.grad(loss, logits, seed, retain_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(first, want) and float(first.float().abs().max()) > 0, "the first backward returns the forward kernel's gradient"
    meets_reference(first, 1.0, "first")
    kept = first.clone()
    _poison(((R, 264), dtype))
    again, = torch.autograd.grad(loss, logits, seed, retain_graph=True)                                  # a second time: recomputed
    assert again.data_ptr() != first.data_ptr() and torch.equal(first, kept) and torch.equal(again, first)
    meets_reference(again, 1.0, "again")
    _poison(((R, 264), dtype))
    other, = torch.autograd.grad(loss, logits, torch.ones((), device=DEV), retain_graph=True)            # another tensor: recomputed
    assert other.data_ptr() != first.data_ptr() and torch.equal(first, kept) and torch.equal(other, first)
    meets_reference(other, 1.0, "other")
    # a seed changed in place between forward and backward: the stale gradient is not handed out
    seed2 = torch.ones((), dtype=F32, device=DEV)
    loss2 = ops.cross_entropy_sum(logits, t, co.IGNORE, seed=seed2)
    seed2.mul_(2.0)
    changed, = torch.autograd.grad(loss2, logits, seed2)
    torch.cuda.synchronize()
    print("elements that differ from the first gradient: again", int((again != first).sum()), "other", int((other != first).sum()),
          "changed", int((changed.float() != first.float() * 2).sum()), "of", first.numel())
    assert _bf16_neighbours(changed.float(), first.float() * 2)
    meets_reference(changed, 2.0, "changed")


def test_fused_route_is_offered_up_to_65536_columns(K):
    for dtype in co.CE_DTYPES[True]:
        assert K.cross_entropy_fwd_grad_ok(torch.empty(2, 65536, device=DEV, dtype=dtype), 65536)
        assert not K.cross_entropy_fwd_grad_ok(torch.empty(2, 65544, device=DEV, dtype=dtype), 65544)
        assert not K.cross_entropy_fwd_grad_ok(torch.empty(2, 65544, device=DEV, dtype=dtype)[:, :65536], 65536)


# ------------------------------------------------------------------------------------------------------------------ label smoothing
def _check_ls(got, ref, bd, b, dtype, tag):
    assert torch.equal(got["row_cnt"].double(), ref["row_cnt"]), (tag, "row_cnt", got["row_cnt"], ref["row_cnt"])
    check_f32("lsce lse", got["lse"], ref["lse"], co.LSE_TOL, dtype, tag)
    check_f32("lsce row_loss", got["row_loss"], ref["row_loss"], co.LSROW_TOL, dtype, tag)
    check_f32("lsce row_nll", got["row_nll"], ref["row_nll"], co.LSROW_TOL, dtype, tag)
    check_grad("lsce d", got["d"], ref["d"], bd, dtype, b["g"], tag)


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=[NAMES[d] for d in co.DTYPES3])
def test_label_smoothed_cross_entropy(K, dtype):
    """lsce_fwd_kernel + lsce_bwd_kernel: one trip, exactly one trip, a second and a fifth trip of the 256-thread loop; no constraint,
    ranges whose edges carry the targets, a per-row byte mask that disallows a row's dominant logit, both together; eps 0 and 0.1;
    row weights 0, 0.5, 1; an ignored row; a padded leading dimension.  row_cnt equals the reference count exactly."""
    for case in co.LS_CASES:
        b = co.build_ls(case, dtype, DEV)
        x, t = b["x"], b["t"]
        R, V = x.shape
        cs, ce = case.crange if case.crange is not None else (-1, -1)
        ref, bd = co.lsce_reference(x, t, b["g"], b["eps"], crange=b["crange"], cmask=b["cmask"], row_w=b["row_w"])
        _poison(*[((R,), F32)] * 4)
        lse, row_loss, row_nll, row_cnt = K.ls_cross_entropy_fwd(x, t, V, co.IGNORE, b["eps"], cs, ce, b["cmask"])
        _poison(((R, x.stride(0)), dtype))
        d = K.ls_cross_entropy_bwd(x, t, lse, row_cnt, b["row_w"], _gs(b["g"]), V, co.IGNORE, b["eps"], cs, ce, b["cmask"])
        torch.cuda.synchronize()
        _check_ls(dict(lse=lse, row_loss=row_loss, row_nll=row_nll, row_cnt=row_cnt, d=d), ref, bd, b, dtype, str(tuple(case)))
    _report("label-smoothed cross entropy")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_drop_worst_rows_through_the_op(dtype):
    """ops.label_smoothed_cross_entropy with drop_worst_ratio > 0 at V = 257: the kept rows are the k = int(n (1 - ratio)) smallest of
    the reference row losses; the gradient the op returns meets the same per-element check with that row_w, the dropped rows exactly 0."""
    from ofasys_amd import ops
    case = co.LSCase("randn3", 257, 0, 0.1, "none", None, 0.37, 990)
    b = co.build_ls(case, dtype, DEV)
    t, ratio = b["t"], 0.4
    ref0, _ = co.lsce_reference(b["x"], t, case.g, case.eps)
    valid = t != co.IGNORE
    k = int(int(valid.sum()) * (1 - ratio))
    key = torch.where(valid, ref0["row_loss"], torch.full_like(ref0["row_loss"], float("inf")))
    gaps = key.sort().values.diff()[:int(valid.sum()) - 1]
    assert float(gaps.min()) > 100 * co.LSROW_TOL, "the reference row losses must order the rows beyond the kernels' fp32 error"
    row_w = torch.zeros_like(key)
    row_w[key.argsort()[:k]] = 1.0
    assert 0 < k < int(valid.sum())
    x = b["x"].contiguous().requires_grad_(True)                 # a dense [rows, 257] tensor: the op pads it itself
    _poison(*[((co.LS_ROWS,), F32)] * 4)
    loss, nll, ntok = ops.label_smoothed_cross_entropy(x, t, co.IGNORE, case.eps, drop_worst_ratio=ratio)
    _poison(((co.LS_ROWS, 264), dtype))
    loss.backward(torch.tensor(case.g, device=DEV))
    torch.cuda.synchronize()
    assert int(ntok) == k
    ref, bd = co.lsce_reference(x.detach(), t, case.g, case.eps, row_w=row_w)
    assert abs(float(loss.detach()) - float((ref["row_loss"] * row_w).sum())) <= co.LS_ROWS * co.LSROW_TOL
    assert abs(float(nll.detach()) - float((ref["row_nll"] * row_w).sum())) <= co.LS_ROWS * co.LSROW_TOL
    check_grad("lsce op d", x.grad, ref["d"], bd, dtype, case.g, "drop_worst")
    assert bool((x.grad[row_w == 0] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ probs
@pytest.mark.parametrize("dtype", co.DTYPES3, ids=[NAMES[d] for d in co.DTYPES3])
def test_probs(K, dtype):
    """probs_fwd_kernel / probs_bwd_kernel: V = 1, one trip short of 256 columns, exactly one, one more, a fifth trip; a padded and an
    unpadded leading dimension; log-softmax and softmax; the backward (of the forward's own stored result) into each type, the row's
    dominant logit and its dominant dy on the trip seams."""
    for case in co.P_CASES:
        b = co.build_probs(case, dtype, DEV)
        x, dy = b["x"], b["dy"]
        R, V = x.shape
        tag = str(tuple(case))
        _poison(((R, V), F32))
        y = K.probs_fwd(x, V, x.stride(0), case.log_probs)
        torch.cuda.synchronize()
        assert y.shape == (R, V)
        check_f32("probs log" if case.log_probs else "probs prob", y, co.probs_reference(x, case.log_probs), co.PROBS_TOL[case.log_probs],
                  dtype, tag)
        ref, bd = co.probs_bwd_reference(dy, y, co.bwd_ld(V), case.log_probs)
        _poison(((R, co.bwd_ld(V)), dtype))
        d = K.probs_bwd(dy, y, V, dtype, case.log_probs)
        torch.cuda.synchronize()
        check_grad("probs d", d, ref, bd, dtype, co.PLANT_DY, tag)
    _report("probs")
