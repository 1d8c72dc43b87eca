"""GPU: the attention side kernels -- csrc/softmax.hip, csrc/bias.hip, csrc/attention_decode.hip, csrc/attention_aux.hip -- at their
register, grid, chunk and LDS seams, against the oracle of tests/attnside_oracle.py.  Every entry point is called through the C ABI
directly, so no wrapper's .contiguous() or assert stands in between.  Every element of every output is compared; every output buffer
holds NaN before the call and the 64 elements behind it are checked untouched; what a kernel must not read is NaN: dy and y above the
causal diagonal, dbias outside the slot's block, cache rows >= S and the cache's padding columns, bias beyond S, delta columns >= T, the
row padding of strided operands (key-padding bytes beyond S are non-zero: read, they would mask).

What each test pins (the gaps the suite had):
  softmax rows up to sk = 1000, rel() ....................... NI = 32 and NI = 64 (sk 1025 ... 4096), forward and backward, 5 / 6 rows, per element
  one attn_softmax shape .................................... bias x kpm x causal, a fully key-padded sample (NaN rows), a NaN score under the diagonal
  the causal backward's y never poisoned .................... NaN above the diagonal of dy and y; in place and out of place
  bias blocks at B=2, A=3, T=7 .............................. below, at and past the 4096-block cap; the rest of bias bit-identical
  bias_block_grad's chunks .................................. n = 63 ... 130 x A = 1 ... 40 on integers, exact; randn against float64
  bias_outer_grad's V = 1 second trip, alignment fallback ... both, and V = 4's second trip, exact
  decode S <= 1500, fp16 once ............................... S = 1 ... 32 768 in three dtypes, both sides of the 64 KB LDS line, strided cache
  mean_heads 5 x 7, transpose / delta / c_attn_grad ......... the 1024-block cap, T / C at 63 / 64 / 65 with zero tails, NaN padding, three trips
Run with -s for the worst figure per kernel and dtype."""
import ctypes

import pytest
import torch

from tests import attnside_oracle as ao

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
IDS = [ao.NAMES[d] for d in ao.DTYPES3]
D16 = (ao.BF16, ao.FP16)
GUARD = 64
NAN = float("nan")
F32 = torch.float32


@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


def out_buf(n, dtype):
    """n elements for the kernel and GUARD behind them, all NaN."""
    return torch.full((n + GUARD,), NAN, dtype=dtype, device=DEV)


def taken(buf, n, tag):
    """The n elements the kernel owns, once the guard behind them is seen untouched."""
    g = buf[n:]
    assert g.numel() == GUARD and bool(torch.isnan(g).all()), (tag, "wrote past its output")
    return buf[:n]


def code_of(K, dtype):
    return K.dtype_code(torch.empty(0, dtype=dtype))


def pitched(t2, ld):
    """A [rows, cols] tensor stored with row pitch ld >= cols in a NaN buffer -> the buffer (its start is the operand)."""
    rows, cols = t2.shape
    buf = torch.full((rows * ld + GUARD,), NAN, dtype=t2.dtype, device=DEV)
    buf[:rows * ld].view(rows, ld)[:, :cols] = t2
    return buf


class Worst:
    def __init__(self):
        self.fig = {}

    def see(self, key, value, name):
        if value > self.fig.get(key, (-1.0, None))[0]:
            self.fig[key] = (value, name)

    def line(self, label, lim):
        return f"\n{label}: " + "; ".join(f"{k} {v:.3g} of {lim:.3g} ({n})" for k, (v, n) in sorted(self.fig.items()))


# ------------------------------------------------------------------------------------------------------------------ softmax family
def run_softmax(K, case, b, dtype):
    call, ptr, st, code, o = K.lib().call, K.ptr, K.stream(), code_of(K, dtype), dict(case.opt)
    n, k = b["rows"] * case.sk, case.kernel
    if k in ao.SM_BWD:
        if o["inplace"]:
            dx = out_buf(n, dtype)
            dx[:n] = b["dy"].reshape(-1)
            dy = dx
        else:
            dx, dy = out_buf(n, dtype), b["dy"]
        if k == "sm_bwd_causal":
            call("ofa_scaled_upper_triang_masked_softmax_bwd", ptr(dy), ptr(b["y"]), ptr(dx), ao.SM_SCALE, case.b, case.sq, code, st)
        else:                                                            # (the masked family's backward is the same launch: both entry points run)
            call("ofa_scaled_masked_softmax_bwd" if o["inplace"] else "ofa_scaled_softmax_bwd", ptr(dy), ptr(b["y"]), ptr(dx), ao.SM_SCALE,
                 case.b, case.np, case.sq, case.sk, code, st)
        torch.cuda.synchronize()
        return taken(dx, n, case.name).view(b["rows"], case.sk)
    y = out_buf(n, dtype)
    if k == "sm_plain":
        call("ofa_scaled_softmax_fwd", ptr(b["x"]), ptr(y), ao.SM_SCALE, case.b, case.np, case.sq, case.sk, code, st)
    elif k == "sm_masked":
        call("ofa_scaled_masked_softmax_fwd", ptr(b["x"]), ptr(b["mask"]), ptr(y), ao.SM_SCALE, case.b, case.np, case.sq, case.sk, o["mask_b"], code, st)
    elif k == "sm_causal":
        call("ofa_scaled_upper_triang_masked_softmax_fwd", ptr(b["x"]), ptr(y), ao.SM_SCALE, case.b, case.sq, code, st)
    else:
        call("ofa_attn_softmax_fwd", ptr(b["x"]), ptr(b["bias"]), ptr(b["kpm"]), ptr(y), ao.SM_SCALE, case.b * case.np, case.np, case.sq, case.sk,
             o["causal"], code, st)
    torch.cuda.synchronize()
    return taken(y, n, case.name).view(b["rows"], case.sk)


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
@pytest.mark.parametrize("kernel", ao.SM_FWD + ao.SM_BWD)
def test_softmax_family_per_element(K, kernel, dtype):
    """scaled_softmax, scaled_masked_softmax (mask batch 1 and b, a fully masked row: uniform), scaled_upper_triang_masked_softmax and
    attn_softmax (bias x key padding x causal; a fully key-padded sample: NaN rows exactly there; a NaN score: 0 before the triangle),
    and the two backward launches (in place and out of place; NaN above the diagonal of dy and y) at sk = 1 ... 4096: every NI of the
    ladder just above its lower seam and at its top, 5 or 6 rows.  Every element within TOL eps of float64 relative to its bound (fp32:
    error / bound within G32), exactly 0 where the bound is 0."""
    w, ran = Worst(), set()
    for case in [c for c in ao.SM_CASES if c.kernel == kernel]:
        b = ao.build_sm(case, dtype, DEV)
        fig = ao.sm_figures(case, b, run_softmax(K, case, b, dtype), dtype)["y"]
        assert fig <= ao.limit(kernel, dtype), (case.name, ao.NAMES[dtype], fig, ao.limit(kernel, dtype))
        w.see("y", fig, case.name)
        ran.add(ao.sm_ni(case.sk))
    assert ran == set(ao.SM_LADDER)
    print(w.line(f"{kernel} {ao.NAMES[dtype]} (NI {sorted(ran)})", ao.limit(kernel, dtype)))


# ------------------------------------------------------------------------------------------------------------------ decode
def run_decode(K, case, b, dtype):
    call, ptr, st, code = K.lib().call, K.ptr, K.stream(), code_of(K, dtype)
    B, H, S = case.B, case.heads, b["S"]
    if case.strided:                                                     # ldk > heads * 64, a batch stride that is not cap * ldk, kpm_ld > S
        ldk, cap, kpm_ld = H * 64 + 16, S + 3, S + 5
        bsk = cap * ldk + 16
    else:
        ldk, cap, kpm_ld = H * 64, S, S
        bsk = cap * ldk
    assert ldk % ao.NVEC[dtype] == 0 and bsk % ao.NVEC[dtype] == 0 and (B - 1) * bsk + cap * ldk <= B * bsk
    cache = []
    for t in (b["k"], b["v"]):
        buf = torch.full((B * bsk + GUARD,), NAN, dtype=dtype, device=DEV)
        torch.as_strided(buf, (B, S, H * 64), (bsk, ldk, 1)).copy_(t.reshape(B, S, H * 64))      # rows >= S and the padding columns stay NaN
        cache.append(buf)
    kpm = None
    if b["kpm"] is not None:
        kpm = torch.full((B, kpm_ld), 1, dtype=torch.uint8, device=DEV)
        kpm[:, :S] = b["kpm"]
    bias = None
    if b["bias"] is not None:
        bias = torch.full((B * H * S + GUARD,), NAN, dtype=dtype, device=DEV)
        bias[:B * H * S] = b["bias"].reshape(-1)
    c_code = code_of(K, b["c"].dtype) if b["c"] is not None else code_of(K, F32)
    out, probs = out_buf(B * H * 64, dtype), out_buf(B * H * S, dtype)
    call("ofa_attn_decode", ptr(b["q"]), ptr(cache[0]), ptr(cache[1]), ptr(bias), ptr(kpm), ptr(b["c"]), c_code, ptr(out), ptr(probs), B, H, 64, S,
         ldk, bsk, kpm_ld, ao.DEC_SCALE, code, st)
    torch.cuda.synchronize()
    return {"out": taken(out, B * H * 64, case.name), "probs": taken(probs, B * H * S, case.name)}


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_attn_decode_per_element(K, dtype):
    """attn_decode's out and probs at S = 1 ... 513 around the keys-per-iteration seams (32 for the 16-bit types, 16 for fp32) and the
    256-stride of the exp loop, at the last S under the 64 KB LDS line and the first above it, and at the cap 32 768; a strided cache
    with NaN rows behind S, kpm_ld > S, bias on / off, c_attn absent, in q's dtype and in fp32; a fully masked row gives zeros."""
    w, lds = Worst(), []
    for case in ao.DEC_CASES:
        b = ao.build_dec(case, dtype, DEV)
        got = run_decode(K, case, b, dtype)
        fig = ao.dec_figures(case, b, got, dtype)
        bad = {n: v for n, v in fig.items() if not v <= ao.limit("decode", dtype)}
        assert not bad, (case.name, ao.NAMES[dtype], bad, ao.limit("decode", dtype))
        for n, v in fig.items():
            w.see(n, v, case.name)
        if case.special == "masked_row":
            assert float(got["out"].view(case.B, -1)[1].abs().max()) == 0.0 and float(got["probs"].view(case.B, -1)[1].abs().max()) == 0.0
        if b["S"] > 513:
            lds.append(f"S={b['S']}: {ao.dec_lds(b['S'], dtype)} bytes")
    print(w.line(f"decode {ao.NAMES[dtype]}", ao.limit("decode", dtype)) + "\n  LDS " + ", ".join(lds))


# ------------------------------------------------------------------------------------------------------------------ bias blocks
@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_bias_block_add_and_slice_below_at_and_past_the_grid_cap(K, dtype):
    """bias_block_add, _add_batch (one rounding of bias + values on the block, every other element of bias bit-identical) and _slice
    (bit for bit, dbias NaN outside the block) below, at (B=1, A=4, n=512: exactly 1 048 576 items) and past the 4096-block cap
    (n = 1025 at an odd start: a second trip of 2049 items)."""
    call, ptr, st, code, w = K.lib().call, K.ptr, K.stream(), code_of(K, dtype), Worst()
    for case in ao.BLK_CASES:
        assert ao.where(ao.blk_work(case), ao.bias_grid(ao.blk_work(case)) * 256) == case.pos
        b = ao.build_blk(case, dtype, DEV)
        n = b["bias"].numel()
        args = (case.B, case.A, case.T, case.start, case.n, code, st)
        if case.kernel == "block_slice":
            inside = torch.zeros_like(b["bias"], dtype=torch.bool)
            ao._blk_view(case, inside).fill_(True)
            dbias = torch.where(inside, b["bias"], torch.full_like(b["bias"], NAN))
            dv = out_buf(ao.blk_work(case), dtype)
            call("ofa_bias_block_slice", ptr(dbias), ptr(dv), *args)
            torch.cuda.synchronize()
            want = ao.blk_slice_expected(case, b)
            assert ao.same_bits(taken(dv, ao.blk_work(case), case.name).view_as(want), want), (case.name, ao.NAMES[dtype], "bits differ")
            continue
        buf = out_buf(n, dtype)
        buf[:n] = b["bias"].reshape(-1)
        call("ofa_bias_" + case.kernel, ptr(buf), ptr(b["values"]), *args)
        torch.cuda.synchronize()
        fig = ao.blk_figures(case, b, taken(buf, n, case.name).view_as(b["bias"]), dtype)
        assert fig["rest"] == 0.0 and fig["y"] <= ao.limit(case.kernel, dtype), (case.name, ao.NAMES[dtype], fig)
        w.see(case.kernel, fig["y"], case.name)
    print(w.line(f"bias blocks {ao.NAMES[dtype]}", ao.limit("block_add", dtype)) + "; block_slice: every bit")


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_bias_block_grad_and_outer_grad_are_the_integer_sums(K, dtype):
    """bias_block_grad over n = 1 ... 130 (one to three 64-column chunks, the partial last one through the LDS turn) x A = 1 ... 40 (a
    second 32-head trip) x B = 1, 3 and bias_outer_grad with V = 4 (one and two column trips) and V = 1 (by shape, with a second trip,
    and by a dbias pointer one element off the 16-byte grid) on integers in [-2, 2], dbias NaN outside the block: the integer sums,
    rounded once, in bits.  One randn case each against float64 within the chain bound."""
    call, ptr, st, code = K.lib().call, K.ptr, K.stream(), code_of(K, dtype)

    def grad(case, randn):
        b = ao.build_grad(case, dtype, DEV, randn)
        dv = out_buf(case.n * case.n * case.A, dtype)
        call("ofa_bias_block_grad", ptr(b["dbias"]), ptr(dv), case.B, case.A, case.T, case.start, case.n, code, st)
        torch.cuda.synchronize()
        return b, taken(dv, case.n * case.n * case.A, case.name).view(case.n, case.n, case.A)

    for case in ao.GRAD_CASES:
        b, got = grad(case, False)
        assert ao.same_bits(got, ao.grad_expected(case, b, dtype)), (case.name, ao.NAMES[dtype], ao.grad_chunks(case.n, case.A))
    case = next(c for c in ao.GRAD_CASES if (c.n, c.A, c.B) == (65, 33, 3))
    b, got = grad(case, True)
    rb = b["dbias"][:, :, case.start:case.start + case.n, case.start:case.start + case.n].double()
    gfig = ao.grad_excess(got, rb.sum(0).permute(1, 2, 0), rb.abs().sum(0).permute(1, 2, 0), dtype)
    assert gfig <= ao.reduction_limit(case.B, dtype), (case.name, gfig)

    def outer(case, randn):
        b = ao.build_outer(case, dtype, DEV, randn)
        n = b["G"].numel()
        base = torch.full((n + 16,), NAN, dtype=dtype, device=DEV)
        G = base[case.offset:case.offset + n]
        G.copy_(b["G"].reshape(-1))
        assert base.data_ptr() % 16 == 0 and ao.outer_v(case.start, case.T, case.P, G.data_ptr() % 16) == ao.outer_case_v(case, dtype)
        nf, np_ = case.F * case.F * case.A, case.P * case.P * case.A
        df, dp = out_buf(nf, dtype), out_buf(np_, dtype)
        call("ofa_bias_outer_grad", ptr(G), ptr(df), ptr(dp), case.A, case.T, case.start, case.F, case.P, code, st)
        torch.cuda.synchronize()
        return b, {"frames": taken(df, nf, case.name).view(case.F, case.F, case.A), "patches": taken(dp, np_, case.name).view(case.P, case.P, case.A)}

    ran = []
    for case in ao.OUTER_CASES:
        b, got = outer(case, False)
        want = ao.outer_expected(case, b, dtype)
        for name in want:
            assert ao.same_bits(got[name], want[name]), (case.name, ao.NAMES[dtype], name, "bits differ")
        V = ao.outer_case_v(case, dtype)
        ran.append(f"V={V} x {ao.outer_col_trips(case.P, V)} trips")
    case = ao.OUTER_CASES[1]
    b, got = outer(case, True)
    n = case.F * case.P
    blk = b["G"][:, case.start:case.start + n, case.start:case.start + n].double().view(case.A, case.F, case.P, case.F, case.P)
    ofig = max(ao.grad_excess(got["frames"], blk.sum((2, 4)).permute(1, 2, 0), blk.abs().sum((2, 4)).permute(1, 2, 0), dtype),
               ao.grad_excess(got["patches"], blk.sum((1, 3)).permute(1, 2, 0), blk.abs().sum((1, 3)).permute(1, 2, 0), dtype))
    assert ofig <= ao.reduction_limit(ao.outer_chain(case, dtype), dtype), (case.name, ofig)
    print(f"\nbias gradients {ao.NAMES[dtype]}: block_grad exact at {len(ao.GRAD_CASES)} shapes, randn {gfig:.3g} of {ao.reduction_limit(3, dtype):.3g}; "
          f"outer_grad exact ({', '.join(ran)}), randn {ofig:.3g} of {ao.reduction_limit(ao.outer_chain(case, dtype), dtype):.3g}")


BUILD_CASES = [(12, 70, ((0, 30), (30, 40)), ao.FP16, True, True), (24, 40, ((8, 32),), ao.BF16, True, True), (25, 40, ((8, 32),), ao.FP16, True, True),
               (49, 40, ((8, 32),), ao.BF16, True, False), (5, 40, tuple((5 * i, 5) for i in range(8)), ao.BF16, True, True),
               (25, 40, tuple((5 * i, 5) for i in range(8)), ao.FP16, False, False)]


@pytest.mark.parametrize("A,T,slots,dtype,with_abs,want_out", BUILD_CASES, ids=[f"A{c[0]}-T{c[1]}-{len(c[2])}slots-{ao.NAMES[c[3]]}-abs{int(c[4])}-out{int(c[5])}"
                                                                                 for c in BUILD_CASES])
def test_bias_build_fp16_launch_seams_eight_slots_and_no_out(K, A, T, slots, dtype, with_abs, want_out):
    """ofa_bias_build where test_bias_build_assembles_and_swizzles does not go: fp16, 24 / 25 / 49 heads (one launch exactly, the seam,
    three launches), 8 slots, out == NULL -- the row-major tensor and both swizzled images bit for bit with the same index
    construction, guards behind all three outputs."""
    g = torch.Generator(device="cpu").manual_seed(A + T + len(slots))
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(DEV)                  # noqa: E731
    abs_b = mk(A, T, T) if with_abs else None
    values = [mk(n, n, A) for _, n in slots]
    sl = K._BiasSlots()
    for i, ((s, n), v) in enumerate(zip(slots, values)):
        sl.values[i], sl.values2[i], sl.inner[i], sl.start[i], sl.n[i] = K.dptr(v), None, 0, s, n
    sl.count = len(slots)
    nswz = K.lib().cdll.ofa_bias_swz_elems(A, T, T)
    nqt = (T + 31) // 32
    assert nswz == A * nqt * nqt * 1024
    out = out_buf(A * T * T, dtype) if want_out else None
    sr, sc = out_buf(nswz, dtype), out_buf(nswz, dtype)
    K.lib().call("ofa_bias_build", K.ptr(abs_b), ctypes.addressof(sl), K.ptr(out), K.ptr(sr), K.ptr(sc), A, T, T, code_of(K, dtype), K.stream())
    torch.cuda.synchronize()
    ref = abs_b.clone() if with_abs else torch.zeros(A, T, T, device=DEV, dtype=dtype)
    for (s, n), v in zip(slots, values):
        ref[:, s:s + n, s:s + n] += v.permute(2, 0, 1)
    if want_out:
        assert ao.same_bits(taken(out, A * T * T, "out").view(A, T, T), ref)
    pad = torch.zeros(A, nqt * 32, nqt * 32, device=DEV, dtype=dtype)
    pad[:, :T, :T] = ref
    lane = torch.arange(64, device=DEV)
    i, hi = lane & 31, lane >> 5
    r = torch.arange(16, device=DEV)
    col = (r & 3)[None, :] + 8 * (r >> 2)[None, :] + 4 * hi[:, None]                # crowl(r, hi): [64, 16]
    tiles = pad.view(A, nqt, 32, nqt, 32).permute(0, 1, 3, 2, 4)                    # [A, qt, kt, row, col]
    row_img = tiles[:, :, :, i[:, None].expand(64, 16), col]
    col_img = tiles[:, :, :, col, i[:, None].expand(64, 16)].permute(0, 2, 1, 3, 4)
    assert ao.same_bits(taken(sr, nswz, "row image").view(A, nqt, nqt, 64, 16), row_img.contiguous())
    assert ao.same_bits(taken(sc, nswz, "column image").view(A, nqt, nqt, 64, 16), col_img.contiguous())


# ------------------------------------------------------------------------------------------------------------------ attention_aux
@pytest.mark.parametrize("dtype", D16, ids=[ao.NAMES[d] for d in D16])
def test_attn_bwd_prep_delta_per_element(K, dtype):
    """attn_delta: B T heads no multiple of the 32 items of a block (one partial block; a partial last block), ldo = heads 64 + 8 with NaN
    padding, Tpad > T: the tail stays NaN."""
    w = Worst()
    for case in ao.DELTA_CASES:
        b = ao.build_delta(case, dtype, DEV)
        ldo, rows = case.heads * 64 + 8, case.B * case.T
        dout, out = (pitched(b[k].reshape(rows, case.heads * 64), ldo) for k in ("dout", "out"))
        n = case.B * case.heads * case.Tpad
        delta = out_buf(n, F32)
        K.lib().call("ofa_attn_bwd_prep", K.ptr(dout), K.ptr(out), K.ptr(delta), case.B, case.heads, case.T, case.Tpad, ldo, code_of(K, dtype), K.stream())
        torch.cuda.synchronize()
        fig = ao.delta_figures(case, b, taken(delta, n, case.name))
        assert fig["tail"] == 0.0 and fig["y"] <= ao.limit("delta", dtype), (case.name, ao.NAMES[dtype], fig)
        w.see("y", fig["y"], case.name)
    print(w.line(f"delta {ao.NAMES[dtype]}", ao.limit("delta", dtype)))


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_transpose_heads_bit_for_bit(K, dtype):
    """[B, T, C] -> [B, C, Tpad] at T = 1, 63, 64, 65 x C = 64, 65, 130, Tpad = T, pad32(T) and T + 70 (a whole block of zeros),
    ld = C and C + 3 with NaN padding: the transposed bits, true zeros for T <= t < Tpad."""
    for case in ao.TR_CASES:
        b = ao.build_tr(case, dtype, DEV)
        x = pitched(b["x"].reshape(ao.TR_B * case.T, case.C), case.ld)
        n = ao.TR_B * case.C * case.Tpad
        xt = out_buf(n, dtype)
        K.lib().call("ofa_transpose_heads", K.ptr(x), K.ptr(xt), ao.TR_B, case.T, case.C, case.Tpad, case.ld, code_of(K, dtype), K.stream())
        torch.cuda.synchronize()
        want = ao.tr_expected(case, b)
        assert ao.same_bits(taken(xt, n, case.name).view_as(want), want), (case.name, ao.NAMES[dtype], "bits differ")
    print(f"\ntranspose_heads {ao.NAMES[dtype]}: {len(ao.TR_CASES)} cases, bit for bit")


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_mean_heads_below_at_and_past_the_grid_cap(K, dtype):
    """mean_heads with 1, 3 and 16 heads below, at and 300 positions past its 1024-block grid (262 144 positions per trip)."""
    w = Worst()
    for case in ao.MEAN_CASES:
        assert ao.where(case.n, ao.mean_grid(case.n) * 256) == case.pos
        b = ao.build_mean(case, dtype, DEV)
        out = out_buf(ao.MEAN_B * case.n, dtype)
        K.lib().call("ofa_mean_heads", K.ptr(b["p"]), K.ptr(out), ao.MEAN_B, case.heads, case.n, code_of(K, dtype), K.stream())
        torch.cuda.synchronize()
        ref, bd = ao.mean_reference(case, b)
        fig = ao.grad_excess(taken(out, ao.MEAN_B * case.n, case.name).view_as(ref), ref, bd, dtype)
        assert fig <= ao.limit("mean_heads", dtype), (case.name, ao.NAMES[dtype], fig)
        w.see("y", fig, case.name)
    print(w.line(f"mean_heads {ao.NAMES[dtype]}", ao.limit("mean_heads", dtype)))


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_c_attn_grad_is_the_integer_sum(K, dtype):
    """c_attn_grad at B T = 5, 1024, 1030 and 2500 (one, one full, two and three trips of the 1024-thread loop), ld > T with NaN in the
    padded tail of delta, overwrite (dc NaN before) and accumulate, c = 1, 2, 0.5 in all three dtypes: the integer sum over c plus the
    gradient already there, rounded once, in bits; the last shape on randn against float64 within the chain bound."""
    def run(case, randn):
        b = ao.build_cg(case, dtype, DEV, randn)
        dc = out_buf(case.heads, dtype)
        if case.acc:
            dc[:case.heads] = b["prev"]
        K.lib().call("ofa_c_attn_grad", K.ptr(b["delta"]), K.ptr(b["c"]), K.ptr(dc), case.B, case.heads, case.T, case.ld, case.acc, code_of(K, dtype),
                     K.stream())
        torch.cuda.synchronize()
        return b, taken(dc, case.heads, case.name)

    for case in ao.CG_CASES:
        b, got = run(case, False)
        assert ao.same_bits(got, ao.cg_expected(case, b, dtype)), (case.name, ao.NAMES[dtype], got, ao.cg_expected(case, b, dtype))
    case = ao.CG_CASES[-1]
    b, got = run(case, True)
    ref, bd = ao.cg_reference(case, b)
    fig = ao.grad_excess(got, ref, bd, dtype)
    print(f"\nc_attn_grad {ao.NAMES[dtype]}: integer sums exact at {len(ao.CG_CASES)} shapes; randn {fig:.3g} of {ao.reduction_limit(ao.CG_CHAIN, dtype):.3g}")
    assert fig <= ao.reduction_limit(ao.CG_CHAIN, dtype), (case.name, fig)
