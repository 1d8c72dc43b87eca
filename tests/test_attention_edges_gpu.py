"""GPU: the fused attention kernels (ofasys_amd.kernels.attn_fwd / attn_bwd, csrc/attention.hip) at tile seams, sharp softmax rows and
the packed layouts the model uses, against the float64 oracle of tests/attn_oracle.py.  Every 16-bit comparison is
excess(kernel, reference, bounds) <= TOL -- a per-element bound in units of the type's eps with no blind rows -- and every call goes
through one helper that hands the kernels NaN-filled outputs, so a value that was not written cannot pass as a stale correct one.

What each test pins (the gaps the suite had):
  near-uniform softmax rows only ............ test_softmax_regimes (+ the branch counts in tests/test_attn_oracle_cpu.py), sharp rows everywhere
  strided production layouts ................ test_packed_layouts_are_bit_identical_to_dense
  ragged kernels vs themselves only ......... test_ragged_cross_... / test_ragged_causal_self_against_reference_per_sample
  a segment without keys / queries .......... test_ragged_empty_segments   (needed a kernel fix: seg_zero_fill)
  fully masked rows of the dense kernels .... test_fully_masked_rows_of_the_dense_kernels, test_masked_key_with_a_dominant_score (a fix: dkv_block)
  lse never compared with a logsumexp ....... check(): lse * ln 2 against the float64 logsumexp in every case
  thin seams ................................ test_seam_sweep (T x S, causal T < S, Tb > T / Sb > S), test_fp16
  unwritten outputs ......................... run(): NaN-filled outs= and poisoned allocator blocks, finiteness asserted
  whole-tensor metric ....................... excess() per element against the magnitude bound, TOL = 2 * EMUL_CEILING"""
import pytest
import torch

from tests import attn_oracle as ao

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
HEADS, SCALE = ao.HEADS, ao.SCALE
NAN = float("nan")


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


def run(K, x, kw, heads=HEADS, scale=SCALE, need_dbias=True, seg=None, outs=None, out_buf=None):
    """attn_fwd + attn_bwd with poisoned outputs -> dict(out, lse, dq, dk, dv, dbias, delta).  outs: caller's (dq, dk, dv) views
    (default: NaN-filled dense tensors); out_buf: a view the forward result is copied into before the backward reads it."""
    q, k, v, dout = x["q"], x["k"], x["v"], x["dout"]
    B, T, D = q.shape
    S = k.shape[1]
    Tpad = K.pad32(T)
    dt = q.dtype
    rows = heads if seg is not None else B * heads
    bias, shared = kw.get("bias"), kw.get("bias_shared", False)
    need_dbias = need_dbias and bias is not None
    _poison(((B, T, D), dt), ((rows, Tpad), torch.float32))
    out, lse = K.attn_fwd(q, k, v, heads, scale, seg=seg, **kw)
    if out_buf is not None:
        out_buf.copy_(out)
        out = out_buf
    if outs is None:
        outs = (_nan((B, T, D), dt), _nan((B, S, D), dt), _nan((B, S, D), dt))
    spec = [((rows, Tpad), torch.float32)]
    if need_dbias:
        spec.append((tuple(bias.shape), torch.float32) if shared else ((B * heads, T, S), dt))
    _poison(*spec)
    dq, dk, dv, dbias, delta = K.attn_bwd(q, k, v, out, dout, lse, heads, scale, need_dbias=need_dbias, outs=outs, seg=seg, **kw)
    torch.cuda.synchronize()
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dbias=dbias, delta=delta)


def check(got, x, kw, dtype, heads=HEADS, scale=SCALE, tag=""):
    """Finite inside the valid region, 16-bit outputs within TOL of the float64 reference per element, lse * ln 2 against logsumexp,
    delta against rowsum(dO * out) and the fp32 shared dbias against the batch sum of dS within their absolute fp32 tolerances."""
    T = x["q"].shape[1]
    args = (x["q"], x["k"], x["v"], x["dout"], heads, scale)
    ref, bd, ones = ao.reference_and_bounds(*args, **kw)
    ref2 = ao.reference(*args, out=got["out"], **kw)               # the backward is handed the stored out: delta and dS follow it
    for n in ("out", "dq", "dk", "dv", "dbias"):
        if got[n] is not None:
            assert bool(torch.isfinite(got[n]).all()), (tag, n, "not finite (an element that was not written reads NaN)")
    lse = got["lse"][:, :T]
    delta = got["delta"][:, :T]
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(delta).all()), (tag, "lse / delta not finite")
    res = {}
    for n in ("out", "dq", "dk", "dv"):
        res[n] = ao.excess(got[n], ref[n], bd[n], ao.EPS[dtype], ones[n] * ao.TINY[dtype])
    if got["dbias"] is not None:
        if got["dbias"].dtype == torch.float32:
            res["dbias32"] = float((got["dbias"].double() - ref2["dbias"]).abs().max()) / ao.DBIAS32_TOL
            assert bool((got["dbias"][bd["dbias"] == 0] == 0).all()), (tag, "shared dbias outside the visible region must be zero")
        else:
            res["dbias"] = ao.excess(got["dbias"], ref["dbias"], bd["dbias"], ao.EPS[dtype], ones["dbias"] * ao.TINY[dtype])
    res["lse"] = float((lse.double() * ao.LN2 - ref["lse"]).abs().max()) / ao.LSE_TOL
    res["delta"] = float((delta.double() - ref2["delta"]).abs().max()) / ao.DELTA_TOL
    print(tag, {n: round(e, 3) for n, e in res.items()})
    for n, e in res.items():
        assert e <= (ao.TOL if n in ("out", "dq", "dk", "dv", "dbias") else 1.0), (tag, n, e)
    return res


def run_case(K, case, dtype):
    x, kw = ao.build_inputs(case, dtype, DEV)
    check(run(K, x, kw), x, kw, dtype, tag=str(tuple(case)))


# ------------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("T", ao.SEAM_T)
def test_seam_sweep(K, T):
    """T x S over the tile seams (32-row waves, 128-row workgroups, key loop unrolled in pairs: 1, 2, 3, 4, 5 key blocks), sharp rows,
    causal off and on incl. T < S, a key-padding mask crossing a 32-key boundary, no / dense / shared / oversized shared bias."""
    for case in ao.seam_cases(T):
        run_case(K, case, torch.bfloat16)


@pytest.mark.parametrize("regime", ["plant_first", "plant_last", "stairs"])
def test_softmax_regimes(K, regime):
    """The online softmax's no-rescale branch in every step (plant_first), one late large rescale (plant_last), a rescale of every
    row by >= 2^8 in every step (stairs): tests/test_attn_oracle_cpu.py proves the inputs reach these branches."""
    for case in ao.REGIME_CASES:
        if case.regime == regime:
            run_case(K, case, torch.bfloat16)


def test_todays_inputs_under_the_per_element_bound(K):
    for case in ao.EXTRA_CASES:
        run_case(K, case, torch.bfloat16)


@pytest.mark.parametrize("part", ["diagonal", "regimes"])
def test_fp16(K, part):
    for case in ao.FP16_CASES:
        if (case.regime == "sharp") == (part == "diagonal"):
            run_case(K, case, torch.float16)


# ------------------------------------------------------------------------------------------------------------------ packed layouts
@pytest.mark.parametrize("T,S", [(129, 129), (33, 97)])
@pytest.mark.parametrize("form", ["self", "cross"])
def test_packed_layouts_are_bit_identical_to_dense(K, T, S, form):
    """The layouts ops.py uses: q, k, v column slices of one [B, T, 3D + 8] buffer in the order k | v | q with the gradients written in
    place into slices of a buffer of the same shape, out / dout slices of [B, T, D + 8]; cross attention with k, v slices of
    [B, S, 2D].  Bit-identical to the dense call; the padding columns are untouched."""
    if form == "self" and T != S:
        S = T
    dtype = torch.bfloat16
    case = ao.Case("sharp", T, S, form == "self", "none", S >= 34, "bf16", 5000 + T)
    x, kw = ao.build_inputs(case, dtype, DEV)
    B, D = ao.BATCH, HEADS * 64
    dense = run(K, x, kw)
    check(dense, x, kw, dtype, tag=f"dense {form} {T}x{S}")
    if form == "self":
        buf = _nan((B, T, 3 * D + 8), dtype)
        gbuf = _nan((B, T, 3 * D + 8), dtype)
        obuf = _nan((2, B, T, D + 8), dtype)
        views = lambda b: (b[:, :, 2 * D:3 * D], b[:, :, :D], b[:, :, D:2 * D])          # noqa: E731  (q, k, v) of k | v | q
        for dst, src in zip(views(buf), (x["q"], x["k"], x["v"])):
            dst.copy_(src)
        obuf[1, :, :, :D].copy_(x["dout"])
        q, k, v = views(buf)
        xp = dict(q=q, k=k, v=v, dout=obuf[1, :, :, :D])
        got = run(K, xp, kw, outs=views(gbuf), out_buf=obuf[0, :, :, :D])
        assert bool(torch.isnan(gbuf[:, :, 3 * D:]).all()) and bool(torch.isnan(obuf[:, :, :, D:]).all()), "padding columns written"
    else:
        kv = _nan((B, S, 2 * D), dtype)
        gkv = _nan((B, S, 2 * D), dtype)
        kv[:, :, :D].copy_(x["k"])
        kv[:, :, D:].copy_(x["v"])
        xp = dict(q=x["q"], k=kv[:, :, :D], v=kv[:, :, D:], dout=x["dout"])
        got = run(K, xp, kw, outs=(_nan((B, T, D), dtype), gkv[:, :, :D], gkv[:, :, D:]))
    for n in ("out", "dq", "dk", "dv"):
        assert torch.equal(got[n], dense[n]), n
    assert torch.equal(got["lse"][:, :T], dense["lse"][:, :T]) and torch.equal(got["delta"][:, :T], dense["delta"][:, :T])


# ------------------------------------------------------------------------------------------------------------------ ragged (segments)
def _segments(qo, ql, ko, kl, rows_q, rows_k):
    from ofasys_amd.packing import Segments
    table = torch.tensor([[qo[i], ql[i], ko[i], kl[i]] for i in range(len(ql))], dtype=torch.int32, device=DEV)
    return Segments(table, len(ql), rows_q, rows_k, max(ql), max(kl))


def _ragged(K, qo, ql, ko, kl, rows_q, rows_k, causal, dtype, seed, bias=None, c_mode="f32"):
    """Run the packed call and check every row: valid rows against reference() evaluated per sample, filler rows (and every row of a
    sample whose other side is empty) exactly zero -- their bound is zero."""
    heads, D = HEADS, HEADS * 64
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda n, amp=1.0: (amp * torch.randn(1, n, D, generator=g)).to(dtype).to(DEV)          # noqa: E731
    x = dict(q=mk(rows_q, 4.0), k=mk(rows_k), v=mk(rows_k), dout=mk(rows_q))                      # (sharp rows: q times 4)
    kw = dict(causal=causal)
    if c_mode != "none":
        c = 1 + 0.2 * torch.randn(heads, generator=g)
        kw["c_attn"] = (c.float() if c_mode == "f32" else c.to(torch.bfloat16)).to(DEV)
    if bias is not None:
        kw["bias"], kw["bias_shared"] = bias, True
    seg = _segments(qo, ql, ko, kl, rows_q, rows_k)
    got = run(K, x, kw, seg=seg)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=DEV)          # noqa: E731
    ref = dict(out=f64(1, rows_q, D), dq=f64(1, rows_q, D), dk=f64(1, rows_k, D), dv=f64(1, rows_k, D), lse=f64(heads, rows_q),
               delta=f64(heads, rows_q))
    bd = {n: torch.zeros_like(ref[n]) for n in ("out", "dq", "dk", "dv")}
    fl = {n: torch.zeros_like(ref[n]) for n in ("out", "dq", "dk", "dv")}
    if bias is not None:
        ref["dbias"], bd["dbias"], ref["dbias2"] = (torch.zeros_like(bias, dtype=torch.float64) for _ in range(3))
    for i in range(len(ql)):
        if ql[i] <= 0 or kl[i] <= 0:
            continue
        qs, ks = slice(qo[i], qo[i] + ql[i]), slice(ko[i], ko[i] + kl[i])
        xi = (x["q"][:, qs], x["k"][:, ks], x["v"][:, ks], x["dout"][:, qs], heads, SCALE)
        r, b, o = ao.reference_and_bounds(*xi, **kw)
        r2 = ao.reference(*xi, out=got["out"][:, qs], **kw)
        for n, sl in (("out", qs), ("dq", qs), ("dk", ks), ("dv", ks)):
            ref[n][:, sl], bd[n][:, sl], fl[n][:, sl] = r[n], b[n], o[n] * ao.TINY[dtype]
        ref["lse"][:, qs], ref["delta"][:, qs] = r["lse"], r2["delta"]
        if bias is not None:
            ref["dbias"] += r["dbias"]
            bd["dbias"] += b["dbias"]
            ref["dbias2"] += r2["dbias"]
    res = {}
    for n in ("out", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n]).all()), (n, "not finite: rows of the packed buffer were not written")
        res[n] = ao.excess(got[n], ref[n], bd[n], ao.EPS[dtype], fl[n])                  # (bound == 0 on filler rows: exactly zero)
    lse, delta = got["lse"][:, :rows_q], got["delta"][:, :rows_q]
    valid = torch.zeros(rows_q, dtype=torch.bool, device=DEV)
    for i in range(len(ql)):
        valid[qo[i]:qo[i] + ql[i]] = True
    assert bool(torch.isfinite(lse[:, valid]).all()) and bool(torch.isfinite(delta).all()), "lse / delta not finite"
    assert bool((delta[:, ~valid] == 0).all()), "delta of filler rows"
    res["lse"] = float((lse[:, valid].double() * ao.LN2 - ref["lse"][:, valid]).abs().max()) / ao.LSE_TOL
    res["delta"] = float((delta.double() - ref["delta"]).abs().max()) / ao.DELTA_TOL
    if bias is not None:
        assert bool(torch.isfinite(got["dbias"]).all())
        res["dbias32"] = float((got["dbias"].double() - ref["dbias2"]).abs().max()) / ao.DBIAS32_TOL
        assert bool((got["dbias"][bd["dbias"] == 0] == 0).all())
    print(res)
    for n, e in res.items():
        assert e <= (ao.TOL if n in ("out", "dq", "dk", "dv") else 1.0), (n, e)
    return got


CROSS = dict(qo=[0, 160, 192, 512], ql=[150, 24, 300, 1], ko=[0, 64, 352, 512], kl=[40, 260, 129, 7], rows_q=576, rows_k=576)
SELF_LENS = [96, 41, 70, 9, 1]
SELF_OFF = [0, 96, 144, 216, 232]            # each offset the previous end rounded up to 8: multiples of 8, not of 32


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ragged_cross_against_reference_per_sample(K, dtype):
    _ragged(K, causal=False, dtype=dtype, seed=61, **CROSS)


@pytest.mark.parametrize("shared", [False, True])
def test_ragged_causal_self_against_reference_per_sample(K, shared):
    bias = None
    if shared:                                # Tb, Sb beyond the longest sample: the tile clamps of the swizzled image
        bias = torch.randn(HEADS, 96 + 37, 96 + 70, generator=torch.Generator().manual_seed(62)).to(torch.bfloat16).to(DEV)
    _ragged(K, SELF_OFF, SELF_LENS, SELF_OFF, SELF_LENS, 240, 240, True, torch.bfloat16, 63, bias=bias, c_mode="bf16")


@pytest.mark.parametrize("causal", [False, True])
def test_ragged_empty_segments(K, causal):
    """A sample with no keys (a decoder sample whose source is all padding) and one with no queries, in the middle of a batch of
    four: every row of theirs in out, dq, delta is exactly 0, lse is 0, dk / dv are exactly 0 -- not what the allocator held."""
    qo, ql = [0, 56, 80, 80], [50, 24, 0, 33]
    ko, kl = [0, 64, 64, 104], [60, 0, 40, 17]
    got = _ragged(K, qo, ql, ko, kl, 128, 128, causal, torch.bfloat16, 64)
    no_keys = slice(56, 80)
    assert bool((got["lse"][:, no_keys] == 0).all()), "lse of a sample without keys"
    for n in ("out", "dq"):
        assert bool((got[n][:, no_keys] == 0).all()), n
    assert bool((got["delta"][:, no_keys] == 0).all())
    for n in ("dk", "dv"):
        assert bool((got[n][:, 64:104] == 0).all()), n


# ------------------------------------------------------------------------------------------------------------------ fully masked rows
@pytest.mark.parametrize("bias", ["none", "dense"])
@pytest.mark.parametrize("which", ["sample", "causal_key0"])
def test_fully_masked_rows_of_the_dense_kernels(K, which, bias):
    """kpm all true for sample 0, and causal with key 0 of sample 1 padded (query 0 sees nothing): out and dq of those rows exactly 0,
    lse 0, dk / dv of masked keys exactly 0, everything finite, the other rows within TOL."""
    dtype, T, S = torch.bfloat16, 70, 70
    case = ao.Case("sharp", T, S, which == "causal_key0", bias, False, "f32", 6000)
    x, kw = ao.build_inputs(case, dtype, DEV)
    kpm = torch.zeros(ao.BATCH, S, dtype=torch.bool, device=DEV)
    if which == "sample":
        kpm[0] = True
        rows, keys = (0, slice(None)), (0, slice(None))
    else:
        kpm[1, 0] = True
        rows, keys = (1, slice(0, 1)), (1, slice(0, 1))
    kw["kpm"] = kpm
    got = run(K, x, kw)
    check(got, x, kw, dtype, tag=f"masked {which} {bias}")       # (the reference has P = 0 there: bound 0, so exactly zero is asserted)
    for n in ("out", "dq"):
        assert bool((got[n][rows] == 0).all()), n
    lse = got["lse"].view(ao.BATCH, HEADS, -1)[:, :, :T]
    assert bool((lse[rows[0], :, rows[1]] == 0).all()), "lse of a fully masked row"
    for n in ("dk", "dv"):
        assert bool((got[n][keys] == 0).all()), n


@pytest.mark.parametrize("bias", ["none", "shared"])
def test_masked_key_with_a_dominant_score(K, bias):
    """A padded key whose score lies far above the row's logsumexp (here > 140 bits: exp2 of the difference overflows float32): the
    mask decides, not the magnitude -- dk / dv of that key are exactly 0 and nothing turns NaN.  (A probability formed as
    exp2(score - lse) * 0 from the padded row's own score would be inf * 0.)"""
    dtype, T, S, key = torch.bfloat16, 64, 64, 40
    case = ao.Case("plant_first", T, S, False, bias, False, "f32", 6100)
    x, kw = ao.build_inputs(case, dtype, DEV)
    D = HEADS * 64
    kh = x["k"].float().view(ao.BATCH, S, HEADS, 64)
    u = kh[0, 0] / kh[0, 0].norm(dim=-1, keepdim=True)          # key 0 is the planted one: its direction is u up to the noise
    kh[1, key] += 320.0 * u
    x["k"] = kh.view(ao.BATCH, S, D).to(dtype)
    kpm = torch.zeros(ao.BATCH, S, dtype=torch.bool, device=DEV)
    kpm[1, key] = True
    kw["kpm"] = kpm
    raw = (x["q"].double().view(ao.BATCH, T, HEADS, 64)[1] * x["k"].double().view(ao.BATCH, S, HEADS, 64)[1, key]).sum(-1) * SCALE
    assert float(raw.min()) * ao.LOG2E > 140, "the masked key must outscore float32's exp2 range"
    got = run(K, x, kw)
    check(got, x, kw, dtype, tag=f"dominant masked key {bias}")
    assert bool((got["dk"][1, key] == 0).all()) and bool((got["dv"][1, key] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ other properties
@pytest.mark.parametrize("S", [33, 97])
@pytest.mark.parametrize("use_kpm", [False, True])
def test_decode_agrees_with_the_fused_forward(K, S, use_kpm):
    """attn_decode on a cache of S rows = attn_fwd with T = 1 on the same rows: both within TOL of the same reference."""
    dtype = torch.bfloat16
    case = ao.Case("sharp", 1, S, False, "none", False, "f32", 7000 + S)
    x, kw = ao.build_inputs(case, dtype, DEV)
    if use_kpm:
        kw["kpm"] = torch.zeros(ao.BATCH, S, dtype=torch.bool, device=DEV)
        kw["kpm"][-1, S - 33:S - 1] = True
    ref, bd, ones = ao.reference_and_bounds(x["q"], x["k"], x["v"], x["dout"], HEADS, SCALE, **kw)
    out, _ = K.attn_fwd(x["q"], x["k"], x["v"], HEADS, SCALE, kpm=kw.get("kpm"), c_attn=kw["c_attn"])
    cap = S + 7
    kc, vc = _nan((ao.BATCH, cap, HEADS * 64), dtype), _nan((ao.BATCH, cap, HEADS * 64), dtype)
    kc[:, :S], vc[:, :S] = x["k"], x["v"]
    dec, _ = K.attn_decode(x["q"][:, 0], kc, vc, S, HEADS, SCALE, kpm=kw.get("kpm"), c_attn=kw["c_attn"])
    for name, t in (("fused", out), ("decode", dec.unsqueeze(1))):
        e = ao.excess(t, ref["out"], bd["out"], ao.EPS[dtype], ones["out"] * ao.TINY[dtype])
        print(name, S, use_kpm, round(e, 3))
        assert e <= ao.TOL, (name, e)
    # against each other: each within TOL of the reference, so within 2 TOL of one another, per element
    assert ao.excess(dec.unsqueeze(1), out.double(), bd["out"], ao.EPS[dtype], ones["out"] * ao.TINY[dtype]) <= 2 * ao.TOL


@pytest.mark.parametrize("bias", ["none", "dense"])
def test_backward_is_deterministic(K, bias):
    case = ao.Case("sharp", 129, 97, False, bias, True, "f32", 8000)
    x, kw = ao.build_inputs(case, torch.bfloat16, DEV)
    a, b = run(K, x, kw), run(K, x, kw)
    for n in ("out", "dq", "dk", "dv", "dbias"):
        if a[n] is not None:
            assert torch.equal(a[n], b[n]), n
    assert torch.equal(a["delta"][:, :129], b["delta"][:, :129]) and torch.equal(a["lse"][:, :129], b["lse"][:, :129])


def test_refusals_leave_the_outputs_untouched(K):
    """scale <= 0, a leading dimension that is no multiple of 8, a shared bias with Tb < T: host-side argument checks that raise OfaError
    before any launch and write nothing."""
    from ofasys_amd.lib import OfaError
    dtype, T, S = torch.bfloat16, 40, 40
    B, D = ao.BATCH, HEADS * 64
    case = ao.Case("uniform", T, S, False, "none", False, "none", 9000)
    x, _ = ao.build_inputs(case, dtype, DEV)
    good = run(K, x, {})
    outs = lambda: (_nan((B, T, D), dtype), _nan((B, S, D), dtype), _nan((B, S, D), dtype))      # noqa: E731
    untouched = lambda ts: all(bool(torch.isnan(t).all()) for t in ts)                            # noqa: E731
    for scale in (0.0, -0.125):
        with pytest.raises(OfaError):
            K.attn_fwd(x["q"], x["k"], x["v"], HEADS, scale)
    # a leading dimension of D + 4
    wide = torch.zeros(B, T, D + 4, dtype=dtype, device=DEV)
    wide[:, :, :D] = x["q"]
    with pytest.raises(OfaError):
        K.attn_fwd(wide[:, :, :D], x["k"], x["v"], HEADS, SCALE)
    o = (_nan((B, T, D + 4), dtype)[:, :, :D],) + outs()[1:]
    with pytest.raises(OfaError):
        K.attn_bwd(wide[:, :, :D], x["k"], x["v"], good["out"], x["dout"], good["lse"], HEADS, SCALE, outs=o)
    torch.cuda.synchronize()
    assert untouched(t._base if t._base is not None else t for t in o)
    # a shared bias smaller than the call
    small = torch.zeros(HEADS, T - 1, S, dtype=dtype, device=DEV)
    with pytest.raises(OfaError):
        K.attn_fwd(x["q"], x["k"], x["v"], HEADS, SCALE, bias=small, bias_shared=True)
    o = outs()
    with pytest.raises(OfaError):
        K.attn_bwd(x["q"], x["k"], x["v"], good["out"], x["dout"], good["lse"], HEADS, SCALE, bias=small, bias_shared=True,
                   need_dbias=True, outs=o)
    torch.cuda.synchronize()
    assert untouched(o)
