"""A plain-torch oracle for the attention side kernels: the row softmax family (csrc/softmax.hip), the position-bias assembly
(csrc/bias.hip), decode attention (csrc/attention_decode.hip) and delta / head mean / head transpose / c_attn gradient
(csrc/attention_aux.hip).  No GPU needed, no dependency on the kernels.  It follows tests/stream_oracle.py and takes excess(),
grad_excess(), floor_of(), EPS, NVEC from tests/rownorm_oracle.py and same_bits(), small_ints(), where(), U32 from tests/stream_oracle.py.

Launch arithmetic, restated, so that every case is named by where it sits:
  sm_ni()            the row lives in NI registers per lane, NI the first of 1, 2, 4, 8, 16, 32, 64 that holds ceil(sk / 64)
  sm_idle_waves()    4 rows per block: waves of the last block that return early
  bias_grid()        bias_block_add / _add_batch / _slice: at most 4096 blocks = 1 048 576 items per trip (BIAS_T)
  grad_chunks()      bias_block_grad: 64-column chunks (the last one partial through the LDS turn) and 32-head trips
  outer_v()          bias_outer_grad: 4 elements per piece iff start, T, P are multiples of 4 and dbias sits on the 16-byte grid;
  outer_col_trips()  trips of its column loop (64 V columns each)
  mean_grid()        mean_heads: at most 1024 blocks = 262 144 positions per trip (MEAN_T)
  dec_kpi()          decode: keys per block iteration (32 for the 16-bit types, 16 for fp32); dec_lds(): the LDS bytes of a launch,
                     (pad4(S) + kpi * 64) * 4, against the 64 KB line behind which the entry point raises the kernel's limit
  cgrad_trips()      c_attn_grad: trips of the 1024-thread loop over B * T

Three kinds of check, as in the stream oracle:
  movers            bias_block_slice, transpose_heads: *_expected(), bit for bit (bias_build's three outputs are built and compared in
                    tests/test_attnside_edges_gpu.py with the index construction of test_bias_build_assembles_and_swizzles)
  exact reductions  bias_block_grad, bias_outer_grad, c_attn_grad (c a power of two) on integers in [-2, 2]: any summation order gives
                    one fp32 answer, a 16-bit output is that integer rounded once; one randn case each against float64 within
                    chain * 2^-24 * sum|terms| (16-bit outputs: one rounding of that)
  one rounding      the softmax family forward and backward, decode (out and probs), bias_block_add / _add_batch, mean_heads, delta:
                    *_reference() in float64 on the stored inputs with the componentwise magnitude bound, *_emulate() in float32 with
                    the kernel's rounding points and nothing else of it, taking one named mutation (MUTATIONS)
A softmax probability's bound is the probability times 1 + k (|t| + max|t|), t the score after scale and bias: the first-order effect
of the fp32 rounding of the scores, k = 1 for fp32 and 2^-24 / eps for a 16-bit output (as _xha of the rownorm oracle).  The bound is
exactly 0 above the causal diagonal, at a padded key, at a key filled with -10000 next to a live one and for t >= T of the transpose,
so excess() demands a true zero there.  A fully key-padded row of attn_softmax is NaN, as torch.softmax gives (the decode and fused
kernels give 0): the reference returns those rows and figures() demands NaN on exactly them.

Inputs: randn; `offset` (+200 on every score of a row: a missing max subtraction overflows); `sharp` (+60 on one seam column of each
row: the rest of the row sits 30 below the max after the scale of 0.5, inside expf's range for fp32, below fp16's subnormals, which
floor_of() allows for).  tests/test_attnside_oracle_cpu.py proves the tables sound; tests/test_attnside_edges_gpu.py runs them."""
import itertools
from collections import namedtuple

import torch

from tests.rownorm_oracle import BF16, DTYPES3, EPS, F32, FP16, NAMES, NVEC, cdiv, excess, floor_of, grad_excess  # noqa: F401
from tests.stream_oracle import U32, _gen, same_bits, small_ints, where  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------- measured constants
# CEILING: the cap on excess(emulate, reference, bound) of the 16-bit outputs over the whole table: one rounding of the result.
# Measured 2026-10-21 (tests/test_attnside_oracle_cpu.py prints the figures with -s), the emulation's worst excess in eps:
#          sm_plain sm_masked sm_causal sm_attn sm_bwd sm_bwd_causal decode out / probs  block_add add_batch mean_heads
#   bf16   0.991    0.985     0.996     0.993   0.990  0.996         0.792 / 0.995        0.996     0.996     0.996
#   fp16   0.952    0.947     0.980     0.988   0.683  0.782         0.845 / 0.948        0.999     0.999     0.999
CEILING = 1.0
# TOL for the kernels = 2 * CEILING: the factor covers device expf / __expf / reciprocal and the summation order.  Never set from a kernel.
TOL = 2.0 * CEILING
# fp32 outputs (fp32 tensors; delta for both 16-bit types): error / bound, 8 x the emulation's worst against float64.
# Measured 2026-10-21, the emulation's worst over the tables:
#   sm_plain 1.08e-7, sm_masked 9.36e-8, sm_causal 1.26e-7, sm_attn 1.23e-7, sm_bwd 1.05e-7, sm_bwd_causal 1.12e-7,
#   decode 7.35e-8 (probs; out 2.33e-8), block_add 5.96e-8, block_add_batch 5.96e-8, mean_heads 2.26e-7, delta 4.47e-8 (bf16), 3.93e-8 (fp16)
G32 = {"sm_plain": 8 * 1.1e-7, "sm_masked": 8 * 9.4e-8, "sm_causal": 8 * 1.3e-7, "sm_attn": 8 * 1.3e-7, "sm_bwd": 8 * 1.1e-7,
       "sm_bwd_causal": 8 * 1.2e-7, "decode": 8 * 7.4e-8, "block_add": 8 * 6.0e-8, "block_add_batch": 8 * 6.0e-8, "mean_heads": 8 * 2.3e-7,
       "delta": 8 * 4.5e-8}
# The kernels themselves on an MI355X, worst over the same tables (tests/test_attnside_edges_gpu.py prints them with -s):
#   2026-10-21, 16-bit outputs, excess in eps against TOL = 2.0:
#          sm_plain sm_masked sm_causal sm_attn sm_bwd sm_bwd_causal decode out / probs  block_add add_batch mean_heads
#   bf16   0.991    0.985     0.996     0.993   0.990  0.996         0.792 / 0.995        0.996     0.996     0.996
#   fp16   0.952    0.947     0.980     0.988   0.683  0.782         0.845 / 0.948        0.999     0.999     0.999
#   fp32 outputs, error / bound, of 8 x the emulation's figure above: sm_plain 8.80e-8, sm_masked 9.36e-8, sm_causal 1.22e-7,
#   sm_attn 1.19e-7, sm_bwd 1.05e-7, sm_bwd_causal 1.11e-7, decode out 1.91e-8 / probs 5.82e-8, block_add 5.96e-8, block_add_batch 5.96e-8,
#   mean_heads 2.26e-7, delta 3.60e-8 (bf16), 3.86e-8 (fp16)
#   every softmax family ran NI = 1, 2, 4, 8, 16, 32, 64; decode ran 65 536 / 65 552 / 139 264 bytes of LDS (fp32: 135 168) -- the launches
#   above the 64 KB line succeed; the bias blocks ran their second trip on 2049 items, mean_heads on 300 positions, bias_outer_grad
#   V = 4 with one and two column trips and V = 1 with one and two and through the misaligned pointer, c_attn_grad one to three trips.
#   movers (block_slice, transpose_heads, bias_build's three outputs) and the integer reductions (block_grad, outer_grad, c_attn_grad):
#   every bit; on randn block_grad 1.09e-7 of 1.79e-7 (fp32; 0.996 / 0.999 eps in bf16 / fp16), outer_grad 5.7e-10 of 3.15e-5,
#   c_attn_grad 2.6e-11 of 1.61e-6.  No fault found.

SM_LADDER = (1, 2, 4, 8, 16, 32, 64)
SM_SK = (1, 63, 64, 65, 129, 257, 513, 1025, 2048, 2049, 4096)
SM_SCALE = 0.5                                                         # a power of two: x * scale is exact, fused or not
BIAS_CAP, MEAN_CAP = 4096, 1024
BIAS_T, MEAN_T = BIAS_CAP * 256, MEAN_CAP * 256
DEC_SCALE, DEC_CAP, LDS_LINE = 0.125, 32768, 64 * 1024
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------- launches, restated
def sm_ni(sk):
    return next(n for n in SM_LADDER if cdiv(sk, 64) <= n)


def sm_idle_waves(rows):
    return cdiv(rows, 4) * 4 - rows


def bias_grid(work):
    return min(max(cdiv(work, 256), 1), BIAS_CAP)


def mean_grid(n):
    return min(cdiv(n, 256), MEAN_CAP)


def grad_chunks(n, A):
    """-> (64-column chunks, columns of the last chunk, 32-head trips)."""
    return cdiv(n, 64), n - (cdiv(n, 64) - 1) * 64, cdiv(A, 32)


def outer_v(start, T, P, offset_bytes):
    return 4 if start % 4 == 0 and T % 4 == 0 and P % 4 == 0 and offset_bytes % 16 == 0 else 1


def outer_col_trips(P, V):
    return cdiv(P, 64 * V)


def dec_kpi(dtype):
    return 256 // (64 // NVEC[dtype])


def dec_lds(S, dtype):
    return (((S + 3) & ~3) + dec_kpi(dtype) * 64) * 4


def dec_last_under(dtype):
    """The largest S whose launch stays at or under the 64 KB line."""
    return LDS_LINE // 4 - dec_kpi(dtype) * 64


def cgrad_trips(n):
    return cdiv(n, 1024)


def pad32(t):
    return cdiv(t, 32) * 32


def _rn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _amp_k(dtype):
    return 1.0 if dtype == F32 else U32 / EPS[dtype]


def limit(kernel, dtype, is_kernel=True):
    """The largest figure an output may show: the emulation's cap, or (is_kernel) what the GPU test allows a kernel."""
    if dtype == F32 or kernel == "delta":
        return G32[kernel] / (1 if is_kernel else 8)
    return TOL if is_kernel else CEILING


# ================================================================================================================ softmax family
Sm = namedtuple("Sm", "name kernel b np sq sk regime opt seed")
SM_FWD = ("sm_plain", "sm_masked", "sm_causal", "sm_attn")
SM_BWD = ("sm_bwd", "sm_bwd_causal")
REGIMES = ("randn", "offset", "sharp")


def _sm_cases():
    out = []

    def add(kernel, b, np_, sq, sk, regime, **opt):
        what = " ".join(f"{k}={v}" for k, v in opt.items())
        out.append(Sm(f"{kernel} b{b} np{np_} sq{sq} sk{sk} NI{sm_ni(sk)} {regime} {what}".strip(), kernel, b, np_, sq, sk, regime, tuple(opt.items()),
                      6000 + len(out)))

    for i, sk in enumerate(SM_SK):
        b, np_ = ((2, 3), (1, 5))[i % 2]                                 # 6 or 5 rows: never a multiple of 4
        add("sm_plain", b, np_, 1, sk, REGIMES[i % 3])
        add("sm_bwd", b, np_, 1, sk, REGIMES[(i + 1) % 3], inplace=i % 2)
        add("sm_masked", 2, 3, 1, sk, REGIMES[(i + 2) % 3], mask_b=(2, 1)[i % 2])
    add("sm_masked", 2, 3, 3, 65, "randn", mask_b=2)                     # 18 rows: the query index inside the mask
    add("sm_masked", 2, 3, 3, 129, "offset", mask_b=1)
    for i, sk in enumerate(SM_SK[:-1]):                                  # causal: sq == sk, [ab, sq, sq]
        ab = 5 if sk == 1 else (3 if sk <= 65 else 1)
        add("sm_causal", ab, 1, sk, sk, REGIMES[i % 3])
        add("sm_bwd_causal", ab, 1, sk, sk, REGIMES[(i + 1) % 3], inplace=(i + 1) % 2)
    combos = list(itertools.product((0, 1), repeat=3))                   # (causal, kpm, bias)
    for i, sk in enumerate(SM_SK):
        causal, kpm, bias = combos[i % 8]
        T = sk if causal and sk <= 129 else (3 if sk <= 513 else 1)
        add("sm_attn", 2, 3, T, sk, REGIMES[i % 3], bias=bias, kpm=kpm, causal=causal)
    add("sm_attn", 2, 3, 63, 63, "randn", bias=0, kpm=0, causal=1)
    add("sm_attn", 2, 3, 65, 65, "sharp", bias=1, kpm=1, causal=1)
    add("sm_attn", 2, 3, 3, 65, "randn", bias=1, kpm=1, causal=0, special="padded_batch")
    add("sm_attn", 2, 3, 65, 65, "randn", bias=1, kpm=0, causal=1, special="nan_score")
    return out


SM_CASES = _sm_cases()
SM_MUTATIONS = {"sm_plain": ("upper_registers_dropped", "max_not_subtracted", "scale_missing"),
                "sm_masked": ("upper_registers_dropped", "max_not_subtracted", "mask_row_from_head", "mask_b_ignored", "mask_query_ignored"),
                "sm_causal": ("upper_registers_dropped", "max_not_subtracted", "causal_diagonal_masked", "row_not_wrapped"),
                "sm_attn": ("upper_registers_dropped", "max_not_subtracted", "kpm_by_bh", "nan_kept", "bias_row_from_batch", "causal_diagonal_masked"),
                "sm_bwd": ("upper_registers_dropped", "bwd_scale_missing", "bwd_sum_dropped"),
                "sm_bwd_causal": ("upper_registers_dropped", "causal_last_off_by_one", "row_not_wrapped")}


def sm_rows(case):
    return case.b * case.np * case.sq


def _sm_x(case, gen, rows):
    x = _rn(gen, rows, case.sk)
    if case.regime == "offset":
        x = x + 200.0
    elif case.regime == "sharp":                                         # the seam columns, dealt over the rows
        ni, sk = sm_ni(case.sk), case.sk
        seams = sorted({0, sk - 1, min(sk - 1, (ni // 2) * 64), max(0, (ni // 2) * 64 - 1), sk // 2})
        r = torch.arange(rows)
        col = torch.tensor(seams)[r % len(seams)]
        if case.kernel in ("sm_causal", "sm_bwd_causal") or dict(case.opt).get("causal"):
            col = torch.minimum(col, r % case.sq)                        # a visible column
        x[r, col] += 60.0
    return x


def build_sm(case, dtype, device="cpu"):
    """The stored inputs of one softmax case: x [rows, sk] (+ mask, bias, kpm); the backward cases: y (the forward emulation's stored
    output) and dy, both NaN above the causal diagonal."""
    gen, rows, sk, o = _gen(case.seed), sm_rows(case), case.sk, dict(case.opt)
    b = dict(rows=rows, x=_sm_x(case, gen, rows).to(dtype), mask=None, bias=None, kpm=None)
    if case.kernel == "sm_masked":
        m = torch.rand(o["mask_b"], case.sq, sk, generator=gen) < 0.3
        if o["mask_b"] == 2:
            m[1, 0, :] = True                                            # a fully masked row: uniform through the -10000 fill
            m[0, 0, :] = False
            m[0, 0, sk // 2] = sk > 1
        b["mask"] = m.to(torch.uint8)
    if case.kernel == "sm_attn":
        if o["bias"]:
            b["bias"] = _rn(gen, rows, sk).to(dtype)
        if o["kpm"]:
            k = torch.rand(case.b, sk, generator=gen) < 0.3
            k[:, 0] = False                                              # column 0 stays visible: no row dies by accident
            k[0, -1], k[1, -1] = sk > 1, False                           # the samples differ in the last column
            if o.get("special") == "padded_batch":
                k[1, :] = True
            b["kpm"] = k.to(torch.uint8)
        if o.get("special") == "nan_score":
            b["x"][7, 2] = NAN                                           # below the diagonal: query 7, key 2
            b["x"][4 * case.sq + 30, 30] = NAN                           # on the diagonal, attention batch 4
            b["x"][9, 40] = NAN                                          # above it: hidden by the triangle either way
    if case.kernel in SM_BWD:
        fwd = case._replace(kernel="sm_causal" if case.kernel == "sm_bwd_causal" else "sm_plain")
        b["y"] = sm_emulate(fwd, b, dtype)
        b["dy"] = _rn(gen, rows, sk).to(dtype)
        if case.kernel == "sm_bwd_causal":                               # what the backward must not read: NaN above the diagonal of y and dy
            q, _, c = _sm_index(case, "cpu")
            for n in ("y", "dy"):
                b[n] = b[n].masked_fill(c[None, :] > q[:, None], NAN)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in b.items()}


def _sm_index(case, dev):
    rows = sm_rows(case)
    r = torch.arange(rows, device=dev)
    return r % case.sq, r // case.sq, torch.arange(case.sk, device=dev)      # q, ab, c


def _sm_scores(case, b, ft, mutation=None):
    """t (scores after scale, bias and fills, -inf where dead), |t| and the dead mask, in float type ft."""
    o, k = dict(case.opt), case.kernel
    q, ab, c = _sm_index(case, b["x"].device)
    scale = 1.0 if mutation == "scale_missing" else SM_SCALE
    t = b["x"].to(ft) * scale
    dead = filled = torch.zeros_like(t, dtype=torch.bool)
    tri = c[None, :] > q[:, None]
    if mutation == "causal_diagonal_masked":
        tri = c[None, :] >= q[:, None]
    if mutation == "row_not_wrapped":                                    # the query index taken from the flat row
        tri = c[None, :] > torch.arange(sm_rows(case), device=t.device)[:, None]
    if k == "sm_masked":
        bi = ab // case.np
        if mutation == "mask_row_from_head":
            bi = ab % case.np
        mb = torch.zeros_like(bi) if (o["mask_b"] == 1 or mutation == "mask_b_ignored") else bi % o["mask_b"]
        mq = torch.zeros_like(q) if mutation == "mask_query_ignored" else q
        filled = b["mask"][mb, mq].bool()
        t = torch.where(filled, torch.full_like(t, -10000.0), t)
    if k == "sm_causal":
        dead = tri
    if k == "sm_attn":
        if b["bias"] is not None:
            bias = b["bias"].to(ft)
            if mutation == "bias_row_from_batch":
                bias = bias[(ab // case.np) * case.np * case.sq + q]
            t = t + bias
        if o["causal"]:
            if mutation != "nan_kept":
                t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
            dead = dead | tri
        if b["kpm"] is not None:
            kb = ab % case.b if mutation == "kpm_by_bh" else ab // case.np
            dead = dead | b["kpm"][kb].bool()
    ta = t.abs().masked_fill(filled, 0.0)                                # (the -10000 fill is a constant: it carries no rounding)
    return t.masked_fill(dead, float("-inf")), ta.masked_fill(dead, 0.0), dead


def sm_reference(case, b):
    """float64 -> (y, bound, rows that are NaN: every key dead)."""
    t, ta, dead = _sm_scores(case, b, torch.float64)
    m = t.amax(-1, keepdim=True)
    nanrow = torch.isinf(m).squeeze(-1)
    e = torch.exp(t - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    y = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    bound = y * (1.0 + _amp_k(b["x"].dtype) * (ta + ta.amax(-1, keepdim=True)))
    return y, bound, nanrow


def _upper_dropped(case):
    """Columns a kernel that used NI / 2 registers would never see."""
    return (sm_ni(case.sk) // 2) * 64


def sm_emulate(case, b, dtype, mutation=None):
    """float32: t = x * scale (+ bias), the fills, e = exp(t - max), y = e * (1 / sum e), rounded once."""
    assert mutation is None or mutation in SM_MUTATIONS[case.kernel], (case.kernel, mutation)
    t, _, _ = _sm_scores(case, b, F32, mutation)
    keep = case.sk
    if mutation == "upper_registers_dropped":
        keep = _upper_dropped(case)
        t = t[:, :keep]
    mx = torch.zeros(t.shape[0], 1, device=t.device) if mutation == "max_not_subtracted" else t.amax(-1, keepdim=True)
    e = torch.exp(t - mx)
    y = e * (1.0 / e.sum(-1, keepdim=True))
    if keep < case.sk:
        y = torch.cat([y, torch.full((t.shape[0], case.sk - keep), NAN, device=t.device)], dim=1)
    return y.to(dtype)


def _bwd_live(case, b):
    q, _, c = _sm_index(case, b["y"].device)
    if case.kernel == "sm_bwd_causal":
        return c[None, :] <= q[:, None]
    return torch.ones_like(b["y"], dtype=torch.bool)


def sm_bwd_reference(case, b):
    """dx = scale y (dy - sum(dy y)) over the live columns; nothing above the causal diagonal is read."""
    live = _bwd_live(case, b)
    y = torch.where(live, b["y"].double(), torch.zeros((), dtype=torch.float64, device=live.device))
    dy = torch.where(live, b["dy"].double(), torch.zeros((), dtype=torch.float64, device=live.device))
    s, sa = (dy * y).sum(-1, keepdim=True), (dy * y).abs().sum(-1, keepdim=True)
    return SM_SCALE * y * (dy - s), SM_SCALE * ((y * dy).abs() + y.abs() * sa)


def sm_bwd_emulate(case, b, dtype, mutation=None):
    assert mutation is None or mutation in SM_MUTATIONS[case.kernel], (case.kernel, mutation)
    live = _bwd_live(case, b)
    q, _, c = _sm_index(case, b["y"].device)
    if mutation == "causal_last_off_by_one":
        live = c[None, :] < q[:, None]
    if mutation == "row_not_wrapped":
        live = c[None, :] <= torch.arange(sm_rows(case), device=live.device)[:, None]
    keep = _upper_dropped(case) if mutation == "upper_registers_dropped" else case.sk
    live = live & (c[None, :] < keep)
    zero = torch.zeros((), device=live.device)
    p = torch.where(live, b["y"].float(), zero)
    g = torch.where(live, b["dy"].float(), zero) * p
    s = torch.zeros_like(g[:, :1]) if mutation == "bwd_sum_dropped" else g.sum(-1, keepdim=True)
    dx = (1.0 if mutation == "bwd_scale_missing" else SM_SCALE) * (g - p * s)
    if keep < case.sk:
        dx[:, keep:] = NAN
    return dx.to(dtype)


def sm_figures(case, b, got, dtype):
    """-> {"y": figure}; inf unless the NaN rows are exactly the fully key-padded ones."""
    if case.kernel in SM_BWD:
        ref, bd = sm_bwd_reference(case, b)
        return {"y": grad_excess(got, ref, bd, dtype)}
    ref, bd, nanrow = sm_reference(case, b)
    got = got.view_as(ref)
    if not bool(torch.isnan(got[nanrow]).all()):
        return {"y": float("inf")}
    ok = ~nanrow
    return {"y": grad_excess(got[ok], ref[ok], bd[ok], dtype)}


def sm_applies(mutation, case, dtype):
    o = dict(case.opt)
    return {"upper_registers_dropped": sm_ni(case.sk) > 1, "mask_row_from_head": o.get("mask_b") == 2, "mask_b_ignored": o.get("mask_b") == 2,
            "mask_query_ignored": case.sq > 1, "kpm_by_bh": bool(o.get("kpm")), "nan_kept": o.get("special") == "nan_score",
            "bias_row_from_batch": bool(o.get("bias")), "causal_diagonal_masked": case.kernel == "sm_causal" or bool(o.get("causal")),
            "row_not_wrapped": case.b > 1 and case.sk > 1, "bwd_sum_dropped": case.sk > 1}.get(mutation, True)


# ================================================================================================================ decode attention
Dec = namedtuple("Dec", "name S B heads strided bias kpm c special seed")
DEC_S = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513, "under", "above", DEC_CAP)
DEC_MUTATIONS = ("last_partial_key_group_dropped", "c_attn_omitted", "bias_before_scale", "kpm_by_bh", "exp_second_trip_skipped", "masked_row_nan",
                 "head_from_batch")


def _dec_cases():
    out = []
    for i, S in enumerate(DEC_S):
        small = isinstance(S, int) and S <= 513
        B, heads = (2, 3) if small else (1, 1)
        c = ("none", "same", "f32")[i % 3]
        out.append(Dec(f"decode S{S} B{B} h{heads} {'strided' if i % 2 == 0 else 'dense'} bias{i % 2} kpm{int(i % 4 < 2)} c_{c}", S, B, heads,
                       i % 2 == 0, i % 2 == 1, i % 4 < 2, c, None, 6500 + i))
    out.append(Dec("decode S33 B2 h3 strided bias1 kpm1 c_same masked_row", 33, 2, 3, True, True, True, "same", "masked_row", 6590))
    out.append(Dec("decode S257 B2 h3 dense bias1 kpm0 c_f32", 257, 2, 3, False, True, False, "f32", None, 6591))
    out.append(Dec("decode S513 B2 h3 strided bias1 kpm1 c_same", 513, 2, 3, True, True, True, "same", None, 6592))
    return out


DEC_CASES = _dec_cases()


def dec_S(case, dtype):
    return {"under": dec_last_under(dtype), "above": dec_last_under(dtype) + 1}.get(case.S, case.S)


def build_dec(case, dtype, device="cpu"):
    """Logical operands: q [B, heads, 64], k / v [B, S, heads, 64] (the GPU test lays them out in a strided cache), bias [B * heads, S],
    kpm [B, S] bytes, c [heads] in q's dtype or fp32."""
    gen, S, B, H = _gen(case.seed), dec_S(case, dtype), case.B, case.heads
    b = dict(S=S, q=_rn(gen, B, H, 64).to(dtype), k=_rn(gen, B, S, H, 64).to(dtype), v=_rn(gen, B, S, H, 64).to(dtype), bias=None, kpm=None, c=None)
    if case.bias:
        b["bias"] = _rn(gen, B * H, S).to(dtype)
    if case.kpm:
        m = torch.rand(B, S, generator=gen) < 0.3
        m[:, 0] = False
        m[0, -1] = S > 1
        if case.special == "masked_row":
            m[1, :] = True
        b["kpm"] = m.to(torch.uint8)
    if case.c != "none":
        b["c"] = (1.0 + 0.5 * _rn(gen, H)).to(dtype if case.c == "same" else F32)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in b.items()}


def _dec_scores(case, b, ft, mutation=None):
    B, H, S = case.B, case.heads, b["S"]
    q = b["q"].to(ft)
    if mutation == "head_from_batch":                                    # the q row of (b, h) taken as b * B + h
        q = q.reshape(B * H, 64)[(torch.arange(B, device=q.device)[:, None] * B + torch.arange(H, device=q.device)[None, :]) % (B * H)]
    d = torch.einsum("bhd,bshd->bhs", q, b["k"].to(ft))
    da = torch.einsum("bhd,bshd->bhs", q.abs(), b["k"].to(ft).abs())
    t, ta = d * DEC_SCALE, da * DEC_SCALE
    if b["bias"] is not None:
        bias = b["bias"].to(ft).view(B, H, S)
        t = (d + bias) * DEC_SCALE if mutation == "bias_before_scale" else t + bias
        ta = ta + bias.abs()
    dead = torch.zeros(B, H, S, dtype=torch.bool, device=t.device)
    if b["kpm"] is not None:
        k = b["kpm"].bool()
        if mutation == "kpm_by_bh":
            k = k[torch.arange(B * H, device=t.device) % B].view(B, H, S)
        else:
            k = k[:, None, :].expand(B, H, S)
        dead = dead | k
    return t.masked_fill(dead, float("-inf")), ta.masked_fill(dead, 0.0), dead


def _dec_c(case, b, ft):
    return torch.ones(case.heads, dtype=ft, device=b["q"].device) if b["c"] is None else b["c"].to(ft)


def dec_reference(case, b):
    """float64 -> {out, probs: (ref, bound)}; a fully masked row gives zeros."""
    t, ta, _ = _dec_scores(case, b, torch.float64)
    m = t.amax(-1, keepdim=True)
    e = torch.exp(t - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    l = e.sum(-1, keepdim=True)
    p = e / torch.where(l > 0, l, torch.ones_like(l))
    pb = p * (1.0 + _amp_k(b["q"].dtype) * (ta + ta.amax(-1, keepdim=True)))
    c, v = _dec_c(case, b, torch.float64), b["v"].double()
    out = torch.einsum("bhs,bshd->bhd", p, v) * c[None, :, None]
    ob = torch.einsum("bhs,bshd->bhd", pb, v.abs()) * c.abs()[None, :, None]
    return {"out": (out, ob), "probs": (p, pb)}


def dec_emulate(case, b, dtype, mutation=None):
    """float32: scores, e = exp(t - max), out = (sum e v) * (1 / sum e) * c and probs = e * (1 / sum e), each rounded once."""
    assert mutation is None or mutation in DEC_MUTATIONS, mutation
    S = b["S"]
    t, _, _ = _dec_scores(case, b, F32, mutation)
    keep = S
    if mutation == "last_partial_key_group_dropped":
        keep = (S // dec_kpi(dtype)) * dec_kpi(dtype)
        t = t[..., :keep]
    m = t.amax(-1, keepdim=True) if keep else torch.zeros_like(t[..., :1])
    allmasked = torch.isinf(m)
    e = torch.exp(t - torch.where(allmasked, torch.zeros_like(m), m))
    if mutation == "masked_row_nan":
        e = torch.where(allmasked, torch.full_like(e, NAN), e)
    if mutation == "exp_second_trip_skipped":
        e[..., 256:] = t[..., 256:]
    l = e.sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    if mutation == "masked_row_nan":
        inv = 1.0 / l
    c = torch.ones(case.heads, device=t.device) if (b["c"] is None or mutation == "c_attn_omitted") else b["c"].float()
    out = torch.einsum("bhs,bshd->bhd", e, b["v"].float()[:, :keep]) * inv * c[None, :, None]
    p = e * inv
    if keep < S:
        p = torch.cat([p, torch.full(p.shape[:-1] + (S - keep,), NAN, device=p.device)], dim=-1)
    return {"out": out.to(dtype), "probs": p.to(dtype)}


def dec_figures(case, b, got, dtype):
    ref = dec_reference(case, b)
    return {n: grad_excess(got[n].view_as(ref[n][0]), ref[n][0], ref[n][1], dtype) for n in ("out", "probs")}


def dec_applies(mutation, case, dtype):
    S = dec_S(case, dtype)
    return {"last_partial_key_group_dropped": S % dec_kpi(dtype) != 0, "c_attn_omitted": case.c != "none", "bias_before_scale": case.bias,
            "kpm_by_bh": case.kpm and case.B > 1, "exp_second_trip_skipped": S > 256, "masked_row_nan": case.special == "masked_row",
            "head_from_batch": case.B > 1}[mutation]


# ================================================================================================================ bias blocks
Blk = namedtuple("Blk", "name kernel pos B A n T start seed")
BLOCK_SHAPES = (("below", 2, 3, 5, 8, 0), ("below", 2, 3, 5, 8, 3), ("at", 1, 4, 512, 515, 3), ("past", 1, 1, 1025, 1030, 3))
BLOCK_KERNELS = ("block_add", "block_add_batch", "block_slice")
BLOCK_MUTATIONS = {"block_add": ("second_trip_skipped", "start_dropped", "values_heads_outermost"),
                   "block_add_batch": ("second_trip_skipped", "start_dropped", "values_of_sample_0"),
                   "block_slice": ("second_trip_skipped", "start_dropped")}
BLK_CASES = [Blk(f"{k} {pos} B{B} A{A} n{n} T{T} start{s}", k, pos, B, A, n, T, s, 6700 + 10 * i + j)
             for i, k in enumerate(BLOCK_KERNELS) for j, (pos, B, A, n, T, s) in enumerate(BLOCK_SHAPES)]


def blk_work(case):
    return case.B * case.A * case.n * case.n


def build_blk(case, dtype, device="cpu"):
    gen = _gen(case.seed)
    b = dict(bias=_rn(gen, case.B, case.A, case.T, case.T).to(dtype))
    if case.kernel == "block_add":
        b["values"] = _rn(gen, case.n, case.n, case.A).to(dtype)
    elif case.kernel == "block_add_batch":
        b["values"] = _rn(gen, case.B, case.A, case.n, case.n).to(dtype)
    return {k: v.to(device) for k, v in b.items()}


def _blk_values(case, b, ft, mutation=None):
    """The addend of every block element, [B, A, n, n]."""
    v = b["values"].to(ft)
    if case.kernel == "block_add":
        if mutation == "values_heads_outermost":
            v = v.reshape(case.A, case.n, case.n)
        else:
            v = v.permute(2, 0, 1)
        return v[None].expand(case.B, case.A, case.n, case.n)
    return v[:1].expand_as(v) if mutation == "values_of_sample_0" else v


def _blk_view(case, t, start=None):
    s = case.start if start is None else start
    return t[:, :, s:s + case.n, s:s + case.n]


def blk_reference(case, b):
    """-> (ref, bound) over the block [B, A, n, n]; the rest of bias keeps its bits."""
    x, v = _blk_view(case, b["bias"]).double(), _blk_values(case, b, torch.float64)
    return x + v, x.abs() + v.abs()


def _first_trip(case, t, old):
    """A [B, A, n, n] result whose items >= BIAS_T were never visited."""
    flat, o = t.reshape(-1).clone(), old.reshape(-1)
    flat[BIAS_T:] = o[BIAS_T:]
    return flat.view(t.shape)


def blk_emulate(case, b, dtype, mutation=None):
    """The whole bias tensor after the call: one rounding of bias + values on the block."""
    assert mutation is None or mutation in BLOCK_MUTATIONS[case.kernel], mutation
    out = b["bias"].clone()
    s = 0 if mutation == "start_dropped" else case.start
    old = _blk_view(case, b["bias"], s)
    new = (old.float() + _blk_values(case, b, F32, mutation)).to(dtype)
    if mutation == "second_trip_skipped":
        new = _first_trip(case, new, old)
    _blk_view(case, out, s).copy_(new)
    return out


def blk_slice_expected(case, b, mutation=None, fill=NAN):
    s = 0 if mutation == "start_dropped" else case.start
    out = _blk_view(case, b["bias"], s).contiguous()
    if mutation == "second_trip_skipped":
        out = _first_trip(case, out, torch.full_like(out, fill))
    return out


def blk_figures(case, b, got, dtype):
    """y: the block against float64; rest: 0 iff everything outside the block kept its bits."""
    ref, bd = blk_reference(case, b)
    inside = torch.zeros_like(b["bias"], dtype=torch.bool)
    _blk_view(case, inside).fill_(True)
    rest = same_bits(torch.where(inside, torch.zeros_like(got), got), torch.where(inside, torch.zeros_like(got), b["bias"]))
    return {"y": grad_excess(_blk_view(case, got), ref, bd, dtype), "rest": 0.0 if rest else float("inf")}


def blk_applies(mutation, case, dtype):
    return {"second_trip_skipped": case.pos == "past", "start_dropped": case.start > 0, "values_of_sample_0": case.B > 1}.get(mutation, True)


# ---------------------------------------------------------------------------------------------------------------- bias_block_grad
Grad = namedtuple("Grad", "name n A B start T seed")
GRAD_SHAPES = ((1, 1, 1), (63, 12, 3), (64, 32, 1), (65, 33, 3), (130, 40, 1), (130, 12, 3), (64, 33, 3), (65, 1, 1), (1, 40, 3), (63, 32, 3))
GRAD_CASES = [Grad(f"block_grad n{n} A{A} B{B} start{3 + 2 * (i % 2)}", n, A, B, 3 + 2 * (i % 2), 3 + 2 * (i % 2) + n + 2, 6800 + i)
              for i, (n, A, B) in enumerate(GRAD_SHAPES)]
GRAD_MUTATIONS = ("a0_trip_skipped", "last_column_chunk_dropped", "batch_takes_first", "start_dropped_on_rows")


def build_grad(case, dtype, device="cpu", randn=False):
    """dbias [B, A, T, T]: integers in [-2, 2] (randn: unit normals) on the slot's block, NaN outside it."""
    g = torch.full((case.B, case.A, case.T, case.T), NAN)
    n, s = case.n, case.start
    blk = _rn(_gen(case.seed), case.B, case.A, n, n) if randn else small_ints(case.B * case.A * n * n, case.seed, F32).view(case.B, case.A, n, n)
    g[:, :, s:s + n, s:s + n] = blk
    return dict(dbias=g.to(dtype).to(device))


def grad_expected(case, b, dtype, mutation=None, fill=NAN):
    """dvalues [n, n, A] = sum_b dbias[b, a, s + i, s + j]: the fp32 sum, rounded once."""
    n, s = case.n, case.start
    r0 = 0 if mutation == "start_dropped_on_rows" else s
    blk = b["dbias"][:, :, r0:r0 + n, s:s + n].float()
    out = (blk[0] if mutation == "batch_takes_first" else blk.sum(0)).permute(1, 2, 0).contiguous()
    if mutation == "a0_trip_skipped":
        out[:, :, 32:] = fill
    if mutation == "last_column_chunk_dropped" and n % 64:
        out[:, (n // 64) * 64:, :] = fill
    return out.to(dtype)


def grad_applies(mutation, case):
    return {"a0_trip_skipped": case.A > 32, "last_column_chunk_dropped": case.n % 64 != 0, "batch_takes_first": case.B > 1,
            "start_dropped_on_rows": True}[mutation]


# ---------------------------------------------------------------------------------------------------------------- bias_outer_grad
Outer = namedtuple("Outer", "name F P start T offset A seed")
OUTER_CASES = (Outer("outer V4 one trip F2 P12", 2, 12, 4, 32, 0, 3, 6900), Outer("outer V4 second trip F1 P260", 1, 260, 0, 260, 0, 2, 6901),
               Outer("outer V1 by shape F3 P13", 3, 13, 5, 50, 0, 3, 6902), Outer("outer V1 second trip F2 P66", 2, 66, 1, 135, 0, 2, 6903),
               Outer("outer V1 by alignment F2 P12", 2, 12, 4, 32, 1, 3, 6904))
OUTER_MUTATIONS = ("f2_stride_wrong", "second_column_trip_skipped", "start_dropped_on_rows")


def outer_case_v(case, dtype):
    return outer_v(case.start, case.T, case.P, case.offset * (4 if dtype == F32 else 2))


def build_outer(case, dtype, device="cpu", randn=False):
    """G [A, T, T]: integers (randn: unit normals) on the slot's block, NaN outside it."""
    n = case.F * case.P
    g = torch.full((case.A, case.T, case.T), NAN)
    blk = _rn(_gen(case.seed), case.A, n, n) if randn else small_ints(case.A * n * n, case.seed, F32).view(case.A, n, n)
    g[:, case.start:case.start + n, case.start:case.start + n] = blk
    return dict(G=g.to(dtype).to(device))


def outer_expected(case, b, dtype, mutation=None, fill=NAN):
    """-> {frames [F, F, A], patches [P, P, A]}: the fp32 sums over the patch / the frame pairs, rounded once."""
    F_, P, s, A = case.F, case.P, case.start, case.A
    n = F_ * P
    r0 = 0 if mutation == "start_dropped_on_rows" else s
    if mutation == "f2_stride_wrong":                                    # the column of frame f2 starts at f2 (P - 1)
        cols = (torch.arange(F_)[:, None] * (P - 1) + torch.arange(P)[None, :]).reshape(-1).to(b["G"].device)
        blk = b["G"][:, r0:r0 + n, s:s + n][:, :, cols]
    else:
        blk = b["G"][:, r0:r0 + n, s:s + n]
    blk = blk.float().view(A, F_, P, F_, P)
    width = 64 * outer_case_v(case, dtype)
    if mutation == "second_column_trip_skipped" and P > width:
        frames = blk[..., :width].sum((2, 4))
        patches = blk.sum((1, 3))
        patches[:, :, width:] = fill
    else:
        frames, patches = blk.sum((2, 4)), blk.sum((1, 3))
    return {"frames": frames.permute(1, 2, 0).contiguous().to(dtype), "patches": patches.permute(1, 2, 0).contiguous().to(dtype)}


def outer_applies(mutation, case, dtype):
    return {"f2_stride_wrong": case.F > 1, "second_column_trip_skipped": case.P > 64 * outer_case_v(case, dtype), "start_dropped_on_rows": case.start > 0}[mutation]


def outer_chain(case, dtype):
    """The longest chain of fp32 additions behind one element: frames (a thread's pieces, 6 shuffle steps, 4 waves), patches (F F)."""
    V = outer_case_v(case, dtype)
    return max(cdiv(case.P, 4) * outer_col_trips(case.P, V) * V + 6 + 3, case.F * case.F)


# ================================================================================================================ attention_aux
Delta = namedtuple("Delta", "name B T heads Tpad seed")
DELTA_CASES = (Delta("delta B1 T5 h3 Tpad8: 15 items, one partial block", 1, 5, 3, 8, 7000),
               Delta("delta B2 T7 h3 Tpad7: 42 items, a partial second block", 2, 7, 3, 7, 7001),
               Delta("delta B2 T33 h3 Tpad40: 198 items, seven blocks", 2, 33, 3, 40, 7002))
DELTA_MUTATIONS = ("tpad_taken_as_T", "head_offset_dropped", "last_block_dropped")


def build_delta(case, dtype, device="cpu"):
    gen = _gen(case.seed)
    return {k: _rn(gen, case.B, case.T, case.heads, 64).to(dtype).to(device) for k in ("dout", "out")}


def delta_reference(case, b):
    """-> (ref, bound) [B * heads, T]: rowsum(dO * O) per (sample, head, query)."""
    pr = b["dout"].double() * b["out"].double()
    f = lambda t: t.sum(-1).permute(0, 2, 1).reshape(case.B * case.heads, case.T)      # noqa: E731
    return f(pr), f(pr.abs())


def delta_emulate(case, b, mutation=None):
    """The whole fp32 buffer [B * heads, Tpad], NaN where the kernel writes nothing."""
    assert mutation is None or mutation in DELTA_MUTATIONS, mutation
    out = b["out"].float()
    if mutation == "head_offset_dropped":
        out = out[:, :, :1].expand_as(out)
    d = (b["dout"].float() * out).sum(-1).permute(0, 2, 1).reshape(case.B * case.heads, case.T)
    if mutation == "last_block_dropped":                                 # the items of the partial last block (32 per block)
        items = case.B * case.T * case.heads
        idx = torch.arange((items // 32) * 32, items, device=d.device)
        row, h = idx // case.heads, idx % case.heads
        d[(row // case.T) * case.heads + h, row % case.T] = NAN
    buf = torch.full((case.B * case.heads * case.Tpad,), NAN, device=d.device)
    if mutation == "tpad_taken_as_T":
        buf[:d.numel()] = d.reshape(-1)
        return buf.view(case.B * case.heads, case.Tpad)
    buf = buf.view(case.B * case.heads, case.Tpad)
    buf[:, :case.T] = d
    return buf


def delta_figures(case, b, got):
    """y: error / bound over t < T; tail: 0 iff the Tpad tail is still NaN."""
    ref, bd = delta_reference(case, b)
    got = got.view(case.B * case.heads, case.Tpad)
    tail = bool(torch.isnan(got[:, case.T:]).all())
    return {"y": excess(got[:, :case.T], ref, bd, 1.0, 2.0 ** -126), "tail": 0.0 if tail else float("inf")}


Tr = namedtuple("Tr", "name T C Tpad ld seed")
TR_SHAPES = tuple((T, (64, 65, 130)[(i + j) % 3], kind, 3 * ((i + j) % 2))                   # every T with every Tpad; C and ld go round
                  for i, T in enumerate((1, 63, 64, 65)) for j, kind in enumerate(("T", "pad32", "T+70")))
TR_CASES = [Tr(f"transpose T{T} C{C} Tpad={kind} ld=C+{e}", T, C, {"T": T, "pad32": pad32(T), "T+70": T + 70}[kind], C + e, 7100 + i)
            for i, (T, C, kind, e) in enumerate(TR_SHAPES)]
TR_B = 2
TR_MUTATIONS = ("tail_not_zeroed", "whole_tail_blocks_skipped", "last_column_block_dropped")


def build_tr(case, dtype, device="cpu"):
    """x [B, T, C] (the GPU test stores it with row pitch ld)."""
    return dict(x=_rn(_gen(case.seed), TR_B, case.T, case.C).to(dtype).to(device))


def tr_expected(case, b, mutation=None, fill=NAN):
    """xt [B, C, Tpad]: x transposed, zeros for T <= t < Tpad."""
    x = b["x"]
    out = torch.zeros(TR_B, case.C, case.Tpad, dtype=x.dtype, device=x.device)
    out[:, :, :case.T] = x.permute(0, 2, 1)
    if mutation == "tail_not_zeroed":
        out[:, :, case.T:] = fill
    if mutation == "whole_tail_blocks_skipped":
        out[:, :, cdiv(case.T, 64) * 64:] = fill
    if mutation == "last_column_block_dropped" and case.C % 64:
        out[:, (case.C // 64) * 64:, :] = fill
    return out


def tr_applies(mutation, case):
    return {"tail_not_zeroed": case.Tpad > case.T, "whole_tail_blocks_skipped": case.Tpad > cdiv(case.T, 64) * 64,
            "last_column_block_dropped": case.C % 64 != 0}[mutation]


Mean = namedtuple("Mean", "name pos n heads seed")
MEAN_B = 2
MEAN_CASES = (Mean("mean_heads below n777 heads16", "below", 777, 16, 7200), Mean("mean_heads below n35 heads3", "below", 35, 3, 7201),
              Mean("mean_heads at heads1", "at", MEAN_T, 1, 7202), Mean("mean_heads past +300 heads3", "past", MEAN_T + 300, 3, 7203),
              Mean("mean_heads past +300 heads1", "past", MEAN_T + 300, 1, 7204))
MEAN_MUTATIONS = ("inv_taken_from_B", "second_trip_skipped", "sample_stride_without_heads")


def build_mean(case, dtype, device="cpu"):
    """p [B, heads, n]: probabilities-like, positive."""
    return dict(p=torch.rand(MEAN_B, case.heads, case.n, generator=_gen(case.seed)).to(dtype).to(device))


def mean_reference(case, b):
    p = b["p"].double()
    return p.sum(1) / case.heads, p.abs().sum(1) / case.heads


def mean_emulate(case, b, dtype, mutation=None):
    """float32: the heads added in order, times the fp32 1 / heads, rounded once."""
    assert mutation is None or mutation in MEAN_MUTATIONS, mutation
    p = b["p"].float()
    if mutation == "sample_stride_without_heads":                        # sample b starts at b * n
        flat = p.reshape(-1)
        p = torch.stack([flat[i * case.n:(i + case.heads) * case.n].view(case.heads, case.n) for i in range(MEAN_B)])
    s = torch.zeros(MEAN_B, case.n, device=p.device)
    for a in range(case.heads):
        s = s + p[:, a]
    inv = torch.tensor(1.0) / torch.tensor(float(MEAN_B if mutation == "inv_taken_from_B" else case.heads))
    y = s * inv.to(p.device)
    if mutation == "second_trip_skipped":
        y[:, MEAN_T:] = NAN
    return y.to(dtype)


def mean_applies(mutation, case):
    return {"inv_taken_from_B": case.heads != MEAN_B, "second_trip_skipped": case.pos == "past", "sample_stride_without_heads": case.heads > 1}[mutation]


CG = namedtuple("CG", "name B T ld heads acc seed")
CG_CASES = (CG("c_attn_grad B1 T5 ld8 overwrite", 1, 5, 8, 3, 0, 7300), CG("c_attn_grad B2 T512 ld512 accumulate: 1024, one full trip", 2, 512, 512, 3, 1, 7301),
            CG("c_attn_grad B2 T515 ld520 overwrite: 1030, a second trip on 6 threads", 2, 515, 520, 3, 0, 7302),
            CG("c_attn_grad B4 T625 ld640 accumulate: 2500, three trips", 4, 625, 640, 2, 1, 7303))
CG_MUTATIONS = ("second_trip_skipped", "accumulate_ignored", "division_dropped", "sample_index_from_ld")
CG_CHAIN = 3 + 6 + 16 + 1 + 1                                            # a thread's trips, wave_sum, the 16 waves, the division, the accumulate


def build_cg(case, dtype, device="cpu", randn=False):
    """delta fp32 [B * heads, ld] with NaN for t >= T; c [heads]: powers of two (randn: 1 + 0.5 randn); prev: the gradient already there."""
    gen = _gen(case.seed)
    d = torch.full((case.B * case.heads, case.ld), NAN)
    d[:, :case.T] = _rn(gen, case.B * case.heads, case.T) if randn else small_ints(case.B * case.heads * case.T, case.seed, F32).view(-1, case.T)
    c = (1.0 + 0.5 * _rn(gen, case.heads)) if randn else torch.tensor([1.0, 2.0, 0.5])[:case.heads]
    prev = _rn(gen, case.heads) if randn else torch.tensor([3.0, -2.0, 1.0])[:case.heads]
    return dict(delta=d.to(device), c=c.to(dtype).to(device), prev=prev.to(dtype).to(device))


def cg_expected(case, b, dtype, mutation=None):
    """dc [heads]: the fp32 sum over (b, t < T), divided by c, plus the gradient already there, rounded once."""
    assert mutation is None or mutation in CG_MUTATIONS, mutation
    d = b["delta"].view(case.B, case.heads, case.ld)[:, :, :case.T]
    if mutation == "sample_index_from_ld":                               # b = i / ld, t = i - b ld over the same B T indices
        i = torch.arange(case.B * case.T, device=d.device)
        d = b["delta"].view(case.B, case.heads, case.ld)[(i // case.ld).clamp_max(case.B - 1), :, i % case.ld].t().reshape(case.heads, case.B, case.T)
        d = d.permute(1, 0, 2)
    flat = d.permute(1, 0, 2).reshape(case.heads, case.B * case.T)
    if mutation == "second_trip_skipped":
        flat = flat[:, :1024]
    tot = flat.sum(-1)
    if mutation != "division_dropped":
        tot = tot / b["c"].float()
    if case.acc and mutation != "accumulate_ignored":
        tot = tot + b["prev"].float()
    return tot.to(dtype)


def cg_reference(case, b):
    d = b["delta"].view(case.B, case.heads, case.ld)[:, :, :case.T].double().permute(1, 0, 2).reshape(case.heads, -1)
    c, prev = b["c"].double(), (b["prev"].double() if case.acc else torch.zeros(case.heads, dtype=torch.float64, device=d.device))
    return d.sum(-1) / c + prev, d.abs().sum(-1) / c.abs() + prev.abs()


def cg_applies(mutation, case):
    return {"second_trip_skipped": case.B * case.T > 1024, "accumulate_ignored": bool(case.acc), "division_dropped": True,
            "sample_index_from_ld": case.ld > case.T and case.B > 1}[mutation]


def reduction_limit(chain, dtype, is_kernel=True):
    """A randn reduction against float64, relative to sum|terms|: fp32 chain 2^-24; 16-bit: one rounding of that (in eps)."""
    if dtype == F32:
        return chain * U32
    return (TOL if is_kernel else CEILING) + chain * U32 / EPS[dtype]
