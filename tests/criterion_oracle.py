"""A plain-torch oracle for the criterion kernels (csrc/loss_optim.hip): no GPU needed, no dependency on the kernels.

Three kernel families -- cross entropy (ce_*: the two-kernel route ce_fwd / ce_bwd and the fused one-pass ce_fwd_grad), label-smoothed
cross entropy (lsce_*) and the fp32 softmax / log-softmax of get_normalized_probs (probs_*) -- each with
  *_reference()  float64 on the stored (16-bit-rounded) inputs, restated from the formulas in the kernel comments, together with the
                 componentwise magnitude bound of every gradient: the same expression with every term replaced by its absolute value.
                 Where the bound is 0 (padding columns V..ld, ignored rows, disallowed columns, row_w = 0) the kernel must write exactly 0.
  *_emulate()    the same arithmetic in float32 with the kernels' roundings and nothing else of the kernels (fused: exp2(x log2e - m log2e)
                 with a max-then-rescale sum; two-kernel: exp(x - lse); one rounding to the output type), able to apply one named mutation.
excess()         max (|got - ref| - floor) / bound in units of the 16-bit eps; inf for a non-finite value or a non-zero where bound == 0.
make_case() / build_*() / CASES   the inputs, from a CPU generator, in two regimes: `randn3` (3 * randn) and `planted` (unit-variance
                 rows with a logit of 12 at a seam column, so that a column the kernel forgets to sum carries the row).
tests/test_criterion_oracle_cpu.py proves the table sound; tests/test_criterion_edges_gpu.py runs it against the kernels.

Conventions: x is a [rows, V] view whose row stride is the leading dimension ld the kernels are given; the gradients are [rows, ld].
The padding columns V..ld of the storage hold PAD_FILL, a logit that would dominate every row if a kernel read it into a sum.
The logits are finite (no caller produces -inf rows: ops.py masks by range and byte mask inside the label-smoothed kernels).
"""
from collections import namedtuple

import torch

L2E = 1.4426950408889634
L2E32 = float(torch.tensor(L2E, dtype=torch.float32))
FLT_MIN = 2.0 ** -126
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
NVEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}          # elements of a 16-byte vector
IGNORE = 1                                                              # ignore_index = the pad token, a valid column
PAD_FILL = 30.0
PLANT = 12.0

# ---------------------------------------------------------------------------------------------------------------- measured constants
# CEILING: the cap on excess(emulate, reference, bound) over the whole table (every route, both regimes, bf16 and fp16).  The emulation
# rounds ONCE on the way to a 16-bit gradient: one rounding to nearest costs at most u = EPS relative to the value, the value is at most the
# bound, and the float32 work before it is ~1e-6 relative to the bound, 2.6e-4 u in bf16 and 2e-3 u in fp16.
# Measured 2026-10-19 (tests/test_criterion_oracle_cpu.py prints the figures with -s), worst excess:
#          ce two-kernel   ce fused   lsce     probs bwd
#   bf16   0.994           0.996      0.992    0.991
#   fp16   0.961           0.968      0.956    0.989
CEILING = 1.0
# TOL for the kernels = 2 * CEILING: the factor 2 covers what the emulation leaves out -- the hardware exp2, the 1024-wide reduction order,
# lse rounded once more.  Never set from what a kernel produced.
TOL = 2.0 * CEILING
# fp32 outputs: 8 x the largest error of the emulation's float32 evaluation against float64 over the table (8: exp / log ulps and the
# summation order, the attention oracle's convention).  lse, row_loss, row_nll and the probs forward are absolute; the fp32 gradients (fp32
# logits through the two-kernel, label-smoothed and probs routes) are relative to their magnitude bound.  Measured 2026-10-19:
#   lse 1.29e-6   row_loss 1.36e-6 (cross entropy)   row_loss / row_nll 1.77e-6 (label-smoothed)
#   probs forward: log 1.52e-6, prob 6.81e-7      fp32 gradients, error / bound: 1.55e-6
LSE_TOL = 8 * 1.3e-6
ROW_TOL = 8 * 1.4e-6
LSROW_TOL = 8 * 1.8e-6
PROBS_TOL = {True: 8 * 1.6e-6, False: 8 * 6.9e-7}                       # keyed by log_probs
G32_TOL = 8 * 1.6e-6
# The kernels themselves on an MI355X, 2026-10-19, worst over the same table (tests/test_criterion_edges_gpu.py prints them with -s):
#   16-bit gradients, excess in eps against TOL = 2.0:   ce two-kernel   ce fused   lsce     probs bwd
#                                                 bf16   0.994           0.996      0.992    0.991
#                                                 fp16   0.961           0.968      0.956    0.989
#   (the kernels sit on the emulation's figures: one rounding of the result; through ops.label_smoothed_cross_entropy with drop_worst 0.85)
#   fp32 gradients, error / bound against G32_TOL = 1.28e-5: two-kernel 1.56e-6, lsce 1.61e-6, probs 2.9e-7
#   fp32 outputs as a share of their tolerance: fused lse 0.34, row_loss 0.27; two-kernel lse 0.07, row_loss 0.09; lsce lse 0.07,
#   row_loss 0.13, row_nll 0.08; probs log 0.12, prob 0.15.  No kernel fault was found: csrc/loss_optim.hip is unchanged.


def excess(got, ref, bound, eps, floor=0.0):
    """max over elements with bound > 0 of (|got - ref| - floor) / bound, in units of eps; where bound == 0 got must be exactly 0
    (returns inf otherwise, and for any non-finite got)."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    zero = bound <= 0
    if bool((got[zero] != 0).any()):
        return float("inf")
    live = ~zero
    if not bool(live.any()):
        return 0.0
    err = ((got - ref).abs() - floor).clamp_min(0)
    return float((err[live] / bound[live]).max()) / eps


def floor_of(dtype, g):
    """The absolute error an underflow may cost: one smallest subnormal of fp16; FLT_MIN * max(1, |g|) for bf16 and fp32 (the fused
    kernel's v_exp_f32 does not return fp32 subnormals, so a probability below FLT_MIN is lost before it meets g)."""
    return 2.0 ** -24 if dtype == torch.float16 else FLT_MIN * max(1.0, abs(g))


def _storage(x):
    """The [rows, ld] storage behind the [rows, V] view x (ld = its row stride)."""
    return torch.as_strided(x, (x.shape[0], x.stride(0)), (x.stride(0), 1), x.storage_offset())


def _ld(x):
    return x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])


def _onehot(t, R, V, dt, dev, live=None):
    oh = torch.zeros(R, V, dtype=dt, device=dev)
    oh[torch.arange(R, device=dev), t] = 1
    return oh if live is None else oh * live[:, None].to(dt)


def _widen(d, ld):
    out = torch.zeros(d.shape[0], ld, dtype=d.dtype, device=d.device)
    out[:, :d.shape[1]] = d
    return out


def _fma(a, b, c):
    """fmaf(a, b, c) for float32 tensors a, c and a float32-valued Python scalar b: the product of two float32 is exact in float64."""
    return (a.double() * b + c.double()).float()


# ---------------------------------------------------------------------------------------------------------------- cross entropy
def ce_reference(x, t, g, ignore=IGNORE):
    """-> (ref, bound): ref = dict(lse, row_loss [rows], d [rows, ld]) in float64; bound: the magnitude bound of d, (p + onehot) |g|."""
    dt = torch.float64
    R, V = x.shape
    ld = _ld(x)
    xv = x.to(dt)
    lse = torch.logsumexp(xv, 1)
    p = torch.exp(xv - lse[:, None])
    live = t != ignore
    oh = _onehot(t, R, V, dt, x.device)
    lv = live[:, None].to(dt)
    row_loss = torch.where(live, lse - xv.gather(1, t[:, None])[:, 0], torch.zeros_like(lse))
    return dict(lse=lse, row_loss=row_loss, d=_widen((p - oh) * g * lv, ld)), _widen((p + oh) * abs(g) * lv, ld)


CE_MUTATIONS = ("drop_last_col", "drop_tail_vector", "drop_slab", "onehot_shift", "onehot_unscaled", "pad_written", "ignored_live",
                "lse_off")


def _kept(V, N, mutation, dev):
    keep = torch.ones(V, dtype=torch.bool, device=dev)
    if mutation == "drop_last_col":
        keep[V - 1] = False
    elif mutation == "drop_tail_vector":
        keep[V // N * N:] = False
    elif mutation == "drop_slab":                   # the fused kernel's second register slab: vector index >= 1024
        keep[8192:] = False
    elif mutation == "drop_trip":                   # the second trip of a 256-thread scalar loop
        keep[256:] = False
    return keep


def _lse32(xs, fused):
    """float32 logsumexp of the rows of xs (-inf: a column left out), max first, then one rescaled sum."""
    m = xs.amax(1, keepdim=True)
    if fused:
        s = torch.exp2(_fma(xs, L2E32, -m * L2E32)).sum(1, keepdim=True)
    else:
        s = torch.exp(xs - m).sum(1, keepdim=True)
    return (m + torch.log(s))[:, 0]


def ce_emulate(x, t, g, dtype, fused, mutation=None, ignore=IGNORE):
    """float32 with the kernels' roundings -> dict(lse, row_loss fp32 [rows], d [rows, ld] of dtype)."""
    assert mutation is None or mutation in CE_MUTATIONS, mutation
    ft = torch.float32
    R, V = x.shape
    ld = _ld(x)
    xv = x.to(ft)
    xs = xv.masked_fill(~_kept(V, NVEC[dtype], mutation, x.device), float("-inf"))
    lse = _lse32(xs, fused)
    if mutation == "lse_off":
        lse = lse.clone()
        lse[0] += 1e-2
    if fused:
        p = torch.exp2(_fma(xv, L2E32, -lse[:, None] * L2E32))
    else:
        p = torch.exp(xv - lse[:, None])
    live = t != ignore
    if mutation == "ignored_live":
        live = torch.ones_like(live)
    oh = _onehot((t + 1) % V if mutation == "onehot_shift" else t, R, V, ft, x.device)
    g32 = torch.tensor(g, dtype=ft, device=x.device)
    d = (p * g32 - oh) if mutation == "onehot_unscaled" else (p - oh) * g32
    d = _widen(d * live[:, None].to(ft), ld)
    if mutation == "pad_written" and ld > V:
        pad = _storage(x)[:, V].to(ft)
        d[:, V] = (torch.exp(pad - lse) * g32).clamp_max(1e4)
    row_loss = torch.where(t != ignore, lse - xv.gather(1, t[:, None])[:, 0], torch.zeros_like(lse))
    return dict(lse=lse, row_loss=row_loss, d=d.to(dtype))


# ---------------------------------------------------------------------------------------------------------------- label smoothing
def ls_allowed(R, V, crange, cmask, dev, inclusive_end=False):
    """bool [R, V]: the whole vocabulary, or [0, 4) U [cstart, cend), intersected with the byte mask."""
    A = torch.ones(R, V, dtype=torch.bool, device=dev)
    if crange is not None:
        c = torch.arange(V, device=dev)
        hi = (c <= crange[1]) if inclusive_end else (c < crange[1])
        A = A & ((c < 4) | ((c >= crange[0]) & hi))[None, :]
    if cmask is not None:
        A = A & cmask.to(dev).bool()
    return A


def lsce_reference(x, t, g, eps, crange=None, cmask=None, row_w=None, ignore=IGNORE):
    """-> (ref, bound): ref = dict(lse, row_loss, row_nll, row_cnt [rows], d [rows, ld]) in float64.
    C = count of allowed columns; eps_i = eps / (C - 1) without constraints, eps / (C - 1 + 1e-6) with them;
    loss = (1 - eps - eps_i) nll + eps_i (C lse - sum x);  d = ((1 - eps - eps_i)(p - onehot) + eps_i (C p - 1)) g row_w on allowed columns."""
    dt = torch.float64
    R, V = x.shape
    ld = _ld(x)
    A = ls_allowed(R, V, crange, cmask, x.device)
    Af = A.to(dt)
    xv = x.to(dt)
    lse = torch.logsumexp(xv.masked_fill(~A, float("-inf")), 1)
    p = torch.exp(xv - lse[:, None]) * Af
    C = Af.sum(1)
    constrained = crange is not None or cmask is not None
    eps_i = eps / (C - 1 + (1e-6 if constrained else 0.0))
    w_nll = 1 - eps - eps_i
    live = t != ignore
    lv = live.to(dt)
    nll = (lse - xv.gather(1, t[:, None])[:, 0]) * lv
    loss = (w_nll * nll + eps_i * (C * lse - (xv * Af).sum(1))) * lv
    oh = _onehot(t, R, V, dt, x.device)
    w = lv * g if row_w is None else lv * g * row_w.to(dt)
    d = (w_nll[:, None] * (p - oh) + eps_i[:, None] * (C[:, None] * p - 1)) * Af * w[:, None]
    bd = (w_nll.abs()[:, None] * (p + oh) + eps_i[:, None] * (C[:, None] * p + 1)) * Af * w.abs()[:, None]
    return dict(lse=lse, row_loss=loss, row_nll=nll, row_cnt=C, d=_widen(d, ld)), _widen(bd, ld)


LSCE_MUTATIONS = ("count_off", "range_edge", "drop_last_col", "drop_trip", "onehot_shift", "pad_written", "ignored_live", "lse_off",
                  "row_w_dropped")


def lsce_emulate(x, t, g, eps, dtype, crange=None, cmask=None, row_w=None, mutation=None, ignore=IGNORE):
    assert mutation is None or mutation in LSCE_MUTATIONS, mutation
    ft = torch.float32
    R, V = x.shape
    ld = _ld(x)
    A = ls_allowed(R, V, crange, cmask, x.device, inclusive_end=mutation == "range_edge")
    Af = A.to(ft)
    xv = x.to(ft)
    summed = A & _kept(V, 1, mutation, x.device)[None, :]
    lse = _lse32(xv.masked_fill(~summed, float("-inf")), False)
    if mutation == "lse_off":
        lse = lse.clone()
        lse[0] += 1e-2
    C = Af.sum(1) + (1.0 if mutation == "count_off" else 0.0)
    constrained = crange is not None or cmask is not None
    eps32 = torch.tensor(eps, dtype=ft, device=x.device)
    eps_i = eps32 / ((C - 1.0 + 1e-6) if constrained else (C - 1.0))
    w_nll = 1.0 - eps32 - eps_i
    live = t != ignore
    lv = live.to(ft)
    nll = (lse - xv.gather(1, t[:, None])[:, 0]) * lv
    loss = (w_nll * nll + eps_i * (C * lse - (xv * Af).sum(1))) * lv
    p = torch.exp(xv - lse[:, None])
    oh = _onehot((t + 1) % V if mutation == "onehot_shift" else t, R, V, ft, x.device)
    w = torch.full((R,), g, dtype=ft, device=x.device)
    if row_w is not None and mutation != "row_w_dropped":
        w = w * row_w.to(ft)
    if mutation != "ignored_live":
        w = w * lv
    d = _widen((w_nll[:, None] * (p - oh) + eps_i[:, None] * (C[:, None] * p - 1.0)) * w[:, None] * Af, ld)
    if mutation == "pad_written" and ld > V:
        d[:, V] = w
    return dict(lse=lse, row_loss=loss, row_nll=nll, row_cnt=C, d=d.to(dtype))


# ---------------------------------------------------------------------------------------------------------------- probs
def probs_reference(x, log_probs):
    """float64 log-softmax / softmax of the rows of x -> [rows, V]."""
    y = torch.log_softmax(x.double(), 1)
    return y if log_probs else torch.exp(y)


def probs_bwd_reference(dy, y, ld, log_probs):
    """The backward of the STORED y (the kernel is handed the forward's fp32 result) -> (d [rows, ld], bound) in float64.
    log: d = dy - exp(y) sum(dy), bound |dy| + p sum|dy|;   prob: d = y (dy - sum(dy y)), bound y (|dy| + sum|dy y|)."""
    dy, y = dy.double(), y.double()
    if log_probs:
        p = torch.exp(y)
        d = dy - p * dy.sum(1, keepdim=True)
        bd = dy.abs() + p * dy.abs().sum(1, keepdim=True)
    else:
        d = y * (dy - (dy * y).sum(1, keepdim=True))
        bd = y * (dy.abs() + (dy * y).abs().sum(1, keepdim=True))
    return _widen(d, ld), _widen(bd, ld)


PROBS_MUTATIONS = ("drop_last_col", "drop_trip", "pad_written")


def probs_emulate(x, log_probs, mutation=None):
    assert mutation is None or mutation in PROBS_MUTATIONS, mutation
    xv = x.float()
    lse = _lse32(xv.masked_fill(~_kept(x.shape[1], 1, mutation, x.device), float("-inf")), False)
    tt = xv - lse[:, None]
    return tt if log_probs else torch.exp(tt)


def probs_bwd_emulate(dy, y, ld, log_probs, dtype, mutation=None):
    assert mutation is None or mutation in PROBS_MUTATIONS, mutation
    dy, y = dy.float(), y.float()
    keep = _kept(y.shape[1], 1, mutation, y.device).float()[None, :]
    if log_probs:
        d = dy - torch.exp(y) * (dy * keep).sum(1, keepdim=True)
    else:
        d = y * (dy - (dy * y * keep).sum(1, keepdim=True))
    d = _widen(d, ld)
    if mutation == "pad_written" and ld > y.shape[1]:
        d[:, y.shape[1]] = dy[:, 0]
    return d.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- inputs
REGIMES = ("randn3", "planted")


def make_case(regime, R, V, ld, cols, seed):
    """-> float32 storage [R, ld] from a CPU generator: columns < V hold 3 * randn (`randn3`) or randn with PLANT + randn / 8 in row r at
    every column of cols[r] (`planted`); the padding columns hold PAD_FILL."""
    assert regime in REGIMES, regime
    g = torch.Generator(device="cpu").manual_seed(seed)
    store = torch.full((R, ld), PAD_FILL)
    x = torch.randn(R, V, generator=g)
    if regime == "randn3":
        x = x * 3
    else:
        for r in range(R):
            for c in cols[r]:
                x[r, c] = PLANT + 0.125 * x[r, c]       # (narrow, so that two planted columns of one row share it about evenly)
    store[:, :V] = x
    return store


def _spread(cols, R, ignored):
    """Seam columns dealt round-robin over the live rows of R -> per-row lists (the ignored row gets the first column too)."""
    live = [r for r in range(R) if r != ignored]
    per = [[] for _ in range(R)]
    for i, c in enumerate(cols):
        per[live[i % len(live)]].append(c)
    for r in live:
        if not per[r]:
            per[r].append(cols[r % len(cols)])
    per[ignored] = [cols[0]]
    return per


# ---- cross entropy
CECase = namedtuple("CECase", "fused regime V ld g seed rot")        # rot: which of a row's seam columns carries its target
TWO_SHAPES = ((3, 8), (8, 8), (1021, 1024), (2048, 2048), (2053, 2056), (2053, 2072),
              (2061, 2064))      # (the last: ce_fwd_kernel's own second trip of 16-bit vectors, V // 8 = 257, with a 5-wide tail)
FUSED_LD = (8, 8192, 8200, 16384, 16392, 32768, 32776, 57344, 57352, 65536)          # both sides of every NV boundary
WIDE = (8189, 8192 + 64)                                                             # a view of wider storage: row stride ld + 64
GS = (1.0, 0.37)
LOSS_SCALE = 128.0
MAX_ROWS = 8


def nv_of(ld):
    """The register-slab count ce_fwd_grad_launch picks: vectors of 8 per thread, 1024 threads."""
    per = (ld // 8 + 1023) // 1024
    return next(nv for nv in (1, 2, 4, 7, 8) if per <= nv)


def ce_seams(V, N, fused):
    """The planted / target columns: row ends, the last full vector's edge, and the trip (two-kernel) or slab and wave (fused) seams."""
    cols = [0, V - 1, V // N * N - 1, V // N * N]
    if fused:
        for k in range(1, (V + 8191) // 8192):
            cols += [8192 * k - 1, 8192 * k]
        cols += [512 * 3 - 1, 512 * 3]              # a wave seam inside a slab: 64 lanes x 8 columns
    else:
        cols += [2047, 2048]
    seen = []
    for c in cols:
        if 0 <= c < V and c != IGNORE and c not in seen:
            seen.append(c)
    return seen


def _ce_cases():
    two, fused, i = [], [], 0
    for V, ld in TWO_SHAPES:
        for regime in REGIMES:
            for g in GS:
                two.append(CECase(False, regime, V, ld, g, 100 + i, 0))
                i += 1
    two.append(CECase(False, "planted", 2053, 2056, LOSS_SCALE, 100 + i, 0))
    for j, ld in enumerate(FUSED_LD):
        for k, V in enumerate((ld, ld - 3, ld - 11)):
            if V <= 0:
                continue
            # (the three cases of V = ld - 3 share one layout and take rot 1, 2, 0: between them every seam column carries a target;
            #  V = ld and V = ld - 11 take rot 0, where the columns that depend on V sit)
            fused.append(CECase(True, "planted", V, ld, GS[(j + k) % 2], 200 + 10 * j + k, k % 2))
        fused.append(CECase(True, "randn3", ld - 3, ld, GS[j % 2], 200 + 10 * j + 5, 2))
        fused.append(CECase(True, "planted", ld - 3, ld, LOSS_SCALE, 200 + 10 * j + 6, 0))
    fused.append(CECase(True, "planted", WIDE[0], WIDE[1], 0.37, 390, 0))
    fused.append(CECase(True, "randn3", WIDE[0], WIDE[1], 1.0, 391, 0))
    return two, fused


CE_TWO_CASES, CE_FUSED_CASES = _ce_cases()
CE_DTYPES = {False: (torch.float32, torch.bfloat16, torch.float16), True: (torch.bfloat16, torch.float16)}


def ce_layout(case, dtype):
    """-> (R, ignored row, per-row seam columns, targets list): at most MAX_ROWS rows, one of them ignored; the seam columns are dealt
    round-robin over the live rows and the target of a live row is its seam column number case.rot (modulo how many it has)."""
    cols = ce_seams(case.V, NVEC[dtype], case.fused)
    R = min(len(cols), MAX_ROWS - 1) + 1
    ignored = R // 2
    per = _spread(cols, R, ignored)
    t = [IGNORE if r == ignored else per[r][case.rot % len(per[r])] for r in range(R)]
    return R, ignored, per, t


def build_ce(case, dtype, device="cpu"):
    """-> dict(x [R, V] view of the [R, ld] storage of dtype, t int64 [R], g float, cols per row, ignored)."""
    R, ignored, per, t = ce_layout(case, dtype)
    store = make_case(case.regime, R, case.V, case.ld, per, case.seed).to(dtype).to(device)
    return dict(x=store[:, :case.V], t=torch.tensor(t, dtype=torch.int64, device=device), g=case.g, cols=per, ignored=ignored)


# ---- label smoothing
LSCase = namedtuple("LSCase", "regime V pad eps variant crange g seed")       # variant: none | range | mask | both
LS_V = (5, 255, 256, 257, 513, 1030)
LS_ROWS, LS_IGNORED = 6, 2
LS_ROW_W = (1.0, 0.0, 1.0, 1.0, 0.5, 1.0)
LS_SPECIAL = lambda V: [c for c in (0, 255, 256, V - 1) if c < V]             # noqa: E731  (mask: allowed in one row, disallowed in another)


def _ls_ranges(V):
    return [r for r in ((4, V), (7, V - 2), (255, 257)) if r[0] >= 4 and r[1] > r[0] and r[1] <= V]


def _ls_cases():
    out, i = [], 0
    for V in LS_V:
        variants = [("none", None)] + [("range", r) for r in _ls_ranges(V)] + [("mask", None)] + [("both", r) for r in _ls_ranges(V)[-1:]]
        for vi, (variant, crange) in enumerate(variants):
            for ei, eps in enumerate((0.0, 0.1)):        # (the regime walks with V and the variant, not with eps: both regimes meet both eps)
                out.append(LSCase(REGIMES[(LS_V.index(V) + vi) % 2], V, 0, eps, variant, crange, GS[(vi + ei) % 2], 500 + i))
                i += 1
    out.append(LSCase("planted", 256, 24, 0.1, "both", (7, 254), 0.37, 500 + i))
    out.append(LSCase("randn3", 256, 24, 0.1, "none", None, 1.0, 501 + i))
    return out


LS_CASES = _ls_cases()
DTYPES3 = (torch.float32, torch.bfloat16, torch.float16)


LS_GRADED = tuple(r for r in range(LS_ROWS) if r != LS_IGNORED and LS_ROW_W[r] > 0)      # the rows whose gradient is checked


def ls_seams(case):
    """The planted / target columns: the range edges cstart and cend - 1, the row ends, the trip seam, the edge of [0, 4) -- those the
    range allows."""
    V = case.V
    seams = []
    if case.crange is not None:
        seams += [case.crange[0], case.crange[1] - 1]
    seams += [0, V - 1, 255, 256, 3, 4]
    ok = []
    for c in seams:
        inside = case.crange is None or c < 4 or case.crange[0] <= c < case.crange[1]
        if 0 <= c < V and c != IGNORE and inside and c not in ok:
            ok.append(c)
    return ok


def ls_layout(case):
    """-> (targets, own, foreign): own[r]: the seam columns dealt round-robin over the graded rows (live, row_w > 0), planted in row r and
    allowed there whatever the byte mask draws; the target of a graded row is the first of them, so the targets walk cstart, cend - 1, ...
    foreign[r] (masked variants): each of LS_SPECIAL's columns is planted once more in another graded row, where the mask DISALLOWS it --
    a dominant logit the kernel must not see: the mask decides, not the size."""
    ok = ls_seams(case)
    own = [[] for _ in range(LS_ROWS)]
    for i, c in enumerate(ok):
        own[LS_GRADED[i % len(LS_GRADED)]].append(c)
    for r in range(LS_ROWS):
        if not own[r]:
            own[r].append(ok[(r + 3) % len(ok)])
    t = [IGNORE if r == LS_IGNORED else own[r][0] for r in range(LS_ROWS)]
    foreign = [[] for _ in range(LS_ROWS)]
    if case.variant in ("mask", "both"):
        for c in LS_SPECIAL(case.V):
            if c not in ok:
                continue
            home = next(r for r in LS_GRADED if c in own[r])
            order = LS_GRADED[LS_GRADED.index(home) + 1:] + LS_GRADED[:LS_GRADED.index(home)]
            other = next((r for r in order if c not in own[r]), None)
            if other is not None:
                foreign[other].append(c)
    return t, own, foreign


def build_ls(case, dtype, device="cpu"):
    """-> dict(x, t, g, eps, crange, cmask (uint8 [R, V] or None), row_w fp32 [R], own, foreign)."""
    V = case.V
    ld = (V + NVEC[dtype] - 1) // NVEC[dtype] * NVEC[dtype] + case.pad
    t, own, foreign = ls_layout(case)
    store = make_case(case.regime, LS_ROWS, V, ld, [own[r] + foreign[r] for r in range(LS_ROWS)], case.seed).to(dtype).to(device)
    cmask = None
    if case.variant in ("mask", "both"):
        gen = torch.Generator(device="cpu").manual_seed(case.seed + 1)
        cmask = torch.rand(LS_ROWS, V, generator=gen) < 0.7
        for c in LS_SPECIAL(V):                  # (allowed in one row and disallowed in another even where no row plants the column)
            cmask[0::2, c] = True
            cmask[1::2, c] = False
        for r in range(LS_ROWS):
            cmask[r, own[r]] = True
            cmask[r, foreign[r]] = False
            cmask[r, t[r]] = True
        cmask = cmask.to(torch.uint8).to(device)
    return dict(x=store[:, :V], t=torch.tensor(t, dtype=torch.int64, device=device), g=case.g, eps=case.eps, crange=case.crange,
                cmask=cmask, row_w=torch.tensor(LS_ROW_W, dtype=torch.float32, device=device), own=own, foreign=foreign)


# ---- probs
PCase = namedtuple("PCase", "regime V pad log_probs seed")
P_V = (1, 255, 256, 257, 1030)
P_ROWS = 5
PLANT_DY = 64.0
P_CASES = [PCase(regime, V, pad, lp, 800 + 16 * i + 4 * j + 2 * k + l) for i, V in enumerate(P_V) for j, pad in enumerate((0, 8))
           for k, lp in enumerate((True, False)) for l, regime in enumerate(REGIMES)]


def p_seams(V):
    return [c for i, c in enumerate((0, 255, 256, V - 1)) if c < V and c not in (0, 255, 256, V - 1)[:i]]


def build_probs(case, dtype, device="cpu"):
    """-> dict(x [R, V] view of [R, V + pad] storage, dy fp32 [R, V], cols): planted rows carry +PLANT in x and +PLANT_DY in dy at the
    row's seam column, so that a column the backward forgets to sum carries that sum."""
    V = case.V
    seams = p_seams(V)
    cols = [[seams[r % len(seams)]] for r in range(P_ROWS)]
    store = make_case(case.regime, P_ROWS, V, V + case.pad, cols, case.seed).to(dtype).to(device)
    gen = torch.Generator(device="cpu").manual_seed(case.seed + 1)
    dy = torch.randn(P_ROWS, V, generator=gen)
    if case.regime == "planted":
        for r in range(P_ROWS):
            dy[r, cols[r][0]] += PLANT_DY
    return dict(x=store[:, :V], dy=dy.to(device), cols=cols)


def bwd_ld(V):
    """The leading dimension kernels.probs_bwd gives its result."""
    return (V + 7) // 8 * 8
