"""A plain-torch oracle for the convolution-stack kernels (csrc/conv.hip): no GPU needed, no dependency on the kernels.

Exact families -- compared bit for bit (same_bits: integer views; a NaN matches any NaN, because a float round trip may quieten it):
  im2col_reference(x, geom, nchw)   plain indexing in the order stated at the head of the im2col kernels: col[(b, oh, ow)][(kh KW + kw) C + c]
                                    = x[b, oh s - p + kh, ow s - p + kw, c], +0 outside the image and in the columns K .. Kpad - 1
                                    (Kpad = K rounded up to 8).  Inputs are random FINITE BIT PATTERNS of the dtype (subnormals and
                                    -0 included), so a misplaced element cannot coincide with its neighbour.
  col2im_reference / maxpool_bwd_reference   inputs are small integers: |v| <= 4 and at most 49 taps (7 x 7) meet in one sum, so every
                                    partial sum is an integer of magnitude <= 196 < 256 = 2^8 -- exact in fp32 in any order, and
                                    representable in bf16 (8 significant bits), fp16 and fp32: the stored result is exact whatever the
                                    order of the additions.  A position no window covers is exactly +0.
  maxpool_reference(x, geom)        an explicit loop over the taps in (kh, kw) order with the kernel's rule `t > best or isnan(t)`: the
                                    first maximum wins, the last NaN wins the index; arg is the tap number kh K + kw (0 for a window of
                                    nothing but -inf).
  relu_reference(x, gate)           x > 0 ? x : (isnan(x) ? x : +0) -- torch.relu's values, NaN propagating; -0.0 and every negative
                                    give +0 (torch's CPU kernel keeps the sign of -0.0, which compares equal), subnormals pass.
                                    gate: x where gate > 0 (false for a NaN, a zero or a negative gate), else +0.

BatchNorm family -- as tests/rownorm_oracle.py does it for the row kernels:
  bn_reference(c, own)  float64 on the stored inputs -> (ref, bound) over y, mean, rstd, running_mean, running_var, dx, dres, dgamma,
                        dbeta and the fp32 `sums`; bound = the same expression with absolute values (x - mean as _xha).  rows == 1:
                        the unbiased variance is the variance itself (the kernel's documented rule).  The backward is staged: it
                        uses the kernel's OWN mean and rstd and (gate read from y) its OWN y, so one stage's rounding is not charged
                        to the next.
  bn_emulate(c, dtype, mutation)   the same arithmetic with the kernels' rounding points -- fp64 column sums, fp32 statistics, fp32
                        apply, one rounding of each stored output -- able to apply one of MUTATIONS.
The recomputed ReLU gate [(x - mean) rstd gamma + beta > 0] (ofa_batchnorm_bwd with beta): an element is gate-ambiguous when
|t| < GATE_MARGIN * gate_bound(t); build_bn moves such elements of x by +0.5 until NONE is left, so the oracle's gate is the kernel's and
every element of dx, the sums and the parameter gradients is compared.

Three modes share one case type: "bn" (ofa_batchnorm_fwd / _bwd), "groups" (ofa_batchnorm_fwd_apply behind G synthetic fp64 partial
rows; one column's partials say variance -eps / 2, as rounded GEMM-epilogue statistics of a constant column can: the clamp is part of
the contract) and "sync" (the SyncBatchNorm entry points in one process: the statistics of rows A + B, the outputs of A).

Regimes: `randn`; `offset` (100 + randn: a one-pass variance in fp32 would lose its digits, fp64 must hold them); `const` (column C / 2
is 0.75: variance 0, rstd = 1 / sqrt(eps)); `prow` (x and dy carry +64 in the LAST row: the one-row tail of the statistics' pair loop).

tests/test_conv_oracle_cpu.py proves the tables sound and confirms every claimed route against the library's host-only entry points
(ofa_batchnorm_route, ofa_im2col_route); tests/test_conv_edges_gpu.py runs the tables against the kernels through tests/conv_gpu.py.
"""
from collections import namedtuple

import torch

from tests.rownorm_oracle import (BF16, DTYPES3, EPS, F32, F64, FP16, NAMES, NVEC, cdiv, excess, floor_of, grad_excess,  # noqa: F401
                                  scalar_err)

PLANT = 64.0
CONST = 0.75
REGIMES = ("randn", "offset", "const", "prow")
KAPPA = {dt: 2.0 ** -22 / e for dt, e in EPS.items()}                  # a float32 rounding in units of the 16-bit eps

# ---------------------------------------------------------------------------------------------------------------- measured constants
# CEILING: the cap on excess(emulate, reference, bound) over the BatchNorm tables (bf16 and fp16).  The emulation rounds an output
# once: at most one eps relative to the value, the value is at most the bound.
# Measured 2026-10-21 (tests/test_conv_oracle_cpu.py prints the figures with -s), the emulation's worst excess:
#          y       dx      dres   dgamma   dbeta
#   bf16   0.996   0.996   0      0.978    0.988
#   fp16   0.998   0.995   0      0.991    0.985
CEILING = 1.0
# TOL for the kernels = 2 * CEILING: the factor 2 covers what the emulation leaves out -- the order of the fp64 column sums, fused
# multiply-adds in the apply and dx expressions, v_rcp / v_rsq sequences.  Never set from what a kernel produced.
TOL = 2.0 * CEILING
# fp32 tensors (fp32 inputs): 8 x the emulation's worst error / bound.  The statistics are fp32 for every dtype: mean and the running
# buffers as |error| / their magnitude bound, rstd relative, `sums` as error / bound: 8 x the emulation's worst, one figure per output.
# Measured 2026-10-21, the emulation's worst over the tables and the three dtypes:
#   fp32 tensors, error / bound: y 2.57e-7 (32897 x 128), dx 1.32e-7, dgamma 1.54e-7, dbeta 1.03e-7; dres exact (the gated dy itself)
#   statistics: mean 4.67e-8, rstd 1.05e-7 (eval mode: 1 / sqrtf in fp32), running_mean 5.93e-8, running_var 5.93e-8, sums 1.49e-7
# Rounded up by 3 ... 10 %: the order of torch's fp64 column sums depends on the host's thread count and moves a figure in its third
# digit (a second host: dgamma 1.55e-7, sums 1.46e-7).  mean and the running buffers are one rounding of a float64 value to fp32:
# at most 2^-24 = 5.96e-8 of the value on any host.
G32 = {"y": 8 * 2.8e-7, "dx": 8 * 1.4e-7, "dres": 0.0, "dgamma": 8 * 1.6e-7, "dbeta": 8 * 1.1e-7}
S32 = {"mean": 8 * 6.0e-8, "rstd": 8 * 1.1e-7, "running_mean": 8 * 6.0e-8, "running_var": 8 * 6.0e-8, "sums": 8 * 1.6e-7}
# The recomputed gate: |t| < GATE_MARGIN * gate_bound(t) is ambiguous.  The emulation's fp32 t against float64 over the tables differs
# by at most 1.67e-7 of gate_bound (measured 2026-10-21): 2^-12 = 2.4e-4 is more than 100 x that.
GATE_MARGIN = 2.0 ** -12
# The kernels themselves on an MI355X, worst over the same tables (tests/test_conv_edges_gpu.py prints them with -s), for the record:
#   2026-10-21, 16-bit tensors, excess in eps against TOL = 2.0:   bf16  y 0.996  dx 0.996  dres 0  dgamma 0.978  dbeta 0.988
#                                                                   fp16  y 0.998  dx 0.995  dres 0  dgamma 0.991  dbeta 0.985
#   fp32 tensors, error / bound, of 8 x the emulation's figure above: y 2.12e-7, dx 1.32e-7, dgamma 1.54e-7, dbeta 1.03e-7, dres 0
#   statistics: mean 4.67e-8, rstd 1.05e-7, running_mean 5.93e-8, running_var 5.93e-8, sums 1.49e-7 -- the emulation's own figures: the
#   kernels round where it does.  im2col, col2im, both pools and relu: bit for bit on every case, subnormal bit patterns included.
# One finding, by `bn nan m2 rows11 ... eval relu1` / `... train relu1 res1` (y_nan) and every relu case (the NaN among the specials):
# bn_apply_kernel and relu_kernel took fmaxf(t, 0), which is 0 for a NaN where torch.relu propagates it -- under the fp16 loss scaler a
# NaN activation would have vanished instead of tripping the overflow check.  Both now keep a NaN (t > 0 ? t : (t != t ? t : 0)); the
# backward gates (y > 0, and the recomputed one) are unchanged.  A second one by reading: ofa_conv_out_size divided a negative
# in + 2 pad - k with C's truncation (k 2 / s 2 on one row: (1 - 2) / 2 + 1 = 1 position where the callers' buffers hold none);
# it now returns 0 there, and col2im and both pools refuse an empty output as im2col did.


def limit(name, dtype, kernel=True):
    """The largest figure output `name` may show: the emulation's cap, or (kernel=True) what the GPU test allows a kernel."""
    if name in ("y_nan",):
        return 0.0
    if name in S32:
        v = S32[name]
    elif dtype == F32:
        v = G32[name]
    else:
        return TOL if kernel else CEILING
    return v if kernel else v / 8


# ---------------------------------------------------------------------------------------------------------------- routes, restated
def grid_1d(work):
    """Blocks of 256 threads of every grid-stride kernel: capped at 4096 -- beyond 4096 * 256 work items a thread takes a second trip."""
    return min(4096, max(1, cdiv(work, 256)))


SWEEP = 4096 * 256


def bn_cw_log2(m):
    """log2 of the column vectors per statistics block: 32, or the largest power of two within the layer's m vectors."""
    l2 = 5
    while l2 > 0 and (1 << l2) > m:
        l2 -= 1
    return l2


def bn_groups(rows):
    return min(256, max(1, cdiv(rows, 128)))


def bn_route(rows, m):
    """-> (groups, cw_log2, apply_blocks), what ofa_batchnorm_route reports for [rows, m vectors]."""
    return bn_groups(rows), bn_cw_log2(m), grid_1d(rows * m)


def bn_step(rows, m):
    """The row stride of one row lane of bn_colstat_kernel: groups * (256 / cw)."""
    g, l2, _ = bn_route(rows, m)
    return g * (256 >> l2)


def lane_rows(rows, m):
    """The set of row counts the row lanes of the statistics kernel execute."""
    step = bn_step(rows, m)
    return {rows // step + 1, rows // step} if rows % step else {rows // step}


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1 if n + 2 * p >= k else 0


def im2col_route(K_pad, C, nchw, dtype):
    """ofa_im2col: 2 the LDS tile kernel (NCHW source, 64 rows of Kpad elements within 48 KB), else im2col_kernel by 16-byte vectors
    (1: NHWC, C and Kpad whole vectors) or by elements (0)."""
    es = 4 if dtype == F32 else 2
    if nchw and (K_pad * es) % 16 == 0 and 64 * K_pad * es <= 48 * 1024:
        return 2
    return 1 if (not nchw and C % NVEC[dtype] == 0 and K_pad % NVEC[dtype] == 0) else 0


# ---------------------------------------------------------------------------------------------------------------- exact families
Geom = namedtuple("Geom", "B H W C kh kw s p")
INT_VIEW = {F32: torch.int32, BF16: torch.int16, FP16: torch.int16}


def geom_out(g):
    return out_size(g.H, g.kh, g.s, g.p), out_size(g.W, g.kw, g.s, g.p)


def kpad(g):
    return cdiv(g.kh * g.kw * g.C, 8) * 8


def same_bits(a, b):
    """Bit for bit, except that any NaN matches any NaN."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.uint8:
        return bool(torch.equal(a, b))
    na, nb = torch.isnan(a), torch.isnan(b)
    iv = INT_VIEW[a.dtype]
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.view(iv)[~na], b.view(iv)[~nb]))


def random_bits(shape, dtype, gen):
    """Random finite bit patterns of the dtype: every exponent but the all-ones one, subnormals and -0 included."""
    if dtype == F32:
        v = torch.randint(0, 2 ** 31, shape, generator=gen, dtype=torch.int64)
        v = torch.where((v >> 23) & 0xFF == 0xFF, v & ~(1 << 30), v)
        sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64)
        v = v - sign * 2 ** 31
        return v.to(torch.int32).view(F32)
    v = torch.randint(0, 2 ** 15, shape, generator=gen, dtype=torch.int64)
    mask, top = (0x7F80, 14) if dtype == BF16 else (0x7C00, 14)
    v = torch.where(v & mask == mask, v & ~(1 << top), v)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64)
    return (v - sign * 2 ** 15).to(torch.int16).view(dtype)


def _nhwc(x, g, nchw):
    return x.view(g.B, g.C, g.H, g.W).permute(0, 2, 3, 1) if nchw else x.view(g.B, g.H, g.W, g.C)


def _padded(t, g, fill=0):
    """[B, H, W, C] -> [B, H + 2p + s, W + 2p + s, C] with `fill` around (the extra s rows keep every strided slice in range)."""
    B, H, W, C = t.shape
    out = torch.full((B, H + 2 * g.p + g.s + g.kh, W + 2 * g.p + g.s + g.kw, C), fill, dtype=t.dtype, device=t.device)
    out[:, g.p:g.p + H, g.p:g.p + W] = t
    return out


def _taps(g):
    Ho, Wo = geom_out(g)
    for kh in range(g.kh):
        for kw in range(g.kw):
            yield kh * g.kw + kw, slice(kh, kh + g.s * Ho, g.s), slice(kw, kw + g.s * Wo, g.s)


def im2col_reference(x, g, nchw):
    """x: NHWC rows [B H W, C] or the [B, C, H, W] image -> col [B Ho Wo, Kpad] of x's dtype, moved as integers."""
    Ho, Wo = geom_out(g)
    xp = _padded(_nhwc(x.view(INT_VIEW[x.dtype]), g, nchw), g)
    col = torch.zeros(g.B, Ho, Wo, kpad(g), dtype=xp.dtype, device=x.device)
    for tap, hs, ws in _taps(g):
        col[..., tap * g.C:(tap + 1) * g.C] = xp[:, hs, ws]
    return col.view(g.B * Ho * Wo, kpad(g)).view(x.dtype)


def col2im_reference(dcol, g):
    """dcol [B Ho Wo, Kpad] of small integers -> dx [B H W, C]: every tap added where it was gathered from."""
    Ho, Wo = geom_out(g)
    d = dcol.double().view(g.B, Ho, Wo, -1)
    dxp = _padded(torch.zeros(g.B, g.H, g.W, g.C, dtype=F64, device=dcol.device), g)
    for tap, hs, ws in _taps(g):
        dxp[:, hs, ws] += d[..., tap * g.C:(tap + 1) * g.C]
    return dxp[:, g.p:g.p + g.H, g.p:g.p + g.W].reshape(g.B * g.H * g.W, g.C).to(dcol.dtype)


def maxpool_reference(x, g):
    """x [B H W, C] -> (y [B Ho Wo, C] of x's dtype, arg uint8): the taps in (kh, kw) order, `t > best or isnan(t)` replaces."""
    Ho, Wo = geom_out(g)
    xp = _padded(x.double().view(g.B, g.H, g.W, g.C), g)
    ok = _padded(torch.ones(g.B, g.H, g.W, g.C, dtype=torch.bool, device=x.device), g, False)
    best = torch.full((g.B, Ho, Wo, g.C), float("-inf"), dtype=F64, device=x.device)
    arg = torch.zeros(g.B, Ho, Wo, g.C, dtype=torch.uint8, device=x.device)
    for tap, hs, ws in _taps(g):
        t = xp[:, hs, ws]
        upd = ok[:, hs, ws] & ((t > best) | torch.isnan(t))
        best = torch.where(upd, t, best)
        arg = torch.where(upd, torch.full_like(arg, tap), arg)
    return best.view(g.B * Ho * Wo, g.C).to(x.dtype), arg.view(g.B * Ho * Wo, g.C)


def maxpool_bwd_reference(dy, arg, g):
    """dy [B Ho Wo, C] of small integers, arg the forward's taps -> dx [B H W, C]."""
    Ho, Wo = geom_out(g)
    d, a = dy.double().view(g.B, Ho, Wo, g.C), arg.view(g.B, Ho, Wo, g.C)
    dxp = _padded(torch.zeros(g.B, g.H, g.W, g.C, dtype=F64, device=dy.device), g)
    for tap, hs, ws in _taps(g):
        dxp[:, hs, ws] += torch.where(a == tap, d, torch.zeros_like(d))
    return dxp[:, g.p:g.p + g.H, g.p:g.p + g.W].reshape(g.B * g.H * g.W, g.C).to(dy.dtype)


def relu_reference(x, gate=None):
    zero = torch.zeros_like(x)
    if gate is not None:
        return torch.where(gate.float() > 0, x, zero)
    return torch.where(x.float() > 0, x, torch.where(torch.isnan(x), x, zero))


def small_ints(shape, dtype, gen):
    return torch.randint(-4, 5, shape, generator=gen).to(dtype)


# ---- the exact tables.  only: the dtypes a case exists for (None: all three); C in vectors (cv) or absolute (C)
IC = namedtuple("IC", "name cv C H W B kh kw s p nchw route only seed")
SIZES = ((7, 8), (1, 1), (2, 5), (8, 7))                 # odd / even, a 1 x 1 image, H < k with padding
_16 = (BF16, FP16)


def _im2col_cases():
    out = []

    def add(what, route, cv=0, C=0, H=7, W=8, B=2, kh=3, kw=3, s=1, p=1, nchw=False, only=None):
        out.append(IC(f"im2col {what} {'cv' + str(cv) if cv else 'C' + str(C)} {H}x{W} B{B} k{kh}x{kw} s{s} p{p}", cv, C, H, W, B, kh, kw, s, p,
                      nchw, route, only, 5000 + len(out)))

    for cv in (1, 2):
        for H, W in SIZES:
            add("vector", 1, cv=cv, H=H, W=W, s=1, p=1)
            add("vector", 1, cv=cv, H=H, W=W, s=2, p=1)
        add("vector", 1, cv=cv, kh=1, kw=1, s=2, p=0)
        add("vector", 1, cv=cv, kh=3, kw=5, s=1, p=1, H=4, W=7)
    add("vector pad vector (K 36, Kpad 40)", 1, C=4, only=(F32,))
    add("vector second sweep", 1, cv=256, B=1, H=65, W=65, kh=1, kw=1, s=1, p=0)
    for C in (1, 3, 12):                                  # (fp32: 12 channels are three whole vectors)
        for H, W in SIZES[:3]:
            add("scalar", 0, C=C, H=H, W=W, s=2 if C == 3 else 1, only=_16 if C == 12 else None)
    for B, H, W in ((1, 3, 5), (1, 15, 16), (1, 9, 25), (2, 30, 26)):          # 6, 64, 65 and 390 output positions
        add("lds stem", 2, C=3, B=B, H=H, W=W, kh=7, kw=7, s=2, p=3, nchw=True)
    add("lds audio", 2, C=1, B=2, H=8, W=10, s=2, p=0, nchw=True)
    add("lds audio", 2, C=1, B=1, H=6, W=12, s=2, p=0, nchw=True)
    add("lds limit (Kpad 384)", 2, C=6, B=1, H=9, W=10, kh=8, kw=8, s=1, p=0, nchw=True, only=_16)
    add("nchw element (Kpad 392)", 0, C=8, B=1, H=9, W=10, kh=7, kw=7, s=2, p=3, nchw=True, only=_16)
    add("lds limit (Kpad 192)", 2, C=3, B=1, H=9, W=10, kh=8, kw=8, s=1, p=0, nchw=True, only=(F32,))
    add("nchw element (Kpad 200)", 0, C=4, B=1, H=9, W=10, kh=7, kw=7, s=2, p=3, nchw=True, only=(F32,))
    return out


IM2COL_CASES = _im2col_cases()


def case_geom(c, dtype):
    return Geom(c.B, c.H, c.W, c.cv * NVEC[dtype] if c.cv else c.C, c.kh, c.kw, c.s, c.p)


def for_dtype(cases, dtype):
    return [c for c in cases if c.only is None or dtype in c.only]


# col2im and the pools: NHWC, whole vectors.  uncovered: trailing input rows / columns no window reaches (dx exactly 0 there)
PC = namedtuple("PC", "name cv C H W B kh kw s p nchw route only seed fill")
POOL_GEOMS = ((3, 2, 1), (3, 1, 1), (2, 2, 0), (5, 3, 2), (5, 3, 0), (1, 2, 0))
POOL_HW = ((1, 1), (2, 3), (3, 2), (4, 7), (7, 4), (8, 8), (7, 8), (10, 5))


def _pool_cases(kind):
    out = []
    fills = ("ties", "relu", "neginf", "nan")
    for k, s, p in POOL_GEOMS:
        for H, W in POOL_HW:
            if min(H, W) + 2 * p < k:
                continue
            for cv in ((1, 2) if (H, W) in ((4, 7), (8, 8)) else (1,)):
                out.append(PC(f"{kind} cv{cv} {H}x{W} k{k} s{s} p{p}", cv, 0, H, W, 2, k, k, s, p, False, None, None, 6000 + len(out),
                              fills[len(out) % 4]))
    if kind == "col2im":
        out.append(PC("col2im cv1 4x7 k3x5 s1 p1", 1, 0, 4, 7, 2, 3, 5, 1, 1, False, None, None, 6900, "ties"))
        out.append(PC("col2im cv1 9x9 k7 s2 p3", 1, 0, 9, 9, 1, 7, 7, 2, 3, False, None, None, 6901, "ties"))
        out.append(PC("col2im second sweep cv256 65x65 k1 s2 p0", 256, 0, 65, 65, 1, 1, 1, 2, 0, False, None, None, 6902, "ties"))
    else:
        out.append(PC(f"{kind} second sweep cv256 65x65 k3 s1 p1", 256, 0, 65, 65, 1, 3, 3, 1, 1, False, None, None, 6903, "relu"))
    return out


COL2IM_CASES = _pool_cases("col2im")
MAXPOOL_CASES = _pool_cases("maxpool")


def uncovered(g):
    """Input rows / columns beyond the last window."""
    Ho, Wo = geom_out(g)
    return max(0, g.H - ((Ho - 1) * g.s - g.p + g.kh)), max(0, g.W - ((Wo - 1) * g.s - g.p + g.kw))


def pool_input(c, g, dtype, gen):
    """Mostly ties: values from {-inf, -1, 0, 0, 0, 1}; a post-ReLU map; one window of nothing but -inf; planted NaN windows."""
    n = g.B * g.H * g.W
    if c.fill == "relu":
        return torch.relu(torch.randn(n, g.C, generator=gen)).to(dtype)
    vals = torch.tensor([float("-inf"), -1.0, 0.0, 0.0, 0.0, 1.0])
    x = vals[torch.randint(0, 6, (n, g.C), generator=gen)]
    if c.fill == "neginf":
        x.view(g.B, g.H, g.W, g.C)[0, :g.kh, :g.kw] = float("-inf")
    if c.fill == "nan":
        xv = x.view(g.B, g.H, g.W, g.C)
        xv[0, 0, 0, 0] = float("nan")
        xv[-1, g.H // 2, g.W // 2, 1:3] = float("nan")
        xv[-1, g.H - 1, g.W - 1, g.C - 1] = float("nan")
    return x.to(dtype)


RELU_N = (1, 255, 256, 257, SWEEP + 257)
SPECIALS = {F32: (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0x3F800000, 0xBF800000),
            BF16: (0x0000, 0x8000, 0x0001, 0x8001, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0xBF80),
            FP16: (0x0000, 0x8000, 0x0001, 0x8001, 0x7C00, 0xFC00, 0x7E00, 0x3C00, 0xBC00)}      # +-0, +-min subnormal, +-inf, NaN, +-1


def relu_input(n, dtype, gen, shift=0):
    """randn with the special values cycling through the first elements and the last (shift: another phase, for the gate)."""
    x = torch.randn(n, generator=gen).to(dtype)
    sp = torch.tensor(SPECIALS[dtype], dtype=torch.int64)
    sp = torch.where(sp >= 2 ** (31 if dtype == F32 else 15), sp - 2 ** (32 if dtype == F32 else 16), sp).to(INT_VIEW[dtype]).view(dtype)
    k = min(n, 4 * len(sp))
    x[:k] = sp[(torch.arange(k) + shift) % len(sp)]
    if n > 300:
        x[n - len(sp):] = sp[(torch.arange(len(sp)) + shift) % len(sp)]
    return x


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
BN = namedtuple("BN", "name m C rows nb regime train relu res gate want_dres acc mom eps mode G nan bwd seed")
# m: C in vectors (C: absolute, when m == 0); rows: of the launch (A); nb: rows of the other rank (sync); gate: "" / "y" / "x";
# mode: bn / groups / sync; G: partial rows (groups); nan: NaN planted (forward only); bwd: the backward is run.
MUTATIONS = ("drop_tail_row", "drop_groups_past_256", "biased_running_var", "no_var_clamp", "gate_from_unrounded", "regate_ignores_beta",
             "dres_ungated", "accumulate_overwrites", "rows_not_total", "eval_subtracts_batch_terms", "relu_eats_nan")
BN_M = (1, 2, 8, 16, 32, 33, 129)
# (train, relu, res, gate, want_dres)
FLAGS = ((True, False, False, "", False), (True, True, False, "x", False), (True, True, True, "y", True), (True, True, True, "y", False),
         (True, False, True, "", True), (False, True, False, "x", False), (False, True, True, "y", True), (True, True, False, "y", False),
         (False, False, False, "", False))


def rows_for(m, want, limit_rows=700):
    """The smallest row count at which some row lane of the statistics kernel executes `want` rows (>= want for want == 5)."""
    for rows in range(1, limit_rows):
        lr = lane_rows(rows, m)
        if (want == 5 and max(lr) >= 5) or want in lr:
            return rows
    return None


def _bn_cases():
    out = []

    def add(what, m=0, C=0, rows=5, nb=0, regime=None, flags=None, acc=None, mode="bn", G=0, nan=False, bwd=True):
        i = len(out)
        train, relu, res, gate, want_dres = flags if flags is not None else FLAGS[i % len(FLAGS)]
        regime = regime or REGIMES[i % 4]
        acc = (i % 3 == 0) if acc is None else acc
        g, l2, blocks = bn_route(rows, m or C // 4)
        out.append(BN(f"bn {what}{' G' + str(G) if G else ''} {'m' + str(m) if m else 'C' + str(C)} rows{rows}{'+' + str(nb) if nb else ''} cw{1 << bn_cw_log2(m) if m else '?'} "
                      f"g{g} {regime} {'train' if train else 'eval'} relu{int(relu)} res{int(res)} gate[{gate}] dres{int(want_dres)} acc{int(acc)}",
                      m, C, rows, nb, regime, train, relu, res, gate, want_dres, acc and bwd, (0.1, 0.01)[i % 2], (1e-5, 1e-3)[(i // 2) % 2],
                      mode, G, nan, bwd, 7000 + i))

    for m in BN_M:                                       # the pair loop and its tail: a lane with 0 / 1, 2, 3 and >= 5 rows where m allows
        for rows in sorted({1, 3} | {r for r in (rows_for(m, w) for w in (2, 3, 5)) if r}):
            add("lanes", m=m, rows=rows)
    for j, fl in enumerate(FLAGS):                       # the flag space on one narrow and one ragged shape, every regime
        add("flags", m=2, rows=37, flags=fl, regime=REGIMES[j % 4], acc=j % 2 == 0)
        add("flags", m=33, rows=19, flags=fl, regime=REGIMES[(j + 1) % 4], acc=j % 2 == 1)
    for fl in (FLAGS[5], FLAGS[6]):                      # eval beyond one block of bn_eval_stats_kernel: 264 channels
        add("eval C264", C=264, rows=9, flags=fl)
    add("groups cap", m=32, rows=32768, flags=FLAGS[1], regime="prow")
    add("groups cap binding", m=32, rows=32768 + 129, flags=FLAGS[2], regime="prow")
    add("second sweep", m=256, rows=4100, flags=FLAGS[1], regime="randn")
    for fl in (FLAGS[5], FLAGS[2]):                      # NaN through the fused ReLU: in x (eval) and in the residual (training)
        add("nan", m=2, rows=11, flags=fl, nan=True, bwd=False, regime="randn")
    for j, G in enumerate((1, 15, 16, 17, 255, 256, 257, 513)):
        add("partial rows", C=(8, 24, 40)[j % 3], rows=37, mode="groups", G=G, bwd=False, flags=FLAGS[(0, 1, 2)[j % 3]], regime=REGIMES[j % 2])
    add("sync", m=2, rows=37, nb=20, mode="sync", flags=FLAGS[1], regime="randn")
    add("sync", m=33, rows=20, nb=37, mode="sync", flags=FLAGS[4], regime="offset")
    add("sync", m=33, rows=41, nb=7, mode="sync", flags=FLAGS[0], regime="prow", acc=True)
    return out


BN_CASES = _bn_cases()
BIG = 1 << 21                                             # elements: the three large cases


def bn_cols(case, dtype):
    return case.m * NVEC[dtype] if case.m else case.C


def bn_m(case, dtype):
    return case.m if case.m else case.C // NVEC[dtype]


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _stats64(c):
    """The float64 statistics of a case: (mean, var, mean|x|) over all rows, or the running ones in eval mode."""
    x = c["x"].double()
    am = torch.nan_to_num(x.abs(), nan=0.0).mean(0)          # (a planted NaN is no magnitude)
    if not c["train"]:
        return c["rm0"].double(), c["rv0"].double(), am
    mu = x.mean(0)
    return mu, ((x - mu) ** 2).mean(0), am


def gate_terms(c, mean, rstd):
    """t = (x - mean) rstd gamma + beta in float64 and its term-by-term magnitude (with mean|x|: what an error of the mean is measured in)."""
    x, g, b = c["x"].double(), c["gamma"].double(), c["beta"].double()
    t = (x - mean) * rstd * g + b
    return t, (x.abs() + mean.abs() + x.abs().mean(0)) * rstd * g.abs() + b.abs()


def ambiguous(c, mean=None, rstd=None, margin=GATE_MARGIN):
    """bool [rows, C]: the gate-ambiguous elements under the given (default: the float64) statistics."""
    if mean is None:
        mu, var, _ = _stats64(c)
        mean, rstd = mu, 1 / torch.sqrt(var + _f32(c["eps"]))
    t, bd = gate_terms(c, mean, rstd)
    return t.abs() < margin * bd


def build_bn(case, dtype, device="cpu"):
    N, C = NVEC[dtype], bn_cols(case, dtype)
    rows, gen = case.rows + case.nb, _gen(case.seed)
    x = torch.randn(rows, C, generator=gen)
    dy = torch.randn(rows, C, generator=gen)
    if case.regime == "offset":
        x += 100.0
    gamma = (1 + 0.1 * torch.randn(C, generator=gen)).to(dtype)
    beta = (0.1 * torch.randn(C, generator=gen)).to(dtype)
    cc = C // 2
    if case.regime == "const" and case.mode != "groups":
        x[:, cc] = CONST
        beta[cc] = 1.0 if case.seed % 2 else -1.0         # (t = beta in that column: well away from the gate)
    if case.regime == "prow":
        x[case.rows - 1] += PLANT
        dy[case.rows - 1] += PLANT
    res = torch.randn(case.rows, C, generator=gen).to(dtype) if case.res else None
    rm0 = (0.1 * torch.randn(C, generator=gen)).float()
    rv0 = (0.5 + torch.rand(C, generator=gen)).float()
    prev = tuple((0.1 * torch.randn(C, generator=gen)).to(dtype) for _ in range(2)) if case.acc else None
    plant = (not case.train) and case.gate == "y" and not case.nan
    if plant:                                             # t = 2^-27 rstd: a positive value that fp16 stores as 0 (gate_from_unrounded)
        x[0, 0], rm0[0], gamma[0], beta[0] = 1.0, 1.0 - 2.0 ** -24, 0.125, 0.0
        if res is not None:
            res[0, 0] = 0.0
    x = x.to(dtype)
    if case.nan:
        if case.train:
            res[3, 1], res[case.rows - 1, C - 1] = float("nan"), float("nan")
        else:
            x[3, 1], x[case.rows - 1, C - 1], x[0, N] = float("nan"), float("nan"), float("nan")
    c = dict(x=x, gamma=gamma, beta=beta, res=res, dy=dy.to(dtype), rm0=rm0, rv0=rv0, prev=prev, train=case.train, relu=case.relu,
             gate=case.gate, want_dres=case.want_dres, mom=case.mom, eps=case.eps, mode=case.mode, na=case.rows, bwd=case.bwd, nan=case.nan,
             negvar=None, partial=None)
    for k, v in c.items():
        if torch.is_tensor(v):
            c[k] = v.to(device)
    if prev is not None:
        c["prev"] = tuple(p.to(device) for p in prev)
    if case.gate == "x" and case.bwd:                     # no gate-ambiguous element may be left
        for _ in range(64):
            amb = ambiguous(c)
            if not bool(amb.any()):
                break
            c["x"] = torch.where(amb, (c["x"].float() + 0.5).to(dtype), c["x"])
        assert not bool(ambiguous(c).any()), case.name
    if case.mode == "groups":
        xd = c["x"].double()
        nv = C - 1
        c["x"][:, nv] = 2.0                                # a constant column whose partials say variance = -eps / 2: the clamp's case
        xd[:, nv] = 2.0
        s, q = xd.sum(0), (xd * xd).sum(0)
        q[nv] = rows * (4.0 - 0.5 * _f32(case.eps))
        w = (torch.rand(case.G, 2, C, generator=gen, dtype=F64) + 0.1).to(device)
        w = w / w.sum(0)
        part = w * torch.stack([s, q])
        part[-1] += torch.stack([s, q]) - part.sum(0)
        c["partial"], c["negvar"] = part, nv
    return c


def _xha(x, mu, rs, dtype):
    """|xh| for the bound: fp32 tensors term by term; 16-bit tensors as ONE term |x - mu| rs plus the float32 error of x, mu and the
    subtraction in units of the 16-bit eps (see rownorm_oracle._xha; the mean of |x| is the column's here)."""
    xa = x.abs()
    if dtype == F32:
        return (xa + mu.abs()) * rs
    return ((x - mu).abs() + KAPPA[dtype] * (xa + mu.abs() + torch.nan_to_num(xa, nan=0.0).mean(0))) * rs


def bn_reference(c, own):
    """own: dict(mean, rstd, y) -- the kernel's (or the emulation's) own stored statistics and output, the inputs of the backward stage.
    -> (ref, bound), float64.  y, dx, dres cover the launch's rows (the first na); dgamma / dbeta are the launch's own column sums
    (+ prev); sums covers every row (sync: both ranks); running_* only in training mode."""
    x_all, g, b = c["x"].double(), c["gamma"].double(), c["beta"].double()
    dtype, na = c["x"].dtype, c["na"]
    R = float(x_all.shape[0])
    eps, mom = _f32(c["eps"]), _f32(c["mom"])
    mu, var, am = _stats64(c)
    if c["negvar"] is not None:
        var = var.clone()
        var[c["negvar"]] = 0.0
    rs = 1 / torch.sqrt(var + eps)
    ref, bd = dict(mean=mu, rstd=rs), dict(mean=am)
    if c["train"]:
        unb = var * R / (R - 1) if R > 1 else var
        ref["running_mean"], bd["running_mean"] = (1 - mom) * c["rm0"].double() + mom * mu, (1 - mom) * c["rm0"].double().abs() + mom * am
        ref["running_var"], bd["running_var"] = (1 - mom) * c["rv0"].double() + mom * unb, (1 - mom) * c["rv0"].double().abs() + mom * unb
    x = x_all[:na]
    t, ta = (x - mu) * rs * g + b, _xha(x_all, mu, rs, dtype)[:na] * g.abs() + b.abs()
    if c["res"] is not None:
        t, ta = t + c["res"].double(), ta + c["res"].double().abs()
    if c["relu"]:
        t = torch.where(torch.isnan(t), t, t.clamp_min(0))
    ref["y"], bd["y"] = t, ta
    if not c["bwd"]:
        return ref, bd
    # ---- backward, from the kernel's own statistics (and y)
    mo, ro = own["mean"].double(), own["rstd"].double()
    xh, xha = (x_all - mo) * ro, _xha(x_all, mo, ro, dtype)
    dy = c["dy"].double()
    if c["gate"] == "x":
        on = gate_terms(c, mo, ro)[0] > 0
    elif c["gate"] == "y":
        on = torch.ones_like(dy, dtype=torch.bool)
        on[:na] = own["y"].double() > 0
    else:
        on = torch.ones_like(dy, dtype=torch.bool)
    gd = torch.where(on, dy, torch.zeros_like(dy))
    ga = gd.abs()
    sg, sx = gd.sum(0), (gd * xh).sum(0)
    sga, sxa = ga.sum(0), (ga * xha).sum(0)
    ref["sums"], bd["sums"] = torch.stack([sg, sx]), torch.stack([sga, sxa])
    lg, lx, lga, lxa = gd[:na].sum(0), (gd[:na] * xh[:na]).sum(0), ga[:na].sum(0), (ga[:na] * xha[:na]).sum(0)
    pg, pb = (c["prev"][0].double(), c["prev"][1].double()) if c["prev"] is not None else (0.0, 0.0)
    ref["dgamma"], bd["dgamma"] = lx + pg, lxa + (pg.abs() if c["prev"] is not None else 0.0)
    ref["dbeta"], bd["dbeta"] = lg + pb, lga + (pb.abs() if c["prev"] is not None else 0.0)
    if c["train"]:
        ref["dx"] = g * ro * (gd[:na] - (sg + xh[:na] * sx) / R)
        bd["dx"] = g.abs() * ro * (ga[:na] + (sga + xha[:na] * sxa) / R)
    else:
        ref["dx"], bd["dx"] = g * ro * gd[:na], g.abs() * ro * ga[:na]
    if c["want_dres"]:
        ref["dres"], bd["dres"] = gd[:na], ga[:na]
    return ref, bd


def kept_rows(rows, m):
    """drop_tail_row: the rows that survive when every row lane with an odd row count loses its last (the one-row tail)."""
    step = bn_step(rows, m)
    i = torch.arange(rows)
    n_lane = rows // step + (i % step < rows % step).long()
    return ~((n_lane % 2 == 1) & (i // step == n_lane - 1))


def _fmax_relu(t, eats_nan):
    return torch.where(t > 0, t, torch.zeros_like(t)) if eats_nan else torch.where(torch.isnan(t), t, t.clamp_min(0))


def bn_emulate(c, dtype, mutation=None):
    """fp64 column sums, fp32 statistics, fp32 apply and dx, one rounding of each stored output -> every output under the oracle's names."""
    assert mutation is None or mutation in MUTATIONS, mutation
    x_all, na = c["x"], c["na"]
    rows_all, C = x_all.shape
    m = C // NVEC[dtype]
    xd, xf = x_all.double(), x_all.float()
    g, b = c["gamma"].float(), c["beta"].float()
    eps, mom = _f32(c["eps"]), _f32(c["mom"])
    R = float(rows_all)
    out = {}

    def colsum(v, lo, hi):
        """fp64 column sums of rows lo .. hi (one launch of the statistics kernel)."""
        v = v[lo:hi]
        if mutation == "drop_tail_row":
            v = v[kept_rows(hi - lo, m).to(v.device)]
        return v.sum(0)

    blocks = [(0, na)] + ([(na, rows_all)] if rows_all > na else [])
    if c["train"]:
        if c["mode"] == "groups":
            p = c["partial"][:256] if mutation == "drop_groups_past_256" else c["partial"]
            s, q = p[:, 0].sum(0), p[:, 1].sum(0)
        else:
            s = sum(colsum(xd, lo, hi) for lo, hi in blocks)
            q = sum(colsum(xd * xd, lo, hi) for lo, hi in blocks)
        mu = s / R
        var = q / R - mu * mu
        if mutation != "no_var_clamp":
            var = var.clamp_min(0)
        mean, rstd = mu.float(), (1.0 / torch.sqrt(var + eps)).float()
        unb = var * R / (R - 1) if (R > 1 and mutation != "biased_running_var") else var
        out["running_mean"] = ((1.0 - mom) * c["rm0"].double() + mom * mu).float()
        out["running_var"] = ((1.0 - mom) * c["rv0"].double() + mom * unb).float()
    else:
        # 1.0f / sqrtf(running_var + eps), each fp32 operation correctly rounded: through float64, where rounding an fp32 sum, square
        # root or quotient a second time is innocuous -- the same bits on every host, whatever its vector maths library does
        rnd = lambda v: v.float().double()                                  # noqa: E731
        mean, rstd = c["rm0"].clone(), (1.0 / rnd(torch.sqrt(rnd(c["rv0"].double() + eps)))).float()
    out["mean"], out["rstd"] = mean, rstd
    t = (xf[:na] - mean) * rstd * g + b
    if c["res"] is not None:
        t = t + c["res"].float()
    if c["relu"]:
        t = _fmax_relu(t, mutation == "relu_eats_nan")
    out["y"] = t.to(dtype)
    out["t32"] = (xf - mean) * rstd * g + b                # (the recomputed gate's expression: measured against float64 by the CPU test)
    if not c["bwd"]:
        return out
    dy = c["dy"].float()
    on = torch.ones_like(dy, dtype=torch.bool)
    if c["gate"] == "x":
        on = ((xf - mean) * rstd * g + (0.0 if mutation == "regate_ignores_beta" else b)) > 0
    elif c["gate"] == "y":
        on[:na] = (t if mutation == "gate_from_unrounded" else out["y"].float()) > 0
    gd = torch.where(on, dy, torch.zeros_like(dy))
    xh = (xf - mean) * rstd
    parts = [(colsum(gd.double(), lo, hi).float(), colsum(gd.double() * xh.double(), lo, hi).float()) for lo, hi in blocks]
    sg, sx = sum(p[0] for p in parts), sum(p[1] for p in parts)             # (sync: the two ranks' fp32 sums added in fp32)
    out["sums"] = torch.stack([sg, sx])
    prev = c["prev"] if (c["prev"] is not None and mutation != "accumulate_overwrites") else None
    out["dgamma"] = ((prev[0].float() if prev else 0.0) + parts[0][1]).to(dtype)
    out["dbeta"] = ((prev[1].float() if prev else 0.0) + parts[0][0]).to(dtype)
    inv = torch.tensor(1.0 / (float(na) if mutation == "rows_not_total" else R), dtype=F32, device=x_all.device)
    if c["train"] or mutation == "eval_subtracts_batch_terms":
        tt = gd[:na] - (sg + xh[:na] * sx) * inv
    else:
        tt = gd[:na]
    out["dx"] = (g * rstd * tt).to(dtype)
    if c["want_dres"]:
        out["dres"] = (dy[:na] if mutation == "dres_ungated" else gd[:na]).to(dtype)
    return out


def bn_figures(c, got, dtype):
    """Every output of one case against its reference -> {output: figure}.  y_nan: 0 when y is NaN exactly where the reference is."""
    ref, bd = bn_reference(c, got)
    fig = {}
    for n in ref:
        if n == "mean":
            fig[n] = scalar_err(got[n], ref[n], bd[n])
        elif n == "rstd":
            fig[n] = scalar_err(got[n], ref[n])
        elif n in ("running_mean", "running_var"):
            fig[n] = scalar_err(got[n], ref[n], bd[n])
        elif n == "sums":
            fig[n] = excess(got[n], ref[n], bd[n], 1.0, floor_of(F32))
        elif n == "y" and c["nan"]:
            nn = torch.isnan(ref[n])
            fig["y_nan"] = 0.0 if bool(torch.equal(torch.isnan(got[n]), nn)) else float("inf")
            z = torch.zeros_like(ref[n])
            fig[n] = grad_excess(torch.where(nn, z, got[n].double()), torch.where(nn, z, ref[n]), torch.where(nn, z, bd[n]), dtype)
        else:
            fig[n] = grad_excess(got[n], ref[n], bd[n], dtype)
    return fig


def applies(mutation, case):
    """Whether a case can notice a mutation at all."""
    fwd_stats = case.train and case.mode != "groups"
    return {"drop_tail_row": fwd_stats or case.bwd, "drop_groups_past_256": case.G > 256, "biased_running_var": case.train,
            "no_var_clamp": case.mode == "groups", "gate_from_unrounded": case.gate == "y" and case.bwd and not case.train,
            "regate_ignores_beta": case.gate == "x" and case.bwd, "dres_ungated": case.want_dres and case.relu and case.bwd,
            "accumulate_overwrites": case.acc, "rows_not_total": case.mode == "sync", "eval_subtracts_batch_terms": case.bwd and not case.train,
            "relu_eats_nan": case.nan}[mutation]
