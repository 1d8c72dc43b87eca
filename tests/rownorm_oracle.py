"""A plain-torch oracle for the row-normalisation kernels (csrc/layernorm.hip, csrc/join.hip): no GPU needed, no dependency on the kernels.

Two kernel families -- LayerNorm / GELU+LayerNorm forward and backward (ln_*) and the fused residual join y = residual + dropout(LN_a(x)),
z = LN_b(y) with its backward (join_*) -- each with
  *_reference()  float64 on the stored (already rounded) inputs, restated from the formulas in the kernel comments, returning EVERY output
                 together with its componentwise magnitude bound: the same expression with every term replaced by its absolute value
                 (fp32 tensors: x - mu counts as two terms, |x| + |mu|; 16-bit tensors: as one, |x - mu|, plus its float32 error
                 in units of the 16-bit eps -- _xha).  Where the bound is 0 the kernel must write exactly 0.
  *_emulate()    the same arithmetic in float32 with the kernels' rounding points and nothing else of the kernels, able to apply one
                 named mutation (LN_FWD_MUTATIONS, LN_BWD_MUTATIONS, JOIN_MUTATIONS).
excess()         max (|got - ref| - floor) / bound in units of the 16-bit eps; inf for a non-finite value or a non-zero where bound == 0.
ln_fwd_figures() / ln_bwd_figures() / join_figures()   every output of one case against its reference -> {output: figure};
limit()          what a figure may be: CEILING for the emulation, TOL = 2 CEILING for a kernel (fp32: G32 / 8 and G32).

The join is checked in stages, because join.hip rounds at documented points (the LN_a output, y, the gradient of y, the dropout
gradient): z and the LN_b statistics against float64 of the kernel's OWN y; dres from dz, that y and dy; dx and the parameter gradients
from the kernel's OWN dres; y against the chain from x.  At most two storage roundings then lie between the reference's inputs and an
output; each adds one eps * |value| pushed through the remaining linear map with absolute values, and is folded into the bound.
The dropout mask is an INPUT of the oracle (the GPU test reads it off the stand-alone dropout kernel, the CPU test draws it).

Inputs come from a CPU generator in four regimes: `randn` (unit rows), `offset` (x = 100 + randn: a one-pass variance loses its digits),
`pcol` (x = 64 at a seam column of every row: that column carries the row's mean and variance) and `prow` (dy / dz = 64 + randn in a
seam row: that row carries the column sums).  Row 1 of every case with three or more rows is constant (variance 0, rstd = 1 / sqrt(eps));
eps alternates between 1e-5 and 1e-3; gamma = 1 + 0.1 randn and beta = 0.1 randn, rounded to the dtype.

Shapes are given in vectors: cols = m * N, N = the elements of a 16-byte vector (8 for the 16-bit types, 4 for fp32), because every
LayerNorm route and the split-row join routes depend on m alone; the row-per-wave join shapes are absolute (256 k columns).
tests/test_rownorm_oracle_cpu.py proves the tables sound and confirms every claimed route against the library's host-only entry points;
tests/test_rownorm_edges_gpu.py runs the tables against the kernels.
"""
import math
from collections import namedtuple

import torch

F64, F32, BF16, FP16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
EPS = {BF16: 2.0 ** -8, FP16: 2.0 ** -11}
NVEC = {F32: 4, BF16: 8, FP16: 8}                                       # elements of a 16-byte vector
DTYPES3 = (F32, BF16, FP16)
NAMES = {F32: "fp32", BF16: "bf16", FP16: "fp16"}
PLANT = 64.0
CONST = 0.75                                                            # the constant row
REGIMES = ("randn", "offset", "pcol", "prow")
LN_BLOCKS = 256                                                         # LN_BWD_BLOCKS == JOIN_BLOCKS: the persistent grid
INV_SQRT2 = 0.7071067811865476
INV_SQRT_2PI = 0.3989422804014327

# ---------------------------------------------------------------------------------------------------------------- measured constants
# CEILING: the cap on excess(emulate, reference, bound) over the whole table (every route, regime, bf16 and fp16), per output family.
# The emulation rounds an output once: at most u = EPS relative to the value, the value is at most the bound, and the float32 work before
# it is ~1e-6 of the bound.  The join's y, dx and LN_a gradients carry one more storage rounding, which the bound already contains.
# Measured 2026-10-20 (tests/test_rownorm_oracle_cpu.py prints the figures with -s), worst excess:
#          ln fwd y   ln bwd dx   dgamma   dbeta   dbias  | join y    z       dres    dx      dgamma_a/b      dbeta_a/b       dx_colsum
#   bf16   0.996      0.825       0.992    0.996   0.697  |      0.996   0.996   0.962   0.879   0.968 / 0.972   0.988 / 0.996   0.996
#   fp16   0.996      0.853       0.991    0.999   0.698  |      0.999   0.999   0.973   0.889   0.968 / 0.988   0.992 / 0.994   0.980
CEILING = 1.0
# TOL for the kernels = 2 * CEILING: the factor 2 covers what the emulation leaves out -- the summation order of the 64-lane and
# cross-wave reductions, v_rsq_f32 in the row-per-wave join, the rational erf of the bf16 GELU.  Never set from what a kernel produced.
TOL = 2.0 * CEILING
# fp32 tensors (fp32 inputs): 8 x the largest error / bound of the emulation's float32 evaluation against float64 over the table.
# The row statistics are fp32 for every dtype: mean as |error| / mean|row|, rstd as relative error, 8 x the emulation's worst.
# Measured 2026-10-20, the emulation's worst over the tables and the three dtypes (each fp32 output has its own figure):
#   fp32 tensors, error / bound: LayerNorm forward y 5.93e-7; backward dx 1.75e-7, dgamma 1.57e-7, dbeta 1.67e-7, dbias 6.55e-8;
#   join y 3.94e-7, z 2.62e-6 (2049 x 1024), dres 2.25e-7, dx 1.94e-7, dgamma_a 2.54e-7, dbeta_a 1.38e-7, dgamma_b 1.46e-6,
#   dbeta_b 1.79e-7, dx_colsum 1.49e-7
#   mean 1.55e-7 (LayerNorm), 1.25e-7 (join);  rstd 1.72e-7 (LayerNorm), 2.10e-7 (join)
G32 = {"ln_fwd": {"y": 8 * 6.0e-7},
       "ln_bwd": {"dx": 8 * 1.8e-7, "dgamma": 8 * 1.6e-7, "dbeta": 8 * 1.7e-7, "dbias": 8 * 6.6e-8},
       "join": {"y": 8 * 4.0e-7, "z": 8 * 2.7e-6, "dres": 8 * 2.3e-7, "dx": 8 * 2.0e-7, "dgamma_a": 8 * 2.6e-7, "dbeta_a": 8 * 1.4e-7,
                "dgamma_b": 8 * 1.5e-6, "dbeta_b": 8 * 1.8e-7, "dx_colsum": 8 * 1.5e-7}}
MEAN_TOL = 8 * 1.6e-7
RSTD_TOL = 8 * 2.2e-7
# The kernels themselves on an MI355X, 2026-10-20, worst over the same tables (tests/test_rownorm_edges_gpu.py prints them with -s):
#   16-bit tensors, excess in eps against TOL = 2.0:
#          ln fwd y   ln bwd dx   dgamma   dbeta   dbias  | join y    z       dres    dx      dgamma_a/b      dbeta_a/b       dx_colsum
#   bf16   0.996      0.825       0.992    0.996   0.697  |      0.996   0.996   0.976   0.879   0.968 / 0.977   0.988 / 0.996   0.996
#   fp16   1.29       0.853       0.991    0.999   0.698  |      0.999   0.998   0.971   0.889   0.968 / 0.988   0.992 / 0.994   0.980
#   (one rounding of the result, as the emulation; fp16 forward y 1.29: a 100 + randn row, where the kernel's mean is 9e-7 of the row's
#    magnitude off and that shows against |x - mu|; the forced forms of the debug library: every figure <= 0.999)
#   fp32 tensors, error / bound, of 8 x the emulation's figure above: LayerNorm forward y 7.6e-7; backward dx 1.75e-7, dgamma 1.57e-7,
#   dbeta 1.67e-7, dbias 4.3e-8; join y 3.2e-7, z 2.65e-6, dres 1.9e-7, dx 2.0e-7, dgamma_a 3.2e-7, dbeta_a 1.3e-7, dgamma_b 4.3e-7,
#   dbeta_b 1.6e-7, dx_colsum 1.5e-7
#   mean <= 9.2e-7 (LayerNorm: fp16 and fp32; bf16 6.2e-7), 1.3e-7 (join) of 1.28e-6;  rstd <= 5.4e-7 (LayerNorm), 3.2e-7 (join) of 1.76e-6
# One finding, by `fwd NV32 m2048 rows3 gelu randn` and `fwd NV32 m2048 rows5 gelu offset` in bf16 and fp16: the mean of the constant
# row of 16384 columns came out 2.57e-6 (bf16) / 2.26e-6 (fp16) of mean|row| off, twice MEAN_TOL, and rstd of the fp16 offset case
# 1.85e-6 off.  ln_fwd_kernel added a lane's up to 256 elements into ONE running sum, which rounds the same way at every step when the
# elements are equal; its NV = 32 instantiations (more than 128 elements per lane) now sum in three levels: a vector's elements, four
# vectors, the groups.  Narrower rows keep their code, and their bits, unchanged; the figures above are from after the change.


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


def floor_of(dtype):
    """The absolute error an underflow may cost: one smallest subnormal step of fp16; nothing to speak of for bf16 and fp32."""
    return 2.0 ** -24 if dtype == FP16 else 2.0 ** -126


def grad_excess(got, ref, bound, dtype):
    """16-bit: in units of the type's eps; fp32: error / bound."""
    return excess(got, ref, bound, EPS.get(dtype, 1.0), floor_of(dtype))


def scalar_err(got, ref, scale=None):
    """fp32 row scalars against float64: max |got - ref| / scale (scale None: relative to |ref|); inf for a non-finite value."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    s = ref.abs() if scale is None else scale.double()
    return float(((got - ref).abs() / s.clamp_min(1e-300)).max())


def limit(family, name, dtype, kernel=True):
    """The largest figure output `name` may show: the emulation's cap, or (kernel=True) what the GPU test allows a kernel."""
    if name.startswith("mean"):
        v = MEAN_TOL
    elif name.startswith("rstd"):
        v = RSTD_TOL
    elif name == "ydrop":
        return 0.0
    elif dtype == F32:
        v = G32[family][name]
    else:
        return TOL if kernel else CEILING
    return v if kernel else v / 8


# ---------------------------------------------------------------------------------------------------------------- routes, restated
def cdiv(a, b):
    return -(-a // b)


def ln_fwd_nv(m):
    """ln_fwd_dispatch: the register-slab count NV for a row of m vectors (64 lanes per slab); None: refused (more than 32)."""
    nv = cdiv(m, 64)
    return next((v for v in (1, 2, 4, 8, 16, 32) if nv <= v), None)


Route = namedtuple("Route", "wpr nv wpb rpb pf")


def ln_bwd_route(m, gelu):
    """ln_check + ln_bwd_wpr + ln_bwd_dispatch for a row of m vectors: waves per row, NV, waves per block, rows per block iteration,
    prefetch ring depth; None: refused."""
    w = 1
    while w < 8 and cdiv(m // w, 64) > 2 and m % (w * 2) == 0:
        w *= 2
    if cdiv(m // w, 64) > 8:
        return None
    if gelu and m == 6 * 64:
        wpr = 6
    else:
        wpr = 1
        while wpr < 8 and cdiv(m // wpr, 64) > (1 if gelu else 2) and m % (wpr * 2) == 0:
            wpr *= 2
    nv = next(v for v in (1, 2, 4, 8) if cdiv(m // wpr, 64) <= v)
    wpb = 12 if wpr == 6 else 16
    pf = 0 if wpr == 1 else (2 if wpb < 16 else (1 if (not gelu and nv == 1) else 0))
    return Route(wpr, nv, wpb, wpb // wpr, pf)


JRoute = namedtuple("JRoute", "kind k wpr nv rpb")          # kind: "row" (row per wave, k = cols / 256) or "split"


def join_route(cols, dtype, backward, keep=True):
    """join_check + join_row_k + join_wpr: None when refused.  keep: the backward is handed the forward's keep bits (or p == 0)."""
    N = NVEC[dtype]
    if cols <= 0 or cols % N or cols > 64 * N * 8:
        return None
    wpr = 1
    while wpr < 8 and cols // wpr > 64 * N:
        wpr *= 2
    if cols % (wpr * N):
        return None
    k = cols // 256 if (dtype != F32 and cols % 256 == 0 and 1 <= cols // 256 <= (4 if backward else 6)) else 0
    if k and (keep or not backward):
        return JRoute("row", k, 0, 0, 8)
    nv = next(v for v in (1, 2, 4, 8) if cdiv(cols, 64 * N) <= v)
    return JRoute("split", 0, wpr, nv, (16 if wpr == 8 else 12) // wpr)


def join_keep_bytes(rows, cols, dtype):
    r = join_route(cols, dtype, True)
    return rows * ((r.k + 1) // 2) * 64 if r is not None and r.kind == "row" else 0


# ---------------------------------------------------------------------------------------------------------------- shared arithmetic
def _gelu_abs(h):
    """The magnitude of Phi = 0.5 (1 + erf(h / sqrt 2)) term by term: 0.5 (1 + |erf|) -- the sum cancels for h << 0."""
    return 0.5 * (1 + torch.erf(h * INV_SQRT2).abs())


def _kappa(dtype):
    """What a float32 rounding weighs in units of the tensor's own rounding: 2^-22 / eps for the 16-bit types."""
    return 2.0 ** -22 / EPS[dtype]


def _xha(u, ua, mu, rs, dtype):
    """The magnitude of the normalised value xh = (u - mu) rs.  fp32 tensors: term by term, (|u| + |mu|) rs -- every rounding is a
    float32 rounding.  16-bit tensors: u - mu subtracts two float32 values and is good to float32, far below the 16-bit eps the bound
    is measured in, so it is ONE term, |u - mu| rs, plus the float32 error of u, mu and the subtraction in those units:
    kappa (|u| + |mu| + mean|u|) rs.  (Term by term, a row of 100 + randn or a constant row would have a bound hundreds of times its
    values, and a 16-bit check of it would see nothing.)"""
    if dtype == F32:
        return (ua + mu.abs()) * rs
    return ((u - mu).abs() + _kappa(dtype) * (ua + mu.abs() + ua.mean(1, keepdim=True))) * rs


def _gpa(h, Phi, phi, dtype):
    """The magnitude of gelu'(h) = Phi + h phi: fp32 term by term (0.5 (1 + |erf|): the sum cancels for h << 0); 16-bit: the value's
    own terms plus the float32 (or rational-erf) error of Phi, 2^-22, in units of eps."""
    return (_gelu_abs(h) if dtype == F32 else Phi + _kappa(dtype)) + h.abs() * phi


def _gelu(h, tanh=False):
    """-> (Phi, phi): the Gaussian cdf and pdf at h (tanh: the tanh approximation's cdf)."""
    if tanh:
        Phi = 0.5 * (1 + torch.tanh(0.7978845608028654 * (h + 0.044715 * h * h * h)))
    else:
        Phi = 0.5 * (1 + torch.erf(h * INV_SQRT2))
    return Phi, torch.exp(-0.5 * h * h) * INV_SQRT_2PI


def _stats64(u, ua, eps):
    mu = u.mean(1, keepdim=True)
    var = ((u - mu) ** 2).mean(1, keepdim=True)
    return mu, 1 / torch.sqrt(var + eps), ua.mean(1)


def _stats32(u, eps, cols):
    mu = u.sum(1, keepdim=True) / cols
    var = ((u - mu) * (u - mu)).sum(1, keepdim=True) / cols
    return mu, 1.0 / torch.sqrt(var + eps)


def _ln_bwd64(gy, xh, xha, rs):
    """The LayerNorm input gradient rs (gy - mean gy - xh mean(gy xh)) and its magnitude bound, float64."""
    gya = gy.abs()
    t = rs * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    ta = rs * (gya + gya.mean(1, keepdim=True) + xha * (gya * xha).mean(1, keepdim=True))
    return t, ta


def _ln_abs64(va, xha, rs):
    """The same map applied to a non-negative perturbation va with absolute values throughout."""
    return rs * (va + va.mean(1, keepdim=True) + xha * (va * xha).mean(1, keepdim=True))


def _ln_bwd32(gy, xh, rs, cols):
    s1 = gy.sum(1, keepdim=True) / cols
    s2 = (gy * xh).sum(1, keepdim=True) / cols
    return rs * (gy - s1 - xh * s2)


def _acc(v, prev, bd=None):
    """Add the gradient's previous content (accumulate); with bd: also widen the bound by |prev|."""
    if prev is None:
        return v if bd is None else (v, bd)
    p = prev.to(v.dtype)
    return v + p if bd is None else (v + p, bd + p.abs())


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_reference(x, gamma, beta, eps, gelu=False):
    """-> (ref, bound): ref = dict(y [rows, cols], mean, rstd [rows]) in float64; bound: y -> |xh| |gamma| + |beta| with |xh| as _xha
    gives it for x's dtype, u = x or gelu(x); mean -> mean|u| (the scale its absolute error is measured in)."""
    h, g, b = x.double(), gamma.double(), beta.double()
    if gelu:
        Phi, _ = _gelu(h)
        u, ua = h * Phi, h.abs() * _gelu_abs(h)
    else:
        u, ua = h, h.abs()
    mu, rs, am = _stats64(u, ua, eps)
    return (dict(y=(u - mu) * rs * g + b, mean=mu[:, 0], rstd=rs[:, 0]),
            dict(y=_xha(u, ua, mu, rs, x.dtype) * g.abs() + b.abs(), mean=am))


def ln_bwd_reference(dy, x, gamma, mean, rstd, gelu=False, dres=None, prev=None, want_dbias=False):
    """The backward of the STORED mean / rstd (the kernel is handed the forward's fp32 statistics) -> (ref, bound), float64:
    xh = (u - mean) rstd;  t = rstd (dy g - mean(dy g) - xh mean(dy g xh)) [* gelu'(x)];  dx = t + dres;
    dgamma = sum_rows dy xh;  dbeta = sum_rows dy;  dbias = sum_rows t;  prev = (dgamma, dbeta, dbias) already in the gradients."""
    d, h, g = dy.double(), x.double(), gamma.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    if gelu:
        Phi, phi = _gelu(h)
        u, ua, gp, gpa = h * Phi, h.abs() * _gelu_abs(h), Phi + h * phi, _gpa(h, Phi, phi, x.dtype)
    else:
        u, ua, gp, gpa = h, h.abs(), 1.0, 1.0
    xh, xha = (u - mu) * rs, _xha(u, ua, mu, rs, x.dtype)
    t, ta = _ln_bwd64(d * g, xh, xha, rs)
    t, ta = t * gp, ta * gpa
    prev = prev or (None, None, None)
    ref, bd = {}, {}
    ref["dx"], bd["dx"] = (t, ta) if dres is None else (t + dres.double(), ta + dres.double().abs())
    ref["dgamma"], bd["dgamma"] = _acc((d * xh).sum(0), prev[0], (d.abs() * xha).sum(0))
    ref["dbeta"], bd["dbeta"] = _acc(d.sum(0), prev[1], d.abs().sum(0))
    if gelu and want_dbias:
        ref["dbias"], bd["dbias"] = _acc(t.sum(0), prev[2], ta.sum(0))
    return ref, bd


LN_FWD_MUTATIONS = ("drop_last_vector", "padded_mean", "one_pass_variance", "no_eps", "tanh_gelu")
LN_BWD_MUTATIONS = ("gamma_no_part_offset", "drop_last_live_row", "stale_ring_slot", "no_dres", "accumulate_overwrites",
                    "dbias_before_gelu", "gelu_no_xphi")


def ln_emulate(x, gamma, beta, eps, dtype, gelu=False, mutation=None):
    """float32 with the kernel's single rounding -> dict(y of dtype, mean, rstd fp32)."""
    assert mutation is None or mutation in LN_FWD_MUTATIONS, mutation
    N, cols = NVEC[dtype], x.shape[1]
    h, g, b = x.float(), gamma.float(), beta.float()
    u = h * _gelu(h, mutation == "tanh_gelu")[0] if gelu else h
    keep = torch.ones(cols, dtype=F32, device=x.device)
    if mutation == "drop_last_vector":
        keep[cols - N:] = 0
    width = cdiv(cols, 64 * N) * 64 * N if mutation == "padded_mean" else cols
    mu = (u * keep).sum(1, keepdim=True) / width
    if mutation == "one_pass_variance":
        var = (u * u * keep).sum(1, keepdim=True) / cols - mu * mu
    else:
        var = ((u - mu) * (u - mu) * keep).sum(1, keepdim=True) / cols
    rs = 1.0 / torch.sqrt(var + (0.0 if mutation == "no_eps" else eps))
    return dict(y=((u - mu) * rs * g + b).to(dtype), mean=mu[:, 0], rstd=rs[:, 0])


def ln_bwd_emulate(dy, x, gamma, mean, rstd, dtype, gelu=False, dres=None, prev=None, want_dbias=False, mutation=None):
    """float32; dx, dgamma, dbeta, dbias each rounded once to dtype.  The route (waves per row, rows per block) matters to three of the
    mutations only."""
    assert mutation is None or mutation in LN_BWD_MUTATIONS, mutation
    rows, cols = x.shape
    route = ln_bwd_route(cols // NVEC[dtype], gelu)
    d, h, g = dy.float(), x.float(), gamma.float()
    mu, rs = mean.float()[:, None], rstd.float()[:, None]
    if mutation == "gamma_no_part_offset" and route.wpr > 1:
        g = g[:cols // route.wpr].repeat(route.wpr)
    sweep = LN_BLOCKS * route.rpb
    if mutation == "stale_ring_slot" and rows > sweep:               # the second sweep works on the first sweep's vectors
        d, h = d.clone(), h.clone()
        d[sweep:], h[sweep:] = dy.float()[:rows - sweep], x.float()[:rows - sweep]
    if gelu:
        Phi, phi = _gelu(h)
        u, gp = h * Phi, (Phi if mutation == "gelu_no_xphi" else Phi + h * phi)
    else:
        u, gp = h, 1.0
    xh = (u - mu) * rs
    t0 = _ln_bwd32(d * g, xh, rs, cols)
    t = t0 * gp
    dx = t if (dres is None or mutation == "no_dres") else t + dres.float()
    live = torch.ones(rows, 1, dtype=F32, device=x.device)
    if mutation == "drop_last_live_row":
        live[rows - 1] = 0
        if route.rpb - 1 < rows:
            live[route.rpb - 1] = 0
    prev = (None, None, None) if (prev is None or mutation == "accumulate_overwrites") else prev
    out = dict(dx=dx.to(dtype), dgamma=_acc((d * xh * live).sum(0), prev[0]).to(dtype), dbeta=_acc((d * live).sum(0), prev[1]).to(dtype))
    if gelu and want_dbias:
        out["dbias"] = _acc(((t0 if mutation == "dbias_before_gelu" else t) * live).sum(0), prev[2]).to(dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------- residual join
JOIN_GRADS = ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b", "dx_colsum")


def join_reference(c, own):
    """c: the case's tensors (build_join); own: dict(y[, dres]) -- the kernel's (or the emulation's) OWN stored y and dres, the inputs of
    the later stages.  -> (ref, bound) in float64 over y, ydrop, z, dres, dx, JOIN_GRADS and the statistics mean_a, rstd_a, mean_b, rstd_b.
      y      = res + m s LN_a(x)                 from x; the LN_a rounding adds m s |LN_a(x)| to the bound        (s = 1 / (1 - p))
      ydrop  = y - res at the dropped elements   bound 0: exactly the residual (exactly 0 without one)
      z, mean_b, rstd_b = LN_b of own y
      dres   = rstd_b (dz gb - mean(dz gb) - yh mean(dz gb yh)) + dy          yh from own y
      dx     = LN_a-backward(g1), g1 = m s dres  from own dres (want_dres=False: from the dres above, its bound as one more rounding);
               the rounding of g1 adds |g1|; without LN_a dx = g1 and its bound is |g1|: exactly 0 at a dropped element
      dgamma_a = sum g1 xh_a, dbeta_a = sum g1, dgamma_b = sum dz yh, dbeta_b = sum dz, dx_colsum = sum dx    (+ prev);
               without LN_a and with p > 0 the summands of dx_colsum are the rounded dx themselves: sum |g1| more in its bound."""
    x = c["x"].double()
    rows, cols = x.shape
    eps, p = c["eps"], c["p"]
    s = 1.0 / (1.0 - p) if p > 0 else 1.0
    m = c["mask"].double() if p > 0 else torch.ones_like(x)
    res = c["res"].double() if c["res"] is not None else torch.zeros_like(x)
    has_a, has_b = c["ga"] is not None, c["gb"] is not None
    ref, bd = {}, {}
    if has_a:
        ga, ba = c["ga"].double(), c["ba"].double()
        mu_a, rs_a, am = _stats64(x, x.abs(), eps)
        xh, xha = (x - mu_a) * rs_a, _xha(x, x.abs(), mu_a, rs_a, c["x"].dtype)
        a, abd = xh * ga + ba, xha * ga.abs() + ba.abs()
        abd = abd + a.abs()                                            # the stored LN_a output: one rounding
        ref["mean_a"], ref["rstd_a"], bd["mean_a"] = mu_a[:, 0], rs_a[:, 0], am
    else:
        a, abd = x, x.abs()
    ref["y"], bd["y"] = res + m * s * a, res.abs() + m * s * abd
    yk = own["y"].double()
    ref["ydrop"], bd["ydrop"] = torch.zeros_like(x), torch.zeros_like(x)
    dy = c["dy"].double() if c["dy"] is not None else torch.zeros_like(x)
    if has_b:
        gb, bb, dz = c["gb"].double(), c["bb"].double(), c["dz"].double()
        mu_b, rs_b, bm = _stats64(yk, yk.abs(), eps)
        yh, yha = (yk - mu_b) * rs_b, _xha(yk, yk.abs(), mu_b, rs_b, c["x"].dtype)
        ref["mean_b"], ref["rstd_b"], bd["mean_b"] = mu_b[:, 0], rs_b[:, 0], bm
        ref["z"], bd["z"] = yh * gb + bb, yha * gb.abs() + bb.abs()
        t, ta = _ln_bwd64(dz * gb, yh, yha, rs_b)
        g0, g0bd = t + dy, ta + dy.abs()
        ref["dgamma_b"], bd["dgamma_b"] = (dz * yh).sum(0), (dz.abs() * yha).sum(0)
        ref["dbeta_b"], bd["dbeta_b"] = dz.sum(0), dz.abs().sum(0)
    else:
        g0, g0bd = dy, dy.abs()
    if c["want_dres"]:
        ref["dres"], bd["dres"] = g0, g0bd
        gin, gin_x = own["dres"].double(), torch.zeros_like(x)
    else:
        gin, gin_x = g0, (g0bd if has_b else torch.zeros_like(x))
    g1, g1_x = m * s * gin, m * s * gin_x
    if has_a:
        extra = g1_x + (g1.abs() if p > 0 else 0.0)                     # the stored dropout gradient: one rounding
        ref["dx"], _ = _ln_bwd64(g1 * ga, xh, xha, rs_a)
        bd["dx"] = _ln_abs64((g1.abs() + extra) * ga.abs(), xha, rs_a)
        ref["dgamma_a"], bd["dgamma_a"] = (g1 * xh).sum(0), ((g1.abs() + extra) * xha).sum(0)
        ref["dbeta_a"], bd["dbeta_a"] = g1.sum(0), (g1.abs() + extra).sum(0)
    else:
        ref["dx"], bd["dx"] = g1, g1.abs() + g1_x
    if c["want_xsum"]:
        ref["dx_colsum"], bd["dx_colsum"] = ref["dx"].sum(0), bd["dx"].sum(0)
        if not has_a and p > 0:                                         # the STORED dropout gradients are summed: one rounding per row
            bd["dx_colsum"] = bd["dx_colsum"] + g1.abs().sum(0)
    for i, n in enumerate(JOIN_GRADS):
        if n in ref and c["prev"][i] is not None:
            ref[n], bd[n] = _acc(ref[n], c["prev"][i], bd[n])
    return ref, bd


JOIN_MUTATIONS = ("no_scale", "mask_shift", "dropout_before_lna", "dres_missing_dy", "dres_dropped", "colsum_before_lna",
                  "ignore_residual", "stats_b_unrounded")


def join_emulate(c, dtype, mutation=None):
    """float32 with join.hip's rounding points (LN_a output, y, the gradient of y, the dropout gradient, every output once)
    -> dict over y, z, dres, dx, JOIN_GRADS + mean_a, rstd_a, mean_b, rstd_b."""
    assert mutation is None or mutation in JOIN_MUTATIONS, mutation
    R = lambda v: v.to(dtype).float()                                    # noqa: E731
    x = c["x"].float()
    rows, cols = x.shape
    eps, p = c["eps"], c["p"]
    drop = p > 0
    m = c["mask"] if drop else None
    if drop and mutation == "mask_shift":
        m = torch.roll(m.flatten(), NVEC[dtype]).view(rows, cols)
    s = float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))) if drop else 1.0
    if mutation == "no_scale":
        s = 1.0
    dropped = lambda v: torch.where(m, v * s, torch.zeros_like(v)) if drop else v          # noqa: E731
    res = c["res"].float() if (c["res"] is not None and mutation != "ignore_residual") else torch.zeros_like(x)
    has_a, has_b = c["ga"] is not None, c["gb"] is not None
    out = {}
    xa = dropped(x) if mutation == "dropout_before_lna" else x
    if has_a:
        ga, ba = c["ga"].float(), c["ba"].float()
        mu_a, rs_a = _stats32(xa, eps, cols)
        a = R((xa - mu_a) * rs_a * ga + ba)
        out["mean_a"], out["rstd_a"] = mu_a[:, 0], rs_a[:, 0]
    else:
        a = xa
    ysum = (a if mutation == "dropout_before_lna" else dropped(a)) + res
    y = R(ysum)
    out["y"] = y.to(dtype)
    g = c["dy"].float() if c["dy"] is not None else torch.zeros_like(x)
    if has_b:
        gb, bb, dz = c["gb"].float(), c["bb"].float(), c["dz"].float()
        mu_b, rs_b = _stats32(ysum if mutation == "stats_b_unrounded" else y, eps, cols)
        out["mean_b"], out["rstd_b"] = mu_b[:, 0], rs_b[:, 0]
        yh = (y - mu_b) * rs_b
        out["z"] = (yh * gb + bb).to(dtype)
        g = R(_ln_bwd32(dz * gb, yh, rs_b, cols) + (0.0 if mutation == "dres_missing_dy" else g))
        out["dgamma_b"], out["dbeta_b"] = (dz * yh).sum(0), dz.sum(0)
    if c["want_dres"]:
        out["dres"] = (R(dropped(g)) if mutation == "dres_dropped" else g).to(dtype)
    if drop:
        g = R(dropped(g))
    g1 = g
    if has_a:
        xh = (x - mu_a) * rs_a
        out["dgamma_a"], out["dbeta_a"] = (g * xh).sum(0), g.sum(0)
        g = _ln_bwd32(g * ga, xh, rs_a, cols)
    out["dx"] = g.to(dtype)
    if c["want_xsum"]:
        out["dx_colsum"] = (g1 if mutation == "colsum_before_lna" else g).sum(0)
    for i, n in enumerate(JOIN_GRADS):
        if n in out:
            out[n] = _acc(out[n], c["prev"][i]).to(c["prev"][i].dtype if c["prev"][i] is not None else dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------- figures
def ln_fwd_figures(b, got, dtype):
    ref, bd = ln_reference(b["x"], b["gamma"], b["beta"], b["eps"], b["gelu"])
    return dict(y=grad_excess(got["y"], ref["y"], bd["y"], dtype), mean=scalar_err(got["mean"], ref["mean"], bd["mean"]),
                rstd=scalar_err(got["rstd"], ref["rstd"]))


def ln_bwd_figures(b, got, dtype):
    ref, bd = ln_bwd_reference(b["dy"], b["x"], b["gamma"], b["mean"], b["rstd"], b["gelu"], b["dres"], b["prev"], b["want_dbias"])
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return {n: grad_excess(got[n], ref[n], bd[n], dtype) for n in ref}


def join_figures(c, got, dtype):
    """got: the kernel's (or emulation's) outputs by name, statistics as mean_a ... rstd_b."""
    ref, bd = join_reference(c, got)
    fig = {}
    for n in ref:
        if n == "ydrop":
            kept = c["mask"] if c["p"] > 0 else torch.ones_like(c["x"], dtype=torch.bool)
            base = c["res"].double() if c["res"] is not None else 0.0
            d = torch.where(kept, torch.zeros_like(ref[n]), got["y"].double() - base)
            fig[n] = 0.0 if excess(d, ref[n], bd[n], 1.0) == 0.0 else float("inf")
        elif n.startswith("mean"):
            fig[n] = scalar_err(got[n], ref[n], bd[n])
        elif n.startswith("rstd"):
            fig[n] = scalar_err(got[n], ref[n])
        else:
            fig[n] = grad_excess(got[n], ref[n], bd[n], got[n].dtype if n in JOIN_GRADS else dtype)
    return fig


# ---------------------------------------------------------------------------------------------------------------- inputs
def _seam_cols(cols, N, parts=1):
    """The planted columns: row ends, both sides of the last vector's edge, of the first 64-lane slab's edge and of every part seam."""
    cand = [0, cols - 1, cols - N, cols - N - 1, 64 * N - 1, 64 * N]
    cpp = cols // parts
    for k in range(1, parts):
        cand += [k * cpp - 1, k * cpp]
    out = []
    for c in cand:
        if 0 <= c < cols and c not in out:
            out.append(c)
    return out


def _x_rows(regime, rows, cols, N, gen, parts=1):
    x = torch.randn(rows, cols, generator=gen)
    if regime == "offset":
        x = x + 100.0
    elif regime == "pcol":
        seams = _seam_cols(cols, N, parts)
        for r in range(rows):
            x[r, seams[r % len(seams)]] = PLANT
    if rows >= 3:
        x[1] = CONST
    return x


def _g_rows(regime, rows, cols, gen, seam_row):
    d = torch.randn(rows, cols, generator=gen)
    if regime == "prow":
        d[seam_row] += PLANT
    return d


def _params(cols, dtype, gen):
    return (1 + 0.1 * torch.randn(cols, generator=gen)).to(dtype), (0.1 * torch.randn(cols, generator=gen)).to(dtype)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ---- LayerNorm forward
LNF = namedtuple("LNF", "name m rows gelu regime eps seed")
FWD_M = (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)       # both sides of every NV boundary, one vector, the widest row
FWD_REFUSED_M = 2049


def _ln_fwd_cases():
    out = []
    for i, m in enumerate(FWD_M):
        for gelu in (False, True):
            for j, regime in enumerate(REGIMES[:3]):
                rows = (1, 3, 5)[(i + j + gelu) % 3]
                out.append(LNF(f"fwd NV{ln_fwd_nv(m)} m{m} rows{rows} {'gelu ' if gelu else ''}{regime}", m, rows, gelu, regime,
                               (1e-5, 1e-3)[(i + j) % 2], 1000 + 10 * i + 2 * j + gelu))
    return out


LN_FWD_CASES = _ln_fwd_cases()


def build_ln_fwd(case, dtype, device="cpu"):
    N = NVEC[dtype]
    cols, gen = case.m * N, _gen(case.seed)
    x = _x_rows(case.regime, case.rows, cols, N, gen).to(dtype)
    gamma, beta = _params(cols, dtype, gen)
    return dict(x=x.to(device), gamma=gamma.to(device), beta=beta.to(device), eps=case.eps, gelu=case.gelu)


# ---- LayerNorm backward
LNB = namedtuple("LNB", "name m rows gelu regime seam_row dres dbias acc eps seed")
# every (NV, WPR) ln_bwd_dispatch can launch, by the smallest m that reaches it (16-bit columns = 8 m):
#   plain  WPR1: NV1 m<=64, NV2 65..128, NV4 129 (odd m: no even split), NV8 511      WPR2: NV2 130 (ragged 65-vector parts) / 256, NV4 258, NV8 514
#          WPR4: NV2 384 / 512, NV4 516, NV8 1028       WPR8: NV2 1024, NV4 2048, NV8 4096 (wider than the forward takes: statistics supplied)
#   GELU   WPR1: NV1 64, NV2 65, NV4 129, NV8 511       WPR2: NV1 96, NV2 130, NV4 258, NV8 514       WPR4: NV1 256, NV2 260, NV4 516, NV8 1028
#          WPR8: NV1 512, NV2 1024, NV4 2048, NV8 4096  WPR6 (12-wave blocks, ring depth 2): m = 384 exactly
#   never launched: plain NV1 with WPR > 1 (a row is split only past two vectors per lane) and with it the ring depth 1.
PLAIN_M = (1, 63, 64, 65, 128, 129, 511, 130, 256, 258, 514, 384, 512, 516, 1028, 1024, 2048, 4096)
GELU_M = (1, 64, 65, 129, 511, 96, 130, 258, 514, 256, 260, 516, 1028, 384, 512, 1024, 2048, 4096)
BWD_REFUSED_M = 513
ROW_SWEEP = ((False, 1), (False, 130), (False, 384), (False, 1024), (True, 96), (True, 384), (True, 512))      # (gelu, m): one per WPR


def _ln_bwd_cases():
    out, i = [], 0

    def add(m, rows, gelu, regime, seam_row, dres, dbias, acc, what):
        nonlocal i
        r = ln_bwd_route(m, gelu)
        out.append(LNB(f"bwd {'gelu ' if gelu else ''}WPR{r.wpr} NV{r.nv} m{m} rows{rows} {regime} {what}".strip(), m, rows, gelu, regime,
                       seam_row, dres and not gelu, dbias and gelu, acc, (1e-5, 1e-3)[i % 2], 2000 + i))
        i += 1

    for j, m in enumerate(PLAIN_M):
        rpb = ln_bwd_route(m, False).rpb
        add(m, rpb + 1, False, REGIMES[j % 4], rpb, j % 2 == 0, False, j % 3 == 0, "shape")
    for j, m in enumerate(GELU_M):
        rpb = ln_bwd_route(m, True).rpb
        for dbias in (False, True):
            add(m, rpb + 1, True, REGIMES[(j + dbias) % 4], rpb - 1, False, dbias, (j + dbias) % 3 == 0, "shape")
    for gelu, m in ROW_SWEEP:
        r = ln_bwd_route(m, gelu)
        sweep = LN_BLOCKS * r.rpb
        for rows in sorted({1, r.rpb - 1, r.rpb + 1, sweep + 1} - {0}):
            add(m, rows, gelu, "prow", rows - 1, rows % 2 == 1, True, rows == sweep + 1, "rows: last row planted")
        add(m, r.rpb + 1, gelu, "prow", r.rpb - 1, True, True, True, "rows: last row of the first block iteration planted")
        if r.pf:                                                       # the prefetch ring: niter = 3 (odd tail) besides 1 and 2 above
            add(m, 2 * sweep + 1, gelu, "prow", 2 * sweep, False, True, False, "rows: niter 3")
            add(m, 2 * sweep + 1, gelu, "randn", 0, False, False, True, "rows: niter 3")
    # (GELU WPR1 NV2: over the 17 rows of its shape case dbias cancels to a fifth of its bound; two rows show its rounding)
    add(65, 2, True, "randn", 1, False, True, False, "dbias: two rows")
    return out


LN_BWD_CASES = _ln_bwd_cases()


def build_ln_bwd(case, dtype, device="cpu"):
    N = NVEC[dtype]
    cols, gen = case.m * N, _gen(case.seed)
    route = ln_bwd_route(case.m, case.gelu)
    x = _x_rows(case.regime, case.rows, cols, N, gen, route.wpr).to(dtype)
    gamma, _ = _params(cols, dtype, gen)
    dy = _g_rows(case.regime, case.rows, cols, gen, case.seam_row).to(dtype)
    dres = torch.randn(case.rows, cols, generator=gen).to(dtype) if case.dres else None
    prev = None
    if case.acc:
        prev = tuple((0.1 * torch.randn(cols, generator=gen)).to(dtype).to(device) for _ in range(3))
        if not case.dbias:
            prev = prev[:2] + (None,)
    x = x.to(device)
    gamma = gamma.to(device)
    st, _ = ln_reference(x, gamma, torch.zeros_like(gamma), case.eps, case.gelu)          # the stored statistics: fp32 of the float64 ones
    return dict(x=x, gamma=gamma, dy=dy.to(device), dres=dres.to(device) if dres is not None else None, prev=prev,
                mean=st["mean"].float(), rstd=st["rstd"].float(), gelu=case.gelu, want_dbias=case.dbias, eps=case.eps)


# ---- residual join
JC = namedtuple("JC", "name cols m rows a b p res dy want_dres xsum keep base regime eps seed")
# cols > 0: absolute columns (the row-per-wave shapes 256 k; fp32 takes the same columns through the split-row kernels);
# cols == 0: m vectors.  Split-row shapes, 16-bit columns = 8 m: m 1 and 33 (WPR 1, forward NV 1), 66 (WPR 2, ragged 33-vector parts,
# NV 2), 228 (WPR 4, ragged 57, NV 4), 264 (WPR 8, ragged 33, NV 8), 512 (WPR 8, full).  520 and 1800 columns, which the issue lists
# for the split-row kernel, are REFUSED by join_check (65 and 225 vectors do not split over 2 and 4 waves): they sit in JOIN_REFUSED.
SPLIT_M = (1, 33, 66, 228, 264, 512)
JOIN_REFUSED = ((BF16, 1032), (BF16, 520), (FP16, 1800), (BF16, 64 * 8 * 8 + 8), (FP16, 64 * 8 * 8 + 8), (F32, 64 * 4 * 8 + 4), (F32, 516),
                (BF16, 12), (F32, 6))
ABP = tuple((a, b, p) for a in (False, True) for b in (False, True) for p in (0.0, 0.1))


def _join_cases():
    out, i = [], 0

    def add(what, cols=0, m=0, rows=7, a=True, b=True, p=0.1, res=True, dy=True, want_dres=True, xsum=False, keep=True, base=0,
            regime=None):
        nonlocal i
        regime = regime or REGIMES[i % 4]
        out.append(JC(f"join {'cols' + str(cols) if cols else 'm' + str(m)} rows{rows} a{int(a)} b{int(b)} p{p} {regime} {what}", cols, m, rows,
                      a, b, p, res, dy, want_dres, xsum, keep, base, regime, (1e-5, 1e-3)[i % 2], 3000 + i))
        i += 1

    for k in (1, 2, 3, 4):                                             # all eight (LN_a, LN_b, p > 0) at every row-per-wave backward shape
        for j, (a, b, p) in enumerate(ABP):
            add("flags", cols=256 * k, rows=(7, 1, 9)[(j + k) % 3], a=a, b=b, p=p, xsum=j % 4 in (0, 3))
    for k in (5, 6):                                                   # forward row-per-wave (RowMap<2,true>, <3,false>), backward split-row
        add("fwd row / bwd split", cols=256 * k, p=0.1)
        add("fwd row / bwd split", cols=256 * k, a=False, p=0.0, rows=5)
    for k in (1, 3):                                                   # keep = None with p > 0: the split-row kernel regenerates the mask
        add("keep=None", cols=256 * k, keep=False, rows=9)
    for j, m in enumerate(SPLIT_M):
        add("split", m=m, rows=(7, 13)[j % 2], p=0.1, xsum=True)
        add("split", m=m, a=j % 2 == 0, b=j % 2 == 1, p=(0.0, 0.3)[j % 2], rows=5)
    for cols, m in ((512, 0), (0, 66)):                                # the flag space, on a row-per-wave and on a split-row shape
        add("dy=None", cols=cols, m=m, dy=False)
        add("residual=None", cols=cols, m=m, res=False)
        add("residual=None", cols=cols, m=m, res=False, a=False, b=False)
        add("want_dres=False", cols=cols, m=m, want_dres=False)
        add("want_dres=False", cols=cols, m=m, want_dres=False, a=False)
        add("dx_colsum", cols=cols, m=m, xsum=True, b=False)
        add("offset_base", cols=cols, m=m, base=12345)
    add("rows", cols=256, rows=4097, regime="prow", xsum=True)            # three persistent iterations in flight (DIST 2)
    add("rows", cols=512, rows=4097, a=False, regime="prow")
    add("rows", cols=768, rows=2049, regime="prow")                       # both LayerNorms at 768: one row ahead
    add("rows", cols=1024, rows=2049, regime="prow", xsum=True)           # both LayerNorms at 1024: 4-wave blocks
    add("rows", cols=1024, rows=2049, b=False, regime="randn")            # 1024 with one LayerNorm: 8 waves, one row ahead
    add("rows", m=66, rows=256 * 6 + 1, regime="prow", xsum=True)         # split-row WPR 2: one live row in the second sweep
    add("rows", m=1, rows=256 * 12 + 1, regime="prow")
    return out


JOIN_CASES = _join_cases()
SEED, OFFSET = 1234, 77                                                 # the Philox stream position of every join case


def join_cols(case, dtype):
    return case.cols if case.cols else case.m * NVEC[dtype]


def build_join(case, dtype, mask=None, device="cpu"):
    """mask: bool [rows, cols] for p > 0 (the stand-alone dropout kernel's on the GPU); None: drawn here from the case's generator."""
    N = NVEC[dtype]
    cols, rows, gen = join_cols(case, dtype), case.rows, _gen(case.seed)
    r = join_route(cols, dtype, True, case.keep)
    x = _x_rows(case.regime, rows, cols, N, gen, max(1, r.wpr)).to(dtype)
    res = torch.randn(rows, cols, generator=gen).to(dtype) if case.res else None
    ga, ba = _params(cols, dtype, gen) if case.a else (None, None)
    gb, bb = _params(cols, dtype, gen) if case.b else (None, None)
    seam = rows - 1
    dy = _g_rows(case.regime, rows, cols, gen, seam).to(dtype) if (case.dy or not case.b) else None
    dz = _g_rows(case.regime, rows, cols, gen, seam).to(dtype) if case.b else None
    drawn = torch.rand(rows, cols, generator=gen) >= case.p
    prev = [(0.1 * torch.randn(cols, generator=gen)).to(dtype) for _ in range(5)]
    on = (case.a, case.a, case.b, case.b, case.xsum)
    dev = lambda t: t.to(device) if t is not None else None               # noqa: E731
    return dict(x=dev(x), res=dev(res), ga=dev(ga), ba=dev(ba), gb=dev(gb), bb=dev(bb), dy=dev(dy), dz=dev(dz), eps=case.eps, p=case.p,
                mask=(dev(mask if mask is not None else drawn) if case.p > 0 else None), prev=[dev(t) if o else None for t, o in zip(prev, on)],
                want_dres=case.want_dres, want_xsum=case.xsum)


def forced_join_cases():
    """The reduced table of the forced forms (debug library): one case per k and flag combination, at 1, 7 and 2049 rows."""
    out = []
    for k in (1, 2, 3, 4):
        for j, (a, b, p) in enumerate(ABP):
            rows = (1, 7, 2049)[(j + k) % 3]
            out.append(JC(f"forced cols{256 * k} rows{rows} a{int(a)} b{int(b)} p{p}", 256 * k, 0, rows, a, b, p, True, True, True, j % 2 == 1,
                          True, 0, REGIMES[(j + k) % 4], (1e-5, 1e-3)[j % 2], 4000 + 8 * k + j))
    return out


FORCED_FORMS = (("0", "0"), ("1", "0"), ("1", "1"), ("1", "2"), ("1", "3"))     # (OFA_JOIN_FWD, OFA_JOIN_BWD): tools/join_bench.py's + (1, 0)


def keep_share_ok(mask, p):
    """The kept share within 5 standard deviations of 1 - p."""
    n = mask.numel()
    return abs(float(mask.double().mean()) - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n) + 1e-12
