"""A plain-torch oracle for the QuickGELU kernels (csrc/quick_gelu.hip) and the ViT backbone (ofasys_amd/module/vit.py): no GPU needed, no
dependency on the kernels.

qgelu_reference()  float64 on the stored (already rounded) inputs: a = h s, dh = dy s (1 + 1.702 h (1 - s)), s = sigmoid(1.702 h), and the
                   column sums of dh -- each output with its componentwise magnitude bound: |h| s; |dy| (s + 1.702 |h| s (1 - s)), with
                   absolute values because 1 + 1.702 h (1 - s) cancels for negative h; sum |dh|.
qgelu_emulate()    the same arithmetic in float32 with ONE rounding of each result and the kernel's summation order of the column sums
                   (lane sums over rows w, w + 4, ... of a slab of ROWS_PER_BLOCK rows, the four added in order, slabs added in order),
                   nothing else of the kernel; can apply one named mutation (MUTATIONS).
excess()           max (|got - ref| - floor) / bound in units of the 16-bit eps (fp32: error / bound); the floor is what an underflow may
                   cost: 2^-126 for bf16 (and fp32), 2^-24 for fp16.  Where the bound is 0 the output must be exactly 0.
vit_backbone()     a restatement of the backbone (patch projection, positions -- resized bilinearly for another grid --, ln_pre, pre-LN
                   blocks with a packed q|k|v projection and a QuickGELU MLP) on batch-major rows, in the dtype of its inputs (float64 in
                   the tests), from a state dict with the reference's keys.

Inputs come from a CPU generator in four regimes: `randn` (h = 3 randn), `sweep` (h evenly spaced over [-12, 12]), `sat` (h in +-30,
+-80, +-0 by vector: the output is exactly h for the positive ones, exactly 0 for the zeros, and within the floor of 0 for the negative
ones) and `prow` (dy = 64 + randn in the last row -- a slab seam for the row counts of the table -- which then carries the column sums).
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

F64, F32, BF16, FP16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
EPS = {BF16: 2.0 ** -8, FP16: 2.0 ** -11}
NVEC = {F32: 4, BF16: 8, FP16: 8}                     # elements of a 16-byte vector
CODE = {F32: 0, BF16: 1, FP16: 2}                     # ofa_dtype
DTYPES3 = (F32, BF16, FP16)
NAMES = {F32: "fp32", BF16: "bf16", FP16: "fp16"}
K = 1.702
ROWS_PER_BLOCK = 32                                   # rows of one backward slab (up to 8192 rows); 4 waves share them
WAVES = 4
SAT = (30.0, -30.0, 80.0, -80.0, 0.0, -0.0)
REGIMES = ("randn", "sweep", "sat", "prow")
OUTPUTS = ("a", "dh", "colsum")

# ---------------------------------------------------------------------------------------------------------------- measured constants
# CEILING: the cap on excess(emulate, reference, bound) over the whole table (every shape, regime, bf16 and fp16).  The emulation rounds
# an output once -- at most one eps relative to the value, which is at most the bound -- and its float32 work before that is ~1e-6 of the
# bound.  Measured 2026-10-20 on the CPU (tests/test_vit_cpu.py prints the figures with -s), worst excess over the table:
#          a        dh       colsum
#   bf16   0.996    0.996    0.997
#   fp16   0.991    0.999    0.996
# (arithmetic carried in the 16-bit type throughout reaches 15 to 4800; each mutation below exceeds 1 on some case.)
CEILING = 1.0
# TOL for the kernels = 2 * CEILING: the factor 2 covers what the emulation leaves out (v_exp_f32 / v_rcp_f32 instead of libm's exp and
# an IEEE division in the 16-bit kernels).  Never set from what a kernel produced.
TOL = 2.0 * CEILING
# fp32 tensors (the outputs of fp32 inputs; the fp32 partial rows of every dtype, judged by their sum over the slots): 8 x the largest
# error / bound of the emulation's float32 evaluation against float64.  Measured 2026-10-20 over the table, the emulation's worst:
#   fp32 inputs: a 1.46e-6, dh 1.44e-6 (both at h = -30: 1.702 h is rounded to fp32 before the exponential, |1.702 h| 2^-24 = 3e-6 of
#   the result), colsum 4.81e-5 (one row: the bound sum |dh| is |dh| itself, which cancels near the zero of the derivative at
#   h = -0.75 while dh's error does not)
#   partial rows: fp32 4.81e-5, bf16 1.65e-5, fp16 1.63e-4 (the same cancellation, on each dtype's own grid of inputs)
# The kernels themselves on an MI355X, 2026-10-20, worst over the same table (tests/test_vit_gpu.py prints them with -s):
#   bf16 a 0.996, dh 0.995, folded column sum 0.996 (the immediate column sum of the STORED dh, two roundings: 1.83); fp16 0.991 / 0.999 /
#   0.996 (1.87); fp32 a 1.35e-6, dh 1.34e-6, column sum 7.45e-5; partial rows fp32 7.45e-5, bf16 2.63e-5, fp16 1.74e-4
G32 = {"a": 8 * 1.5e-6, "dh": 8 * 1.5e-6, "colsum": 8 * 4.9e-5}
G32_PARTIAL = {F32: 8 * 4.9e-5, BF16: 8 * 1.7e-5, FP16: 8 * 1.7e-4}


def floor_of(dtype):
    return 2.0 ** -24 if dtype == FP16 else 2.0 ** -126


def excess(got, ref, bound, dtype):
    """16-bit dtype: in units of its eps; fp32: error / bound.  inf for a non-finite value or a non-zero where the bound is 0."""
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
    err = ((got - ref).abs() - floor_of(dtype)).clamp_min(0)
    return float((err[live] / bound[live]).max()) / EPS.get(dtype, 1.0)


def limit(name, dtype, kernel=True):
    """The largest figure output `name` (a, dh, colsum, partial) may show for inputs of `dtype`: the emulation's cap, or (kernel=True)
    what the GPU test allows a kernel.  The partial rows are fp32 tensors whatever the input dtype, judged as error / bound."""
    if name == "partial":
        return G32_PARTIAL[dtype] if kernel else G32_PARTIAL[dtype] / 8
    if dtype == F32:
        return G32[name] if kernel else G32[name] / 8
    return TOL if kernel else CEILING


def slots_of(rows):
    """Partial rows the backward writes for `rows` rows (restated; confirmed against ofa_quick_gelu_bwd_slots by the CPU test)."""
    return 0 if rows <= 0 else -(-rows // rows_per_block(rows))


def rows_per_block(rows):
    """32 up to 8192 rows, then as many (a multiple of the 4 waves) as keep the slab count at 256."""
    per = -(-rows // 256)
    return max(ROWS_PER_BLOCK, -(-per // WAVES) * WAVES)


# ---------------------------------------------------------------------------------------------------------------- reference / emulation
def qgelu_reference(h, dy):
    """-> {name: (value, bound)} in float64 for a, dh, colsum."""
    h, dy = h.double(), dy.double()
    a = K * h
    s, q = torch.sigmoid(a), torch.sigmoid(-a)
    dh = dy * s * (1 + a * q)
    dh_b = dy.abs() * (s + a.abs() * s * q)
    return {"a": (h * s, h.abs() * s), "dh": (dh, dh_b), "colsum": (dh.sum(0), dh.abs().sum(0))}


MUTATIONS = ("sigmoid_16bit", "const_1p7", "bwd_no_hterm", "colsum_skip_last_row")


def qgelu_emulate(h, dy, dtype, mutation=None):
    """-> {a, dh (dtype), colsum (dtype), partial (fp32 [slots, cols])}: float32 arithmetic, one rounding per output."""
    assert mutation is None or mutation in MUTATIONS, mutation
    h, dy = h.float(), dy.float()
    k = torch.tensor(1.7 if mutation == "const_1p7" else K, dtype=F32)
    t = k * h
    z = torch.exp(-t.abs())
    r = 1.0 / (1.0 + z)
    zr = z * r
    s, q = torch.where(t >= 0, r, zr), torch.where(t >= 0, zr, r)
    if mutation == "sigmoid_16bit":
        s, q = s.to(dtype).float(), q.to(dtype).float()
    a = h * s
    dh = dy * s if mutation == "bwd_no_hterm" else dy * s * (1.0 + t * q)
    rows, cols = h.shape
    ns, rpb = slots_of(rows), rows_per_block(rows)
    last = rows - 1 if mutation == "colsum_skip_last_row" else rows
    partial = torch.zeros(ns, cols, dtype=F32)
    for b in range(ns):
        lanes = []
        for w in range(WAVES):
            acc = torch.zeros(cols, dtype=F32)
            for rr in range(b * rpb + w, min((b + 1) * rpb, last), WAVES):
                acc = acc + dh[rr]
            lanes.append(acc)
        tot = lanes[0]
        for w in range(1, WAVES):
            tot = tot + lanes[w]
        partial[b] = tot
    colsum = torch.zeros(cols, dtype=F32)
    for b in range(ns):
        colsum = colsum + partial[b]
    return {"a": a.to(dtype), "dh": dh.to(dtype), "colsum": colsum.to(dtype), "partial": partial}


def figures(ref, got, dtype):
    """{output: excess} of a result dict (a, dh, colsum[, partial]) against qgelu_reference's; `partial` is judged by its sum over the
    slots as an fp32 tensor."""
    out = {n: excess(got[n], ref[n][0], ref[n][1], dtype) for n in OUTPUTS if n in got}
    if "partial" in got:
        out["partial"] = excess(got["partial"].double().sum(0), ref["colsum"][0], ref["colsum"][1], F32)
    return out


# ---------------------------------------------------------------------------------------------------------------- the table
QC = namedtuple("QC", "name m rows regime seed")
M = (1, 3, 64, 65, 384)                               # vectors per row: cols 8, 24, 512, 520, 3072 (16-bit); 4, 12, 256, 260, 1536 (fp32)
ROWS = (1, 3, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK + 1)
# The forward is a grid-stride kernel: at most FWD_GRID blocks of 256 threads, one 16-byte vector per thread and sweep.  SWEEP_ROWS rows of
# the widest shape are one row more than a full sweep (1366 x 384 = 524544 vectors already exceed 2048 x 256 = 524288): the loop's second
# iteration runs, in a ragged last sweep.  SLAB_ROWS is past the 8192 rows up to which a backward slab is 32 rows: 36-row slabs, 228 of
# them, a wave covering 9 rows, the last slab ragged.
FWD_GRID, FWD_BLOCK = 2048, 256
SWEEP_ROWS = -(-FWD_GRID * FWD_BLOCK // M[-1]) + 1
SLAB_ROWS = 8200
LARGE = ((M[-1], SWEEP_ROWS, "randn"), (M[0], SLAB_ROWS, "randn"), (M[0], SLAB_ROWS, "prow"))


def _cases():
    out = []
    for m in M:
        for rows in ROWS:
            for regime in REGIMES:
                out.append(QC(f"m{m} rows{rows} {regime}", m, rows, regime, 1000 + len(out)))
    for m, rows, regime in LARGE:
        out.append(QC(f"m{m} rows{rows} {regime}", m, rows, regime, 1000 + len(out)))
    return tuple(out)


CASES = _cases()


def build(case, dtype):
    """-> (h, dy) on the CPU, rounded to dtype."""
    g = torch.Generator().manual_seed(case.seed)
    N = NVEC[dtype]
    rows, cols = case.rows, case.m * N
    h = 3.0 * torch.randn(rows, cols, generator=g)
    dy = torch.randn(rows, cols, generator=g)
    if case.regime == "sweep":
        h = torch.linspace(-12.0, 12.0, rows * cols).view(rows, cols)
    elif case.regime == "sat":
        idx = (torch.arange(rows)[:, None] + torch.arange(cols)[None, :] // N) % len(SAT)
        h = torch.tensor(SAT)[idx]
    elif case.regime == "prow":
        dy[rows - 1] += 64.0
    return h.to(dtype), dy.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- the backbone, restated
def _ln(x, state, key):
    return F.layer_norm(x, (x.shape[-1],), state[key + ".weight"], state[key + ".bias"], 1e-5)


def quick_gelu(x):
    return x * torch.sigmoid(K * x)


def vit_block(state, prefix, x, heads):
    """One pre-LN block on [B, T, D] rows: x + out_proj(attention(ln_1 x)), then + c_proj(quick_gelu(c_fc(ln_2 .)))."""
    B, T, D = x.shape
    hd = D // heads
    n = _ln(x, state, prefix + "ln_1")
    qkv = n @ state[prefix + "attn.in_proj_weight"].t() + state[prefix + "attn.in_proj_bias"]
    q, k, v = (t.reshape(B, T, heads, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
    p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), dim=-1)
    a = (p @ v).transpose(1, 2).reshape(B, T, D)
    x = x + a @ state[prefix + "attn.out_proj.weight"].t() + state[prefix + "attn.out_proj.bias"]
    n = _ln(x, state, prefix + "ln_2")
    hmid = quick_gelu(n @ state[prefix + "mlp.c_fc.weight"].t() + state[prefix + "mlp.c_fc.bias"])
    return x + hmid @ state[prefix + "mlp.c_proj.weight"].t() + state[prefix + "mlp.c_proj.bias"]


def vit_backbone(state, input_resolution, patch, heads, img, prefix=""):
    """[B, 3, H, W] -> [B, h * w, width] with the state dict of a VisionTransformer (keys under `prefix`)."""
    width = state[prefix + "conv1.weight"].shape[0]
    x = F.conv2d(img, state[prefix + "conv1.weight"], stride=patch)
    B, _, h, w = x.shape
    x = x.flatten(2).transpose(1, 2)
    n = input_resolution // patch
    pe = state[prefix + "positional_embedding"][1:]
    if (h, w) != (n, n):
        pe = F.interpolate(pe.reshape(1, n, n, width).permute(0, 3, 1, 2), size=(h, w), mode="bilinear")
        pe = pe.permute(0, 2, 3, 1).reshape(h * w, width)
    x = _ln(x + pe, state, prefix + "ln_pre")
    i = 0
    while f"{prefix}transformer.resblocks.{i}.ln_1.weight" in state:
        x = vit_block(state, f"{prefix}transformer.resblocks.{i}.", x, heads)
        i += 1
    return x


def vit_adaptor_embed(state, prefix, input_resolution, patch, heads, img):
    """image_proj(backbone(img)): what the adaptor hands to its post-forward hook, [B, T, embed_dim]."""
    x = vit_backbone(state, input_resolution, patch, heads, img, prefix + "embed_images.")
    return x @ state[prefix + "image_proj.weight"].t() + state[prefix + "image_proj.bias"]
