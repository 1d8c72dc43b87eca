"""A plain-torch oracle for the fused attention kernels (csrc/attention.hip): no GPU, no dependency on the kernels.

reference()  float64 on the 16-bit-rounded inputs: out, natural-log lse, dq, dk, dv, dbias, dc_attn, delta.
bounds()     the componentwise magnitude bound of each output (the classical forward-error bound of a product: the same sums
             with every factor replaced by its absolute value), plus an absolute underflow floor for the 16-bit type.
excess()     max |got - ref| / bound in units of the 16-bit eps; where bound == 0 the kernel must have written exactly 0.
emulate()    the same arithmetic in float32 with the kernels' roundings and nothing else of the kernels; a blockwise form walks
             the online softmax as 32 query rows x 32 keys, counts the branches taken and can apply one named mutation.
make_case()  inputs from a CPU generator: near-uniform softmax rows, sharp rows, planted dominant keys, a rising staircase.
CASES        the table tests/test_attention_edges_gpu.py runs and tests/test_attn_oracle_cpu.py proves sound.

Conventions of the kernels that the oracle states (not NaN): a fully masked row has P = 0, so out = 0, zero gradients, lse = 0.
The kernels keep lse in base 2 (log2 of the sum of 2^(score * log2 e)); reference() returns natural log: lse_kernel * ln 2.
"""
from collections import namedtuple

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
SCALE = 128.0 ** -0.5          # the score scale every case uses (head_dim 64, as the existing kernel tests)
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# smallest positive (subnormal) number of the 16-bit type: a stored value or a rounded P / dS below it is lost absolutely
TINY = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}

# ---------------------------------------------------------------------------------------------------------------- measured constants
# EMUL_CEILING: the cap on excess(emulate, reference, bounds) over CASES and FP16_CASES, both 16-bit types, every 16-bit output.
# emulate() rounds twice on the way to each 16-bit output (P or dS, then the result); two roundings to nearest cost at most
# 2 u + u^2 (u = EPS, the unit roundoff) relative to the magnitude bound, the float32 work in between ~ S * 2^-24: 2.05 in units of u.
# Measured 2026-10-17 over the whole table (tests/test_attn_oracle_cpu.py prints the figures with -s), worst excess:
#          out    dq     dk     dv     dbias
#   bf16   1.58   0.51   0.78   1.97   0.54
#   fp16   1.58   0.52   0.66   1.92   0.53
# (dv and out reach the two-rounding limit at T = 1 / short rows, where one term carries the sum; dq / dk / dbias sit lower because
# their bound also holds the |dO| @ |V|^T + |dO . O| magnitudes that the difference dP - delta cancels.)
EMUL_CEILING = 2.05
# TOL for the kernels = 2 * EMUL_CEILING: the factor 2 covers what emulate() does not model, each an O(1) eps effect: the MFMA
# accumulation order, the hardware exp2, P rounded relative to the running maximum instead of the final one, and the shared-bias
# form feeding the bias through the score accumulator.  Never set from what a kernel produced.
TOL = 2.0 * EMUL_CEILING
# fp32 outputs, absolute: 8 x the largest error of emulate()'s float32 evaluation against float64 over the table (8: exp2 / log2
# ulps and summation order).  Measured 2026-10-17: lse 2.9e-5, held as 3.0e-5 (natural log; |lse| reaches 82 in the stairs regime), delta 6.7e-6
# (against rowsum(dO * out) of the SAME stored out), shared fp32 dbias 1.5e-5 (against the float64 dS formed with delta of the same
# stored out: the backward takes out as an input, and a delta from a 16-bit out differs from the exact one by 16-bit eps, which is the
# forward's rounding and not the backward's error).
LSE_TOL = 8 * 3.0e-5
DELTA_TOL = 8 * 6.7e-6
DBIAS32_TOL = 8 * 1.5e-5
# Branch counts of the blockwise online softmax at T = S = 160, B = heads = 2 (80 (sample, head, wave, key block) steps behind the
# first block), asserted by the CPU test:  uniform: no-rescale 0 / 80;  plant_first: no-rescale 80 / 80;
# stairs: every row rescaled by >= 2^8 in 80 / 80 (and 72 / 72 of each at T = 96, S = 200).
# The kernels themselves on an MI355X, 2026-10-17, worst over the same table: out 1.58, dq 0.51, dk 0.78, dv 1.97, dbias 0.54 (units of
# eps, against TOL = 4.1); lse 0.05, delta 0.07, fp32 shared dbias 0.07 of their absolute tolerances.


def rnd(x, dtype):
    """Round to the 16-bit type and come back to x's own dtype."""
    return x.to(dtype).to(x.dtype)


def _split(x, heads):
    B, T, D = x.shape
    return x.reshape(B, T, heads, D // heads).permute(0, 2, 1, 3)


def _merge(x):
    B, H, T, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, T, H * hd)


def dead_mask(B, T, S, kpm, causal, device):
    """bool [B, 1, T, S]: True where the key is invisible to the query (causal: key > query; kpm: padded key)."""
    dead = torch.zeros(B, 1, T, S, dtype=torch.bool, device=device)
    if causal:
        dead = dead | torch.triu(torch.ones(T, S, dtype=torch.bool, device=device), 1)
    if kpm is not None:
        dead = dead | kpm.bool()[:, None, None, :S]
    return dead


def _bias4(bias, B, heads, T, S, shared, dt):
    if bias is None:
        return None
    if shared:                                     # [heads, Tb, Sb], indexed by position: the same for every sample
        return bias[None, :, :T, :S].to(dt)
    return bias.reshape(B, heads, T, S).to(dt)


def _c4(c_attn, heads, dt, device):
    if c_attn is None:
        return torch.ones(1, heads, 1, 1, dtype=dt, device=device)
    return c_attn.to(dt).view(1, heads, 1, 1)


def _core64(q, k, v, dout, heads, scale, bias, kpm, c_attn, causal, bias_shared, out):
    dt = torch.float64
    B, T, D = q.shape
    S = k.shape[1]
    Q, K, V, dO = (_split(t.to(dt), heads) for t in (q, k, v, dout))
    c = _c4(c_attn, heads, dt, q.device)
    s = Q @ K.transpose(-1, -2) * scale
    b4 = _bias4(bias, B, heads, T, S, bias_shared, dt)
    if b4 is not None:
        s = s + b4
    dead = dead_mask(B, T, S, kpm, causal, q.device)
    s = s.masked_fill(dead, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)                                         # exp(-inf) = 0: a dead key, and every key of a fully masked row
    l = e.sum(-1, keepdim=True)
    l1 = torch.where(l > 0, l, torch.ones_like(l))
    P = e / l1
    lse = (m + torch.log(l1)).squeeze(-1)                        # 0 for a fully masked row
    O = P @ V * c
    Od = O if out is None else _split(out.to(dt), heads)         # the stored out the backward is given (delta is formed from it)
    delta = (dO * Od).sum(-1, keepdim=True)
    dP = dO @ V.transpose(-1, -2) * c
    dS = P * (dP - delta)
    r = dict(out=_merge(O), lse=lse.reshape(B * heads, T), delta=delta.squeeze(-1).reshape(B * heads, T),
             dq=_merge(dS @ K * scale), dk=_merge(dS.transpose(-1, -2) @ Q * scale), dv=_merge(P.transpose(-1, -2) @ dO * c))
    r["dc"] = None if c_attn is None else delta.sum((0, 2, 3)) / c.view(-1)
    # magnitude bounds: every factor by its absolute value
    aV, aK, aQ, adO, ac = V.abs(), K.abs(), Q.abs(), dO.abs(), c.abs()
    dSa = P * (adO @ aV.transpose(-1, -2) * ac + (adO * Od.abs()).sum(-1, keepdim=True))
    bd = dict(out=_merge(P @ aV * ac), dq=_merge(dSa @ aK * scale), dk=_merge(dSa.transpose(-1, -2) @ aQ * scale),
              dv=_merge(P.transpose(-1, -2) @ adO * ac))
    # what an underflow in the 16-bit type can cost, in units of its smallest subnormal: the stored value itself (1) plus a lost P / dS
    # entry per term of the sum (|other factor| each)
    ones = dict(out=_merge(1 + (aV * ac).sum(2, keepdim=True).expand(B, heads, T, -1)),
                dq=_merge(1 + (aK * scale).sum(2, keepdim=True).expand(B, heads, T, -1)),
                dk=_merge(1 + (aQ * scale).sum(2, keepdim=True).expand(B, heads, S, -1)),
                dv=_merge(1 + (adO * ac).sum(2, keepdim=True).expand(B, heads, S, -1)))
    if bias is not None:
        if bias_shared:
            full = torch.zeros(2, heads, bias.shape[1], bias.shape[2], dtype=dt, device=q.device)
            full[0, :, :T, :S] = dS.sum(0)
            full[1, :, :T, :S] = dSa.sum(0)
            r["dbias"], bd["dbias"] = full[0], full[1]
            ones["dbias"] = torch.full_like(full[0], float(B))
        else:
            r["dbias"], bd["dbias"] = dS.reshape(B * heads, T, S), dSa.reshape(B * heads, T, S)
            ones["dbias"] = torch.ones_like(r["dbias"])
    else:
        r["dbias"] = None
    return r, bd, ones


def reference(q, k, v, dout, heads, scale, bias=None, kpm=None, c_attn=None, causal=False, bias_shared=False, out=None):
    """float64 attention forward + backward on the given (16-bit-rounded) inputs -> dict(out, lse (natural log), delta, dq, dk, dv,
    dbias, dc).  bias: dense [B*heads, T, S], or with bias_shared [heads, Tb, Sb] (dbias is then the sum over the batch, zero outside
    [:T, :S]).  out: the stored forward result the backward is handed; delta = rowsum(dO * out) is formed from it when given."""
    return _core64(q, k, v, dout, heads, scale, bias, kpm, c_attn, causal, bias_shared, out)[0]


def bounds(q, k, v, dout, heads, scale, bias=None, kpm=None, c_attn=None, causal=False, bias_shared=False, out=None):
    """-> (bound, floor_units): per output the componentwise magnitude bound, and the underflow floor in units of TINY[dtype]."""
    _, bd, ones = _core64(q, k, v, dout, heads, scale, bias, kpm, c_attn, causal, bias_shared, out)
    return bd, ones


def reference_and_bounds(q, k, v, dout, heads, scale, bias=None, kpm=None, c_attn=None, causal=False, bias_shared=False, out=None):
    """-> (reference dict, bound dict, floor_units dict) from one float64 evaluation."""
    return _core64(q, k, v, dout, heads, scale, bias, kpm, c_attn, causal, bias_shared, out)


def excess(got, ref, bound, eps, floor=None):
    """max over elements with bound > 0 of (|got - ref| - floor) / bound, in units of eps; where bound == 0 got must be exactly 0
    (returns inf otherwise, and for any non-finite got)."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    zero = bound <= 0
    if bool((got[zero] != 0).any()):
        return float("inf")
    err = (got - ref).abs()
    if floor is not None:
        err = (err - floor.double()).clamp_min(0)
    live = ~zero
    if not bool(live.any()):
        return 0.0
    return float((err[live] / bound[live]).max()) / eps


# ---------------------------------------------------------------------------------------------------------------- emulation
MUTATIONS = ("drop_last_key", "diag_hidden", "diag_leak", "skip_alpha", "kpm_shift", "lse_off")


def _mutated_dead(dead, mutation, T, S, causal):
    """The visibility mask a subtly wrong kernel would use.  The 32 x 32 block hit is the LAST diagonal block both sides reach."""
    if mutation == "drop_last_key":                # key S-1 lost for the 32 rows of the first wave
        dead = dead.clone()
        dead[:, :, :32, S - 1] = True
    elif mutation in ("diag_hidden", "diag_leak"):
        w = (min(T, S) - 1) // 32
        r0, r1, c0, c1 = w * 32, min(T, w * 32 + 32), w * 32, min(S, w * 32 + 32)
        qi = torch.arange(r0, r1, device=dead.device)[:, None]
        kj = torch.arange(c0, c1, device=dead.device)[None, :]
        dead = dead.clone()
        if mutation == "diag_hidden":              # key >= q dead: the diagonal itself hidden
            dead[:, :, r0:r1, c0:c1] |= kj >= qi
        else:                                      # key > q + 1 dead: the diagonal leaks one key
            dead[:, :, r0:r1, c0:c1] &= ~(kj == qi + 1)
    return dead


def emulate(q, k, v, dout, heads, scale, bias=None, kpm=None, c_attn=None, causal=False, dtype=torch.bfloat16, bias_shared=False,
            blockwise=False, mutation=None):
    """float32 with the kernels' roundings: unnormalised P rounded before P @ V, out rounded, delta from the rounded out, dS rounded
    before dS @ K and dS^T @ Q, P rounded before P^T @ dO, the 16-bit outputs rounded.  lse is returned in natural log.
    blockwise: the forward walks key blocks of 32 with a running maximum per row and the kernels' wave-wide branch (32 rows)
    `any(m_new != m_run)`; -> r["stats"] = dict(steps, norescale, big): the (sample, head, wave, key block) steps behind a wave's first
    block, how many took the no-rescale branch, how many rescaled EVERY row of the wave by >= 2^8."""
    assert mutation is None or mutation in MUTATIONS
    ft = torch.float32
    B, T, D = q.shape
    S = k.shape[1]
    dev = q.device
    Q, K, V, dO = (_split(t.to(ft), heads) for t in (q, k, v, dout))
    c = _c4(c_attn, heads, ft, dev)
    if mutation == "kpm_shift" and kpm is not None:              # sample b's padding mask applied to sample b-1
        kpm = torch.roll(kpm, -1, 0)
    sc = scale * LOG2E
    t = Q @ K.transpose(-1, -2) * sc
    b4 = _bias4(bias, B, heads, T, S, bias_shared, ft)
    if b4 is not None:
        t = t + b4 * LOG2E
    dead = dead_mask(B, T, S, kpm, causal, dev)
    if mutation in ("drop_last_key", "diag_hidden", "diag_leak"):
        dead = _mutated_dead(dead, mutation, T, S, causal)
    t = t.masked_fill(dead, float("-inf"))
    stats = None
    if not blockwise:
        assert mutation != "skip_alpha", "skip_alpha lives in the blockwise form"
        m = t.amax(-1, keepdim=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        p = torch.exp2(t - m)
        l = p.sum(-1, keepdim=True)
        acc = rnd(p, dtype) @ V
    else:
        neg = torch.full((B, heads, T, 1), float("-inf"), dtype=ft, device=dev)
        m_run, l = neg.clone(), torch.zeros_like(neg)
        acc = torch.zeros(B, heads, T, D // heads, dtype=ft, device=dev)
        nw, nkb = (T + 31) // 32, (S + 31) // 32
        stats = dict(steps=0, norescale=0, big=0)
        for kb in range(nkb):
            tb = t[..., kb * 32:kb * 32 + 32]
            m_new = torch.maximum(m_run, tb.amax(-1, keepdim=True))
            m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            p = torch.exp2(tb - m_use)
            alpha = torch.exp2(m_run - m_use)
            moved = m_new != m_run
            take = torch.zeros_like(moved)
            for w in range(nw):
                rows = slice(w * 32, min(T, w * 32 + 32))
                any_w = moved[:, :, rows].any(2, keepdim=True)                    # [B, heads, 1, 1]: the wave-wide branch
                take[:, :, rows] = any_w
                visited = not (causal and kb * 32 > w * 32 + 31)
                if visited and kb > 0:                                            # (a wave's first block is always key block 0)
                    stats["steps"] += B * heads
                    stats["norescale"] += int((~any_w).sum())
                    stats["big"] += int((alpha[:, :, rows] <= 2.0 ** -8).all(2).sum())
            if mutation == "skip_alpha" and kb == 1:                             # the rescale forgotten at one key block
                take = torch.zeros_like(take)
            a_eff = torch.where(take, alpha, torch.ones_like(alpha))
            l = l * a_eff + p.sum(-1, keepdim=True)
            acc = acc * a_eff + rnd(p, dtype) @ V[:, :, kb * 32:kb * 32 + 32]
            m_run = m_new
        m = torch.where(torch.isinf(m_run), torch.zeros_like(m_run), m_run)
    l1 = torch.where(l > 0, l, torch.ones_like(l))
    inv = torch.where(l > 0, 1.0 / l1, torch.zeros_like(l))
    out = rnd(acc * (c * inv), dtype)
    lse2 = m + torch.log2(l1)                                    # base 2, as the kernels keep it
    if mutation == "lse_off":                                    # one row's lse too large by 1e-3 (natural log), fed to the backward
        lse2 = lse2.clone()
        lse2[0, 0, min(T - 1, 5)] += 1e-3 * LOG2E
    pn = torch.exp2(t - lse2)                                    # dead keys: exp2(-inf) = 0
    delta = (dO * out).sum(-1, keepdim=True)
    dP = dO @ V.transpose(-1, -2)
    dS = pn * (dP * c - delta)
    dS16 = rnd(dS, dtype)
    r = dict(out=_merge(out).to(dtype), lse=(lse2 * LN2).squeeze(-1).reshape(B * heads, T), delta=delta.squeeze(-1).reshape(B * heads, T),
             dq=_merge(dS16 @ K * scale).to(dtype), dk=_merge(dS16.transpose(-1, -2) @ Q * scale).to(dtype),
             dv=_merge(rnd(pn, dtype).transpose(-1, -2) @ dO * c).to(dtype), dbias=None, stats=stats)
    if bias is not None:
        if bias_shared:                                          # fp32 [heads, Tb, Sb]: the batch sum of the unrounded dS
            g = torch.zeros(heads, bias.shape[1], bias.shape[2], dtype=ft, device=dev)
            g[:, :T, :S] = dS.sum(0)
            r["dbias"] = g
        else:
            r["dbias"] = dS16.reshape(B * heads, T, S).to(dtype)
    return r


# ---------------------------------------------------------------------------------------------------------------- inputs
REGIMES = ("uniform", "sharp", "plant_first", "plant_last", "stairs")
PLANT_Q, PLANT_K = 6.0, 16.0          # plant_first / plant_last: q += 6u, k[key] += 16u  -> the planted score leads by ~ 8.5 nats
STAIR_Q, STAIR_STEP = 8.0, 16.0       # stairs: q += 8u, k[32 j] += 16 (j + 1) u  -> each key block leads the last by ~ 16 bits


def make_case(regime, B, heads, T, S, seed):
    """-> dict(q [B,T,D], k, v [B,S,D], dout [B,T,D]) float32 from a CPU generator, D = heads * 64.
    The planted regimes first remove q's and k's own components along the unit vector u of each head, so that every query row scores
    a planted key alike (and no other key at all along u) and the branch counts hold by construction rather than by luck."""
    assert regime in REGIMES, regime
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = heads * 64
    q, dout = torch.randn(B, T, D, generator=g), torch.randn(B, T, D, generator=g)
    k, v = torch.randn(B, S, D, generator=g), torch.randn(B, S, D, generator=g)
    if regime == "sharp":
        q = q * 4
    elif regime != "uniform":
        u = torch.randn(heads, 64, generator=g)
        u = u / u.norm(dim=1, keepdim=True)
        qh = q.view(B, T, heads, 64)
        qh = qh - (qh * u).sum(-1, keepdim=True) * u
        kh = k.view(B, S, heads, 64)
        kh = kh - (kh * u).sum(-1, keepdim=True) * u
        if regime == "stairs":
            qh = qh + STAIR_Q * u
            for j in range((S + 31) // 32):
                kh[:, 32 * j] += STAIR_STEP * (j + 1) * u
        else:
            qh = qh + PLANT_Q * u
            kh[:, 0 if regime == "plant_first" else S - 1] += PLANT_K * u
        q, k = qh.reshape(B, T, D), kh.reshape(B, S, D)
    return dict(q=q, k=k, v=v, dout=dout)


# ---------------------------------------------------------------------------------------------------------------- the table
Case = namedtuple("Case", "regime T S causal bias kpm c seed")      # bias: none | dense | shared | shared_big;  c: none | f32 | bf16
BATCH, HEADS = 2, 2
SEAM_T = (1, 31, 32, 33, 127, 128, 129, 160)
SEAM_S = (1, 31, 32, 33, 64, 65, 96, 97, 129)
SEAM_S_BIASED = (33, 65, 97)                                        # the thinned key set of the three biased forms
BIAS_MODES = ("none", "dense", "shared", "shared_big")
C_MODES = ("none", "f32", "bf16")


def _seam(T, S, causal, bias):
    return Case("sharp", T, S, causal, bias, S >= 34, C_MODES[(T + S + int(causal)) % 3], 1000 + 7 * T + S)


def seam_cases(T):
    return [_seam(T, S, causal, bias) for bias in BIAS_MODES for S in (SEAM_S if bias == "none" else SEAM_S_BIASED)
            for causal in (False, True)]


REGIME_SHAPES = ((160, 160), (96, 200))
REGIME_CASES = [Case(regime, T, S, causal, bias, False, C_MODES[(i + j) % 3], 2000 + 31 * i + j)
                for i, regime in enumerate(("plant_first", "plant_last", "stairs")) for j, (T, S) in enumerate(REGIME_SHAPES)
                for causal in (False, True) for bias in ("none", "dense", "shared")]
# today's regime and the sharper one, so that the ceiling is measured over them too (the issue's twelve indicative runs)
EXTRA_CASES = [Case("uniform", 160, 160, False, "none", False, "f32", 3000), Case("uniform", 160, 160, True, "dense", True, "f32", 3001),
               Case("uniform", 7, 300, False, "dense", True, "none", 3002), Case("uniform", 1, 3, False, "none", False, "f32", 3003),
               Case("sharp", 200, 131, True, "dense", True, "bf16", 3004)]
CASES = [c for T in SEAM_T for c in seam_cases(T)] + REGIME_CASES + EXTRA_CASES
# fp16: the seam sweep's diagonal and the three regimes
FP16_CASES = [_seam(T, T, causal, bias) for T in SEAM_T for causal in (False, True) for bias in ("none", "dense", "shared")] + \
             REGIME_CASES


def build_inputs(case, dtype, device="cpu", B=BATCH, heads=HEADS):
    """The tensors of one table entry, rounded to dtype, on device -> (dict q k v dout, kwargs for reference / emulate / the kernels)."""
    x = {n: t.to(dtype).to(device) for n, t in make_case(case.regime, B, heads, case.T, case.S, case.seed).items()}
    g = torch.Generator(device="cpu").manual_seed(case.seed + 1)
    kw = dict(causal=case.causal)
    if case.bias != "none":
        shared = case.bias != "dense"
        Tb, Sb = (case.T + 37, case.S + 70) if case.bias == "shared_big" else (case.T, case.S)
        shape = (heads, Tb, Sb) if shared else (B * heads, case.T, case.S)
        kw["bias"] = torch.randn(*shape, generator=g).to(dtype).to(device)
        kw["bias_shared"] = shared
    if case.kpm:                                   # the last sample only, crossing a 32-key boundary
        kpm = torch.zeros(B, case.S, dtype=torch.bool)
        kpm[-1, case.S - 33:] = True
        kw["kpm"] = kpm.to(device)
    if case.c != "none":
        c = 1 + 0.2 * torch.randn(heads, generator=g)
        kw["c_attn"] = (c.float() if case.c == "f32" else c.to(torch.bfloat16)).to(device)
    return x, kw


def check16(got, ref, bd, ones, dtype, names=("out", "dq", "dk", "dv", "dbias")):
    """-> {name: excess} of the 16-bit outputs present in got (a 16-bit dbias only)."""
    res = {}
    for n in names:
        if got.get(n) is None or (n == "dbias" and got[n].dtype == torch.float32):
            continue
        res[n] = excess(got[n], ref[n], bd[n], EPS[dtype], ones[n] * TINY[dtype])
    return res
