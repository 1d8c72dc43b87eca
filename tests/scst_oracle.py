"""A plain-torch oracle for the SCST criterion kernels (csrc/loss_optim.hip: scst_fwd_grad_kernel, the registers form, and
scst_stream_kernel, the streaming form): no GPU needed, no dependency on the kernels.  Built like tests/criterion_oracle.py, whose
`excess`, tolerances, PAD_FILL and case generator it reuses.

  scst_reference()  float64 on the stored (16-bit-rounded) inputs, restated from the formulas of include/ofasys_amd.h:
                        w = reward[sentence of the row],  A = the whole vocabulary or [0,4) U [cstart,cend)
                        lse = log sum_{v in A} exp(x_v);  row_loss = w (lse - x_t);  d_v = w g (exp(x_v - lse) - [v == t]) on A
                    with the componentwise magnitude bound |w g| (p + onehot) of d.  Where the bound is 0 -- columns outside A, padding
                    columns V..ld, ignored rows, rows of weight 0, rows whose target is not an allowed column -- the kernel must write
                    exactly 0; the row_loss of an ignored row is 0 and of a disallowed target +inf.
  scst_emulate()    the same arithmetic in float32 with the kernels' roundings and nothing else of them (registers form:
                    exp2(x log2e - m log2e) with a max-then-rescale sum; streaming form: exp(x - lse); one rounding to the output type),
                    able to apply one named mutation.
  CASES             12 rows = 4 sentences of 3 rows, rewards 1.5, -0.75, 0 and 3e-3, one pad-target row, in the regimes of the
                    criterion oracle: `randn3`, and `planted`, where the row's dominant logit sits on each seam column in turn -- the
                    seams here include both sides of cstart and cend, so a disallowed column that leaks into a sum carries the row.
tests/test_scst_cpu.py proves the oracle sound (it sees the mutations) and checks it against the reference's own loss and gradient
(tests/golden/scst.npz); tests/test_scst_kernel_gpu.py runs it against the kernels.
"""
from collections import namedtuple

import torch

from tests import criterion_oracle as co

IGNORE = co.IGNORE
ROWS, SENTENCES, ROWS_PER_SEQ = 12, 4, 3
REWARDS = (1.5, -0.75, 0.0, 3e-3)
IGNORED_ROW = 4                                         # a pad-target row, inside the sentence of reward -0.75
PERM_SEQ = tuple((5 * r + 1) % SENTENCES for r in range(ROWS))         # an explicit row -> sentence map that is no r // 3


def allowed(V, crange, dev):
    """bool [V]: the whole vocabulary, or [0, 4) U [cstart, cend)."""
    c = torch.arange(V, device=dev)
    if crange is None:
        return torch.ones(V, dtype=torch.bool, device=dev)
    return (c < 4) | ((c >= crange[0]) & (c < crange[1]))


def _valid(t, A, V, ignore):
    """Rows whose target is an allowed column of [0, V) (the ignored row's target, the pad token, is one)."""
    inside = (t >= 0) & (t < V)
    return inside & A[t.clamp(0, V - 1)]


def scst_reference(x, t, reward, seq, g, crange=None, ignore=IGNORE):
    """x [R, V] view of [R, ld] storage; t int64 [R]; reward [nseq]; seq int64 [R] (the sentence of each row); g float.
    -> (ref, bound): ref = dict(lse, row_loss [R], d [R, ld]) in float64."""
    dt = torch.float64
    R, V = x.shape
    ld = co._ld(x)
    A = allowed(V, crange, x.device)
    xv = x.to(dt)
    lse = torch.logsumexp(xv.masked_fill(~A[None, :], float("-inf")), 1)
    p = torch.exp(xv - lse[:, None]) * A[None, :].to(dt)
    w = reward.to(dt)[seq]
    live = t != ignore
    valid = _valid(t, A, V, ignore)
    tc = t.clamp(0, V - 1)
    nll = lse - xv.gather(1, tc[:, None])[:, 0]
    row_loss = torch.where(live, torch.where(valid, w * nll, torch.full_like(nll, float("inf"))), torch.zeros_like(nll))
    oh = co._onehot(tc, R, V, dt, x.device) * valid[:, None].to(dt)
    k = (w * g * (live & valid).to(dt))[:, None]
    return dict(lse=lse, row_loss=row_loss, d=co._widen((p - oh) * k, ld)), co._widen((p + oh) * k.abs(), ld)


MUTATIONS = ("neighbour_reward", "leak_below_cstart", "leak_at_cend", "reward_sign", "onehot_shift", "pad_written", "ignored_live",
             "zero_reward_live")


def scst_emulate(x, t, reward, seq, g, dtype, fused, crange=None, mutation=None, ignore=IGNORE):
    """float32 with the kernels' roundings -> dict(lse, row_loss fp32 [R], d [R, ld] of dtype)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    ft = torch.float32
    R, V = x.shape
    ld = co._ld(x)
    A = allowed(V, crange, x.device)
    summed = A.clone()
    if crange is not None and mutation == "leak_below_cstart":
        summed[crange[0] - 1] = True
    if crange is not None and mutation == "leak_at_cend" and crange[1] < V:
        summed[crange[1]] = True
    xv = x.to(ft)
    lse = co._lse32(xv.masked_fill(~summed[None, :], float("-inf")), fused)
    if fused:
        p = torch.exp2(co._fma(xv, co.L2E32, -lse[:, None] * co.L2E32))
    else:
        p = torch.exp(xv - lse[:, None])
    r32 = reward.to(ft)
    if mutation == "zero_reward_live":
        r32 = torch.where(r32 == 0, torch.ones_like(r32), r32)
    w = r32[(seq + 1) % reward.numel() if mutation == "neighbour_reward" else seq]
    if mutation == "reward_sign":
        w = w.abs()
    live = t != ignore
    valid = _valid(t, A, V, ignore)
    tc = t.clamp(0, V - 1)
    oh = co._onehot((tc + 1) % V if mutation == "onehot_shift" else tc, R, V, ft, x.device) * valid[:, None].to(ft)
    on = valid if mutation == "ignored_live" else (live & valid)
    wg = w * torch.tensor(g, dtype=ft, device=x.device) * on.to(ft)
    d = co._widen((p - oh) * wg[:, None] * A[None, :].to(ft), ld)
    if mutation == "pad_written" and ld > V:
        d[:, V] = wg
    nll = lse - xv.gather(1, tc[:, None])[:, 0]
    row_loss = torch.where(live, torch.where(valid, w * nll, torch.full_like(nll, float("inf"))), torch.zeros_like(nll))
    return dict(lse=lse, row_loss=row_loss, d=d.to(dtype))


# ---------------------------------------------------------------------------------------------------------------- cases
ScstCase = namedtuple("ScstCase", "regime V ld crange g perm seed rot")     # ld: the row stride of the storage the [rows, V] view sits in
# (V, ld): the registers form with 1, 2 (8200 columns as a view of 8256-wide storage too), 7 and 8 slabs; the streaming form for a row
# the registers cannot hold, and for fp32
SHAPES16 = ((204, 208), (4097, 4104), (8193, 8200), (8200, 8256), (51265, 51272), (59457, 59464))
STREAM16 = ((65540, 65544),)
SHAPES32 = ((4097, 4100),)
GS = (None, 1.0, 128.0)                                 # grad_scale: NULL, 1, a loss scale


def ranges_of(V):
    """None; (5, V - 3): neither bound on a vector edge; and a range that starts inside the second slab (column 8192 + 13), or for
    short rows one whose two cuts fall into one vector's neighbours."""
    out = [None, (5, V - 3)]
    out.append((8192 + 13, V - 3) if V > 8192 + 64 else (V // 2 + 1, V // 2 + 22))
    return out


def registers_form(dtype, ld):
    return dtype != torch.float32 and ld <= 65536


def seams(V, N, crange, fused):
    """The planted / target columns: the row ends, the edge of [0, 4), the first vector's end, the last full vector's edge, both sides
    of cstart and cend and the ends of the vectors they cut, and (registers form) the slab seams 8192 k and a wave seam."""
    cols = [0, 3, 4, N - 1, N, V - 1, V // N * N - 1, V // N * N]
    if crange is not None:
        cs, ce = crange
        cols += [cs - 1, cs, ce - 1, ce, cs // N * N, cs // N * N + N - 1, ce // N * N, (ce - 1) // N * N + N - 1, ce // N * N + N]
    if fused:
        for k in range(1, (V + 8191) // 8192):
            cols += [8192 * k - 1, 8192 * k]
        cols += [1535, 1536]
    seen = []
    for c in cols:
        if 0 <= c < V and c != IGNORE and c not in seen:
            seen.append(c)
    return seen


def _cases(shapes):
    out, i = [], 0
    combos = [(perm, g) for perm in (False, True) for g in GS]
    for V, ld in shapes:
        for crange in ranges_of(V):
            for regime in co.REGIMES:
                perm, g = combos[i % len(combos)]
                out.append(ScstCase(regime, V, ld, crange, g, perm, 900 + i, i % 3))
                i += 1
    return out


CASES16, CASES_STREAM16, CASES32 = _cases(SHAPES16), _cases(STREAM16), _cases(SHAPES32)


def layout(case, dtype):
    """-> (per-row seam columns, targets): the seam columns -- allowed and disallowed alike -- are dealt round-robin over the live rows
    and planted there; the target of a live row is the case.rot-th ALLOWED one of them (column 0 if it has none)."""
    fused = registers_form(dtype, case.ld)
    cols = seams(case.V, co.NVEC[dtype], case.crange, fused)
    per = co._spread(cols, ROWS, IGNORED_ROW)
    A = allowed(case.V, case.crange, "cpu")
    t = []
    for r in range(ROWS):
        ok = [c for c in per[r] if bool(A[c])]
        t.append(IGNORE if r == IGNORED_ROW else (ok[case.rot % len(ok)] if ok else 0))
    return per, t


def build(case, dtype, device="cpu"):
    """-> dict(x [R, V] view of [R, ld] storage, t int64 [R], reward fp32 [4], seq int64 [R], row_seq int32 [R] or None, g float or
    None, cols).  The storage beyond column V holds PAD_FILL."""
    per, t = layout(case, dtype)
    store = co.make_case(case.regime, ROWS, case.V, case.ld, per, case.seed).to(dtype).to(device)
    seq = list(PERM_SEQ) if case.perm else [r // ROWS_PER_SEQ for r in range(ROWS)]
    return dict(x=store[:, :case.V], t=torch.tensor(t, dtype=torch.int64, device=device),
                reward=torch.tensor(REWARDS, dtype=torch.float32, device=device), seq=torch.tensor(seq, dtype=torch.int64, device=device),
                row_seq=torch.tensor(seq, dtype=torch.int32, device=device) if case.perm else None, g=case.g, cols=per)

