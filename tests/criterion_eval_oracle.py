"""A plain-torch oracle for the validation criterion (ofa_criterion_eval + ofa_eval_stats_add, csrc/loss_optim.hip and the node form in
csrc/trie_loss.hip): no GPU needed, no dependency on the kernels.  The pattern and the helpers are tests/criterion_oracle.py's.

eval_reference()   float64 on the stored logits: row_loss, row_nll, row_hit and the four sums [ntokens, loss_sum, nll_sum, n_correct],
                   restated from the formulas in the kernel comments over an explicit allowed set A (bool [rows, V]).
eval_emulate()     the same arithmetic in float32 (max first, one rescaled sum; exp2(x log2e - m log2e) for the registers form) and nothing
                   else of the kernels, able to apply one named mutation.
CASES              at most MAX_ROWS rows each: the registers form on both sides of every NV boundary, the streaming form over LS_V with
                   none / range / mask / both (and every registers shape again in fp32), the node form over the synthetic tries of
                   tests/closed_set_train_case.py.  Every case is `planted`-style: see build().
tests/test_criterion_eval_cpu.py proves the table sound; tests/test_criterion_eval_gpu.py runs it against the kernels.
"""
from collections import namedtuple

import torch

from tests import closed_set_train_case as cst
from tests import criterion_oracle as co
from tests.criterion_oracle import IGNORE, L2E32, NVEC, PAD_FILL, PLANT, _fma

MAX_ROWS = 8
TARGET_FILL = 13.0       # a seam row's target column: above every planted column (PLANT + randn / 8) of the row, so it IS the arg-max
TIE_FILL = 14.0          # the two equal maxima of a tie row (exact in bf16 and fp16)
FOREIGN_FILL = 16.0      # a disallowed column that would win the arg-max and dominate the sums if a kernel let it in

# ---------------------------------------------------------------------------------------------------------------- measured constants
# fp32 outputs: 8 x the largest error of eval_emulate against eval_reference over the whole table (8: exp / log ulps and the summation
# order, criterion_oracle's convention for LSROW_TOL).  Measured on the CPU 2026-10-20 (tests/test_criterion_eval_cpu.py prints the figures
# with -s), worst of row_loss / row_nll: registers form 1.14e-6 (bf16) / 1.36e-6 (fp16), streaming form 7.1e-7 / 8.2e-7 / 8.8e-7 (bf16 /
# fp16 / fp32), node form 6.0e-7 / 6.1e-7 / 6.9e-7.  Never set from what a kernel produced.  row_hit, n_correct and ntokens are compared
# exactly; the sums against (live rows) x EVAL_TOL.
EVAL_WORST = 1.4e-6
EVAL_TOL = 8 * EVAL_WORST

MUTATIONS = ("argmax_last_on_tie", "argmax_sees_disallowed", "argmax_sees_padding", "hit_counts_ignored", "nll_uses_smoothed",
             "drop_last_col", "drop_slab", "range_edge", "count_off", "node_sibling_leak")


# ---------------------------------------------------------------------------------------------------------------- allowed sets
def allowed_set(R, V, crange=None, cmask=None, nodes=None, trie=None, inclusive_end=False, sibling_leak=False):
    """bool [R, V]: the whole vocabulary, [0,4) U [cstart,cend), that intersected with the byte mask, or the children of trie node
    nodes[r] (optionally inside the range).  sibling_leak: the children of node + 1 too (a mutation)."""
    A = co.ls_allowed(R, V, crange, cmask, "cpu", inclusive_end=inclusive_end)
    if nodes is not None:
        off, tok = trie["node_edge_off"].cpu(), trie["edge_token"].cpu()
        N = cst.nodes_to_masks(nodes.cpu(), off, tok, V)
        if sibling_leak:
            nxt = nodes.cpu().clone()
            nxt[nxt >= 0] += 1
            N = N | cst.nodes_to_masks(nxt, off, tok, V)
        A = A & N
    return A


def _finish(row_loss, row_nll, hit, t, ignore, count_ignored=False):
    live = t != ignore
    ntok = float(t.numel() if count_ignored else live.sum())
    return dict(row_loss=row_loss, row_nll=row_nll, row_hit=hit.to(torch.int32),
                sums=[ntok, float(row_loss.double().sum()), float(row_nll.double().sum()), float(hit.sum())])


def _lowest_argmax(xs):
    """The lowest column holding the row maximum of xs (-inf: a column left out); V for a row of -inf only."""
    V = xs.shape[1]
    m = xs.amax(1, keepdim=True)
    cols = torch.arange(V)[None, :].expand_as(xs)
    return torch.where((xs == m) & (m > float("-inf")), cols, torch.full_like(cols, V)).amin(1)


def eval_reference(x, t, A, eps, constrained, ignore=IGNORE):
    """float64 on the stored logits -> dict(row_loss, row_nll float64 [R], row_hit int32 [R], sums [ntokens, loss, nll, n_correct]).
    A live target outside A (or outside [0, V)): row_loss = row_nll = +inf, hit 0; an ignored row: 0, 0, 0 and not counted."""
    dt = torch.float64
    R, V = x.shape
    xv = x.to(dt).cpu()
    t, A = t.cpu(), A.cpu()
    Af = A.to(dt)
    xs = xv.masked_fill(~A, float("-inf"))
    live = t != ignore
    inside = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)
    valid = live & inside & A[torch.arange(R), tc]
    lse = torch.logsumexp(xs, 1)
    C = Af.sum(1)
    eps_i = eps / (C - 1 + (1e-6 if constrained else 0.0))
    nll = lse - xv[torch.arange(R), tc]
    loss = (1 - eps - eps_i) * nll + eps_i * (C * lse - (xv * Af).sum(1))
    inf, zero = torch.full_like(nll, float("inf")), torch.zeros_like(nll)
    nll = torch.where(valid, nll, torch.where(live, inf, zero))
    loss = torch.where(valid, loss, torch.where(live, inf, zero))
    hit = valid & (_lowest_argmax(xs) == t)
    return _finish(loss, nll, hit, t, ignore)


def eval_emulate(x, t, A, eps, constrained, fused, mutation=None, ignore=IGNORE, leaks=None):
    """float32 with the kernels' arithmetic -> the same dict (row_loss, row_nll float32).  fused: the registers form's exp2 route.
    leaks: {mutation: allowed set} for `range_edge` / `node_sibling_leak` (built by the caller, who knows the constraint)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    ft = torch.float32
    R, V = x.shape
    xv = x.to(ft).cpu()
    t, A = t.cpu(), A.cpu()
    if mutation in ("range_edge", "node_sibling_leak") and leaks and leaks.get(mutation) is not None:
        A = leaks[mutation].cpu()
    keep = torch.ones(V, dtype=torch.bool)
    if mutation == "drop_last_col":
        keep[V - 1] = False
    elif mutation == "drop_slab":
        keep[8192:] = False
    S = A & keep[None, :]
    Af = A.to(ft)
    xs = xv.masked_fill(~S, float("-inf"))
    live = t != ignore
    inside = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)
    valid = live & inside & A[torch.arange(R), tc]
    m = xs.amax(1, keepdim=True)
    m = torch.where(m > float("-inf"), m, torch.zeros_like(m))           # (a row that allows nothing: its outputs are masked below)
    if fused:
        s = torch.exp2(_fma(xs, L2E32, -m * L2E32)).sum(1, keepdim=True)
    else:
        s = torch.exp(xs - m).sum(1, keepdim=True)
    lse = (m + torch.log(s))[:, 0]
    C = Af.sum(1) + (1.0 if mutation == "count_off" else 0.0)
    eps32 = torch.tensor(eps, dtype=ft)
    eps_i = eps32 / ((C - 1.0 + 1e-6) if constrained else (C - 1.0))
    nll = lse - xv[torch.arange(R), tc]
    loss = (1.0 - eps32 - eps_i) * nll + eps_i * (C * lse - (xv * S.to(ft)).sum(1))
    if mutation == "nll_uses_smoothed":
        nll = loss
    seen = xs
    if mutation == "argmax_sees_disallowed":
        seen = xv
    elif mutation == "argmax_sees_padding":
        seen = co._storage(x).to(ft).cpu()
        seen = seen.masked_fill(~torch.nn.functional.pad(S, (0, seen.shape[1] - V), value=True), float("-inf"))
    am = _lowest_argmax(seen)
    if mutation == "argmax_last_on_tie":
        mm = seen.amax(1, keepdim=True)
        cols = torch.arange(seen.shape[1])[None, :].expand_as(seen)
        am = torch.where(seen == mm, cols, torch.full_like(cols, -1)).amax(1)
    hit = am == t
    inf, zero = torch.full_like(nll, float("inf")), torch.zeros_like(nll)
    nll = torch.where(valid, nll, torch.where(live, inf, zero))
    loss = torch.where(valid, loss, torch.where(live, inf, zero))
    counted = mutation == "hit_counts_ignored"
    hit = hit & (valid | (~live if counted else torch.zeros_like(valid)))
    out = _finish(loss, nll, hit, t, ignore, count_ignored=counted)
    out["sums"][1] = float(loss.sum().double())                          # (the kernel sums the rows in float32)
    out["sums"][2] = float(nll.sum().double())
    return out


def row_errors(got, ref):
    """-> (exact, err): exact: row_hit, the +inf rows and the zero rows agree exactly; err: the largest |got - ref| of row_loss and
    row_nll over the finite rows."""
    exact = bool(torch.equal(got["row_hit"].cpu().to(torch.int32), ref["row_hit"]))
    err = 0.0
    for n in ("row_loss", "row_nll"):
        g, r = got[n].double().cpu(), ref[n].double()
        fin = torch.isfinite(r)
        exact = exact and bool(torch.equal(g[~fin], r[~fin])) and bool(torch.isfinite(g[fin]).all()) and bool((g[r == 0] == 0).all())
        if bool(fin.any()) and bool(torch.isfinite(g[fin]).all()):
            err = max(err, float((g[fin] - r[fin]).abs().max()))
    return exact, err


def sums_agree(got, ref, live_rows, tol=EVAL_TOL):
    """[ntokens, loss_sum, nll_sum, n_correct]: counts exactly, sums within live rows x tol (both +inf where a row is +inf)."""
    if got[0] != ref[0] or got[3] != ref[3]:
        return False
    for g, r in ((got[1], ref[1]), (got[2], ref[2])):
        if r == float("inf"):
            if g != r:
                return False
        elif not abs(g - r) <= max(live_rows, 1) * tol:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------- the table
EvalCase = namedtuple("EvalCase", "form V ld eps variant crange rot seed trie")   # form: regs | stream | node;  trie: a cst.TrieCase
TIE_PAIRS = ((2, 3), (8, 24), (16, 17), (100, 1541), (40, 8192 + 40), (100, 8192 + 1000), (8191, 8192), (1535, 1536), (0, 4))


def _regs_ranges(V):
    out = []
    if V > 24:
        out.append((11, V - 2))                     # both edges inside a vector
    if V > 16400:
        out.append((8192 - 3, 16384 + 5))           # the range cuts a vector on each side of a slab seam
    return out


def _cases():
    out, i = [], 0
    for j, ld in enumerate(co.FUSED_LD):
        for k, V in enumerate((ld, ld - 3, ld - 11)):
            if V <= 1:
                continue
            out.append(EvalCase("regs", V, ld, (0.0, 0.1)[(j + k) % 2], "none", None, k, 2000 + i, None))
            i += 1
        for k, r in enumerate(_regs_ranges(ld - 3)):
            out.append(EvalCase("regs", ld - 3, ld, (0.1, 0.0)[(j + k) % 2], "range", r, k, 2000 + i, None))
            i += 1
    out.append(EvalCase("regs", co.WIDE[0], co.WIDE[1], 0.1, "none", None, 0, 2000 + i, None))
    out.append(EvalCase("regs", co.WIDE[0], co.WIDE[1], 0.0, "range", (11, co.WIDE[0] - 2), 1, 2001 + i, None))
    i += 2
    for V in co.LS_V:
        rs = co._ls_ranges(V)
        variants = [("none", None)] + [("range", r) for r in rs] + [("mask", None)] + [("both", r) for r in rs[-1:]]
        for vi, (variant, crange) in enumerate(variants):
            for ei, eps in enumerate((0.0, 0.1)):
                out.append(EvalCase("stream", V, None, eps, variant, crange, vi + ei, 2000 + i, None))
                i += 1
    out.append(EvalCase("stream", 66000, 66000, 0.1, "range", (8192 - 3, 65540), 0, 2000 + i, None))      # a row the registers form does not hold
    out.append(EvalCase("stream", 1030, 1035, 0.1, "none", None, 1, 2001 + i, None))                      # an ld that is no multiple of the vector
    i += 2
    for tc in cst.TRIE_CASES:
        out.append(EvalCase("node", tc.V, tc.ld, tc.eps, "node", tc.crange, 0, 2000 + i, tc))
        i += 1
    return out


CASES = _cases()
DTYPES = {"regs": (torch.bfloat16, torch.float16), "stream": co.DTYPES3, "node": co.DTYPES3}
# (the registers shapes in fp32 take the streaming kernel: the same table entry, another route)
ROUTES = [(c, d) for c in CASES for d in DTYPES[c.form]] + [(c, torch.float32) for c in CASES if c.form == "regs"]


def seams(case):
    """The planted columns of a dense case: the row ends, the last full vector's edge, every slab seam, a wave seam (ce_seams), the
    range's own edges -- those of them the range allows."""
    cols = co.ce_seams(case.V, 8, True)
    if case.crange is not None:
        cols = [case.crange[0], case.crange[1] - 1] + cols
    ok = []
    for c in cols:
        if c not in ok and c != IGNORE and (case.crange is None or c < 4 or case.crange[0] <= c < case.crange[1]):
            ok.append(c)
    return ok


def _inside(c, V, crange):
    return 0 <= c < V and c != IGNORE and (crange is None or c < 4 or crange[0] <= c < crange[1])


def layout(case):
    """A dense case's rows -> dict(t, plant (per-row planted columns), tie (row -> (low, high) columns), foreign (row -> a disallowed
    column), kinds).  Rows: up to three `seam` rows (the seam columns dealt round-robin; the target of a row is its seam column number
    case.rot, raised to TARGET_FILL: the arg-max), one `ignored` row whose maximum sits ON the ignore column, a `tie_low` and a
    `tie_high` row (two equal maxima, the target the lower / the higher one) and a `foreign` row (its target the arg-max of the allowed
    set while a larger logit sits just outside the range / under a zero of the mask) and a `dead` row (a live target that is not an
    allowed column: +inf, no hit)."""
    V, cr = case.V, case.crange
    cols = seams(case)
    n_seam = min(3, len(cols))
    plant = [[] for _ in range(n_seam)]
    for i, c in enumerate(cols):
        plant[i % n_seam].append(c)
    t = [p[case.rot % len(p)] for p in plant]
    kinds = ["seam"] * n_seam
    plant.append([IGNORE]), t.append(IGNORE), kinds.append("ignored")
    pairs = [p for p in TIE_PAIRS if p[0] != p[1] and _inside(p[0], V, cr) and _inside(p[1], V, cr)]
    if not pairs:
        pairs = [(0, 2)]
    tie = {}
    for k, kind in enumerate(("tie_low", "tie_high")):
        lo, hi = pairs[(case.seed + k) % len(pairs)]
        tie[len(t)] = (lo, hi)
        plant.append([]), t.append(lo if kind == "tie_low" else hi), kinds.append(kind)
    foreign = {}
    if case.variant != "none":
        own = cols[(case.rot + 1) % len(cols)]
        out = None
        if cr is not None:
            out = cr[1] if cr[1] < V else (cr[0] - 1 if cr[0] > 4 else None)
        if out is None and case.variant in ("mask", "both"):
            out = next(c for c in (V - 1, V - 2, 0, 2, 3) if _inside(c, V, cr) and c != own)
        if out is not None:
            foreign[len(t)] = out
            plant.append([own]), t.append(own), kinds.append("foreign")
    # a live target that is no allowed column: the foreign column where there is one, else a column outside [0, V) -- never dereferenced
    dead = next(iter(foreign.values()), V + 7 if case.seed % 2 else -3)
    plant.append([cols[0]]), t.append(dead), kinds.append("dead")
    assert len(t) <= MAX_ROWS, case
    return dict(t=t, plant=plant, tie=tie, foreign=foreign, kinds=kinds)


def build(case, dtype, device="cpu"):
    """-> dict(x [R, V] view of the [R, ld] storage of dtype (padding: PAD_FILL), t int64 [R], eps, crange, cmask (uint8 [R, V] or
    None), nodes (int32 [R] or None), trie, A bool [R, V] (CPU), leaks ({mutation: the allowed set of the case's range_edge /
    node_sibling_leak mutation}), constrained, fused, kinds)."""
    if case.form == "node":
        return _build_node(case, dtype, device)
    V = case.V
    ld = case.ld if case.ld is not None else (V + NVEC[dtype] - 1) // NVEC[dtype] * NVEC[dtype]
    lay = layout(case)
    R = len(lay["t"])
    store = co.make_case("planted", R, V, ld, lay["plant"], case.seed)
    for r, kind in enumerate(lay["kinds"]):
        if kind in ("seam", "foreign", "ignored"):
            store[r, lay["t"][r]] = TARGET_FILL
    for r, (lo, hi) in lay["tie"].items():
        store[r, lo] = store[r, hi] = TIE_FILL
    cmask = None
    if case.variant in ("mask", "both"):
        gen = torch.Generator(device="cpu").manual_seed(case.seed + 1)
        cmask = torch.rand(R, V, generator=gen) < 0.7
        for r in range(R):
            cmask[r, lay["plant"][r]] = True
            cmask[r, lay["t"][r]] = lay["kinds"][r] != "dead"          # (the dead row's target is the column the mask takes away)
            if r in lay["tie"]:
                cmask[r, list(lay["tie"][r])] = True
    for r, c in lay["foreign"].items():
        store[r, c] = FOREIGN_FILL
        if cmask is not None and (case.crange is None or _inside(c, V, case.crange)):
            cmask[r, c] = False
    store = store.to(dtype).to(device)
    t = torch.tensor(lay["t"], dtype=torch.int64)
    A = allowed_set(R, V, case.crange, cmask)
    leaks = {"range_edge": allowed_set(R, V, case.crange, cmask, inclusive_end=True)} if case.crange is not None else {}
    return dict(x=store[:, :V], t=t.to(device), eps=case.eps, crange=case.crange,
                cmask=None if cmask is None else cmask.to(torch.uint8).to(device), nodes=None, trie=None, A=A, leaks=leaks,
                constrained=case.variant != "none", fused=case.form == "regs" and dtype != torch.float32, kinds=lay["kinds"])


def _build_node(case, dtype, device):
    """A synthetic trie of closed_set_train_case with the validation planting on top: in every live row the target is raised to
    TARGET_FILL (the arg-max of the node's children; in every other live row a second child too: equal maxima, the lower token wins
    whatever the edge order) and a column that is NOT a child -- a child of node + 1 where there is one: the sibling -- to FOREIGN_FILL."""
    b = cst.build_trie_case(case.trie, dtype, "cpu")
    V = case.V
    store, t, nodes, A = b["store"].float(), b["t"], b["nodes"], b["A"]
    sib = allowed_set(len(t), V, case.crange, None, nodes, b["trie"], sibling_leak=True)
    for r, kind in enumerate(b["kinds"]):
        if kind != "live":
            continue
        store[r, int(t[r])] = TARGET_FILL
        others = [c for c in A[r].nonzero()[:, 0].tolist() if c != int(t[r]) and c != IGNORE]
        if r % 2 and others:                               # an equal maximum at another child: the lower TOKEN wins, whatever the edge order
            store[r, others[(case.seed + r) % len(others)]] = TARGET_FILL
        cand = (sib[r] & ~A[r]).nonzero()[:, 0].tolist() or (~A[r]).nonzero()[:, 0].tolist()
        cand = [c for c in cand if c != IGNORE]
        if cand:
            store[r, cand[0]] = FOREIGN_FILL
    store = store.to(dtype).to(device)
    trie = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in b["trie"].items()}
    return dict(x=store[:, :V], t=t.to(device), eps=case.eps, crange=case.crange, cmask=None, nodes=nodes.to(device), trie=trie, A=A,
                leaks={"node_sibling_leak": sib}, constrained=True, fused=False, kinds=b["kinds"])
