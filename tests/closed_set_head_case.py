"""The trie-edge head (csrc/trie_head.hip, ops.trie_head_cross_entropy): the cases and the float64 oracle shared by
tests/test_closed_set_head_cpu.py and tests/test_closed_set_head_gpu.py.  TEST INFRASTRUCTURE: plain torch / numpy, no dependency on
the kernels or on ofasys_amd.

head_reference()   rows x children in float64 from the STORED inputs: z from the features and weights in their storage dtype read as
                   float64 (or a given z: the kernel's own), the loss and the compact gradient g by criterion_oracle.lsce_reference's
                   formulas on the children, every magnitude bound beside its value.
dx_reference() / dw_reference()   the two gradient sums from a given g (the oracle's or the kernel's own), with their bounds.
dense_autograd()   the same loss through x @ W^T, the masks nodes_to_masks gives and the masked label-smoothed loss, by torch autograd.
HEAD_CASES / build_head_case()   closed_set_train_case.TRIE_CASES' layouts with features and a projection behind the logits, D rotating
                   through 8 / 512 / 520 / 768, and DW_CASE: the rows that share nodes and tokens.
"""
from collections import namedtuple

import numpy as np
import torch

from tests import closed_set_train_case as cst
from tests import criterion_oracle as co

U32 = 2.0 ** -24
# unit roundoff 2^-p of the storage dtypes (p significand bits, the implicit one included: 24, 8, 11) -- criterion_oracle.EPS's figures
U_T = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DS = (8, 512, 520, 768)          # one bf16 vector; one vector per lane (16-bit); one over; the model width
PLANT = 12.0

HeadCase = namedtuple("HeadCase", "trie D bias idx")
HEAD_CASES = [HeadCase(c, DS[i % len(DS)], i % 3 == 1, i) for i, c in enumerate(cst.TRIE_CASES)]
assert {c.D for c in HEAD_CASES} == set(DS) and {(c.trie.regime, c.D) for c in HEAD_CASES} >= {(r, 8) for r in co.REGIMES}


def invert_brute(edge_token):
    """-> (head_tokens [U] ascending, tok_edge_off [U + 1], tok_edge [E] ascending within a token), int32: the inverse of an edge list
    by brute force -- every distinct token (junk included: it is a value like any other) with the edges that carry it."""
    by = {}
    for e, t in enumerate(np.asarray(edge_token).tolist()):
        by.setdefault(int(t), []).append(e)
    toks = sorted(by)
    off = np.zeros(len(toks) + 1, np.int32)
    off[1:] = np.cumsum([len(by[t]) for t in toks])
    edges = [e for t in toks for e in by[t]]
    return np.array(toks, np.int32), off, np.array(edges, np.int32).reshape(-1)


def trie_dict(node_edge_off, edge_token, device="cpu"):
    """The device arrays the head's wrappers take (what TraversePlan.head_arrays hands out), from a CSR by node."""
    off, tok = np.asarray(node_edge_off, np.int32), np.asarray(edge_token, np.int32)
    N, E = len(off) - 1, len(tok)
    edge_node = np.repeat(np.arange(N, dtype=np.int32), np.diff(off))
    head, toff, tedge = invert_brute(tok)
    d = {k: torch.from_numpy(v).to(device) for k, v in
         dict(node_edge_off=off, edge_token=tok, edge_node=edge_node, head_tokens=head, tok_edge_off=toff, tok_edge=tedge).items()}
    d["node_ids"] = torch.arange(N + 1, dtype=torch.int32, device=device)
    d.update(N=N, E=E, U=len(head), max_degree=int(np.diff(off).max()))
    return d


# the rows that meet on nodes and tokens: node 0 carries three rows, node 1 two, token 9 hangs under both and is the target of rows
# 1, 2, 3 and a non-target child of rows 0 and 4; node 2's two children have bit-identical weight rows (the hit tie); node 3 has no
# row (tokens 33, 34 are touched by nobody); node 4's only row is ignored (tokens 35, 36 likewise)
DW_V = 40
DW_OFF = [0, 4, 7, 9, 11, 13]
DW_TOK = [5, 9, 12, 7, 9, 20, 3, 30, 31, 33, 34, 35, 36]
DW_NODES = [0, 0, 0, 1, 1, 4, 2, 2]
DW_TARGETS = [5, 9, 9, 9, 20, co.IGNORE, 30, 31]
DW_TWINS = (30, 31)
DW_UNTOUCHED = (33, 34, 35, 36)
DW_ROW_W = (1.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0)


def _f32(v):
    """the value as the fp32 device scalar holds it"""
    return float(torch.tensor(v, dtype=torch.float32))


def _features(R, V, D, regime, targets, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(R, D, generator=g)
    W = torch.randn(V, D, generator=g) * ((3.0 if regime == "randn3" else 1.0) / D ** 0.5)     # logits ~ 3 randn / randn, as make_case
    b = torch.randn(V, generator=g) * 0.5
    if regime == "planted":
        for r, t in enumerate(targets):
            if t != co.IGNORE and 0 <= t < V:
                W[t] += PLANT * x[r] / float((x[r] * x[r]).sum())
    return x, W, b


def build_head_case(case, dtype, device="cpu"):
    """-> dict(x [R, D], W [V, D], bias [V] or None (of dtype), t int64 [R], nodes int32 [R], trie, row_w fp32 [R], gs, eps, crange, kinds)."""
    tc = case.trie
    lay = cst.trie_layout(tc)
    R = len(lay["nodes"])
    x, W, b = _features(R, tc.V, case.D, tc.regime, lay["targets"], tc.seed)
    return dict(x=x.to(dtype).to(device), W=W.to(dtype).to(device), bias=b.to(dtype).to(device) if case.bias else None,
                t=torch.tensor(lay["targets"], dtype=torch.int64, device=device),
                nodes=torch.tensor(lay["nodes"], dtype=torch.int32, device=device),
                trie=trie_dict(lay["node_edge_off"], lay["edge_token"], device),
                row_w=torch.tensor(cst.ROW_W[tc.seed % 2][:R], dtype=torch.float32, device=device), gs=_f32(tc.g), eps=tc.eps, crange=tc.crange,
                kinds=lay["kinds"], V=tc.V, D=case.D)


def build_dw_case(dtype, D=72, device="cpu", bias=True):
    x, W, b = _features(len(DW_NODES), DW_V, D, "randn3", DW_TARGETS, 4242)
    W[DW_TWINS[1]] = W[DW_TWINS[0]]
    b[DW_TWINS[1]] = b[DW_TWINS[0]]
    return dict(x=x.to(dtype).to(device), W=W.to(dtype).to(device), bias=b.to(dtype).to(device) if bias else None,
                t=torch.tensor(DW_TARGETS, dtype=torch.int64, device=device), nodes=torch.tensor(DW_NODES, dtype=torch.int32, device=device),
                trie=trie_dict(DW_OFF, DW_TOK, device), row_w=torch.tensor(DW_ROW_W, dtype=torch.float32, device=device), gs=_f32(0.37), eps=0.1,
                crange=None, kinds=["live"] * 5 + ["ignored", "live", "live"], V=DW_V, D=D)


# ---------------------------------------------------------------------------------------------------------------- the oracle
def slots_of(b):
    """-> (tok int64 [R, Cmax] (-1 past the degree), A bool [R, Cmax]: the slot is an allowed child, deg [R]) on the CPU."""
    trie = b["trie"]
    off, etok = trie["node_edge_off"].cpu().numpy().astype(np.int64), trie["edge_token"].cpu().numpy().astype(np.int64)
    N, Cmax, V = trie["N"], trie["max_degree"], b["V"]
    nodes = b["nodes"].cpu().tolist()
    tok = torch.full((len(nodes), Cmax), -1, dtype=torch.int64)
    deg = torch.zeros(len(nodes), dtype=torch.int64)
    for r, n in enumerate(nodes):
        if 0 <= n < N:
            ch = etok[off[n]:off[n + 1]][:Cmax]
            tok[r, :len(ch)] = torch.from_numpy(ch)
            deg[r] = len(ch)
    inside = torch.arange(Cmax)[None, :] < deg[:, None]
    A = inside & (tok >= 0) & (tok < V)
    if b["crange"] is not None:
        A = A & ((tok < 4) | ((tok >= b["crange"][0]) & (tok < b["crange"][1])))
    return tok, A, deg


def head_reference(b, z=None):
    """float64, on the CPU.  z None: from the stored features and weights; else the given [R, Cmax] (the kernel's own stored z).
    -> dict(tok, A, deg, z, zbound [R, Cmax]; good, dead, ignored bool [R]; lse, row_loss, row_nll, row_cnt, hit [R]; g, gbound
    [R, Cmax]).  lse / row_loss / row_nll / g / gbound are filled on the good rows (an allowed child exists and the target is ignored
    or an allowed child) and zero elsewhere; g is the UNSCALED compact gradient, zero on ignored rows."""
    dt = torch.float64
    tok, A, deg = slots_of(b)
    R, Cmax = tok.shape
    x, W = b["x"].cpu().to(dt), b["W"].cpu().to(dt)
    t = b["t"].cpu()
    safe = tok.clamp(0, b["V"] - 1)
    Af = A.to(dt)
    zr = torch.stack([W[safe[r]] @ x[r] for r in range(R)]) * Af
    zb = W.shape[1] * U32 * torch.stack([W[safe[r]].abs() @ x[r].abs() for r in range(R)]) * Af
    if b["bias"] is not None:
        zr = zr + b["bias"].cpu().to(dt)[safe] * Af
        zb = zb + U32 * zr.abs()
    zz = zr if z is None else z.cpu().to(dt).masked_fill(~A, 0.0)
    ignored = t == co.IGNORE
    is_t = A & (tok == t[:, None])
    found = is_t.any(1)
    good = A.any(1) & (ignored | found)
    dead = ~ignored & ~found
    out = dict(tok=tok, A=A, deg=deg, z=zr, zbound=zb, good=good, dead=dead, ignored=ignored, row_cnt=Af.sum(1))
    for k in ("lse", "row_loss", "row_nll"):
        out[k] = torch.zeros(R, dtype=dt)
    out["g"], out["gbound"] = torch.zeros(R, Cmax, dtype=dt), torch.zeros(R, Cmax, dtype=dt)
    out["hit"] = torch.zeros(R, dtype=torch.int32)
    idx = good.nonzero()[:, 0]
    if idx.numel():
        # criterion_oracle.lsce_reference on the children: one more (disallowed) column stands for "ignored"
        xs = torch.cat([zz[idx], torch.zeros(idx.numel(), 1, dtype=dt)], 1).contiguous()
        cm = torch.cat([A[idx], torch.zeros(idx.numel(), 1, dtype=torch.bool)], 1)
        ts = torch.where(ignored[idx], torch.full_like(idx, Cmax), is_t[idx].to(torch.int64).argmax(1))
        ref, bd = co.lsce_reference(xs, ts, 1.0, b["eps"], cmask=cm, ignore=Cmax)
        for k in ("lse", "row_loss", "row_nll"):
            out[k][idx] = ref[k]
        out["g"][idx], out["gbound"][idx] = ref["d"][:, :Cmax], bd[:, :Cmax]
        # the arg-max of the allowed children as (value, lowest token)
        for i, r in enumerate(idx.tolist()):
            if ignored[r]:
                continue
            zrow = zz[r].masked_fill(~A[r], float("-inf"))
            best = tok[r][zrow == zrow.max()].min()
            out["hit"][r] = int(best == t[r])
    return out


def dx_reference(b, g, tok, A):
    """-> (dX, bound magnitude sum) float64 [R, D]: gs row_w[r] sum_j g[r, j] W[tok_j] over the allowed slots and sum |.|."""
    dt = torch.float64
    W = b["W"].cpu().to(dt)
    gg = g.cpu().to(dt).masked_fill(~A, 0.0) * (b["gs"] * b["row_w"].cpu().to(dt))[:, None]      # (slots past the degree are never read)
    safe = tok.clamp(0, b["V"] - 1)
    R = gg.shape[0]
    return (torch.stack([gg[r] @ W[safe[r]] for r in range(R)]), torch.stack([gg[r].abs() @ W[safe[r]].abs() for r in range(R)]))


def dw_reference(b, g, tok, A):
    """-> (dW [V, D], sum |g x| [V, D], n [V] contributing (row, edge) pairs, dbias [V], sum |g| [V]) float64: gs sum row_w g x."""
    dt = torch.float64
    x = b["x"].cpu().to(dt)
    V, D = b["V"], x.shape[1]
    c = g.cpu().to(dt).masked_fill(~A, 0.0) * (b["gs"] * b["row_w"].cpu().to(dt))[:, None]
    dW, mag, n = torch.zeros(V, D, dtype=dt), torch.zeros(V, D, dtype=dt), torch.zeros(V, dtype=dt)
    db, dbm = torch.zeros(V, dtype=dt), torch.zeros(V, dtype=dt)
    for r in range(c.shape[0]):
        on = A[r] & (c[r] != 0)
        if not bool(on.any()):
            continue
        tk, cr = tok[r][on], c[r][on]
        dW.index_add_(0, tk, cr[:, None] * x[r][None, :])
        mag.index_add_(0, tk, cr.abs()[:, None] * x[r].abs()[None, :])
        n.index_add_(0, tk, torch.ones_like(cr))
        db.index_add_(0, tk, cr)
        dbm.index_add_(0, tk, cr.abs())
    return dW, mag, n, db, dbm


def dense_autograd(b):
    """The loss the head stands for, by torch autograd in float64: logits = x W^T (+ bias), the masks the nodes stand for
    (closed_set_train_case.nodes_to_masks, the range cut in), the masked label-smoothed loss of the good rows at gs row_w.
    -> (loss_sum, dX [R, D], dW [V, D], dbias [V] or None, per-row loss [R])."""
    dt = torch.float64
    x = b["x"].cpu().to(dt).requires_grad_(True)
    W = b["W"].cpu().to(dt).requires_grad_(True)
    bias = b["bias"].cpu().to(dt).requires_grad_(True) if b["bias"] is not None else None
    t, V = b["t"].cpu(), b["V"]
    trie = b["trie"]
    # (the head clamps a degree to max_degree = the widest node: nothing is cut here)
    M = cst.nodes_to_masks(b["nodes"].cpu(), trie["node_edge_off"], trie["edge_token"], V)
    if b["crange"] is not None:
        c = torch.arange(V)
        M = M & ((c < 4) | ((c >= b["crange"][0]) & (c < b["crange"][1])))[None, :]
    R = x.shape[0]
    ignored = t == co.IGNORE
    good = M.any(1) & (ignored | M[torch.arange(R), t])
    logits = x @ W.t()
    if bias is not None:
        logits = logits + bias
    lp = torch.log_softmax(logits[good].masked_fill(~M[good], float("-inf")), 1)
    live = (~ignored[good]).to(dt)
    tg = torch.where(ignored[good], M[good].to(torch.int64).argmax(1), t[good])      # (an ignored row gathers an allowed column, times 0)
    C = M[good].sum(1).to(dt)
    eps_i = b["eps"] / (C - 1 + 1e-6)
    nll = -lp.gather(1, tg[:, None])[:, 0]
    smooth = -lp.masked_fill(~M[good], 0.0).sum(1)
    rows = ((1 - b["eps"] - eps_i) * nll + eps_i * smooth) * live
    total = (rows * b["row_w"].cpu().to(dt)[good]).sum() * b["gs"]
    total.backward()
    full = torch.zeros(R, dtype=dt)
    full[good] = rows.detach()
    return total.detach(), x.grad, W.grad, None if bias is None else bias.grad, full
