"""Closed-set training by trie node ids: the helpers and the kernel cases shared by tests/test_closed_set_nodes_cpu.py and
tests/test_closed_set_train_gpu.py.  TEST INFRASTRUCTURE: plain torch / numpy, no dependency on the kernels.

nodes_to_masks()   the bool [..., V] constraint masks a tensor of node ids stands for (the reference's sample["constraint_masks"]).
TRIE_CASES / build_trie_case()   synthetic tries and rows for ofa_trie_ls_cross_entropy_fwd / _bwd (csrc/trie_loss.hip), at most
                   MAX_ROWS rows each, logits from criterion_oracle.make_case in its two regimes.
step_batch()       a B = 4 closed-set micro-batch over tests/traverse_case.ANSWERS for the train-step tests.
"""
from collections import namedtuple

import numpy as np
import torch

from tests import criterion_oracle as co

MAX_ROWS = 8
FILL_TRIP = {torch.float32: 1024, torch.bfloat16: 2048, torch.float16: 2048}      # columns one trip of the 256-thread zero fill covers
GATHER_TRIP = 1024                                                                # edges one trip of the gather loop covers (256 x 4)


def nodes_to_masks(nodes, node_edge_off, edge_token, V):
    """bool [..., V]: row i allows the children of node nodes[i] that are columns of [0, V); a node outside [0, N) (-1: no closed set
    at that position) expands to an all-False row."""
    nodes = torch.as_tensor(np.asarray(nodes.cpu() if isinstance(nodes, torch.Tensor) else nodes)).long()
    off = np.asarray(node_edge_off.cpu() if isinstance(node_edge_off, torch.Tensor) else node_edge_off).astype(np.int64)
    tok = np.asarray(edge_token.cpu() if isinstance(edge_token, torch.Tensor) else edge_token).astype(np.int64)
    N = len(off) - 1
    flat = nodes.reshape(-1)
    out = torch.zeros(flat.numel(), V, dtype=torch.bool)
    for i, n in enumerate(flat.tolist()):
        if 0 <= n < N:
            ch = tok[off[n]:off[n + 1]]
            ch = ch[(ch >= 0) & (ch < V)]
            out[i, torch.from_numpy(ch)] = True
    return out.view(*nodes.shape, V)


# ---------------------------------------------------------------------------------------------------------------- kernel cases
# degrees: the number of children of the node of each live row.  1 is a finished answer (EOS only: eps_i = eps * 1e6), 63 / 64 / 65 a
# wave, 255 / 256 / 257 the block, 1023 / 1024 / 1025 one trip of the gather loop, 2049 one above two trips.
TrieCase = namedtuple("TrieCase", "V ld extra regime eps g crange degrees seed")     # extra: the row stride is ld + extra (a view)
# children first dealt from these columns: 0, 2 (EOS), 3, 4, the row's last, both sides of the 16-byte seams of fp32 (3|4, 7|8) and of
# the 16-bit types (7|8, 15|16), two in one vector (2, 3 / 8, 9), adjacent vectors (7, 8)
def SPECIAL(V):
    out = []
    for c in (0, 2, 3, 4, V - 1, 7, 8, 9, 16, 15):
        if c < V and c not in out:
            out.append(c)
    return out



JUNK = (-1, -7, 2 ** 31 - 1, 70000)            # edge tokens outside [0, V) (with V and V + 3): skipped, never dereferenced
GS = (1.0, 0.37, 128.0)
EPSS = (0.0, 0.1)


def _trie_cases():
    layouts = [
        (5, 8, 0, (1, 2, 4)),
        (257, 264, 0, (1, 2, 63, 64)),
        (257, 264, 0, (65, 255, 256, 257)),
        (257, 264, 64, (2, 64, 255, 257)),                   # a view of wider storage
        (1021, 1024, 0, (1, 63, 256, 1021)),                 # fp32: exactly one trip of the zero fill
        (1029, 1032, 0, (2, 65, 1023, 1025)),                # fp32: a second trip; the gather's trip seam
        (2045, 2048, 0, (1, 255, 1024, 2045)),               # 16-bit: exactly one trip of the zero fill
        (2053, 2056, 0, (1, 2, 1023, 1024)),                 # 16-bit: a second trip
        (2053, 2056, 0, (1025, 2049, 64, 257)),              # two trips of the gather loop and one edge more
    ]
    out, i = [], 0
    for V, ld, extra, degrees in layouts:
        for regime in co.REGIMES:
            out.append(TrieCase(V, ld, extra, regime, EPSS[(i // 2) % 2], GS[i % 3], None, degrees, 1300 + i))   # (eps walks with the layout)
            i += 1
    # a constraint range that cuts children away on both sides; the last special row's target is a child the range cuts
    out.append(TrieCase(257, 264, 0, "planted", 0.1, 0.37, (60, 200), (64, 255, 2), 1300 + i))
    out.append(TrieCase(257, 264, 0, "randn3", 0.0, 128.0, (60, 200), (65, 257, 1), 1301 + i))
    out.append(TrieCase(2053, 2056, 0, "planted", 0.1, 1.0, (1000, 2040), (1024, 2049, 2), 1302 + i))
    return out


TRIE_CASES = _trie_cases()
assert {c.g for c in TRIE_CASES} == set(GS) and {c.eps for c in TRIE_CASES} == set(EPSS)
assert {(c.regime, c.eps) for c in TRIE_CASES} == {(r, e) for r in co.REGIMES for e in EPSS}


def _children(V, degree, rng):
    """`degree` distinct columns: [2] alone for a finished answer, else the special columns first, the rest drawn from the other columns
    (the pad column 1 only when nothing else is left); in a shuffled edge order."""
    if degree == 1:
        return [2]
    sp = SPECIAL(V)
    ch = sp[:degree]
    if len(ch) < degree:
        rest = [c for c in range(V) if c not in sp and c != co.IGNORE]
        ch = ch + [rest[j] for j in rng.permutation(len(rest))[:degree - len(ch)]]
        if len(ch) < degree:
            ch.append(co.IGNORE)
    assert len(ch) == degree == len(set(ch)), (V, degree)
    order = rng.permutation(degree)
    return [int(ch[j]) for j in order]


def _in_range(c, crange):
    return crange is None or c < 4 or crange[0] <= c < crange[1]


def trie_layout(case):
    """-> dict(node_edge_off, edge_token (numpy int32), nodes, targets (lists), kinds, plant): one live row per degree on its own node,
    then an ignored row on the widest node, a filler row (node -1, <pad> target), a live target on node -1, a live target that is no
    child of its node and, with a constraint range, a live target that is a child the range cuts.  Node 0's edge list also carries the
    JUNK tokens.  plant[r]: the columns the `planted` regime raises in row r -- one allowed child and one disallowed column."""
    rng = np.random.Generator(np.random.Philox(key=case.seed))
    V, sp = case.V, SPECIAL(case.V)
    lists = [_children(V, d, rng) for d in case.degrees]
    junk = list(JUNK) + [V, V + 3]
    edges = [lists[0][:1] + junk[:3] + lists[0][1:] + junk[3:]] + lists[1:]
    off = np.zeros(len(edges) + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e in edges])
    tok = np.array([t for e in edges for t in e], np.int64).astype(np.int32)
    nodes, targets, kinds, plant = [], [], [], []
    for i, ch in enumerate(lists):
        ok = [c for c in ch if _in_range(c, case.crange) and c != co.IGNORE]
        edges_of_range = [] if case.crange is None else [case.crange[0], case.crange[1] - 1]       # (targets there where they are children)
        seams = [c for c in edges_of_range + sp if c in ok] or ok
        t = seams[i % len(seams)]
        allowed = seams[(i + 1) % len(seams)]
        cut = [c for c in ch if not _in_range(c, case.crange) and c != co.IGNORE]
        outside = cut or [c for c in sp + list(range(V)) if c not in ch and c != co.IGNORE]
        nodes.append(i), targets.append(t), kinds.append("live"), plant.append([allowed] + outside[:1])
    widest = int(np.argmax(case.degrees))
    narrow = next(i for i, d in enumerate(case.degrees) if d < V - 1)
    stranger = next(c for c in sp + list(range(V)) if c not in lists[narrow] and c != co.IGNORE)
    nodes += [widest, -1, -1, narrow]
    targets += [co.IGNORE, co.IGNORE, sp[1 % len(sp)], stranger]
    kinds += ["ignored", "filler", "dead_node", "not_child"]
    plant += [[lists[widest][0]], [], [sp[0]], [stranger]]
    if case.crange is not None:
        i = next(i for i, ch in enumerate(lists) if any(not _in_range(c, case.crange) for c in ch))
        t = next(c for c in lists[i] if not _in_range(c, case.crange) and c != co.IGNORE)
        nodes.append(i), targets.append(t), kinds.append("cut_target"), plant.append([t])
    assert len(nodes) <= MAX_ROWS, case
    return dict(node_edge_off=off, edge_token=tok, nodes=nodes, targets=targets, kinds=kinds, plant=plant)


ROW_W = ((1.0, 0.5, 1.0, 0.0, 1.0, 1.0, 0.5, 1.0), (0.0, 1.0, 0.5, 1.0, 0.5, 1.0, 1.0, 0.0))      # by the parity of the case's seed


def build_trie_case(case, dtype, device="cpu"):
    """-> dict(x [R, V] view of the [R, ld + extra] storage of dtype (padding: PAD_FILL), t int64 [R], nodes int32 [R], trie (the dict
    kernels take), row_w fp32 [R], A bool [R, V] (the allowed sets, range included), good (rows the float64 oracle covers: a valid node
    with an allowed child and a target that is ignored or allowed), kinds)."""
    lay = trie_layout(case)
    R, V, stride = len(lay["nodes"]), case.V, case.ld + case.extra
    base = co.make_case(case.regime, R, V, case.ld, lay["plant"], case.seed)
    store = torch.full((R, stride), co.PAD_FILL)
    store[:, :case.ld] = base
    store = store.to(dtype).to(device)
    t = torch.tensor(lay["targets"], dtype=torch.int64)
    nodes = torch.tensor(lay["nodes"], dtype=torch.int32)
    A = nodes_to_masks(nodes, lay["node_edge_off"], lay["edge_token"], V)
    if case.crange is not None:
        c = torch.arange(V)
        A = A & ((c < 4) | ((c >= case.crange[0]) & (c < case.crange[1])))[None, :]
    hit = A[torch.arange(R), t]
    good = A.any(1) & ((t == co.IGNORE) | hit)
    dead = (t != co.IGNORE) & ~hit
    want_dead = torch.tensor([k in ("dead_node", "not_child", "cut_target") for k in lay["kinds"]])
    assert torch.equal(dead, want_dead), (case, dead, lay["kinds"])
    assert torch.equal(A.sum(1)[:len(case.degrees)], torch.tensor(case.degrees)) or case.crange is not None
    trie = {"node_edge_off": torch.from_numpy(lay["node_edge_off"]).to(device), "edge_token": torch.from_numpy(lay["edge_token"]).to(device),
            "N": len(lay["node_edge_off"]) - 1, "E": len(lay["edge_token"])}
    return dict(x=store[:, :V], store=store, t=t.to(device), nodes=nodes.to(device), trie=trie,
                row_w=torch.tensor(ROW_W[case.seed % 2][:R], dtype=torch.float32, device=device), A=A.to(device), good=good.to(device),
                dead=dead.to(device), kinds=lay["kinds"], g=case.g, eps=case.eps, crange=case.crange)


# ---------------------------------------------------------------------------------------------------------------- the train-step batch
STEP_ANSWERS = ([[17, 23, 99], [40, 8, 120, 33], [17], [90, 150, 7]],          # two batches of other answers, the same lengths
                [[90, 12, 64], [17, 23, 99, 5], [61], [17, 23, 99]])


def step_batch(which, plan, V, bos=0, pad=1, eos=2):
    """-> dict(prev, target int64 [4, 5], nodes int32 [4, 5] (-1 at <pad> targets), masks bool [4, 5, V]) of STEP_ANSWERS[which];
    plan: the traverse.TraversePlan of tests/traverse_case.ANSWERS."""
    answers = STEP_ANSWERS[which]
    T = max(len(a) for a in answers) + 1
    prev = torch.full((len(answers), T), pad, dtype=torch.int64)
    target = torch.full((len(answers), T), pad, dtype=torch.int64)
    nodes = torch.full((len(answers), T), -1, dtype=torch.int32)
    for r, a in enumerate(answers):
        prev[r, :len(a) + 1] = torch.tensor([bos] + a)
        target[r, :len(a) + 1] = torch.tensor(a + [eos])
        nodes[r, :len(a) + 1] = torch.from_numpy(plan.walk(a))
    return dict(prev=prev, target=target, nodes=nodes, masks=nodes_to_masks(nodes, plan.node_edge_off, plan.edge_token, V))
