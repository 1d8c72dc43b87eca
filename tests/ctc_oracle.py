"""CTC loss (csrc/ctc.hip, ops.ctc_loss / ops.ctc_greedy_decode): the float64 oracle and the cases shared by tests/test_ctc_cpu.py and
tests/test_ctc_gpu.py.  TEST INFRASTRUCTURE: numpy and torch on the CPU, no dependency on the kernels or on ofasys_amd.

ctc_reference()   F.ctc_loss(log_softmax(x), blank=0, reduction="sum", zero_infinity) restated in float64 numpy: the loss, the
                  per-sentence NLL, the gradient with respect to the logits and the greedy decode.  An infeasible sentence has
                  nll = +inf and NaN gradient rows (torch's values), 0 and zero rows under zero_infinity.
torch_reference() the same through torch on the CPU in a given dtype: what test_ctc_cpu pins the oracle against (float64) and what
                  gives the GPU tests their measured bound (float32: the reference's own error).
CASES / build()   the case list; every case is a padded T x B x C batch, a packed form of the same sentences is derived from it.
"""
from collections import namedtuple

import numpy as np
import torch

DS, PAD, EOS = 10, 1, 2          # <phone>_dict_begin, <pad>, <eos> of the test dictionary: labels are encoder_target - DS
ALIGN = 8                        # packing.ALIGN: a packed sentence starts on an 8-row boundary

Case = namedtuple("Case", "name C sents scale feasible tight", defaults=(False,))
# sents: ((T, labels), ...); scale: the logits are unit normal times it; tight: the target row is exactly the labels (no <eos>, no <pad>),
# so that its width -- which picks the recursion kernel -- is L


def _norep(L, C, seed):
    """L labels in [1, C) without equal neighbours (C >= 3): feasible at T = L."""
    r = np.random.RandomState(seed)
    out = []
    for _ in range(L):
        c = int(r.randint(1, C))
        while out and c == out[-1]:
            c = int(r.randint(1, C))
        out.append(c)
    return out


def _cases():
    cs = [
        Case("t1_l0", 5, ((1, []),), 1.0, True),
        Case("t1_l1", 5, ((1, [3]),), 1.0, True),
        Case("t_eq_l", 7, ((6, [1, 2, 3, 4, 5, 6]),), 1.0, True),
        Case("l0_t7", 5, ((7, []),), 1.0, True),
        Case("repeat_t3", 5, ((3, [2, 2]),), 1.0, True),
        Case("repeat_t2", 5, ((2, [2, 2]),), 1.0, False),
        Case("t_lt_l", 5, ((2, [1, 2, 3, 4]),), 1.0, False),
    ]
    # S = 2 L + 1 around a wave (63, 65), two waves (127, 129), the workgroup (255, 257) and the three-states-per-thread kernel (767, 769)
    for L in (31, 32, 63, 64, 127, 128, 383, 384):
        cs.append(Case(f"S{2 * L + 1}", 5, ((L + 9, _norep(L, 5, L)),), 1.0, True, True))
    for C in (2, 5, 64, 65, 300):
        lab = [1, 1, 1, 1] if C == 2 else [1, C - 1, C - 1, 2]
        cs.append(Case(f"C{C}", C, ((12, lab),), 1.0, True))
    cs.append(Case("mixed", 11, ((9, [3, 4, 4]), (5, [1, 2, 3, 4, 5]), (1, []), (7, [10, 9]), (12, [6, 6, 6, 1, 6])), 1.0, True))
    cs.append(Case("mixed_inf", 11, ((9, [3, 4, 4]), (3, [1, 2, 3, 4, 5]), (4, [7, 7, 7]), (7, [10, 9]), (2, [])), 1.0, False))
    cs.append(Case("sharp", 32, ((600, _norep(40, 32, 7)),), 20.0, True))
    return cs


CASES = _cases()
CASE = {c.name: c for c in CASES}


def build(case, seed=0):
    """-> dict(x float64 [T, B, C] (rows past a sentence's length are random too: nothing may read them), lengths [B], labels (lists),
    target int64 [B, Lmax]: the labels + DS, with an interior EOS and trailing PAD in the rows that have room."""
    B = len(case.sents)
    T = max(t for t, _ in case.sents)
    Lmax = max(1, max(len(l) for _, l in case.sents)) + (0 if case.tight else 2)
    r = np.random.RandomState(1000 + seed + sum(map(ord, case.name)))
    x = r.randn(T, B, case.C) * case.scale
    target = np.full((B, Lmax), PAD, np.int64)
    for b, (_, lab) in enumerate(case.sents):
        row = [v + DS for v in lab]
        if case.tight:
            target[b, :len(row)] = row
            continue
        if len(lab) >= 2:
            row.insert(len(lab) // 2, EOS)           # an interior <eos>: skipped, the labels behind it still count
        row.append(EOS)
        target[b, :len(row)] = row                   # (an empty sentence: <eos> then <pad>; see `all_pad` in the GPU tests for the all-pad row)
    return dict(x=x, lengths=np.array([t for t, _ in case.sents], np.int64), labels=[list(l) for _, l in case.sents], target=target,
                T=T, B=B, C=case.C)


def labels_of(target_row, ds=DS, pad=PAD, eos=EOS):
    return [int(v) - ds for v in target_row if v != pad and v != eos]


def pack(x, lengths):
    """The packed rows of a padded [T, B, C] batch as packing._layout lays them out: -> (rows [R, C], offsets); filler rows are random."""
    T, B, C = x.shape
    offs, n = [], 0
    for b in range(B):
        offs.append(n)
        n += (int(lengths[b]) + ALIGN - 1) // ALIGN * ALIGN
    rows = np.random.RandomState(5).randn(max(n, ALIGN), C)
    for b in range(B):
        rows[offs[b]:offs[b] + int(lengths[b])] = x[:int(lengths[b]), b]
    return rows, offs


def _lse(a, axis=None):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True))).squeeze(axis)


def sentence_reference(x, labels):
    """x float64 [T, C], labels: list in [1, C).  -> (nll, grad [T, C] of nll, NaN if infeasible)."""
    T, C = x.shape
    lp = x - _lse(x, axis=1)[:, None]
    L = len(labels)
    S = 2 * L + 1
    ext = np.zeros(S, np.int64)
    ext[1::2] = labels
    skip_f = np.zeros(S, bool)
    skip_f[3::2] = ext[3::2] != ext[1:-2:2]
    skip_b = np.zeros(S, bool)
    skip_b[1:-2:2] = ext[1:-2:2] != ext[3::2]
    NEG = -np.inf
    alpha = np.full((T, S), NEG)
    beta = np.full((T, S), NEG)
    alpha[0, 0] = lp[0, 0]
    if S > 1:
        alpha[0, 1] = lp[0, ext[1]]
    beta[T - 1, S - 1] = lp[T - 1, 0]
    if S > 1:
        beta[T - 1, S - 2] = lp[T - 1, ext[S - 2]]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            p = alpha[t - 1]
            a1 = np.concatenate([[NEG], p])[:S]
            a2 = np.where(skip_f, np.concatenate([[NEG, NEG], p])[:S], NEG)
            alpha[t] = lp[t, ext] + _lse(np.stack([p, a1, a2]), axis=0)
        for t in range(T - 2, -1, -1):
            p = beta[t + 1]
            b1 = np.concatenate([p, [NEG]])[1:]
            b2 = np.where(skip_b, np.concatenate([p, [NEG, NEG]])[2:], NEG)
            beta[t] = lp[t, ext] + _lse(np.stack([p, b1, b2]), axis=0)
    tail = alpha[T - 1, S - 2:] if S > 1 else alpha[T - 1, S - 1:]
    nll = -float(_lse(tail))
    if not np.isfinite(nll):
        return np.inf, np.full((T, C), np.nan)
    ab = alpha + beta
    occ = np.zeros((T, C))
    with np.errstate(over="ignore"):
        for s in range(S):
            occ[:, ext[s]] += np.exp(ab[:, s] - lp[:, ext[s]] + nll)
    return nll, np.exp(lp) - occ


def greedy_reference(x):
    """x [T, C] -> the greedy decode: row arg-max (the LOWEST class among equal maxima: np.argmax's rule and the kernel's), consecutive
    duplicates collapsed, blanks dropped."""
    am = np.argmax(x, axis=1).tolist() if len(x) else []
    return [c for i, c in enumerate(am) if c != 0 and (i == 0 or c != am[i - 1])]


def ctc_reference(x, lengths, labels, zero_infinity):
    """x float64 [T, B, C] -> dict(loss, nll [B], grad [T, B, C] (exact zeros past each length), decode: list of lists)."""
    T, B, C = x.shape
    nll = np.zeros(B)
    grad = np.zeros_like(x)
    dec = []
    for b in range(B):
        n = int(lengths[b])
        lab = labels[b]
        if n == 0:
            v, g = (0.0 if not lab else np.inf), np.zeros((0, C))
        elif any(not 1 <= c < C for c in lab):
            v, g = np.inf, np.full((n, C), np.nan)
        else:
            v, g = sentence_reference(x[:n, b], lab)
        if not np.isfinite(v) and zero_infinity:
            v, g = 0.0, np.zeros((n, C))
        nll[b] = v
        grad[:n, b] = g
        dec.append(greedy_reference(x[:n, b]))
    return dict(loss=float(nll.sum()), nll=nll, grad=grad, decode=dec)


def torch_reference(x, lengths, labels, zero_infinity, dtype):
    """x: tensor [T, B, C] -> (loss, nll [B], grad [T, B, C]) by torch on the CPU in `dtype`: log_softmax, F.ctc_loss, autograd."""
    xt = x.detach().to("cpu", dtype).clone().requires_grad_(True)
    flat = torch.tensor([c for l in labels for c in l], dtype=torch.int64)
    tl = torch.tensor([len(l) for l in labels], dtype=torch.int64)
    il = torch.as_tensor(np.asarray(lengths), dtype=torch.int64)
    lp = torch.log_softmax(xt, -1)
    nll = torch.nn.functional.ctc_loss(lp, flat, il, tl, blank=0, reduction="none", zero_infinity=zero_infinity)
    loss = torch.nn.functional.ctc_loss(lp, flat, il, tl, blank=0, reduction="sum", zero_infinity=zero_infinity)
    loss.backward()
    return float(loss.detach()), nll.detach().double().numpy(), xt.grad.double().numpy()


def levenshtein_pairs():
    """Hand-worked (a, b, distance) triples for the host edit distance."""
    return [([], [], 0), ([1, 2, 3], [], 3), ([], [4], 1), ([1, 2, 3], [1, 2, 3], 0), ([1, 2, 3], [1, 3], 1), ([1, 2, 3], [2, 3, 4], 2),
            ([5, 6, 7, 8], [5, 7, 6, 8], 2), ([1, 1, 1], [2, 2, 2], 3), ([1, 2], [2, 1], 2), ([3, 4, 5, 6, 7], [4, 5, 9, 7], 2)]
