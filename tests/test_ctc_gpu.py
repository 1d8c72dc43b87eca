"""GPU: the CTC kernels (csrc/ctc.hip) through ops.ctc_loss / ops.ctc_greedy_decode against the float64 oracle of tests/ctc_oracle.py.

Bound (the project's own-reference-gap convention), per case and zero_infinity value, on the inputs the kernel reads
(16-bit cases: the rounded logits), as the issue states it:
    e_ref   = |torch fp32 CPU (log_softmax + F.ctc_loss + autograd) - oracle|, taken for the loss, for each sentence's nll and for EACH
              gradient element on its own
    floor   = eps32 * T, absolute: fp32 epsilon times the number of sequential log-add steps
    bound   = 2 * e_ref + floor, plus for a gradient stored in bf16 / fp16 half an ulp of the stored value (u_T |g|, and half the fp16
              subnormal spacing 2^-25)
The measured ratios error / bound go to the file $OFA_CTC_PARITY_OUT names (tools/ctc_bench.py collects profiles/ctc_parity_measured.txt).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import ctc_oracle as co

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
U_T = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
BOTH = ("repeat_t3",)            # a feasible case that runs with zero_infinity on and off, like the infeasible ones


def _params():
    out = []
    for c in co.CASES:
        for dt in DTYPES:
            for zi in ((False, True) if (not c.feasible or c.name in BOTH) else (False,)):
                out.append(pytest.param(c.name, dt, zi, id=f"{c.name}-{dt}-{'zi' if zi else 'inf'}"))
    return out


@functools.lru_cache(maxsize=None)
def _prepared(name, dt):
    """The case's inputs rounded to the dtype, on the CPU, with the oracle's and torch-fp32's results for both zero_infinity values."""
    d = co.build(co.CASE[name])
    xq = torch.from_numpy(d["x"]).to(DTYPES[dt])
    d["xq"] = xq
    x64 = xq.double().numpy()
    d["ref"], d["t32"] = {}, {}
    for zi in (False, True):
        d["ref"][zi] = co.ctc_reference(x64, d["lengths"], d["labels"], zi)
        d["t32"][zi] = co.torch_reference(xq, d["lengths"], d["labels"], zi, torch.float32)
    return d


def _run(xq, lengths, target, zi, layout="padded", seed=None, want_decode=False):
    """-> (loss, nll [B], grad [T, B, C] as float64 numpy from the kernel's dtype, decode) through the public ops on cuda:0."""
    from ofasys_amd import ops
    T, B, C = xq.shape
    dev = "cuda:0"
    tgt = torch.from_numpy(np.asarray(target)).to(dev)
    if layout == "padded":
        x = xq.to(dev).clone().requires_grad_(True)
        lay = ops.CtcLayout.padded(torch.as_tensor(np.asarray(lengths)).to(dev), T)
    else:
        rows, offs = co.pack(xq.double().numpy(), lengths)
        x = torch.from_numpy(rows).to(xq.dtype).to(dev).view(-1, 1, C).requires_grad_(True)
        seg = torch.tensor([[offs[b], int(lengths[b]), offs[b], int(lengths[b])] for b in range(B)], dtype=torch.int32, device=dev)
        lay = ops.CtcLayout(seg, 1, (int(max(lengths)) + 31) // 32 * 32)
    loss, nll = ops.ctc_loss(x, lay, tgt, co.DS, co.PAD, co.EOS, zi, seed=seed)
    if seed is not None:
        loss.backward(seed)
    else:
        loss.backward()
    dec = None
    if want_decode:
        toks, n = ops.ctc_greedy_decode(x.detach(), lay)
        toks, n = toks.cpu().numpy(), n.cpu().numpy()
        dec = [toks[b, :n[b]].tolist() for b in range(B)]
        assert all((toks[b, n[b]:] == -1).all() for b in range(B))
    g = x.grad
    if layout == "packed":
        full = torch.zeros(T, B, C, dtype=g.dtype, device=dev)
        live = torch.zeros(g.shape[0], dtype=torch.bool, device=dev)
        for b in range(B):
            n_b = int(lengths[b])
            full[:n_b, b] = g[offs[b]:offs[b] + n_b, 0]
            live[offs[b]:offs[b] + n_b] = True
        assert bool((g[~live] == 0).all()), "a packed row outside every sentence has a non-zero gradient"
        g = full
    return float(loss), nll.double().cpu().numpy(), g, dec


def _record(line):
    path = os.environ.get("OFA_CTC_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check(name, dt, zi, loss, nll, g_t, layout="padded"):
    d = _prepared(name, dt)
    _check_against(name, dt, zi, d, d["ref"][zi], d["t32"][zi], loss, nll, g_t, layout)


def _check_against(name, dt, zi, d, ref, t32, loss, nll, g_t, layout="padded"):
    """d: the case (T, B, lengths); ref: the oracle's result; t32: torch's fp32 CPU result on the same inputs."""
    tl, tn, tg = t32
    T = d["T"]
    g = g_t.double().cpu().numpy()
    assert not np.isnan(nll).any()
    fin_s = np.isfinite(ref["nll"])
    assert (np.isposinf(nll) == ~fin_s).all(), (nll, ref["nll"])
    # per-sentence nll and the loss
    e_ref = np.abs(tn[fin_s] - ref["nll"][fin_s])
    err = np.abs(nll[fin_s] - ref["nll"][fin_s])
    bound = 2 * e_ref + EPS32 * T
    r_nll = float((err / bound).max()) if fin_s.any() else 0.0
    if fin_s.all():
        lb = 2 * abs(tl - ref["loss"]) + EPS32 * T
        r_loss = abs(loss - ref["loss"]) / lb
    else:
        assert loss == float("inf")
        r_loss = 0.0
    # the gradient: NaN exactly where the oracle's is (the live rows of an infeasible sentence without zero_infinity), exact zeros past
    # every length, and the bound elsewhere
    fin = np.isfinite(ref["grad"])
    assert (np.isnan(g) == ~fin).all()
    for b in range(d["B"]):
        assert (g[int(d["lengths"][b]):, b] == 0).all(), "a row past the sentence's length has a non-zero gradient"
    e_g = float(np.abs(tg[fin] - ref["grad"][fin]).max()) if fin.any() else 0.0
    with np.errstate(invalid="ignore"):
        gb = 2 * np.abs(tg - ref["grad"]) + EPS32 * T + U_T[dt] * np.abs(ref["grad"]) + (2.0 ** -25 if dt == "fp16" else 0.0)
    r_g = float((np.abs(g - ref["grad"])[fin] / gb[fin]).max()) if fin.any() else 0.0
    line = (f"{name:10s} {dt} {layout:6s} zero_infinity={int(zi)} T={T} loss {ref['loss']:.6g}: error/bound loss {r_loss:.3f} nll {r_nll:.3f} "
            f"grad {r_g:.3f}   (torch fp32 error: loss {abs(tl - ref['loss']) if fin_s.all() else 0:.3g} grad {e_g:.3g})")
    print(line)
    _record(line)
    assert r_loss <= 1.0 and r_nll <= 1.0 and r_g <= 1.0, line


@pytest.mark.parametrize("name,dt,zi", _params())
def test_case_against_the_oracle(name, dt, zi):
    d = _prepared(name, dt)
    loss, nll, g, _ = _run(d["xq"], d["lengths"], d["target"], zi)
    _check(name, dt, zi, loss, nll, g)


def test_feasible_cases_have_finite_oracle_values():
    for c in co.CASES:
        ref = _prepared(c.name, "fp32")["ref"][False]
        assert np.isfinite(ref["loss"]) == c.feasible, c.name


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name,zi", [("mixed", False), ("mixed_inf", True), ("mixed_inf", False)])
def test_packed_layout_equals_padded_bit_for_bit(name, dt, zi):
    d = _prepared(name, dt)
    lp, np_, gp, _ = _run(d["xq"], d["lengths"], d["target"], zi, "padded")
    lk, nk, gk, _ = _run(d["xq"], d["lengths"], d["target"], zi, "packed")
    _check(name, dt, zi, lk, nk, gk, "packed")
    assert np.array_equal(np_, nk) and (lp == lk or (lp != lp and lk != lk))
    assert torch.equal(gp.view(torch.int16 if dt != "fp32" else torch.int32), gk.view(torch.int16 if dt != "fp32" else torch.int32))


def test_all_pad_target_row_and_interior_eos():
    """An all-<pad> target row is the empty label sequence; <eos> inside a row is skipped and the labels behind it still count."""
    d = _prepared("mixed", "fp32")
    target = d["target"].copy()
    labels = [list(l) for l in d["labels"]]
    target[0, :] = co.PAD
    labels[0] = []
    assert any(co.EOS in row[:len(l)] for row, l in zip(target.tolist(), labels) if len(l) >= 2)        # (build() plants it)
    assert [co.labels_of(r) for r in target] == labels
    ref = co.ctc_reference(d["xq"].double().numpy(), d["lengths"], labels, False)
    t32 = co.torch_reference(d["xq"], d["lengths"], labels, False, torch.float32)
    loss, nll, g, _ = _run(d["xq"], d["lengths"], target, False)
    _check_against("all_pad", "fp32", False, d, ref, t32, loss, nll, g)


def test_label_outside_the_classes_is_infeasible_not_a_wild_read():
    d = _prepared("mixed", "fp32")
    target = d["target"].copy()
    target[1, 0] = co.DS + d["C"]                     # label C: one past the last class
    target[3, 0] = co.DS                              # label 0: the blank row itself is no label
    for zi in (True, False):
        loss, nll, g, _ = _run(d["xq"], d["lengths"], target, zi)
        g = g.double().cpu().numpy()
        for b in (1, 3):
            n = int(d["lengths"][b])
            if zi:
                assert nll[b] == 0 and (g[:, b] == 0).all()
            else:
                assert nll[b] == float("inf") and np.isnan(g[:n, b]).all() and (g[n:, b] == 0).all()
        assert np.isfinite(nll[[0, 2, 4]]).all() and np.isfinite(g[:, [0, 2, 4]]).all()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_two_calls_give_equal_bits_and_the_seeded_forward_equals_the_backward(dt):
    d = _prepared("mixed", dt)
    a = _run(d["xq"], d["lengths"], d["target"], False)
    b = _run(d["xq"], d["lengths"], d["target"], False)
    one = torch.ones((), dtype=torch.float32, device="cuda:0")
    c = _run(d["xq"], d["lengths"], d["target"], False, seed=one)
    for o in (b, c):
        assert a[0] == o[0] and np.array_equal(a[1], o[1]) and torch.equal(a[2], o[2])
    # a seed other than one scales the gradient (fp16 loss scaling): the seeded forward and a backward given another tensor agree
    s = torch.full((), 0.5, dtype=torch.float32, device="cuda:0")
    e = _run(d["xq"], d["lengths"], d["target"], False, seed=s)
    # (a power of two: exact in every dtype but for fp16 subnormals, which may round: half their spacing)
    assert float((e[2].float() - a[2].float() * 0.5).abs().max()) <= (2.0 ** -25 if dt == "fp16" else 0.0)


def test_capture_replays_with_changed_lengths_in_the_same_buffers():
    from ofasys_amd import ops
    d = _prepared("mixed", "bf16")
    dev = "cuda:0"
    T, B, C = d["xq"].shape
    x = d["xq"].to(dev)
    lengths = torch.as_tensor(d["lengths"]).to(dev)
    tgt = torch.from_numpy(d["target"]).to(dev)
    seed = torch.ones((), dtype=torch.float32, device=dev)
    lay = ops.CtcLayout.padded(lengths, T)
    variants = [(d["lengths"], d["target"])]
    l2 = d["lengths"].copy()
    l2[0], l2[4] = 4, 9
    t2 = d["target"].copy()
    t2[3] = t2[0]
    variants.append((l2, t2))

    def step():
        xx = x.detach().requires_grad_(True)
        loss, nll = ops.ctc_loss(xx, lay, tgt, co.DS, co.PAD, co.EOS, True, seed=seed)
        loss.backward(seed)
        return loss.detach(), nll, xx.grad

    eager = []
    for ln, tg in variants:
        lay.seg[:, 1].copy_(torch.as_tensor(ln).to(dev))
        tgt.copy_(torch.from_numpy(tg).to(dev))
        eager.append([t.clone() for t in step()])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for rep in range(2):
        for (ln, tg), want in zip(variants, eager):
            lay.seg[:, 1].copy_(torch.as_tensor(ln).to(dev))
            tgt.copy_(torch.from_numpy(tg).to(dev))
            g.replay()
            torch.cuda.synchronize()
            for got, w in zip(out, want):
                assert torch.equal(got, w)
    assert not torch.equal(eager[0][2], eager[1][2])


def test_greedy_decode_equals_the_oracle_with_ties():
    """Tie rule: among equal top logits the LOWEST class wins (a tie with the blank decodes as blank)."""
    d = _prepared("mixed", "fp32")
    x = d["xq"].clone()
    top = float(x.max()) + 1.0
    x[0, 0, 4], x[0, 0, 7] = top, top                 # row 0 of sentence 0: classes 4 and 7 tie -> 4
    x[1, 0, 0], x[1, 0, 9] = top, top                 # row 1: the blank ties with class 9 -> blank
    x[2, 0, 4] = top                                  # rows 2, 3: 4 twice -> one 4 (a new token: a blank lies between it and row 0's)
    x[3, 0, 4] = top
    ref = co.ctc_reference(x.double().numpy(), d["lengths"], d["labels"], True)
    assert ref["decode"][0][:2] == [4, 4]
    for layout in ("padded", "packed"):
        dec = _run(x, d["lengths"], d["target"], True, layout, want_decode=True)[3]
        assert dec == ref["decode"], (layout, dec, ref["decode"])


def test_wrapper_refuses_too_many_classes_and_states():
    from ofasys_amd import kernels as K, ops
    cmax, lmax = K.ctc_limits()
    dev = "cuda:0"
    lay = ops.CtcLayout.padded(torch.tensor([2], device=dev), 2)
    with pytest.raises(ValueError, match="classes"):
        ops.ctc_loss(torch.zeros(2, 1, cmax + 1, device=dev), lay, torch.full((1, 3), co.PAD, device=dev), co.DS, co.PAD, co.EOS, True)
    with pytest.raises(ValueError, match="states"):
        ops.ctc_loss(torch.zeros(2, 1, 8, device=dev), lay, torch.full((1, lmax + 1), co.PAD, device=dev), co.DS, co.PAD, co.EOS, True)


def test_encoder_ctc_logits_projects_the_slice_and_lands_its_gradient_in_those_rows():
    from ofasys_amd import ops
    torch.manual_seed(0)
    dev = "cuda:0"
    enc = torch.randn(6, 2, 16, device=dev, requires_grad=True)
    w = torch.randn(40, 16, device=dev, requires_grad=True)
    ds, de = 8, 24
    y = ops.encoder_ctc_logits(enc, w, ds, de)
    dy = torch.randn_like(y)
    y.backward(dy)
    e2 = enc.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    y2 = torch.nn.functional.linear(e2, w2[ds:de])
    y2.backward(dy)
    assert torch.allclose(y, y2, rtol=1e-5, atol=1e-5) and torch.allclose(enc.grad, e2.grad, rtol=1e-5, atol=1e-5)
    assert torch.allclose(w.grad, w2.grad, rtol=1e-5, atol=1e-5)
    assert bool((w.grad[:ds] == 0).all()) and bool((w.grad[de:] == 0).all())
