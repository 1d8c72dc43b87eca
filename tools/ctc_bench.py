"""The CTC loss launches (csrc/ctc.hip through ops.ctc_loss: row pass, alpha / beta, gradient, loss sum) against torch's own device
composition -- log_softmax (fp32) + F.ctc_loss(reduction="sum", zero_infinity) forward and backward -- on the SAME tensors, GPU only.
Shapes: B = 32, T = 500, Lmax = 100, C = 256 in bf16 (an ASR micro-batch: input lengths 300 .. 500, 40 .. 100 labels), and a small
one (B = 4, T = 50, Lmax = 12, C = 32).  Each arm is forward + gradient of the logits.  Times are device events around `inner`
back-to-back calls (warm: the inputs stay in the caches), after a warm-up, the two arms alternated, median / min / max over the runs;
a cold figure evicts the caches before every single call (a 512 MiB fill) and times that one call.  --parity FILE: the error / bound
lines tests/test_ctc_gpu.py wrote ($OFA_CTC_PARITY_OUT) are copied to profiles/ctc_parity_measured.txt under the same source id.
Writes what it prints to profiles/ctc_bench.txt (--out).  Usage: python tools/ctc_bench.py"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LINES = []
DS, PAD, EOS = 10, 1, 2


def say(s):
    print(s, flush=True)
    LINES.append(s)


def batch(B, T, Lmax, C, tmin, lmin, dev, dtype):
    r = np.random.RandomState(3)
    x = torch.from_numpy(r.randn(T, B, C)).to(dtype).to(dev)
    lengths = r.randint(tmin, T + 1, size=B)
    lengths[0] = T
    nlab = r.randint(lmin, Lmax + 1, size=B)
    nlab[0] = Lmax
    target = np.full((B, Lmax), PAD, np.int64)
    labels = []
    for b in range(B):
        lab = r.randint(1, C, size=nlab[b])
        target[b, :nlab[b]] = lab + DS
        labels.append(lab)
    return x, torch.from_numpy(lengths).to(dev), torch.from_numpy(target).to(dev), labels


def arms(x, lengths, target, labels):
    from ofasys_amd import ops
    T, B, C = x.shape
    dev = x.device
    lay = ops.CtcLayout.padded(lengths, T)
    seed = torch.ones((), dtype=torch.float32, device=dev)
    flat = torch.from_numpy(np.concatenate(labels)).to(dev)
    tl = torch.tensor([len(l) for l in labels], device=dev)

    def ours():
        xx = x.detach().requires_grad_(True)
        loss, _ = ops.ctc_loss(xx, lay, target, DS, PAD, EOS, True, seed=seed)
        loss.backward(seed)
        return loss.detach(), xx.grad

    def theirs():
        xx = x.detach().requires_grad_(True)
        lp = torch.log_softmax(xx.float(), -1)
        loss = torch.nn.functional.ctc_loss(lp, flat, lengths, tl, blank=0, reduction="sum", zero_infinity=True)
        loss.backward()
        return loss.detach(), xx.grad

    return ours, theirs


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def shape_bench(tag, B, T, Lmax, C, tmin, lmin, dev, runs=7, inner=20):
    x, lengths, target, labels = batch(B, T, Lmax, C, tmin, lmin, dev, torch.bfloat16)
    ours, theirs = arms(x, lengths, target, labels)
    lo, go = ours()
    lt, gt = theirs()
    say(f"({tag}) B = {B}, T = {T}, Lmax = {Lmax}, C = {C}, bf16 logits; input lengths {int(lengths.min())} .. {int(lengths.max())}, "
        f"{min(map(len, labels))} .. {max(map(len, labels))} labels; forward + gradient, {runs} alternated runs of {inner} calls, device events")
    say(f"    loss: csrc/ctc.hip {float(lo):.4f}, torch {float(lt):.4f}; largest gradient difference {float((go.float() - gt.float()).abs().max()):.3g}")
    for fn in (ours, theirs):
        timed(fn, 5)
    res = {"ours": [], "torch": []}
    for _ in range(runs):
        res["ours"].append(timed(ours, inner))
        res["torch"].append(timed(theirs, inner))
    evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    cold = {"ours": [], "torch": []}
    for _ in range(5):
        for name, fn in (("ours", ours), ("torch", theirs)):
            evict.fill_(1)
            torch.cuda.synchronize()
            cold[name].append(timed(fn, 1))
    names = {"ours": "csrc/ctc.hip, 4 launches + zero fill", "torch": "torch log_softmax + F.ctc_loss     "}
    for k in ("ours", "torch"):
        v, c = res[k], cold[k]
        say(f"    {names[k]}: warm median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f}); "
            f"cold single call median {statistics.median(c):8.1f} us (min {min(c):.1f}, max {max(c):.1f})")
    mo, mt = statistics.median(res["ours"]), statistics.median(res["torch"])
    say(f"    csrc/ctc.hip / torch = {mo / mt:.2f} (warm medians; both include the host's launch work of an eager call)")
    # the same arm replayed from a captured graph: the launches without the host
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ours()
    timed(g.replay, 5)
    v = [timed(g.replay, inner) for _ in range(runs)]
    say(f"    csrc/ctc.hip replayed from a captured graph: median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_bench.txt"))
    ap.add_argument("--parity", default=None)
    ap.add_argument("--parity-out", default=os.path.join(ROOT, "profiles", "ctc_parity_measured.txt"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ctc_bench.py needs a GPU: there is no fallback")
    dev = torch.device("cuda")
    say("tools/ctc_bench.py -- CTC loss forward + gradient: csrc/ctc.hip against torch's device log_softmax + F.ctc_loss on the same tensors")
    say(f"source_id {bench.source_id()}")
    shape_bench("a", 32, 500, 100, 256, 300, 40, dev)
    shape_bench("b", 4, 50, 12, 32, 30, 4, dev)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    if opt.parity:
        rows = [l.rstrip("\n") for l in open(opt.parity) if l.strip()]
        with open(opt.parity_out, "w") as f:
            f.write("tests/test_ctc_gpu.py -- measured error / bound per case (bound: 2 x torch's fp32 CPU error against the float64 oracle "
                    "+ eps32 * T, + half an ulp of a 16-bit gradient); every ratio must be <= 1\n")
            f.write(f"source_id {bench.source_id()}\n")
            f.write(f"{len(rows)} lines; largest ratio {max(float(t) for l in rows for t in l.split('error/bound')[1].split('(')[0].split()[1::2]):.3f}\n")
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
