"""The trie-edge head against the dense head on a closed-set train step, at the cfg-2 size (OFA-base, bf16, V = 51 265 + specials) and
on the closed set of tools/closed_set_train_bench.py (3129 answers, tests/traverse_case.random_answers, seed 7).
(a) one closed-set micro-batch of 32 through TrainStep, packed, captured and replayed: the node step with the dense head (vocabulary
    projection + ofa_trie_ls_cross_entropy_fwd) against TrainStep(closed_set_edge_head=True); ms per step by a host clock around
    synchronised runs of 10 steps, the two arms alternated in one run, with the spread.
(b) the three launches of csrc/trie_head.hip and the step's row buckets alone, by device events, on the rows of that micro-batch
    (bf16 features of the model width), next to the dense head's three products and node criterion on the same rows.
Writes what it prints to profiles/closed_set_head_bench.txt (--out).  Usage: python tools/closed_set_head_bench.py"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ofasys_amd.preprocessor import ModalityType, Slot  # noqa: E402
from ofasys_amd.traverse import TraversePlan  # noqa: E402
from tools.closed_set_train_bench import BSZ, LINES, N_ANSWERS, SEED, closed_set, dictionary, fresh, say  # noqa: E402


def batch(answers, plan, d, V, dev):
    from ofasys_amd.packing import build_pack_plan
    g = torch.Generator().manual_seed(1234)
    rng = np.random.default_rng(SEED + 2)
    img = torch.randn(BSZ, 3, 224, 224, generator=g).bfloat16()
    src = torch.randint(4, V, (BSZ, 191), generator=g)
    slen = torch.randint(95, 192, (BSZ,), generator=g)
    slen[0] = 191
    picks = [answers[int(i)] for i in rng.integers(len(answers), size=BSZ)]
    Tt = 8
    prev = torch.full((BSZ, Tt), d.pad(), dtype=torch.int64)
    target = torch.full((BSZ, Tt), d.pad(), dtype=torch.int64)
    nodes = torch.full((BSZ, Tt), -1, dtype=torch.int32)
    for b, a in enumerate(picks):
        src[b, slen[b]:] = d.pad()
        prev[b, :len(a) + 1] = torch.tensor([d.bos()] + a)
        target[b, :len(a) + 1] = torch.tensor(a + [d.eos()])
        nodes[b, :len(a) + 1] = torch.from_numpy(plan.walk(a))
    s = {"slots": [Slot(ModalityType.IMAGE, True, img.to(dev), attributes=["adaptor=image_patch_embed"]),
                   Slot(ModalityType.TEXT, True, src.to(dev)), Slot(ModalityType.TEXT, False, prev.to(dev))],
         "target": target.to(dev), "constraint_nodes": nodes.to(dev), "constraint_trie": plan.head_arrays(dev)}
    enc_mask = torch.cat([torch.zeros(BSZ, 257, dtype=torch.bool), src.eq(d.pad())], 1)
    s["pack"] = build_pack_plan(enc_mask, prev.eq(d.pad()), bucket=512, dec_bucket=256).to(dev)
    return s, target, nodes


def step_bench(answers, plan, dev):
    from ofasys_amd.trainer import TrainStep
    arms = {}
    for arm in ("dense head", "edge head"):
        args = argparse.Namespace(arch="base", workload="cfg2", batch=BSZ)
        model, d = bench.build(args, dev)
        s, target, _ = batch(answers, plan, d, len(d), dev)
        engine = TrainStep(model, lr=1e-5, clip_norm=1.0, use_graph=True, graph_warmup=1, label_smoothing=0.1,
                           closed_set_edge_head=arm == "edge head")
        arms[arm] = (engine, s, int(target.ne(d.pad()).sum()))
    last = {}
    from ofasys_amd import ops
    for arm, (engine, s, _) in arms.items():
        ops.manual_seed(1234)                                # (the same dropout stream for both arms' first steps)
        for _ in range(4):                                   # warm-up, capture, first replays
            last[arm] = float(engine.train_step([fresh(s)])["stats"][1])
        torch.cuda.synchronize()
    times = {a: [] for a in arms}
    for _ in range(7):
        for a, (engine, s, _) in arms.items():
            batches = [fresh(s) for _ in range(10)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in batches:
                engine.train_step([b])
            torch.cuda.synchronize()
            times[a].append((time.perf_counter() - t0) / 10 * 1e3)
    say(f"(a) one closed-set micro-batch of {BSZ} at the cfg-2 model size (image 257 + text <= 191 -> answer + EOS in 8 positions, "
        f"{arms['edge head'][2]} target tokens), nodes packed, label smoothing 0.1, captured and replayed; 7 alternated runs of 10 steps")
    for a, (engine, _, _) in arms.items():
        v = times[a]
        say(f"    {a}: median {statistics.median(v):7.3f} ms/step (min {min(v):.3f}, max {max(v):.3f}, spread {max(v) - min(v):.3f}); "
            f"loss after 4 steps {last[a]:.4f}; captured graphs {engine.captured_graphs()}")
    md, mh = statistics.median(times["dense head"]), statistics.median(times["edge head"])
    say(f"    edge head - dense head = {mh - md:+.3f} ms/step ({(mh / md - 1) * 100:+.1f} %), measured against the dense head in this run")


def kernel_bench(answers, plan, d, dev, many=0):
    """many = 0: the rows of step_bench's micro-batch; else that many rows of answers drawn as tools/closed_set_train_bench.py (a) does."""
    from ofasys_amd import kernels as K
    from tools.beam_bench import timed
    V, D = len(d), 768
    if many:
        rng = np.random.default_rng(SEED + many)
        t, n = [], []
        while len(t) < many:
            a = answers[int(rng.integers(len(answers)))]
            t += a + [d.eos()]
            n += plan.walk(a).tolist()
        t, n = torch.tensor(t[:many]).to(dev), torch.tensor(n[:many], dtype=torch.int32).to(dev)
    else:
        _, target, nodes = batch(answers, plan, d, V, dev)
        live = target.reshape(-1).ne(d.pad())
        t = target.reshape(-1)[live].to(dev)
        n = nodes.reshape(-1)[live].to(dev)
    rows = t.numel()
    rows_pad = (rows + 255) // 256 * 256                     # the packed decoder's row bucket: filler rows on node -1
    t = torch.cat([t, torch.full((rows_pad - rows,), d.pad(), dtype=t.dtype, device=dev)])
    n = torch.cat([n, torch.full((rows_pad - rows,), -1, dtype=n.dtype, device=dev)])
    g = torch.Generator().manual_seed(99)
    x = torch.randn(rows_pad, D, generator=g).bfloat16().to(dev)
    W = (torch.randn(V, D, generator=g) * 0.05).bfloat16().to(dev)
    trie = plan.head_arrays(dev)
    gs = torch.ones(1, device=dev)
    dW = torch.zeros_like(W)
    out = K.trie_head_fwd(x, W, None, t, n, trie, d.pad(), 0.1)
    bk = K.trie_head_buckets(n, trie)
    ld = (V + 63) // 64 * 64
    logits = torch.empty(rows_pad, ld, dtype=torch.bfloat16, device=dev)[:, :V]
    K.gemm(x, W, False, True, out=logits)
    dl = K.trie_ls_cross_entropy_fwd(logits, t, n, trie, V, d.pad(), 0.1, grad_scale=gs, want_grad=True)[4]
    arms = [
        ("ofa_trie_head_fwd (z, loss, g)            ", lambda: K.trie_head_fwd(x, W, None, t, n, trie, d.pad(), 0.1)),
        ("ofa_trie_head_bwd_dx                      ", lambda: K.trie_head_bwd_dx(out["g"], W, t, n, trie, None, gs, d.pad())),
        ("row buckets (torch.sort + searchsorted)   ", lambda: K.trie_head_buckets(n, trie)),
        ("ofa_trie_head_bwd_dw                      ", lambda: K.trie_head_bwd_dw(out["g"], x, trie, bk, None, gs, dW)),
        ("dense: logits = x W^T                     ", lambda: K.gemm(x, W, False, True, out=logits)),
        ("dense: ofa_trie_ls_cross_entropy_fwd + grad", lambda: K.trie_ls_cross_entropy_fwd(logits, t, n, trie, V, d.pad(), 0.1, grad_scale=gs, want_grad=True)),
        ("dense: dX = dlogits W                     ", lambda: K.gemm(dl[:, :V], W, False, False, a_kpad_zero=True)),
        ("dense: dW = dlogits^T x                   ", lambda: K.gemm(dl[:, :V], x, True, False)),
    ]
    res = {name: [] for name, _ in arms}
    for _ in range(5):
        for name, fn in arms:
            res[name].append(timed(fn, 20) * 1e3)
    deg = np.diff(plan.node_edge_off)
    say(f"({'c' if many else 'b'}) the launches alone, device events, 5 alternated runs of 20: {rows} live rows in {rows_pad} (bf16, D = {D}, V = {V}); "
        f"{int((n == 0).sum())} rows at the root (degree {int(deg[0])}), max_degree {plan.max_degree}, {plan.U} distinct tokens")
    for name, _ in arms:
        v = res[name]
        say(f"    {name}: median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})")
    head = sum(statistics.median(res[name]) for name, _ in arms[:4])
    dense = sum(statistics.median(res[name]) for name, _ in arms[4:])
    say(f"    edge head, four launches: {head:.1f} us; dense head, four launches: {dense:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closed_set_head_bench.txt"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/closed_set_head_bench.py needs a GPU: there is no fallback")
    del LINES[:]
    d = dictionary()
    V = len(d)
    answers = closed_set(V)
    plan = TraversePlan(answers, d.bos(), d.eos(), d.pad())
    say(f"tools/closed_set_head_bench.py -- the trie-edge head against the dense head; dictionary of {V} symbols, {N_ANSWERS} answers "
        f"(tests/traverse_case.random_answers, seed {SEED}): {plan.N} trie nodes, {plan.E} edges, root degree {int(plan.node_edge_off[1])}")
    say(f"source_id {bench.source_id()}")
    dev = torch.device("cuda")
    step_bench(answers, plan, dev)
    kernel_bench(answers, plan, d, dev)
    kernel_bench(answers, plan, d, dev, many=1536)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
