"""Trie-constrained beam search at the cfg-2 model size (OFA-base, bf16, 32 sentences, beam 5) for closed sets of C = 64, 512 and
3129 random answers of 1-5 tokens (the sets of tools/traverse_bench.py):
  1. TraverseTask.inference(search="beam") next to search="all" in one process, alternated, medians: ms per batch, sentences/s,
     and the share of sentences whose beam answer is the exact arg-max (informational: the weights are random);
  2. a trie step next to a plain SequenceGenerator step at the same rows and decoder capacity: generate() per step, and the replay
     of one captured step graph alone (sentences reopened and rows put back on inner nodes before every replay, on both sides);
  3. the row pass alone (ofa_trie_beam_topk) at the root (step 0) and at inner nodes, next to ofa_beam_topk on [rows, V] logits.
Usage: python tools/trie_beam_bench.py            (every C in a child process of its own, each under a time limit)
       python tools/trie_beam_bench.py --one C"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BSZ, BEAM, SIZES, STEP_LIMIT = 32, 5, (64, 512, 3129), 240


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def timed_us(fn, n=50, before=None):
    import torch
    for _ in range(3):
        if before is not None:
            before()
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        if before is not None:
            before()
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def one(C):
    import numpy as np
    import torch
    torch.set_grad_enabled(False)
    import bench
    from tools.traverse_bench import random_answers
    from ofasys_amd import TraverseTask
    from ofasys_amd import kernels as K
    from ofasys_amd.generator import SequenceGenerator
    dev = torch.device("cuda")
    model, d = bench.build(argparse.Namespace(arch="base", workload="cfg2", batch=BSZ), dev)
    model.eval()
    batch, _, _ = bench.make_batch(d, BSZ, 191, 8, 0, dev, "cfg2")
    sample = {"net_input": {"slots": batch["slots"]}}
    task = TraverseTask(name="vqa", instruction="[IMAGE:image] what is it? -> [TEXT:answer]", beam=BEAM)
    task.initialize(d, closed_set=random_answers(C, d, C))
    plan = task.plan
    W, bias = task.output_projection(model)
    V, D, rows = W.shape[0], W.shape[1], BSZ * BEAM
    print(f"C={C}: N={plan.N} E={plan.E} root={plan.max_degree} edges Tmax={plan.Tmax} V={V} D={D} "
          f"row-pass grid ({K.trie_beam_splits(plan.max_degree, V)}, {rows})", flush=True)
    # 1. the whole pass, both searches alternated (the first two rounds: eager warm-up and graph capture of the beam route)
    tb, ta = [], []
    for rep in range(7):
        dt, beam_ans = wall(lambda: task.inference(model, sample, search="beam"))
        tb.append(dt)
        dt, all_ans = wall(lambda: task.inference(model, sample, search="all"))
        ta.append(dt)
    mb, ma = statistics.median(tb[2:]), statistics.median(ta[2:])
    gen = task.trie_generator(beam=BEAM)
    agree = sum(a == b for a, b in zip(beam_ans, all_ans))
    print(f"inference bsz={BSZ} C={C}: search=beam {mb * 1e3:9.2f} ms (min {min(tb[2:]) * 1e3:.2f} max {max(tb[2:]) * 1e3:.2f}) "
          f"{BSZ / mb:8.1f} sentences/s in {gen.steps_run} steps | search=all {ma * 1e3:9.2f} ms (min {min(ta[2:]) * 1e3:.2f} max "
          f"{max(ta[2:]) * 1e3:.2f}) {BSZ / ma:8.1f} sentences/s | all / beam = {ma / mb:6.1f} | beam answer is the arg-max for "
          f"{agree}/{BSZ} sentences", flush=True)
    # 2. per step, next to plain beam search at the same rows and capacity (min_len = max_len keeps it open for all its steps)
    L = min(256, plan.Tmax)
    plain = SequenceGenerator(d, beam_size=BEAM, max_len=L, min_len=L, normalize_scores=False)
    tp, tt = [], []
    for rep in range(7):
        dt, _ = wall(lambda: plain.generate(model, sample))
        tp.append((dt, plain.steps_run))
        dt, _ = wall(lambda: gen.generate(model, sample))
        tt.append((dt, gen.steps_run))
    (dp, sp), (dt_, st_) = sorted(tp[2:])[len(tp[2:]) // 2], sorted(tt[2:])[len(tt[2:]) // 2]
    print(f"generate rows={rows} capacity={L + 1}: trie {dt_ * 1e3:8.2f} ms / {st_} steps = {dt_ / st_ * 1e3:6.3f} ms/step | plain "
          f"{dp * 1e3:8.2f} ms / {sp} steps = {dp / sp * 1e3:6.3f} ms/step (both incl. the encoder)", flush=True)
    inner = np.nonzero(plan.edge_child[:plan.node_edge_off[1]] >= 0)[0]
    inner_nodes = torch.from_numpy(plan.edge_child[inner[np.arange(rows) % len(inner)]]).to(dev)      # children of the root
    deg = np.diff(plan.node_edge_off)[plan.edge_child[inner]]
    t = 1
    if t in gen._dec._graphs and t in plain._dec._graphs:
        gs, ps = gen._state, plain._state

        def reopen_trie():
            gs["done"].zero_()
            gs["node"].copy_(inner_nodes)

        def reopen_plain():
            ps["done"].zero_()
            ps["ignore"].zero_()
        gen._dec._set_lengths(t + 1)
        us_t = timed_us(gen._dec._graphs[t][0].replay, before=reopen_trie)
        plain._dec._set_lengths(t + 1)
        us_p = timed_us(plain._dec._graphs[t][0].replay, before=reopen_plain)
        print(f"step graph replay (step {t}, incl. two small resets): trie {us_t:8.1f} us | plain {us_p:8.1f} us", flush=True)
    # 3. the row pass alone
    pd = gen._plan_on(dev)
    h = torch.randn(rows, D, device=dev, dtype=W.dtype)
    ws = gen._state["ws"]
    done = torch.zeros(BSZ, dtype=torch.int32, device=dev)
    tokens = torch.zeros(rows, L + 1, dtype=torch.long, device=dev)
    kw = dict(tokens=tokens, done=done, min_len=1, max_len=L, pad=d.pad(), unk=d.unk(), eos=d.eos())
    root = torch.zeros(rows, dtype=torch.int32, device=dev)
    us_root0 = timed_us(lambda: K.trie_beam_topk(h, W, bias, pd, root, BEAM, 0, ws, **kw))
    us_root1 = timed_us(lambda: K.trie_beam_topk(h, W, bias, pd, root, BEAM, 1, ws, **kw))
    us_inner = timed_us(lambda: K.trie_beam_topk(h, W, bias, pd, inner_nodes, BEAM, 1, ws, **kw))
    logits = torch.randn(rows, V, device=dev, dtype=W.dtype)
    us_plain = timed_us(lambda: K.beam_topk(logits, BEAM, 1, ws, **kw))
    us_proj = timed_us(lambda: torch.nn.functional.linear(h, W, bias))
    print(f"row pass rows={rows}: root at step 0 ({BSZ} rows x {plan.max_degree} edges) {us_root0:7.1f} us | all rows at the root "
          f"{us_root1:7.1f} us | rows on the root's children (degree median {int(np.median(deg))} max {int(deg.max())}) {us_inner:7.1f} us "
          f"| ofa_beam_topk on [rows, V] {us_plain:7.1f} us + the projection GEMM it needs {us_proj:7.1f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, default=None)
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one)
    for C in SIZES:                                           # a fresh process per size; a failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--one", str(C)]).returncode
        if rc != 0:
            print(f"trie_beam_bench: C={C} ended with status {rc}; stopping")
            sys.exit(rc)


if __name__ == "__main__":
    main()
