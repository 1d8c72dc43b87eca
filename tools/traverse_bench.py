"""Closed-set inference at the cfg-2 model size (OFA-base, bf16, 32 sentences): sentences/s of TraverseTask.inference for closed
sets of C = 64, 512 and 3129 random answers of 1-5 tokens, and next to it the scoring stage alone -- the three fused kernels of
csrc/closed_set_score.hip against the DENSE formulation of the reference in plain torch on the same GPU (output projection GEMM ->
masked_fill -> log_softmax -> gather, one sentence's C x Tmax rows at a time so that the [rows, V] logits fit), on the same decoder
features.  The two sides are timed alternately in one process, medians over the repeats.
Usage: python tools/traverse_bench.py            (every C in a child process of its own, each under a time limit)
       python tools/traverse_bench.py --one C"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BSZ, SIZES, STEP_LIMIT = 32, (64, 512, 3129), 150


def random_answers(C, d, seed):
    """1-5 tokens from the '<text>' range, skewed towards low ids so that answers share first tokens and prefixes."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lo, hi = d.get_start_end_idx("<text>")
    pool = min(hi - lo, 20000)
    return [tuple(int(lo + pool * rng.random() ** 3) for _ in range(int(rng.integers(1, 6)))) for _ in range(C)]


def median_ms(fn, reps, inner):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return out


def one(C):
    import numpy as np
    import torch
    torch.set_grad_enabled(False)                             # inference only: nothing may keep the dense logits alive
    import bench
    from ofasys_amd import TraverseTask
    from ofasys_amd import kernels as K
    dev = torch.device("cuda")
    model, d = bench.build(argparse.Namespace(arch="base", workload="cfg2", batch=BSZ), dev)
    model.eval()
    batch, _, _ = bench.make_batch(d, BSZ, 191, 8, 0, dev, "cfg2")
    sample = {"net_input": {"slots": batch["slots"]}}
    task = TraverseTask(name="vqa", instruction="[IMAGE:image] what is it? -> [TEXT:answer]")
    task.initialize(d, closed_set=random_answers(C, d, C))
    plan = task.plan
    # 1. the whole pass
    runs = []
    for rep in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        task.inference(model, sample)
        runs.append(time.perf_counter() - t0)
    dt = statistics.median(runs[2:])
    print(f"traverse inference bsz={BSZ} C={C} (N={plan.N} E={plan.E} root={int(plan.node_edge_off[1])} Tmax={plan.Tmax}, "
          f"{-(-C // max(1, task.max_rows // BSZ))} chunks of <= {task.max_rows} rows): {dt * 1e3:9.2f} ms  {BSZ / dt:8.1f} sentences/s",
          flush=True)
    # 2. the scoring stage alone, both formulations on the same features (rows of equal prefixes hold equal features)
    pd = task._plan_on(dev)
    W, bias = task.output_projection(model)
    T, D, V = plan.Tmax, W.shape[1], W.shape[0]
    src_row = np.arange(C * T).reshape(C, T)
    mask_rows, mask_toks = [], []
    for c in range(C):
        for t in range(int(plan.lengths[c])):
            n = plan.node_of(c, t)
            src_row[c, t] = int(plan.rep_ans[n]) * T + int(plan.rep_pos[n])
            a = plan.allowed(c, t)
            mask_rows += [c * T + t] * len(a)
            mask_toks += a
    h = torch.randn(BSZ, C * T, D, device=dev, dtype=W.dtype)[:, torch.from_numpy(src_row.reshape(-1)).to(dev)].contiguous()
    mask = torch.zeros(C * T, V, dtype=torch.bool, device=dev)
    mask[torch.tensor(mask_rows, device=dev), torch.tensor(mask_toks, device=dev)] = True
    tgt = torch.from_numpy(plan.target).to(dev).reshape(-1)
    pad = tgt == d.pad()
    mask[pad] = True
    ws = task._buffers(BSZ, dev)["ws"]
    h2d = h.reshape(-1, D)

    def fused():
        return K.closed_set_score(h2d, W, bias, pd, BSZ, ws)

    def dense():
        out = torch.empty(BSZ, C, device=dev)
        for b in range(BSZ):
            logits = torch.nn.functional.linear(h[b], W, bias)
            logits.masked_fill_(~mask, float("-inf"))
            lp = torch.log_softmax(logits.float(), -1).gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
            out[b] = lp.masked_fill(pad, 0).view(C, T).sum(1)
        return out

    a, b = fused(), dense()                                   # warm-up of both, and the outputs side by side
    torch.cuda.synchronize()
    diff = float((a - b).abs().max())
    inner = max(1, min(200, int(20000 / max(C, 1))))
    tf, td = [], []
    for rep in range(5):                                      # alternated
        tf += median_ms(fused, 1, inner)
        td += median_ms(dense, 1, 1)
    mf, md = statistics.median(tf), statistics.median(td)
    print(f"scoring stage  bsz={BSZ} C={C} D={D} V={V} {str(W.dtype).replace('torch.', '')}: fused {mf * 1e3:9.1f} us "
          f"(min {min(tf) * 1e3:.1f} max {max(tf) * 1e3:.1f})   dense torch {md * 1e3:11.1f} us (min {min(td) * 1e3:.1f} max "
          f"{max(td) * 1e3:.1f})   dense / fused = {md / mf:8.1f}   max |fused - dense| = {diff:.3e} (dense logits are {W.dtype})",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, default=None)
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one)
    for C in SIZES:                                           # a fresh process per size; a failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--one", str(C)]).returncode
        if rc != 0:
            print(f"traverse_bench: C={C} ended with status {rc}; stopping")
            sys.exit(rc)


if __name__ == "__main__":
    main()
