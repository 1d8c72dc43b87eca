"""The EMA pass on the cfg-2 arena, and the cfg-2 step with and without it.

    python tools/ema_bench.py [--steps 20] [--rounds 3] [--kernels-only | --steps-only]

Kernels: ofa_ema_step (fp32 state + bf16 shadow: 4 + 4 + 2 + 2 = 12 B per parameter; bf16 state: 2 + 2 + 2 = 6 B) next to ofa_adam_step
(28 B) on an arena of the cfg-2 model's size, 20 back-to-back launches between events, medians of 5.
Steps: bench.py's cfg-2 workload through TrainStep with ema off, ema_fp32=True and ema_fp32=False -- one model each, every arm a
captured graph, `--rounds` interleaved timings of `--steps` replays.  The EMA-off arm against the PARENT commit is tools/ab_step.sh
(bench.py does not enable the EMA).
"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ofasys_amd import kernels as K  # noqa: E402


def bench_mod():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def kernels(n):
    dev = "cuda"
    p = (torch.randn(n, device=dev) * 0.02).bfloat16()
    grad = (torch.randn(n, device=dev) * 1e-3).bfloat16()
    master, m, v = p.float(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    state32, shadow, state16 = p.float(), p.clone(), p.clone()
    step = torch.tensor([7.0], dtype=torch.float64, device=dev)
    sched = torch.tensor([1.0, 1e-4, 1e-4, 0.0, 0.0], device=dev)
    arms = {
        "adam_step (28 B/param)": lambda: K.adam_step(master, m, v, grad, p, sched, 0.0, 0.9, 0.999, 1e-8, 0.01, 0),
        "ema_step fp32 state + bf16 shadow (12 B/param)": lambda: K.ema_step(state32, p, shadow, step, sched, 0.9999),
        "ema_step bf16 state (6 B/param)": lambda: K.ema_step(state16, p, None, step, sched, 0.9999),
    }
    bytes_per = {"adam": 28, "fp32": 12, "bf16 state": 6}
    res = {k: [] for k in arms}
    for _ in range(5):
        for k, fn in arms.items():
            res[k].append(timed(fn))
    print(f"arena: {n} parameters ({n * 2 / 2**20:.0f} MiB of bf16)")
    for k, v_ in res.items():
        us = statistics.median(v_)
        b = next(b for key, b in bytes_per.items() if key in k)
        print(f"  {k}: {us:.1f} us  ({n * b / us / 1e6:.2f} TB/s; runs {[round(x, 1) for x in v_]})", flush=True)
    sched[3] = 1.0
    print(f"  ema_step, update skipped (returns at once): {statistics.median([timed(arms['ema_step fp32 state + bf16 shadow (12 B/param)']) for _ in range(3)]):.1f} us")


def steps(n_steps, rounds):
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    B = bench_mod()
    args = argparse.Namespace(arch="base", workload="cfg2", dtype="bf16", batch=32, dropout=None)
    arms = {"ema off": None, "ema_fp32=True": dict(store_ema=True, ema_fp32=True), "ema_fp32=False": dict(store_ema=True)}
    run = {}
    for name, ema in arms.items():
        model, d = B.build(args, torch.device("cuda"))
        ops.manual_seed(1)
        tr = TrainStep(model, lr=1e-4, clip_norm=1.0, use_graph=True, ema=ema)
        batches = [B.make_step(d, args, args.batch, 97 * i, torch.device("cuda"), True) for i in range(4)]
        for b in batches:
            for _ in range(tr.graph_warmup + 1):
                tr.train_step(b[0])
        run[name] = (tr, batches)
        print(f"{name}: {tr.captured_graphs()} graphs captured, arena {tr.fp.numel} parameters", flush=True)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for name, (tr, batches) in run.items():
            for i in range(5):
                tr.train_step(batches[i % 4][0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n_steps):
                tr.train_step(batches[i % 4][0])
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / n_steps * 1e3)
    for name, v in res.items():
        print(f"  cfg-2 step, {name}: median {statistics.median(v):.3f} ms  (rounds {[round(x, 3) for x in v]})", flush=True)
    return run["ema off"][0].fp.numel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--numel", type=int, default=0, help="arena size of the kernel arms (0: the cfg-2 model's)")
    a = ap.parse_args()
    n = a.numel
    if not a.kernels_only:
        n = steps(a.steps, a.rounds) if not n else (steps(a.steps, a.rounds), n)[1]
    if not a.steps_only:
        if not n:
            from ofasys_amd.trainer import FlatParams
            model, _ = bench_mod().build(argparse.Namespace(arch="base", workload="cfg2", dtype="bf16", dropout=None), torch.device("cuda"))
            n = FlatParams(model).numel
            del model
        torch.cuda.empty_cache()
        kernels(n)


if __name__ == "__main__":
    main()
