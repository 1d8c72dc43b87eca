"""Self-critical sequence training at the cfg-2 model size (OFA-base, bf16; 32 sentences x K = 5 hypotheses, max_len 16, V = 51 265).
(a) ofa_scst_loss_fwd_grad alone on the step's [rows, V] logits against the route the library offered before it -- ofa_ls_cross_entropy_fwd
    + _bwd with eps 0 and row_w = the row's reward, which computes the same numbers in two reads and a write -- alternated in one run;
    the spread of the repeated runs of each (A/A) is printed next to the difference.
(b) one SCST step in its four parts -- generate, host decode + CIDEr-D, batch build, train step -- next to a plain cross-entropy step
    of the same B*K batch.
Prints the id of the sources it ran on (tools/build_id.py).  Usage: python tools/scst_bench.py [--sampling]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ofasys_amd import Task, TaskConfig  # noqa: E402
from ofasys_amd import kernels as K  # noqa: E402
from ofasys_amd.scst import ScstRewardCriterion, hypothesis_batch, repeat_sources, self_critical_reward  # noqa: E402
from ofasys_amd.trainer import TrainStep  # noqa: E402
from tools.beam_bench import timed  # noqa: E402

dev = torch.device("cuda")
BSZ, KHYP, MAX_LEN = 32, 5, 16


def kernel_ab(rows, V, Tt, pad):
    ld = (V + 7) // 8 * 8
    g = torch.Generator().manual_seed(0)
    store = (torch.randn(rows, ld, generator=g) * 3).bfloat16().to(dev)
    x = store[:, :V]
    t = torch.randint(4, V, (rows,), generator=g)
    t[torch.rand(rows, generator=g) < 0.35] = pad                       # about the share of padding of a hypothesis batch
    t = t.to(dev)
    reward = torch.randn(rows // Tt, generator=g).to(dev)
    row_w = reward.repeat_interleave(Tt).contiguous()
    gs = torch.ones(1, device=dev)
    d = torch.empty_like(store)

    def two():
        lse, _, _, cnt = K.ls_cross_entropy_fwd(x, t, V, pad, 0.0)
        K.ls_cross_entropy_bwd(x, t, lse, cnt, row_w, gs, V, pad, 0.0)

    def one():
        K.scst_loss_fwd_grad(x, t, reward, gs, V, pad, Tt, dlogits=d)
    # the two routes agree (same numbers): a sanity check before timing them
    lse, _, _, cnt = K.ls_cross_entropy_fwd(x, t, V, pad, 0.0)
    want = K.ls_cross_entropy_bwd(x, t, lse, cnt, row_w, gs, V, pad, 0.0)
    K.scst_loss_fwd_grad(x, t, reward, gs, V, pad, Tt, dlogits=d)
    err = float((d.float() - want.float()).abs().max())
    res = {"two": [], "one": []}
    for _ in range(7):
        res["two"].append(timed(two, 30) * 1e3)
        res["one"].append(timed(one, 30) * 1e3)
    nbytes = rows * ld * 2
    print(f"(a) rows={rows} V={V} ld={ld} bf16 ({nbytes / 1e6:.1f} MB of logits); max |one - two| = {err:.3g}")
    for name, v in res.items():
        med, spread = statistics.median(v), max(v) - min(v)
        passes = 2 if name == "one" else 3
        print(f"    {'ofa_scst_loss_fwd_grad (one pass)' if name == 'one' else 'ofa_ls_cross_entropy_fwd + _bwd  '}: median {med:7.1f} us, "
              f"A/A spread {spread:5.1f} us over 7 runs of 30 ({passes * nbytes / med / 1e3:6.0f} GB/s over {passes} passes)")
    m1, m2 = statistics.median(res["one"]), statistics.median(res["two"])
    print(f"    one-pass - two-kernel = {m1 - m2:+.1f} us ({m2 / m1:.2f}x)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampling", action="store_true", help="K independent samples (top-k 256) instead of the beam")
    opt = ap.parse_args()
    args = argparse.Namespace(arch="base", workload="cfg2", batch=BSZ)
    model, d = bench.build(args, dev)
    print(f"source_id {bench.source_id()}")
    cfg = TaskConfig()
    cfg.scst = True
    cfg.scst_args = ('{"sampling": true, "sampling_topk": 256, "seed": 1, ' if opt.sampling else '{') + \
        f'"beam": {KHYP}, "max_len": {MAX_LEN}, "max_len_b": {MAX_LEN}, "min_len": 1}}'
    cfg.text.pad_to_multiple = 8
    task = Task(cfg, name="caption", instruction="[IMAGE:image,adaptor=image_patch_embed] [TEXT:src] -> [TEXT:caption]")
    task.initialize(d)
    crit = ScstRewardCriterion(task, cfg.criterion)
    batch, _, _ = bench.make_batch(d, BSZ, 191, 8, 0, dev, "cfg2")
    sample = {"net_input": {"slots": batch["slots"]}, "target": batch["target"]}
    engine = TrainStep(model, lr=1e-5, clip_norm=1.0, use_graph=True, graph_warmup=1)
    gen, text = task.scst_generator, crit.text
    parts, plain, shapes = [], [], None
    for it in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.eval()
        with torch.no_grad():
            out = gen.generate(model, sample)
        t1 = time.perf_counter()
        toks = [h.tokens for hyps in out for h in hyps]
        assert len(toks) == BSZ * KHYP, "fewer than K hypotheses for a sentence"
        scores = crit.scores([text.decode(t).strip() for t in toks], crit.references(sample), KHYP)
        reward = self_critical_reward(scores, KHYP)
        t2 = time.perf_counter()
        prev, target = hypothesis_batch(toks, d.pad(), d.bos(), cfg.text.pad_to_multiple)
        mb = {"slots": repeat_sources(sample["net_input"]["slots"], KHYP, prev.to(dev)), "target": target.to(dev),
              "reward": torch.as_tensor(reward, dtype=torch.float32).to(dev), "task": "caption"}
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        engine.train_step([mb])
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        ce = {"slots": mb["slots"], "target": mb["target"], "task": "caption-ce"}
        engine.train_step([ce])
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        parts.append((t1 - t0, t2 - t1, t3 - t2, t4 - t3))
        plain.append(t5 - t4)
        shapes = (tuple(target.shape), gen.steps_run, int(target.ne(d.pad()).sum()), float(scores.mean()))
        print(f"    iteration {it}: target {shapes[0]}, {shapes[1]} generation steps, {shapes[2]} tokens; "
              + ", ".join(f"{x * 1e3:.1f}" for x in parts[-1]) + f" ms; plain CE step {plain[-1] * 1e3:.1f} ms", flush=True)
    last = parts[-3:]
    med = [statistics.median(p[i] for p in last) * 1e3 for i in range(4)]
    total = sum(med)
    print(f"(b) one SCST step, {BSZ} sentences x K={KHYP} ({'sampling top-k 256' if opt.sampling else 'beam search'}), median of the last 3 of 7:")
    for name, v in zip(("generate", "host decode + CIDEr-D + reward", "batch build", "train step"), med):
        print(f"    {name:32s} {v:8.2f} ms  {100 * v / total:5.1f} %")
    print(f"    {'total':32s} {total:8.2f} ms;  a plain cross-entropy step of the same {BSZ * KHYP}-row batch: "
          f"{statistics.median(plain[-3:]) * 1e3:.2f} ms;  captured step graphs: {engine.captured_graphs()}")
    rows = shapes[0][0] * shapes[0][1]
    kernel_ab(rows, len(d), shapes[0][1], d.pad())


if __name__ == "__main__":
    main()
