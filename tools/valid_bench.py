"""On-device validation at the cfg-2 size (OFA-base, bf16, V = 51 265): the one-pass criterion kernel against the route the parent
commit had to the same numbers, the validation step captured against eager, and the launch count of the captured TRAIN step.
(1) kernels alone on [1536, V] bf16 logits (ld = V rounded up to 8), label smoothing 0.1, the two sides alternated in one process,
    device events, 7 runs of 30:
      new     ofa_criterion_eval + ofa_eval_stats_add (loss, NLL, hits and their sums: two launches)
      parent  ofa_ls_cross_entropy_fwd (or ofa_trie_ls_cross_entropy_fwd) for loss and NLL, torch.argmax over the fp32 log-softmax
              (ops.log_softmax_fp32; with a constraint: masked first, as the reference masks its logits) for the hits, K.sum_f32 x 2,
              the hit count and the token count
    plain, with a constraint range, and the node form (the closed set of tools/closed_set_train_bench.py).  Bytes per second are
    rows x V x 2 over the new side's time, as a share of the MI355X's 8 TB/s HBM peak.
(2) TrainStep.valid_step on one packed cfg-2 batch of 32: captured (replayed) against eager, ms per batch by a host clock around
    synchronised runs of 10, alternated.
(3) the launches of one captured train step (C-ABI calls + torch-native ops recorded during the capture) of an engine that never
    validates; `--count-launches --tree DIR` counts them for another checkout of the project (the parent commit) with this library.
Writes what it prints to profiles/valid_bench.txt (--out).  Usage: python tools/valid_bench.py [--parent-count N]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
LINES = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    LINES.append(line)


def med(v):
    return f"median {statistics.median(v):7.1f} us, A/A spread {max(v) - min(v):5.1f} us over {len(v)} runs of 30"


def kernel_bench(d, dev):
    from ofasys_amd import kernels as K
    from ofasys_amd import ops
    from ofasys_amd.traverse import TraversePlan
    from tests.traverse_case import random_answers
    from tools.beam_bench import timed
    V, pad, rows, eps = len(d), d.pad(), 1536, 0.1
    ld = (V + 7) // 8 * 8
    g = torch.Generator().manual_seed(5)
    store = (torch.randn(rows, ld, generator=g) * 3).bfloat16().to(dev)
    x = store[:, :V]
    answers = random_answers(np.random.default_rng(7), 3129, V=V, max_len=5)
    plan = TraversePlan(answers, d.bos(), d.eos(), pad)
    trie = {"node_edge_off": torch.from_numpy(plan.node_edge_off).to(dev), "edge_token": torch.from_numpy(plan.edge_token).to(dev),
            "N": plan.N, "E": plan.E}
    rng = np.random.default_rng(11)
    tn, nn = [], []
    while len(tn) < rows:
        a = answers[int(rng.integers(len(answers)))]
        tn += a + [2]
        nn += plan.walk(a).tolist()
    t_node, nodes = torch.tensor(tn[:rows]).to(dev), torch.tensor(nn[:rows], dtype=torch.int32).to(dev)
    off, tok = trie["node_edge_off"].long(), trie["edge_token"].long()
    node_mask = torch.zeros(rows, V, dtype=torch.bool, device=dev)
    for r in range(rows):
        node_mask[r, tok[off[nodes[r]]:off[nodes[r] + 1]]] = True
    crange = (4, 50264)
    cols = torch.arange(V, device=dev)
    range_mask = ((cols < 4) | ((cols >= crange[0]) & (cols < crange[1])))[None, :]
    t_plain = torch.randint(4, crange[1], (rows,), generator=g).to(dev)
    t_plain[::3] = x[::3, :crange[1]].float().argmax(1)        # a third of the rows hit (their largest logit inside the range)
    t_plain[::9] = pad
    say(f"(1) kernels alone: rows={rows} V={V} ld={ld} bf16 ({rows * V * 2 / 1e6:.1f} MB of logits), eps {eps}; trie N={plan.N} E={plan.E}")
    for name, t, cr, nd, mask in (("plain", t_plain, None, None, None), (f"range [{crange[0]}, {crange[1]})", t_plain, crange, None, range_mask),
                                  ("node form", t_node, None, nodes, node_mask)):
        cs, ce = cr if cr is not None else (-1, -1)
        acc = torch.zeros(4, dtype=torch.float64, device=dev)

        def new():
            rl, rn, rh = K.criterion_eval(x, t, V, pad, eps, cs, ce, None, nd, trie if nd is not None else None)
            K.eval_stats_add(acc, rl, rn, rh, t, pad)
            return rl, rn, rh

        def parent():
            if nd is not None:
                _, rl, rn, _, _ = K.trie_ls_cross_entropy_fwd(x, t, nd, trie, V, pad, eps)
            else:
                _, rl, rn, _ = K.ls_cross_entropy_fwd(x, t, V, pad, eps, cs, ce)
            lp = ops.log_softmax_fp32(x)
            if mask is not None:
                lp = lp.masked_fill(~mask, float("-inf"))
            live = t.ne(pad)
            hit = lp.argmax(1).eq(t) & live
            return K.sum_f32(rl), K.sum_f32(rn), hit.sum(), live.sum(), hit

        rl, rn, rh = new()
        pl, pn, ph, pt, hit = parent()
        torch.cuda.synchronize()
        differ = int((rh.bool() != hit).sum())             # (torch's device argmax promises no lowest column on equal maxima)
        same = float(acc[0]) == float(pt)
        ntok, nhit = int(acc[0]), int(acc[3])              # (one batch: the timed runs below keep adding to acc)
        dl = abs(float(acc[1]) - float(pl)) / max(float(pt), 1.0)
        res = {"new": [], "parent": []}
        for _ in range(7):
            for k, fn in (("new", new), ("parent", parent)):
                res[k].append(timed(fn, 30) * 1e3)
        n_us = statistics.median(res["new"])
        say(f"    {name}: token counts equal the parent route's: {same}; rows whose hit differs: {differ} ({nhit} of {ntok} tokens hit "
            f"here, {int(ph)} there); |loss_sum difference| per token {dl:.2g}")
        say(f"        new    ofa_criterion_eval + ofa_eval_stats_add          : {med(res['new'])}")
        say(f"        parent ls_cross_entropy_fwd + argmax(log_softmax) + sums: {med(res['parent'])}")
        say(f"        parent / new = {statistics.median(res['parent']) / n_us:.1f}x; new side: {rows * V * 2 / (n_us * 1e-6) / 1e12:.2f} TB/s of logits = "
            f"{rows * V * 2 / (n_us * 1e-6) / HBM_PEAK * 100:.0f} % of the 8 TB/s HBM peak")


def step_bench(d, dev, bench):
    from ofasys_amd.trainer import TrainStep
    args = argparse.Namespace(arch="base", workload="cfg2", batch=32)
    Ts_text, Tt, _, _ = bench.WORKLOADS["cfg2"]
    arms = {}
    for arm in ("captured", "eager"):
        model, _ = bench.build(args, dev)                  # (the same seed: the same weights; an engine owns its model's arena)
        arms[arm] = TrainStep(model, lr=1e-5, clip_norm=1.0, use_graph=arm == "captured", graph_warmup=1, label_smoothing=0.1)

    def batch(seed):
        return bench.make_batch(d, 32, Ts_text, Tt, seed, dev, "cfg2", pack=True)[0]
    for engine in arms.values():
        engine.valid_begin()
        for i in range(4):
            engine.valid_step([batch(i)])
        torch.cuda.synchronize()
    times = {a: [] for a in arms}
    for _ in range(5):
        for a, engine in arms.items():
            batches = [batch(10 + i) for i in range(10)]
            engine.valid_begin()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in batches:
                engine.valid_step([b])
            torch.cuda.synchronize()
            times[a].append((time.perf_counter() - t0) / 10 * 1e3)
    r = {a: e.valid_result() for a, e in arms.items()}
    say(f"(2) TrainStep.valid_step, one packed cfg-2 batch of 32 (image 257 + text <= {Ts_text} -> <= {Tt} target positions), label smoothing 0.1; "
        f"5 alternated runs of 10 batches; the two arms' passes agree bit for bit: {r['captured'] == r['eager']} "
        f"(loss {r['captured']['loss']:.4f}, {int(r['captured']['ntokens'])} tokens)")
    for a, engine in arms.items():
        v = times[a]
        say(f"    {a}: median {statistics.median(v):7.2f} ms/batch (min {min(v):.2f}, max {max(v):.2f}); captured validation graphs "
            f"{engine.captured_valid_graphs()}, captured train graphs {engine.captured_graphs()}")


def count_launches(dev, bench):
    """(C-ABI calls, torch-native ops) recorded while ONE train step of a tiny text model is captured: what its replays launch."""
    import torch.utils._python_dispatch as tpd
    import ofasys_amd.lib as L
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    from tests.model_util import build_model, make_slots
    case = {"arch": "tiny", "active": {"text"}, "overrides": {"use_self_attn_bias": False, "entangle_position_embedding": True},
            "adaptor_overrides": {"text": {"entangle_position_embedding": True}}}
    model, d = build_model(case, dev, torch.bfloat16)
    ops.manual_seed(1)
    g = torch.Generator().manual_seed(2)
    V = len(d)
    src, prev = torch.randint(4, V, (4, 16), generator=g), torch.randint(4, V, (4, 8), generator=g)
    s = {"slots": make_slots([("TEXT", True, src, None), ("TEXT", False, prev, None)], dev, torch.bfloat16),
         "target": torch.randint(4, V, (4, 8), generator=g).to(dev)}
    engine = TrainStep(model, lr=1e-4, clip_norm=1.0, use_graph=True, graph_warmup=0, label_smoothing=0.1)
    counts = {"abi": 0, "aten": 0}
    names = {}
    real = L._Lib.call

    def counting(self, name, *a):
        counts["abi"] += 1
        names[name] = names.get(name, 0) + 1
        return real(self, name, *a)

    class Count(tpd.TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            counts["aten"] += 1
            names[str(func)] = names.get(str(func), 0) + 1
            return func(*args, **(kwargs or {}))
    L._Lib.call = counting
    try:
        with Count():
            engine.train_step([s])
    finally:
        L._Lib.call = real
    torch.cuda.synchronize()
    assert engine.captured_graphs() == 1
    if os.environ.get("VALID_BENCH_NAMES"):               # (per-name counts, for comparing two checkouts)
        with open(os.environ["VALID_BENCH_NAMES"], "w") as f:
            f.write("".join(f"{n} {c}\n" for n, c in sorted(names.items())))
    return counts["abi"], counts["aten"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "valid_bench.txt"))
    ap.add_argument("--count-launches", action="store_true", help="part (3) alone: print the two counts and stop")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose ofasys_amd / bench / tests are imported (default: this one)")
    ap.add_argument("--parent-count", default=None, help="'ABI,ATEN' as --count-launches --tree <parent checkout> printed them")
    opt = ap.parse_args()
    sys.path.insert(0, os.path.abspath(opt.tree))
    import bench
    if not torch.cuda.is_available():
        raise SystemExit("tools/valid_bench.py needs a GPU: there is no fallback")
    dev = torch.device("cuda")
    if opt.count_launches:
        print("%d,%d" % count_launches(dev, bench))
        return
    from tools.closed_set_train_bench import dictionary
    d = dictionary()
    say(f"tools/valid_bench.py -- on-device validation; dictionary of {len(d)} symbols")
    say(f"source_id {bench.source_id()}")
    abi, aten = count_launches(dev, bench)                 # (first: a fresh process, as --count-launches --tree counts the parent)
    kernel_bench(d, dev)
    step_bench(d, dev, bench)
    say(f"(3) one captured train step of a tiny text model (4 x 16 -> 4 x 8 tokens, label smoothing 0.1), an engine that never validates: "
        f"{abi} C-ABI calls and {aten} torch-native ops recorded during the capture")
    if opt.parent_count:
        say(f"    the parent commit's checkout with this library (--count-launches --tree): {opt.parent_count.replace(',', ' C-ABI calls and ')} "
            f"torch-native ops -- {'the same' if opt.parent_count == f'{abi},{aten}' else 'NOT the same'}")
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
