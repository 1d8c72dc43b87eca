"""Closed-set training from trie node ids against vocabulary masks, at the cfg-2 size (OFA-base, bf16, V = 51 265 + specials).
The closed set: 3129 answers drawn by tests/traverse_case.random_answers (seed 7) over the whole dictionary, so the root has more than
a thousand children and the deep nodes a handful.
(c) CPU, no GPU needed (--collate-only): collation of a batch of 32 [TEXT:src] -> [TEXT:answer,closed_set] samples, masks against nodes.
(a) the criterion alone on [rows, V] bf16 logits, rows in {128, 1536}, the rows being the positions of real answers: today's mask form
    (ofa_ls_cross_entropy_fwd + _bwd with the byte mask) against the node form (ofa_trie_ls_cross_entropy_fwd writing the gradient in
    the same launch), alternated in one process, device events, 7 runs of 30; next to them a zero fill of rows x ld, the node form's floor.
(b) one closed-set micro-batch of 32 through TrainStep (captured, replayed): masks padded, nodes padded, nodes packed; ms per step by a
    host clock around synchronised runs of 10 steps, the arms alternated, and the bytes a replay copies into the static inputs.
Writes what it prints to profiles/closed_set_train_bench.txt (--out).  Usage: python tools/closed_set_train_bench.py [--collate-only]"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ofasys_amd.preprocessor import (DefaultTextPreprocess, Dictionary, GeneralPreprocess, Instruction, ModalityType,  # noqa: E402
                                     Slot)
from ofasys_amd.preprocessor.collate import TextPreprocessConfig  # noqa: E402
from ofasys_amd.traverse import TraversePlan  # noqa: E402
from tests.traverse_case import random_answers  # noqa: E402

BSZ, N_ANSWERS, SEED = 32, 3129, 7
LINES = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    LINES.append(line)


def dictionary():
    d = Dictionary()
    for i in range(bench.V_TEXT):
        d.add_symbol(f"<text>_{i}")
    d.add_symbol("<mask>")
    d.add_bins(1000)
    return d


def closed_set(V):
    return random_answers(np.random.default_rng(SEED), N_ANSWERS, V=V, max_len=5)


def collate_bench(d, answers):
    rng = np.random.default_rng(SEED + 1)
    picks = [answers[int(i)] for i in rng.integers(len(answers), size=BSZ)]
    srcs = [torch.from_numpy(rng.integers(4, len(d), size=int(rng.integers(8, 24)))) for _ in range(BSZ)]
    res = {}
    for mode in ("masks", "nodes"):
        cfg = TextPreprocessConfig()
        cfg.closed_set_nodes = mode == "nodes"
        t0 = time.perf_counter()
        gp = GeneralPreprocess(d, {"text": DefaultTextPreprocess(d, cfg, closed_set=answers)})
        prep = time.perf_counter() - t0
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            samples = [gp(Instruction([Slot(ModalityType.TEXT, True, s, global_position=0, split="train"),
                                       Slot(ModalityType.TEXT, False, torch.tensor(a), global_position=1, attributes=["closed_set"],
                                            split="train")], "c", {})) for s, a in zip(srcs, picks)]
            out = gp.collate(samples)
            times.append(time.perf_counter() - t0)
        key = "constraint_masks" if mode == "masks" else "constraint_nodes"
        nbytes = out[key].numel() * out[key].element_size()
        res[mode] = out
        say(f"    {mode}: median {statistics.median(times) * 1e3:8.2f} ms per batch of {BSZ} (min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}, "
            f"5 batches); {key} {tuple(out[key].shape)} {str(out[key].dtype).replace('torch.', '')} = {nbytes} bytes; "
            f"prepare_for_generation {prep * 1e3:.0f} ms once")
    assert torch.equal(res["masks"]["target"], res["nodes"]["target"])
    return res


def criterion_bench(V, pad, plan, answers, dev):
    from ofasys_amd import kernels as K
    from tools.beam_bench import timed
    ld = (V + 7) // 8 * 8
    trie = {"node_edge_off": torch.from_numpy(plan.node_edge_off).to(dev), "edge_token": torch.from_numpy(plan.edge_token).to(dev),
            "N": plan.N, "E": plan.E}
    deg = np.diff(plan.node_edge_off)
    say(f"(a) criterion alone: V={V} ld={ld} bf16, eps 0.1; trie N={plan.N} E={plan.E}, root degree {int(deg[0])}, median degree {int(np.median(deg))}")
    for rows in (128, 1536):
        rng = np.random.default_rng(SEED + rows)
        t, n = [], []
        while len(t) < rows:
            a = answers[int(rng.integers(len(answers)))]
            t += a + [2]
            n += plan.walk(a).tolist()
        t, n = torch.tensor(t[:rows]), torch.tensor(n[:rows], dtype=torch.int32)
        g = torch.Generator().manual_seed(rows)
        store = (torch.randn(rows, ld, generator=g) * 3).bfloat16().to(dev)
        x, t, n = store[:, :V], t.to(dev), n.to(dev)
        off, tok = trie["node_edge_off"].long(), trie["edge_token"].long()
        cm = torch.zeros(rows, V, dtype=torch.bool, device=dev)
        for r in range(rows):
            cm[r, tok[off[n[r]]:off[n[r] + 1]]] = True
        gs = torch.ones(1, device=dev)
        zero = torch.empty_like(store)

        def masks():
            lse, _, _, cnt = K.ls_cross_entropy_fwd(x, t, V, pad, 0.1, -1, -1, cm)
            return K.ls_cross_entropy_bwd(x, t, lse, cnt, None, gs, V, pad, 0.1, -1, -1, cm)

        def nodes():
            return K.trie_ls_cross_entropy_fwd(x, t, n, trie, V, pad, 0.1, grad_scale=gs, want_grad=True)[4]

        def fill():
            zero.zero_()
        err = float((masks().float() - nodes().float()).abs().max())
        res = {"masks": [], "nodes": [], "fill": []}
        for _ in range(7):
            for name, fn in (("masks", masks), ("nodes", nodes), ("fill", fill)):
                res[name].append(timed(fn, 30) * 1e3)
        say(f"    rows={rows} ({rows * ld * 2 / 1e6:.1f} MB of logits, {rows * V / 1e6:.1f} MB of mask bytes, {rows * 4} bytes of nodes; "
            f"{int((n == 0).sum())} rows at the root); max |nodes - masks| gradient = {err:.3g}")
        for name, label in (("masks", "ofa_ls_cross_entropy_fwd + _bwd, byte mask"), ("nodes", "ofa_trie_ls_cross_entropy_fwd, one launch  "),
                            ("fill", "zero fill of rows x ld (torch)            ")):
            v = res[name]
            say(f"        {label}: median {statistics.median(v):7.1f} us, A/A spread {max(v) - min(v):5.1f} us over 7 runs of 30")
        say(f"        masks / nodes = {statistics.median(res['masks']) / statistics.median(res['nodes']):.1f}x; "
            f"nodes / fill = {statistics.median(res['nodes']) / statistics.median(res['fill']):.2f}x")


def fresh(s):
    """The sample as a new batch from the collator would arrive: new tensors for the slots, the target and the masks / nodes (a dict
    of the same tensors would copy nothing into the static inputs: dst is src)."""
    out = dict(s)
    out["slots"] = []
    for sl in s["slots"]:
        c = copy.copy(sl)
        c.value = sl.value.clone()
        out["slots"].append(c)
    for k in ("target", "constraint_masks", "constraint_nodes"):
        if k in out:
            out[k] = out[k].clone()
    return out


def step_bench(answers, plan, dev):
    from ofasys_amd.packing import build_pack_plan
    from ofasys_amd.trainer import TrainStep, sample_tensors
    from tests.closed_set_train_case import nodes_to_masks
    arms = {}
    for arm in ("masks padded", "nodes padded", "nodes packed"):
        args = argparse.Namespace(arch="base", workload="cfg2", batch=BSZ)
        model, d = bench.build(args, dev)
        V = len(d)
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
             "target": target.to(dev)}
        trie = {"node_edge_off": torch.from_numpy(plan.node_edge_off).to(dev), "edge_token": torch.from_numpy(plan.edge_token).to(dev),
                "N": plan.N, "E": plan.E}
        if arm == "masks padded":
            s["constraint_masks"] = nodes_to_masks(nodes, plan.node_edge_off, plan.edge_token, V).to(dev)
        else:
            s["constraint_nodes"], s["constraint_trie"] = nodes.to(dev), trie
        if arm == "nodes packed":
            enc_mask = torch.cat([torch.zeros(BSZ, 257, dtype=torch.bool), src.eq(d.pad())], 1)
            s["pack"] = build_pack_plan(enc_mask, prev.eq(d.pad()), bucket=512, dec_bucket=256).to(dev)
        engine = TrainStep(model, lr=1e-5, clip_norm=1.0, use_graph=True, graph_warmup=1, label_smoothing=0.1)
        # what a replay copies: every tensor of a new batch that is not the very tensor of the static sample (the trie's arrays and,
        # here, the pack plan's tables are; a new batch's plan would add its tables)
        copied = sum(a.numel() * a.element_size() for (_, a), (_, b) in zip(sample_tensors([s]), sample_tensors([fresh(s)])) if a is not b)
        arms[arm] = (engine, s, copied, int(target.ne(d.pad()).sum()))
    for engine, s, _, _ in arms.values():
        for _ in range(4):                                   # warm-up, capture, first replays
            loss = float(engine.train_step([fresh(s)])["stats"][1])
        torch.cuda.synchronize()
    times = {a: [] for a in arms}
    for _ in range(5):
        for a, (engine, s, _, _) in arms.items():
            batches = [fresh(s) for _ in range(10)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in batches:
                engine.train_step([b])
            torch.cuda.synchronize()
            times[a].append((time.perf_counter() - t0) / 10 * 1e3)
    say(f"(b) one closed-set micro-batch of {BSZ} at the cfg-2 model size (image 257 + text <= 191 -> answer + EOS in 8 positions, "
        f"{arms['nodes padded'][3]} target tokens), label smoothing 0.1, captured and replayed; 5 alternated runs of 10 steps; last loss {loss:.3f}")
    for a, (engine, s, copied, _) in arms.items():
        v = times[a]
        say(f"    {a}: median {statistics.median(v):7.2f} ms/step (min {min(v):.2f}, max {max(v):.2f}); {copied} bytes copied into the static "
            f"inputs per replay; captured graphs {engine.captured_graphs()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--collate-only", action="store_true", help="the CPU part alone (needs no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closed_set_train_bench.txt"))
    opt = ap.parse_args()
    d = dictionary()
    V = len(d)
    answers = closed_set(V)
    plan = TraversePlan(answers, d.bos(), d.eos(), d.pad())
    say(f"tools/closed_set_train_bench.py -- closed-set training from trie node ids; dictionary of {V} symbols, {N_ANSWERS} answers "
        f"(tests/traverse_case.random_answers, seed {SEED}): {plan.N} trie nodes, {plan.E} edges, root degree {int(plan.node_edge_off[1])}")
    say(f"source_id {bench.source_id()}")
    say(f"(c) collation on the CPU ({os.cpu_count()} logical CPUs, one thread of Python): [TEXT:src] -> [TEXT:answer,closed_set]")
    collate_bench(d, answers)
    if not opt.collate_only:
        if not torch.cuda.is_available():
            raise SystemExit("parts (a) and (b) need a GPU: there is no fallback (--collate-only for the CPU part)")
        dev = torch.device("cuda")
        criterion_bench(V, d.pad(), plan, answers, dev)
        step_bench(answers, plan, dev)
    else:
        say("(a), (b): not measured in this run (--collate-only)")
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
