"""Beam-search generation at the cfg-2 model size (OFA-base, bf16; 32 sentences x beam 5 = 160 rows, no_repeat_ngram_size 3,
max_len 32): ms per generation step and sentences/s through the captured per-step graphs, next to StepDecoder.greedy on the
same 160 rows; then the two beam kernels alone (us, and GB/s against the bytes of the logits they read) and the
self-attention cache reorder alone.  With --prefix-width W the same generation runs under a forced target prefix of W tokens per
sentence, and the policy launches of a prefix step (row pass, fill, sentence pass) are timed next to a free step's in the same run.
Usage: python tools/beam_bench.py [--prefix-width W]"""
import os
import sys
import time
import argparse

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ofasys_amd import kernels as K  # noqa: E402
from ofasys_amd.generator import SequenceGenerator, StepDecoder  # noqa: E402

dev = torch.device("cuda")
BSZ, BEAM, MAX_LEN, NGRAM = 32, 5, 32, 3


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
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefix-width", type=int, default=0, help="force a target prefix of this many tokens on every sentence")
    width = ap.parse_args().prefix_width
    args = argparse.Namespace(arch="base", workload="cfg2", batch=BSZ)
    model, d = bench.build(args, dev)
    model.eval()
    batch, _, _ = bench.make_batch(d, BSZ, 191, 8, 0, dev, "cfg2")
    sample = {"net_input": {"slots": batch["slots"]}}
    if width > 0:
        sample["prefix_tokens"] = torch.randint(4, len(d), (BSZ, width), generator=torch.Generator().manual_seed(0)).to(dev)
    # 1. generation: min_len = max_len keeps every sentence open for all max_len + 1 steps (a fixed amount of work to time)
    gen = SequenceGenerator(d, beam_size=BEAM, max_len=MAX_LEN, min_len=MAX_LEN, no_repeat_ngram_size=NGRAM, normalize_scores=False)
    runs = []
    for rep in range(4):                                  # eager warm-up, capture, then replays
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen.generate(model, sample)
        runs.append((time.perf_counter() - t0, gen.steps_run))
    dt, steps = min(runs[2:])
    print(f"beam generate  rows={BSZ * BEAM} beam={BEAM} ngram={NGRAM}: {dt * 1e3:8.2f} ms for {steps} steps "
          f"({dt / steps * 1e3:6.3f} ms/step incl. encoder), {BSZ / dt:8.1f} sentences/s")
    src = [s for s in batch["slots"] if s.is_src]
    order = torch.arange(BSZ, device=dev).repeat_interleave(BEAM)
    dec = StepDecoder(model, MAX_LEN + 1, use_graph=True)
    gr = []
    for rep in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.greedy(src, d.bos(), MAX_LEN + 1, beam_order=order)
        torch.cuda.synchronize()
        gr.append(time.perf_counter() - t0)
    g = min(gr[2:])
    print(f"greedy         rows={BSZ * BEAM}: {g * 1e3:8.2f} ms for {MAX_LEN + 1} steps ({g / (MAX_LEN + 1) * 1e3:6.3f} ms/step incl. "
          f"encoder and the per-step logits copy)")
    # 2. the beam kernels alone, at a mid step of the same shape
    rows, V = BSZ * BEAM, len(d)
    st = gen._state
    st["tokens"] = gen._dec.tokens
    logits = torch.randn(rows, V, device=dev).bfloat16()
    ws = st["ws"]
    step = 8
    st["done"].zero_()
    kw = dict(tokens=st["tokens"], done=st["done"], min_len=1, max_len=MAX_LEN, ngram=NGRAM, pad=d.pad(), unk=d.unk(), eos=d.eos())
    t_topk = timed(lambda: K.beam_topk(logits, BEAM, step, ws, **kw)) * 1e3
    t_sel = timed(lambda: K.beam_select(ws, st, BEAM, V, step, MAX_LEN, eos=d.eos(), unk=d.unk())) * 1e3
    nbytes = logits.numel() * 2
    print(f"ofa_beam_topk   rows={rows} V={V} bf16: {t_topk:7.1f} us  {nbytes / t_topk / 1e3:7.1f} GB/s over {nbytes / 1e6:.1f} MB")
    print(f"ofa_beam_select bsz={BSZ} beam={BEAM}: {t_sel:7.1f} us")
    t_re = timed(lambda: gen._dec.reorder(st["reorder"], caches_only=True)) * 1e3
    print(f"self-attention cache reorder (all layers, full capacity): {t_re:7.1f} us")
    if width > 0:
        # 3. a prefix step's policy launches at the same shape and step: every row forced (the collator's case while the prefix lasts)
        st["prefix"][:, :width] = sample["prefix_tokens"]
        st["prefix"][:, step] = torch.randint(4, V, (BSZ,), generator=torch.Generator().manual_seed(1)).to(dev)
        st["plen"].fill_(step + 1)
        pol = dict(tokens=st["tokens"], done=st["done"], pad=d.pad(), unk=d.unk(), ngram=NGRAM)
        t_row = timed(lambda: K.beam_prefix_topk(logits, BEAM, step, ws, st["plen"], prefix=st["prefix"], glogit=st["glogit"],
                                                 min_len=1, max_len=MAX_LEN, eos=d.eos(), **pol)) * 1e3
        t_fill = timed(lambda: K.beam_prefix_fill(ws, rows, V, BEAM, step, st["prefix"], st["plen"], st["glogit"], **pol)) * 1e3
        t_psel = timed(lambda: K.beam_prefix_select(ws, st, BEAM, V, step, MAX_LEN, st["prefix"], pad=d.pad(), eos=d.eos(),
                                                    unk=d.unk())) * 1e3
        print(f"ofa_beam_prefix_topk (all rows forced) rows={rows} V={V} bf16: {t_row:7.1f} us  {nbytes / t_row / 1e3:7.1f} GB/s")
        print(f"ofa_beam_prefix_fill   rows={rows}: {t_fill:7.1f} us")
        print(f"ofa_beam_prefix_select bsz={BSZ} beam={BEAM}: {t_psel:7.1f} us")
        print(f"policy launches of a step: prefix {t_row + t_fill + t_psel:7.1f} us, free {t_topk + t_sel:7.1f} us")


if __name__ == "__main__":
    main()
