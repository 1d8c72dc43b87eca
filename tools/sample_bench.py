"""Sampling generation at the cfg-2 model size (OFA-base, bf16; 32 sentences x 5 samples = 160 rows, max_len 32, V = 51 265)
next to beam generation of the same shape in the same run -- the only yardstick: ms per generation step through the captured
per-step graphs for plain sampling, top-k 256 and top-p 0.9 (min_len = max_len keeps every sentence open for all max_len + 1
steps; best of two replayed runs), then the sampling kernels alone at a mid step, next to the two beam kernels.  Prints the id
of the sources it ran on (tools/build_id.py).
Usage: python tools/sample_bench.py"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ofasys_amd import Sampling  # noqa: E402
from ofasys_amd import kernels as K  # noqa: E402
from ofasys_amd.generator import SequenceGenerator  # noqa: E402
from tools.beam_bench import BEAM, BSZ, MAX_LEN, timed  # noqa: E402

dev = torch.device("cuda")


def generate_ms(gen, model, sample):
    runs = []
    for rep in range(4):                                  # eager warm-up, capture, then two replays
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen.generate(model, sample)
        runs.append((time.perf_counter() - t0, gen.steps_run))
    return min(runs[2:])


def main():
    args = argparse.Namespace(arch="base", workload="cfg2", batch=BSZ)
    model, d = bench.build(args, dev)
    model.eval()
    batch, _, _ = bench.make_batch(d, BSZ, 191, 8, 0, dev, "cfg2")
    sample = {"net_input": {"slots": batch["slots"]}}
    print(f"source_id {bench.source_id()}")
    common = dict(beam_size=BEAM, max_len=MAX_LEN, min_len=MAX_LEN, normalize_scores=False)
    gens = [("beam", SequenceGenerator(d, **common))]
    for name, topk, topp in (("sample plain", -1, -1.0), ("sample top-k 256", 256, -1.0), ("sample top-p 0.9", -1, 0.9)):
        gens.append((name, SequenceGenerator(d, search_strategy=Sampling(d, topk, topp), seed=1, **common)))
    for name, gen in gens:
        dt, steps = generate_ms(gen, model, sample)
        print(f"{name:18s} generate rows={BSZ * BEAM}: {dt * 1e3:8.2f} ms for {steps} steps ({dt / steps * 1e3:6.3f} ms/step incl. "
              f"encoder), {BSZ / dt:8.1f} sentences/s")
    # the kernels alone, at a mid step of the same shape
    rows, V, step = BSZ * BEAM, len(d), 8
    beam, samp = gens[0][1], gens[1][1]
    logits = torch.randn(rows, V, device=dev).bfloat16()
    nbytes = logits.numel() * 2
    for gen in (beam, samp):
        gen._state["tokens"] = gen._dec.tokens
        gen._state["done"].zero_()
    kw = dict(min_len=1, max_len=MAX_LEN, pad=d.pad(), unk=d.unk(), eos=d.eos())
    st = beam._state
    t = timed(lambda: K.beam_topk(logits, BEAM, step, st["ws"], tokens=st["tokens"], done=st["done"], **kw)) * 1e3
    print(f"ofa_beam_topk     rows={rows} V={V} bf16: {t:7.1f} us  {nbytes / t / 1e3:7.1f} GB/s over {nbytes / 1e6:.1f} MB")
    t = timed(lambda: K.beam_select(st["ws"], st, BEAM, V, step, MAX_LEN, eos=d.eos(), unk=d.unk())) * 1e3
    print(f"ofa_beam_select   bsz={BSZ} beam={BEAM}: {t:7.1f} us")
    st = samp._state
    u = torch.rand(rows, device=dev)
    for name, topk, topp in (("plain", -1, -1.0), ("top-k 256", 256, -1.0), ("top-p 0.9", -1, 0.9)):
        t = timed(lambda: K.sample_draw(logits, BEAM, step, st["sample_ws"], u, topk=topk, topp=topp, tokens=st["tokens"],
                                        done=st["done"], **kw)) * 1e3
        print(f"ofa_sample_draw   {name:9s} rows={rows} V={V} bf16: {t:7.1f} us  ({nbytes / 1e6:.1f} MB of logits)")
    st["done"].zero_()
    st["fin_cnt"].zero_()
    t = timed(lambda: K.sample_select(st["sample_ws"], st, BEAM, step, MAX_LEN, eos=d.eos())) * 1e3
    print(f"ofa_sample_select bsz={BSZ} slots={BEAM}: {t:7.1f} us")


if __name__ == "__main__":
    main()
