"""Diverse decoding at the cfg-2 model size (OFA-base, bf16; 32 sentences, max_len 32, V = 51 265) next to plain beam search of the
same shape IN THE SAME RUN -- the only yardstick: ms per generation step through the captured per-step graphs (min_len = max_len
keeps every sentence open for all max_len + 1 steps; best of two replayed runs).  Beam 5: plain beam search twice, from two
generators (their difference is the run-to-run spread a diverse figure has to be read against), 5 groups and siblings; beam 4: plain
and 2 groups.  Then the sentence passes alone at a mid step (a diverse step differs from a plain one in nothing else).  Prints the id
of the sources it ran on (tools/build_id.py).
Usage: python tools/diverse_bench.py"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ofasys_amd import DiverseBeamSearch, DiverseSiblingsSearch  # noqa: E402
from ofasys_amd import kernels as K  # noqa: E402
from ofasys_amd.generator import SequenceGenerator  # noqa: E402
from tools.beam_bench import BSZ, MAX_LEN, timed  # noqa: E402
from tools.sample_bench import generate_ms  # noqa: E402

dev = torch.device("cuda")


def main():
    args = argparse.Namespace(arch="base", workload="cfg2", batch=BSZ)
    model, d = bench.build(args, dev)
    model.eval()
    batch, _, _ = bench.make_batch(d, BSZ, 191, 8, 0, dev, "cfg2")
    sample = {"net_input": {"slots": batch["slots"]}}
    print(f"source_id {bench.source_id()}")
    common = dict(max_len=MAX_LEN, min_len=MAX_LEN, normalize_scores=False)
    gens = [("beam 5 plain (a)", 5, None), ("beam 5 plain (b)", 5, None), ("beam 5 groups 5 x 0.5", 5, DiverseBeamSearch(d, 5, 0.5)),
            ("beam 5 siblings 0.5", 5, DiverseSiblingsSearch(d, 0.5)), ("beam 4 plain", 4, None),
            ("beam 4 groups 2 x 0.5", 4, DiverseBeamSearch(d, 2, 0.5))]
    built = {}
    for name, beam, strategy in gens:
        gen = built[name] = SequenceGenerator(d, beam_size=beam, search_strategy=strategy, **common)
        dt, steps = generate_ms(gen, model, sample)
        print(f"{name:22s} generate rows={BSZ * beam}: {dt * 1e3:8.2f} ms for {steps} steps ({dt / steps * 1e3:6.3f} ms/step incl. "
              f"encoder), {BSZ / dt:8.1f} sentences/s")
    # the sentence passes alone, at a mid step of the same shape, after one row pass over random logits
    V, step = len(d), 8
    for beam, passes in ((5, (("ofa_beam_select", None), ("ofa_diverse_group_select G=5", ("groups", 5, 0.5)),
                              ("ofa_diverse_sibling_select", ("siblings", 0.5)))),
                         (4, (("ofa_beam_select", None), ("ofa_diverse_group_select G=2", ("groups", 2, 0.5))))):
        gen = built[f"beam {beam} plain (a)" if beam == 5 else "beam 4 plain"]
        st = gen._state
        st["tokens"] = gen._dec.tokens
        logits = torch.randn(BSZ * beam, V, device=dev).bfloat16()
        kw = dict(eos=d.eos(), unk=d.unk())
        for name, strategy in passes:
            st["done"].zero_()
            st["fin_cnt"].zero_()
            K.beam_topk(logits, beam, step, st["ws"], tokens=st["tokens"], done=st["done"], min_len=1, max_len=MAX_LEN, pad=d.pad(),
                        unk=d.unk(), eos=d.eos())
            if strategy is None:
                fn = lambda: K.beam_select(st["ws"], st, beam, V, step, MAX_LEN, **kw)                          # noqa: E731
            elif strategy[0] == "groups":
                fn = lambda: K.diverse_group_select(st["ws"], st, beam, V, step, MAX_LEN, strategy[1], strategy[2], **kw)  # noqa: E731
            else:
                fn = lambda: K.diverse_sibling_select(st["ws"], st, beam, V, step, MAX_LEN, strategy[1], **kw)  # noqa: E731
            t = timed(fn) * 1e3
            print(f"{name:30s} bsz={BSZ} beam={beam} V={V}: {t:7.1f} us ({int(st['done'].sum())} sentences finished meanwhile)")


if __name__ == "__main__":
    main()
