"""The four regions AROUND the layer stacks in the output of tools/prof_last_step.py (one replayed cfg-2 step): launches and kernel time of
the front (adaptors, packing, zero_grad), the decoder token embedding, the decoder embedding gradients and the tail (encoder-side
embedding / adaptor gradients, gradient norm, schedule).  python tools/prof_step_edges.py last_step.txt [more.txt ...]
Regions are cut at named kernels (the first layer GEMM, the unpack of the decoder rows, ...), not at offsets."""
import re, sys
def load(p):
    rows = []
    for l in open(p):
        m = re.match(r"\s*([\d.]+) us\s+\+\s*([\d.]+)\s+gap\s+[-\d.]+\s+grid\s+\d+\s+(.*)", l)
        if m: rows.append((float(m.group(1)), float(m.group(2)), m.group(3)))
    return rows
def first(rows, pat, start=0):
    for i in range(start, len(rows)):
        if pat in rows[i][2]: return i
    raise KeyError(pat)
def last(rows, pat, stop=None):
    for i in range((stop or len(rows)) - 1, -1, -1):
        if pat in rows[i][2]: return i
    raise KeyError(pat)
def report(p):
    r = load(p)
    out = [("launches per step", len(r), r[-1][0] + r[-1][1])]
    a, b = 0, first(r, "gemm_big_kernel")                                   # front: up to the first layer GEMM
    out.append(("front: adaptors, packing, zero_grad", b - a, sum(x[1] for x in r[a:b])))
    a = first(r, "embedding_fwd_kernel", b); b2 = first(r, "gemm_big_kernel", a)
    out.append(("decoder token embedding", b2 - a, sum(x[1] for x in r[a:b2])))
    g = first(r, "gather_rows_kernel", first(r, "step_stats_add"))          # backward: unpack of the decoder rows
    a = g + 1; e = last(r, "embedding_bwd", first(r, "gemm_big_mixed_kernel", a)) + 1
    out.append(("decoder embedding gradients", e - a, sum(x[1] for x in r[a:e])))
    a = first(r, "scatter_rows_part_kernel"); e = first(r, "step_schedule_kernel", a) + 1
    out.append(("tail: encoder-side embedding / adaptor gradients, norm", e - a, sum(x[1] for x in r[a:e])))
    return out
for p in sys.argv[1:]:
    print(p)
    for name, n, t in report(p):
        print(f"  {name:58s} {n:4d} launches {t:9.1f} us")
