"""GPU side of the row-normalisation oracle: runs one case of tests/rownorm_oracle.py through kernels.layernorm_fwd / layernorm_bwd /
join_fwd / join_bwd with every output NaN beforehand, and returns the outputs under the oracle's names.  tests/test_rownorm_edges_gpu.py
uses it in-process; run as a program it is the child process of the forced join forms:
    python tests/rownorm_gpu.py forced
loads the debug library (as tools/join_bench.py does), sets OFA_JOIN_FWD / OFA_JOIN_BWD before each call, checks the reduced table
against the same float64 oracle, prints one JSON line of worst figures and exits 1 on a miss."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    os.environ["OFASYS_AMD_LIB"] = os.path.join(ROOT, "ofasys_amd", "libofasys_amd_dbg.so")

from tests import rownorm_oracle as ro  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32 = torch.float32


def nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def poison(*specs):
    """Allocate and free NaN-filled tensors of exactly the sizes the wrapper is about to torch.empty: the caching allocator hands those
    blocks straight back, so an element the kernels leave unwritten reads NaN instead of an earlier call's number."""
    keep = [nan(shape, dtype) for shape, dtype in specs]
    torch.cuda.synchronize()
    del keep


def run_ln_fwd(K, b):
    x = b["x"]
    poison((x.shape, x.dtype), ((x.shape[0],), F32), ((x.shape[0],), F32))
    y, mean, rstd = K.layernorm_fwd(x, b["gamma"], b["beta"], b["eps"], fuse_gelu=b["gelu"])
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd)


def run_ln_bwd(K, b):
    """Accumulating cases hand in gradients that already hold prev; the others let the wrapper allocate (poisoned)."""
    x, prev = b["x"], b["prev"]
    cols = x.shape[1]
    kw = dict(fuse_gelu=b["gelu"], dres=b["dres"])
    if prev is not None:
        kw.update(dgamma=prev[0].clone(), dbeta=prev[1].clone(), dbias=prev[2].clone() if prev[2] is not None else None)
        poison((x.shape, x.dtype))
    else:
        kw.update(want_dbias=b["want_dbias"])
        poison((x.shape, x.dtype), *[((cols,), x.dtype)] * (3 if b["want_dbias"] else 2))
    dx, dgamma, dbeta, dbias = K.layernorm_bwd(b["dy"], x, b["gamma"], b["mean"], b["rstd"], **kw)
    torch.cuda.synchronize()
    out = dict(dx=dx, dgamma=dgamma, dbeta=dbeta)
    if b["gelu"] and b["want_dbias"]:
        out["dbias"] = dbias
    return out


def base_tensor(case):
    return torch.tensor([case.base], dtype=torch.int64, device=DEV) if case.base else None


def dropout_mask(K, case, dtype):
    """The keep decisions of the stand-alone dropout kernel (csrc/elementwise.hip) for the same flat size and stream position, which
    join.hip promises to reproduce per element -> bool [rows, cols]; its kept values are rnd(1 / (1 - p)) and the kept share lies
    within 5 standard deviations of 1 - p."""
    rows, cols = case.rows, ro.join_cols(case, dtype)
    v = K.dropout_add(torch.ones(rows, cols, dtype=dtype, device=DEV), None, case.p, ro.SEED, ro.OFFSET, base_tensor(case))
    mask = v != 0
    scale = (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(case.p))).to(dtype)
    assert bool((v[mask] == scale.to(DEV)).all()), (case.name, "kept values are not rnd(1 / (1 - p))")
    assert ro.keep_share_ok(mask, case.p), (case.name, float(mask.double().mean()))
    return mask


def run_join(K, case, c):
    """-> the outputs of join_fwd + join_bwd under the oracle's names; c = build_join(case, dtype, mask, DEV)."""
    x = c["x"]
    rows, cols = x.shape
    base = base_tensor(case)
    poison((x.shape, x.dtype), *([(x.shape, x.dtype)] if case.b else []), ((4, rows), F32))
    y, z, stats, keep = K.join_fwd(x, c["res"], (c["ga"], c["ba"]) if case.a else None, (c["gb"], c["bb"]) if case.b else None, c["eps"],
                                   c["p"], ro.SEED, ro.OFFSET, base)
    torch.cuda.synchronize()
    grads = [t.clone() if t is not None else None for t in c["prev"]]
    ns = K.lib().cdll.ofa_join_bwd_slots(rows, cols, K.dtype_code(x))
    poison(*([(x.shape, x.dtype)] if case.want_dres else []), (x.shape, x.dtype), ((5 * ns * cols,), F32))
    dres, dx = K.join_bwd(c["dy"], c["dz"], x if case.a else None, y if case.b else None, c["ga"], c["gb"], stats, c["p"], ro.SEED, ro.OFFSET,
                          base, tuple(grads if case.xsum else grads[:4]), want_dres=case.want_dres, keep=keep if case.keep else None)
    torch.cuda.synchronize()
    out = dict(y=y, dx=dx)
    if case.a:
        out.update(mean_a=stats[0], rstd_a=stats[1])
    if case.b:
        out.update(z=z, mean_b=stats[2], rstd_b=stats[3])
    if case.want_dres:
        out["dres"] = dres
    out.update({n: g for n, g in zip(ro.JOIN_GRADS, grads) if g is not None})
    out["keep"] = keep
    return out


def check(family, fig, dtype, tag, worst):
    """Every figure within what the oracle allows a kernel; worst: {(output, dtype name): largest figure so far}."""
    bad = []
    for n, v in fig.items():
        key = (n, ro.NAMES[dtype])
        worst[key] = max(worst.get(key, 0.0), v)
        if not v <= ro.limit(family, n, dtype, kernel=True):
            bad.append((n, v, ro.limit(family, n, dtype, kernel=True)))
    assert not bad, (tag, ro.NAMES[dtype], bad)


def join_case(K, case, dtype, worst, tag="", stash=None):
    """stash: a dict that receives the kernel's outputs (the forced forms compare the statistics of two forward forms)."""
    mask = dropout_mask(K, case, dtype) if case.p > 0 else None
    c = ro.build_join(case, dtype, mask, DEV)
    got = run_join(K, case, c)
    keep = got.pop("keep")
    if stash is not None:
        stash.update(got)
    check("join", ro.join_figures(c, got, dtype), dtype, case.name + tag, worst)
    return keep


def forced():
    from ofasys_amd import kernels as K
    from ofasys_amd import lib as L
    assert L.LIB_PATH.endswith("_dbg.so"), L.LIB_PATH
    # Forms: (fwd 0, bwd 0) the split-row pair; (fwd 1, bwd 0) the row-per-wave forward without keep bits, its mask regenerated by the
    # split-row backward; (fwd 1, bwd 1 / 2 / 3) the row-per-wave pairs.  (fwd 0, bwd 1 ... 3) is no valid pair: the split-row forward
    # writes no keep bits for the row-per-wave backward to read.  That OFA_JOIN_BWD took effect shows in the keep bits; that
    # OFA_JOIN_FWD did shows in the row statistics: the row-per-wave forward multiplies by 1 / cols and takes v_rsq_f32 where the
    # split-row forward divides and takes 1 / sqrt, so over the table their fp32 statistics cannot agree in every bit.
    worst, failed, differ = {}, [], 0
    for dtype in (ro.BF16, ro.FP16):
        for case in ro.forced_join_cases():
            stats = {}
            for fv, bv in ro.FORCED_FORMS:
                os.environ["OFA_JOIN_FWD"], os.environ["OFA_JOIN_BWD"] = fv, bv
                got = {}
                try:
                    keep = join_case(K, case, dtype, worst, f" fwd{fv} bwd{bv}", got)
                    assert (keep is not None) == (bv != "0" and case.p > 0), "keep bits: the forced form did not take its route"
                except AssertionError as e:
                    failed.append(f"{case.name} fwd{fv} bwd{bv} {ro.NAMES[dtype]}: {e}")
                stats.setdefault(fv, [got[n] for n in ("rstd_a", "rstd_b", "mean_a", "mean_b") if n in got])
            differ += any(not torch.equal(a, b) for a, b in zip(stats["0"], stats["1"]))
    if not differ:
        failed.append("OFA_JOIN_FWD changed no bit of any row statistic: the forward forms were not switched")
    print(json.dumps({"worst": {f"{n} {d}": v for (n, d), v in sorted(worst.items())}, "failed": failed}))
    return 1 if failed else 0


if __name__ == "__main__":
    assert sys.argv[1:] == ["forced"], "usage: python tests/rownorm_gpu.py forced"
    sys.exit(forced())
