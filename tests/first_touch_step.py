"""Subprocess entry of tests/test_grad_first_touch_gpu.py (debug library in OFASYS_AMD_LIB, whose OFA_STEP_TAIL_OLD switch is read at
every call): three train steps of the tiny two-task x two-micro-batch model (tied embedding, parameters that get no gradient) with the
gradient arena pre-filled with 3.0 before every step, run three ways -- first-touch eager, first-touch captured and replayed, and the
arena-wide fill of before -- and compared as numbers.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

STEPS = 3


def run(old, use_graph):
    from oracle import trainstep_case as TC
    from oracle.cases import VOCAB_EXTRA
    from tests.model_util import build_model, make_slots
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    os.environ["OFA_STEP_TAIL_OLD"] = "7" if old else "0"      # all three items: the fill, the separate norm / schedule, criterion launches
    case = {"arch": TC.ARCH, "active": TC.ACTIVE, "overrides": TC.OVERRIDES, "adaptor_overrides": {}}
    ops.manual_seed(7)
    model, _ = build_model(case, "cuda", torch.bfloat16)
    samples = []
    for t, task in enumerate(TC.TASKS):
        for specs in task:
            vals, target = TC.micro_batch(specs, 4 + VOCAB_EXTRA)
            samples.append({"slots": make_slots(vals, "cuda", torch.bfloat16), "target": target.to("cuda"), "task": f"task{t}"})
    tr = TrainStep(model, lr=1e-3, clip_norm=1.0, use_graph=use_graph, graph_warmup=1)
    rec = []
    for _ in range(STEPS):
        tr.fp.grad.fill_(3.0)                        # nothing may depend on what the arena held
        out = tr.train_step(samples)
        torch.cuda.synchronize()
        rec.append({"grad": tr.fp.grad.clone(), "gnorm": out["gnorm"].clone(), "stats": out["stats"].clone(), "master": tr.master.clone()})
    info = {"graphs": tr.captured_graphs(), "prezero": sum(len(v) for v in tr._prezero.values()),
            "unused": sum(hi - lo for lo, hi in ops._Touched.unused),
            "gaps": sum((-p.numel()) % 8 for p in tr.fp.params), "rng": sum(int(b) for b in ops._Rng.base.values()),
            "finite": bool(all(torch.isfinite(r["grad"].float()).all() for r in rec)),
            "nonzero": int((rec[-1]["grad"] != 0).sum()), "numel": tr.fp.numel}
    return rec, info


def same(a, b):
    return [all(torch.equal(x[k], y[k]) for k in ("grad", "gnorm", "stats", "master")) for x, y in zip(a, b)]


def main():
    from ofasys_amd import lib as L
    assert L.LIB_PATH.endswith("_dbg.so"), L.LIB_PATH
    new, info_new = run(False, False)
    old, info_old = run(True, False)
    rep, info_rep = run(False, True)
    print(json.dumps({"new_vs_old": same(new, old), "eager_vs_replay": same(new, rep), "new": info_new, "old": info_old,
                      "replay": info_rep, "gnorm": [float(r["gnorm"]) for r in new]}))


if __name__ == "__main__":
    main()
