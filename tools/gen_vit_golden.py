"""Generate tests/golden/vit.npz (+ vit.manifest.json) by RUNNING THE REFERENCE on the CPU (build container only) on the cases of
tests/vit_case.py.

TEST INFRASTRUCTURE.  Usage:  python tools/gen_vit_golden.py
Only data is stored -- no reference source:
  * backbone cases: the reference's VisionTransformer (module/vit.py) with recipe weights on a recipe image; its output as the adaptor
    flattens it ([B, T, width]), and for loss = sum(output * dout) every parameter gradient as (norm, evenly strided sample);
  * the model case: the reference GeneralistModel with image_vit (vit_base) active -- logits, loss, image_proj's output (strided), and
    the gradients of every parameter of the adaptor in the same form;
  * the key|shape list of the adaptor's state dict and the defaults of its config;
  * for every recorded output and gradient sample, the reference's OWN bf16-vs-fp32 gap (the same run with the module and the inputs
    in bfloat16), as max |a - b| / max |b| -- the bf16 tests hold the implementation to twice that gap.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import recipe  # noqa: E402
from oracle.cases import VOCAB_EXTRA, make_target, make_value  # noqa: E402
from oracle.ref_import import build_reference_model, install  # noqa: E402
from tests import vit_case as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vit.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "vit.manifest.json")


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def grads_of(named):
    keys = [k for k, p in named if p.grad is not None]
    params = dict(named)
    return keys, [params[k].grad.detach().float() for k in keys]


def record_grads(out, tag, keys, grads, grads16):
    out[tag + ".gkeys"] = np.array(keys)
    out[tag + ".gnorm"] = np.array([float(g.double().norm()) for g in grads], np.float64)
    samples = [C.sample(g) for g in grads]
    out[tag + ".gcount"] = np.array([s.numel() for s in samples], np.int64)
    out[tag + ".gsample"] = torch.cat(samples).numpy()
    out[tag + ".gap_g"] = np.array([rel(C.sample(b), C.sample(a)) for a, b in zip(grads, grads16)], np.float64)


def run_backbone(name, VisionTransformer, dtype):
    args, _ = C.BACKBONE_CASES[name]
    torch.manual_seed(1)
    m = VisionTransformer(*args)
    C.fill_backbone_state(name, m.state_dict())
    m = m.to(dtype)
    x, dout = C.backbone_inputs(name)
    y = m(x.to(dtype)).flatten(2).transpose(1, 2)
    (y.float() * dout).sum().backward()
    return m, y.detach().float()


def run_model(dtype, rec):
    import ofasys  # noqa: F401
    from ofasys import ModalityType
    from ofasys.engine.criterion.cross_entropy import nll_loss
    from ofasys.preprocessor import Slot
    case = C.MODEL_CASE
    model, d = build_reference_model(case["arch"], VOCAB_EXTRA, case["active"], case["overrides"], case["adaptor_overrides"])
    recipe.fill_state(model.state_dict())
    model = model.to(dtype)
    model.eval()
    slots, prev = [], None
    for mod, is_src, spec, attrs in case["slots"]:
        v = make_value(spec, len(d))
        if v.is_floating_point():
            v = v.to(dtype)
        slots.append(Slot(ModalityType[mod], is_src, v, attributes=attrs))
        if not is_src:
            prev = v
    target = make_target(prev)
    h = model.encoder.adaptor.image_vit.image_proj.register_forward_hook(lambda m, i, o: rec.__setitem__("embed", o.detach().float()))
    logits, extra = model(slots)[:2]
    lprobs = model.get_normalized_probs((logits, extra), log_probs=True)
    loss = nll_loss(lprobs.view(-1, lprobs.size(-1)), target.view(-1), ignore_index=d.pad(), reduce=True)
    model.zero_grad()
    loss.backward()
    h.remove()
    return model, logits.detach().float(), loss.detach().float(), target


def main():
    install()
    from ofasys.module.vit import VisionTransformer
    out, manifest = {}, {"backbone": {}, "model": {}}
    for name in C.BACKBONE_CASES:
        m32, y32 = run_backbone(name, VisionTransformer, torch.float32)
        m16, y16 = run_backbone(name, VisionTransformer, torch.bfloat16)
        tag = "bb." + name
        out[tag + ".out"] = y32.numpy()
        out[tag + ".gap_out"] = np.array([rel(y16, y32)])
        keys, g32 = grads_of(list(m32.named_parameters()))
        keys16, g16 = grads_of(list(m16.named_parameters()))
        assert keys == keys16 and len(keys) == len(list(m32.parameters()))
        record_grads(out, tag, keys, g32, g16)
        manifest["backbone"][name] = {"args": C.BACKBONE_CASES[name][0], "image": C.BACKBONE_CASES[name][1], "tokens": y32.shape[1],
                                      "gap_out": float(out[tag + ".gap_out"][0]), "gap_g_max": float(out[tag + ".gap_g"].max())}
        print(name, tuple(y32.shape), "ref bf16 gap: out", manifest["backbone"][name]["gap_out"], "grads max",
              manifest["backbone"][name]["gap_g_max"])

    rec32, rec16 = {}, {}
    model, logits, loss, target = run_model(torch.float32, rec32)
    model16, logits16, loss16, _ = run_model(torch.bfloat16, rec16)
    P = C.MODEL_PREFIX
    out["model.logits"] = logits.numpy()
    out["model.loss"] = loss.numpy().reshape(1)
    out["model.target"] = target.numpy()
    out["model.embed"] = rec32["embed"].reshape(-1)[::C.EMBED_STRIDE].numpy()
    out["model.gap_logits"] = np.array([rel(logits16, logits)])
    out["model.gap_embed"] = np.array([rel(rec16["embed"], rec32["embed"])])
    named = [(k, p) for k, p in model.named_parameters() if k.startswith(P)]
    named16 = [(k, p) for k, p in model16.named_parameters() if k.startswith(P)]
    keys, g32 = grads_of(named)
    keys16, g16 = grads_of(named16)
    assert keys == keys16
    record_grads(out, "model", keys, g32, g16)
    state = model.encoder.adaptor.image_vit.state_dict()
    out["model.state_keys"] = np.array([f"{k}|{tuple(v.shape)}" for k, v in state.items()])
    cfg_cls = type(model.cfg.adaptor.image_vit)
    defaults = {f.name: (f.default if f.default is not dataclasses.MISSING else None) for f in dataclasses.fields(cfg_cls)
                if not f.name.startswith("_")}
    defaults = {k: (str(v) if not isinstance(v, (int, float, bool, type(None))) else v) for k, v in defaults.items()}
    out["model.cfg_defaults"] = np.array([f"{k}={v!r}" for k, v in defaults.items()])
    manifest["model"] = {"case": {k: (sorted(v) if isinstance(v, set) else v) for k, v in C.MODEL_CASE.items()},
                         "loss": float(loss), "gap_logits": float(out["model.gap_logits"][0]),
                         "gap_embed": float(out["model.gap_embed"][0]), "gap_g_max": float(out["model.gap_g"].max()),
                         "params": len(keys), "state_keys": len(state), "cfg_defaults": defaults}
    manifest["inputs"] = "recipe keys: vit.<case>.image, vit.<case>.dout, vit.<case>.<state key>; model: oracle.recipe.fill_state"
    print("model loss", float(loss), "ref bf16 gap: logits", manifest["model"]["gap_logits"], "embed", manifest["model"]["gap_embed"],
          "grads max", manifest["model"]["gap_g_max"])
    np.savez_compressed(OUT, **out)
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
