"""GPU half of the image_vit tests: the QuickGELU kernels against the float64 oracle of tests/vit_oracle.py over its table, the
VisionTransformer backbone, the whole model with the adaptor active and one TrainStep against tests/golden/vit.npz (the reference's own
run on the CPU, tools/gen_vit_golden.py).  fp32 is held to the project's parity bound 1e-3; bf16 to twice the reference's OWN
bf16-vs-fp32 gap recorded per output (max |a - b| / max |b| on the recorded tensor: the output, or a gradient's strided sample)."""
import pytest
import torch

from ofasys_amd.module.vit import VisionTransformer
from tests import vit_case as C
from tests import vit_oracle as O
from tests.golden_util import case_inputs, load_golden, rel_err
from tests.model_util import build_model, make_slots

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
FP32_BOUND = 1e-3


@pytest.fixture(scope="module")
def golden():
    return load_golden("vit")


# ------------------------------------------------------------------------------------------------------------------ kernels
def _run_kernels(h, dy):
    from ofasys_amd import kernels as K
    a = K.quick_gelu_fwd(h)
    dh, part = K.quick_gelu_bwd(dy, h, want_partials=True)
    return a, dh, part


@pytest.mark.parametrize("dtype", O.DTYPES3, ids=lambda d: O.NAMES[d])
def test_quick_gelu_kernels_over_the_table(dtype):
    from ofasys_amd import kernels as K
    worst = {}
    for case in O.CASES:
        h, dy = O.build(case, dtype)
        ref = O.qgelu_reference(h, dy)
        hd, dyd = h.to(DEV), dy.to(DEV)
        a, dh, part = _run_kernels(hd, dyd)
        a2, dh2, part2 = _run_kernels(hd, dyd)
        assert torch.equal(a, a2) and torch.equal(dh, dh2) and torch.equal(part, part2), case.name      # two calls: equal bits
        assert part.shape == (O.slots_of(case.rows), h.shape[1])
        dh_plain = K.quick_gelu_bwd(dyd, hd)                                                             # ws == NULL: the same dh
        assert torch.equal(dh_plain, dh), case.name
        # the fold of the partial rows, as the FoldQueue finishes it, twice; and the immediate column sum of the stored dh
        folds = []
        for _ in range(2):
            out = torch.zeros(h.shape[1], dtype=dtype, device=DEV)
            K.ImmediateFold().add(part, 0, out, h.shape[1], h.shape[1], part.shape[0], 1.0, False)
            folds.append(out)
        assert torch.equal(folds[0], folds[1]), case.name
        immediate = K.colsum(dh, out_dtype=dtype)
        got = {"a": a.cpu(), "dh": dh.cpu(), "colsum": folds[0].cpu(), "partial": part.cpu()}
        f = O.figures(ref, got, dtype)
        f["immediate"] = O.excess(immediate.cpu(), ref["colsum"][0], ref["colsum"][1], dtype)
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
            lim = O.limit("colsum" if k == "immediate" else k, dtype)
            assert v <= lim, (case.name, k, v, lim)
        if case.regime == "sat":
            pos, zero = h.float() > 0, h.float() == 0
            assert torch.equal(got["a"][pos], h[pos]) and bool((got["a"][zero] == 0).all()), case.name
    print(O.NAMES[dtype], {k: f"{v:.3g}" for k, v in worst.items()})


def test_quick_gelu_refuses_ragged_columns():
    from ofasys_amd import kernels as K
    from ofasys_amd.lib import OfaError
    x = torch.zeros(4, 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(OfaError):
        K.quick_gelu_fwd(x)
    with pytest.raises(OfaError):
        K.quick_gelu_bwd(x, x)
    e = torch.zeros(0, 16, dtype=torch.bfloat16, device=DEV)
    assert K.quick_gelu_fwd(e).shape == (0, 16) and K.quick_gelu_bwd(e, e).shape == (0, 16)


@pytest.mark.parametrize("deferred", (False, True), ids=("immediate-fold", "fold-queue"))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
def test_quick_gelu_delivers_the_bias_gradient_to_an_arena_sink(dtype, deferred):
    """ops.quick_gelu with a gradient sink on the bias, with the step's fold queue (deferred reductions) and without it (gradients consumed
    inside backward: data-parallel bucket all-reduces, the eager fallback) -- the partial rows are folded only after the kernel that
    writes them.  The sink starts at 1: the gradient is ADDED to it."""
    from ofasys_amd import kernels as K
    from ofasys_amd import ops
    case = next(c for c in O.CASES if c.m == 65 and c.rows == O.ROWS_PER_BLOCK + 1 and c.regime == "prow")
    h, dy = (t.to(DEV) for t in O.build(case, dtype))
    ref = O.qgelu_reference(h.cpu(), dy.cpu())
    bias = torch.nn.Parameter(torch.zeros(h.shape[1], dtype=dtype, device=DEV))
    was_on = ops._Fold.queue is not None
    results = []
    try:
        ops.defer_reductions(deferred)
        for _ in range(2):
            # (a fresh buffer per run, filled with a poison first so that a fold of unwritten partial rows cannot pass by luck)
            poison = [torch.full((4, h.shape[1]), 1e30, device=DEV) for _ in range(8)]
            del poison
            bias._ofa_grad = torch.ones(h.shape[1], dtype=dtype, device=DEV)
            x = h.clone().requires_grad_(True)
            ops.quick_gelu(x, bias).backward(dy)
            torch.cuda.synchronize()
            assert bias.grad is None                                             # delivered to the sink, not through autograd
            assert torch.equal(x.grad, K.quick_gelu_bwd(dy, h))
            results.append(bias._ofa_grad.clone())
    finally:
        ops.defer_reductions(was_on)
        del bias._ofa_grad
    assert torch.equal(results[0], results[1])
    got = results[0].double().cpu() - 1.0
    # one more rounding than the oracle's column sum: the 16-bit sink holds round(1 + sum)
    bound = ref["colsum"][1] + (1.0 if dtype != O.F32 else 0.0)
    fig = O.excess(got, ref["colsum"][0], bound, dtype)
    print(O.NAMES[dtype], "deferred" if deferred else "immediate", f"{fig:.3g}")
    assert fig <= O.limit("colsum", dtype)
    # and without a sink the gradient comes back through autograd as a separate column sum
    plain = torch.nn.Parameter(torch.zeros(h.shape[1], dtype=dtype, device=DEV))
    x = h.clone().requires_grad_(True)
    ops.quick_gelu(x, plain).backward(dy)
    assert O.excess(plain.grad.double().cpu(), ref["colsum"][0], ref["colsum"][1], dtype) <= O.limit("colsum", dtype)


# ------------------------------------------------------------------------------------------------------------------ backbone
def _grad_figures(golden, tag, grads):
    """[(key, |norm - want| / want, rel_err of the strided sample, the reference's own bf16 gap of that sample)]."""
    keys = [str(k) for k in golden[tag + ".gkeys"]]
    counts, norms, flat, gaps = golden[tag + ".gcount"], golden[tag + ".gnorm"], torch.from_numpy(golden[tag + ".gsample"]), golden[tag + ".gap_g"]
    out, o = [], 0
    for k, n, want, gap in zip(keys, counts, norms, gaps):
        g = grads[k].detach().float().cpu()
        out.append((k, abs(float(g.double().norm()) - want) / want, rel_err(C.sample(g), flat[o:o + n]), float(gap)))
        o += int(n)
    return out


def _check_grads(golden, tag, grads, dtype):
    figs = _grad_figures(golden, tag, grads)
    assert len(figs) == len(grads)
    worst = max(figs, key=lambda f: f[2] / (FP32_BOUND if dtype == torch.float32 else 2 * f[3]))
    print(tag, str(dtype), "worst gradient", worst)
    for k, e_norm, e_s, gap in figs:
        if dtype == torch.float32:
            assert e_norm < FP32_BOUND and e_s < FP32_BOUND, (k, e_norm, e_s)
        else:
            assert e_s <= 2 * gap, (k, e_s, gap)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("name", list(C.BACKBONE_CASES))
def test_backbone_against_the_golden(golden, name, dtype):
    args, _ = C.BACKBONE_CASES[name]
    m = VisionTransformer(*args)
    C.fill_backbone_state(name, m.state_dict())
    m = m.to(DEV).to(dtype)
    img, dout = C.backbone_inputs(name)
    rows, h, w = m(img.to(DEV).to(dtype))
    assert (h, w) == C.grid_of(name) and rows.shape == (C.B * h * w, args[2])
    y = rows.view(C.B, h * w, args[2])
    (y.float() * dout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    e = rel_err(y.detach().float().cpu(), torch.from_numpy(golden[f"bb.{name}.out"]))
    gap = float(golden[f"bb.{name}.gap_out"][0])
    print(name, str(dtype), "output", f"{e:.3e}", "reference bf16 gap", f"{gap:.3e}")
    assert e < FP32_BOUND if dtype == torch.float32 else e <= 2 * gap
    _check_grads(golden, "bb." + name, {k: p.grad for k, p in m.named_parameters()}, dtype)


def test_fused_and_unfused_tiers_are_the_ones_claimed():
    from ofasys_amd import ops
    x = torch.zeros(2, 16, 128, dtype=torch.bfloat16, device=DEV)
    assert ops.in_proj_self_attention_ok(x, 2) and not ops.in_proj_self_attention_ok(x.float(), 2)
    assert not ops.in_proj_self_attention_ok(torch.zeros(2, 16, 160, dtype=torch.bfloat16, device=DEV), 2)


# ------------------------------------------------------------------------------------------------------------------ whole model
def _model_run(dtype):
    from ofasys_amd import ops
    model, d = build_model(C.MODEL_CASE, DEV, dtype)
    model.eval()
    vals, target = case_inputs(C.MODEL_CASE)
    slots = make_slots(vals, DEV, dtype)
    hooked = {}
    adaptor = model.encoder.adaptor.image_vit
    hk = adaptor.image_proj.register_forward_hook(lambda m, i, o: hooked.__setitem__("embed", o.detach().float()))
    assert model.encoder.adaptor.get_adaptor(slots[0]) is adaptor                       # `adaptor=image_vit` routes there
    logits, _ = model(slots)[:2]
    loss = ops.cross_entropy_sum(logits, target.to(DEV), d.pad())
    loss.backward()
    hk.remove()
    torch.cuda.synchronize()
    return model, logits.detach().float().cpu(), float(loss), hooked["embed"].cpu()


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_model_with_image_vit_against_the_golden(golden, dtype):
    model, logits, loss, embed = _model_run(dtype)
    e_l = rel_err(logits, torch.from_numpy(golden["model.logits"]))
    e_e = rel_err(embed.reshape(-1)[::C.EMBED_STRIDE], torch.from_numpy(golden["model.embed"]))
    e_loss = abs(loss - float(golden["model.loss"][0])) / float(golden["model.loss"][0])
    gl, ge = float(golden["model.gap_logits"][0]), float(golden["model.gap_embed"][0])
    print(str(dtype), "logits", f"{e_l:.3e}", "embed", f"{e_e:.3e}", "loss", f"{e_loss:.3e}", "reference bf16 gaps", gl, ge)
    if dtype == torch.float32:
        assert e_l < FP32_BOUND and e_e < FP32_BOUND and e_loss < FP32_BOUND
    else:
        assert e_l <= 2 * gl and e_e <= 2 * ge
    grads = {k: p.grad for k, p in model.named_parameters() if k.startswith(C.MODEL_PREFIX) and p.grad is not None}
    assert any("image_proj" in k for k in grads) and any("image_rel_pos_table_list" in k for k in grads)
    assert any("embed_image_positions" in k for k in grads) and any("in_proj_weight" in k for k in grads)
    _check_grads(golden, "model", grads, dtype)


# ------------------------------------------------------------------------------------------------------------------ TrainStep
def _step_engine(use_graph):
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    model, d = build_model(C.MODEL_CASE, DEV, torch.bfloat16)
    ops.manual_seed(1234)
    return TrainStep(model, lr=1e-3, clip_norm=1.0, label_smoothing=0.1, use_graph=use_graph, graph_warmup=1)


def test_train_step_graph_equals_eager_and_updates_every_vit_parameter():
    vals, target = case_inputs(C.MODEL_CASE)
    runs = {}
    for mode in ("eager", "graph", "graph2"):
        tr = _step_engine(mode != "eager")
        before = {k: p.detach().clone() for k, p in tr.model.named_parameters() if k.startswith(C.MODEL_PREFIX)}
        sample = {"slots": make_slots(vals, DEV, torch.bfloat16), "target": target.to(DEV), "task": "caption"}
        losses = [float(tr.train_step([sample])["stats"][1]) for _ in range(3)]
        torch.cuda.synchronize()
        runs[mode] = (losses, tr.fp.flat.clone())
        if mode == "graph":
            assert sum(1 for e in tr._graphs.values() if "graphs" in e) == 1
        if mode == "eager":
            still = [k for k, p in tr.model.named_parameters() if k in before and torch.equal(p.detach(), before[k])]
            assert not still, still
    print(runs["eager"][0], runs["graph"][0])
    assert all(l == l and l > 0 for l in runs["eager"][0])
    assert runs["eager"][0] == runs["graph"][0] and torch.equal(runs["eager"][1], runs["graph"][1])       # captured == eager, bit for bit
    assert runs["graph"][0] == runs["graph2"][0] and torch.equal(runs["graph"][1], runs["graph2"][1])     # two replayed runs are equal
