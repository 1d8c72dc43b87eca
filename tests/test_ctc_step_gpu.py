"""GPU: the speech-to-text criterion inside TrainStep -- a micro-batch that carries "encoder_target" and "ctc_range" trains on
ce_weight * label-smoothed CE (decoder) + ctc_weight * CTC (encoder output . embed_tokens[ds:de]^T); speech_to_text_loss.py:197-241.

The audio batches ([AUDIO fbank][TEXT] -> [TEXT], oracle.cases "tiny_audio") run padded, as every audio micro-batch of the project
does; the packed-layout and captured-graph steps use a text source, whose encoder rows pack."""
import numpy as np
import pytest
import torch

from oracle import recipe
from oracle.cases import CASES, VOCAB_EXTRA, make_target
from tests import ctc_oracle as co
from tests.golden_util import case_inputs
from tests.model_util import build_model, make_slots

pytestmark = pytest.mark.gpu

DEV = "cuda"
V = 4 + VOCAB_EXTRA
DS, DE = 8, 40                   # the "phone" rows of the test vocabulary: 32 classes, class 0 (row DS) the blank
TEXT_CASE = {"arch": "tiny", "active": {"text"}, "overrides": {"use_self_attn_bias": False, "entangle_position_embedding": True, "dropout": 0.0},
             "adaptor_overrides": {}}


def _encoder_target(B, lens, seed, pad, eos):
    r = np.random.RandomState(seed)
    L = max(lens) + 1
    t = np.full((B, L), pad, np.int64)
    for b, n in enumerate(lens):
        t[b, :n] = r.randint(DS + 1, DE, size=n)
        t[b, n] = eos
    return torch.from_numpy(t)


def _audio_sample(dtype, ctc=None, lens=(3, 2), seed=3):
    vals, target = case_inputs(CASES["tiny_audio"])
    s = {"slots": make_slots(vals, DEV, dtype), "target": target.to(DEV)}
    if ctc is not None:
        s.update(encoder_target=_encoder_target(2, lens, seed, 1, 2).to(DEV), ctc_range=f"{DS},{DE}", **ctc)
    return s


def _engine(case, dtype, **kw):
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    model, d = build_model(case, DEV, dtype)
    assert (d.pad(), d.eos()) == (1, 2)
    ops.manual_seed(1234)
    return TrainStep(model, lr=1e-3, clip_norm=1.0, label_smoothing=0.1, **kw)


def _grads(tr):
    names = {id(p): n for n, p in tr.model.named_parameters()}
    # (FlatParams._view: a spatial convolution weight lives in the arena in channels-last order)
    return {names.get(id(p), str(i)): tr.fp._view(tr.fp.grad, o, p).float().clone()
            for i, (p, o) in enumerate(zip(tr.fp.params, tr.fp.offsets))}


def test_fp32_step_equals_torch_ctc_on_the_projected_encoder_output():
    """(a) loss and every parameter gradient within the project's fp32 bar (1e-3 relative, README), the embedding rows DS:DE and a row
    outside them included.  The KEY-side biases -- k_proj.bias and pos_k_linear.bias, the key projection of the position bias -- shift
    every score of a query row by one constant, which softmax does not see: their gradient is identically zero and what either run
    holds is the rounding residue of a sum that cancels.  They are held to 1e-3 of the largest gradient entry of the model instead, as
    tests/test_closed_set_head_gpu.py does for k_proj.bias."""
    from ofasys_amd import ops
    w = dict(ce_weight=0.7, ctc_weight=0.3, zero_infinity=True)
    tr = _engine(CASES["tiny_audio"], torch.float32)
    s = _audio_sample(torch.float32, w)
    out = tr.train_step([s], eager=True)
    got_loss, got_ctc, got = float(out["stats"][1]), float(out["ctc_loss"]), _grads(tr)
    # the same model, eagerly: the project's forward and label-smoothed op, torch's log_softmax + F.ctc_loss on the encoder side
    model, d = build_model(CASES["tiny_audio"], DEV, torch.float32)
    model.train()
    logits, _, enc = model(s["slots"], return_encoder_out=True)
    ce = ops.label_smoothed_cross_entropy(logits, s["target"], d.pad(), 0.1, None, None, 0.0)[0]
    W = model.decoder.adaptor.embed_tokens.weight
    x = torch.nn.functional.linear(enc["encoder_out"][0], W[DS:DE])
    masks = enc["encoder_padding_mask"][0]
    lengths = (~masks).sum(1)
    et = s["encoder_target"]
    keep = (et != d.pad()) & (et != d.eos())
    ctc = torch.nn.functional.ctc_loss(torch.log_softmax(x.float(), -1), (et - DS)[keep], lengths, keep.sum(1), blank=0, reduction="sum",
                                       zero_infinity=True)
    loss = 0.7 * ce + 0.3 * ctc
    loss.backward()
    torch.cuda.synchronize()
    want = {n: p.grad.float() for n, p in model.named_parameters() if p.grad is not None}
    assert float(ctc) > 0 and int(lengths.min()) < masks.shape[1]              # a live CTC term and a sentence with pad rows
    print(f"\nloss {got_loss:.6f} vs {float(loss):.6f}; ctc {got_ctc:.6f} vs {float(ctc):.6f}")
    assert abs(got_loss - float(loss)) <= 1e-3 * abs(float(loss)) and abs(got_ctc - float(ctc)) <= 1e-3 * abs(float(ctc))
    top = max(float(g.abs().max()) for g in want.values())
    worst = (0.0, None)
    for n, g in want.items():
        scale = top if n.endswith(("k_proj.bias", "pos_k_linear.bias")) else float(g.abs().max())
        if scale == 0:
            assert float(got[n].abs().max()) == 0, n
            continue
        share = float((got[n] - g).abs().max()) / scale
        worst = max(worst, (share, n))
        assert share <= 1e-3, (n, share)
    for n in got:
        if n not in want:
            assert float(got[n].abs().max()) == 0, n
    print(f"worst gradient tensor {worst[1]}: {worst[0]:.2e} of its max-abs")
    emb = next(n for n in want if n.endswith("decoder.adaptor.embed_tokens.weight") or n.endswith("encoder.adaptor.embed_tokens.weight"))
    ge, we = got[emb], want[emb]
    scale = float(we.abs().max())
    assert float(we[DS:DE].abs().max()) > 0
    assert float((ge[DS:DE] - we[DS:DE]).abs().max()) <= 1e-3 * scale and float((ge[DE + 5] - we[DE + 5]).abs().max()) <= 1e-3 * scale


def test_ctc_weight_zero_is_todays_label_smoothed_step_bit_for_bit():
    """(b)"""
    a = _engine(CASES["tiny_audio"], torch.float32)
    plain = a.train_step([_audio_sample(torch.float32)], eager=True)
    assert "ctc_loss" not in plain                                             # a step without such a micro-batch reports what it always did
    b = _engine(CASES["tiny_audio"], torch.float32)
    out = b.train_step([_audio_sample(torch.float32, dict(ce_weight=1.0, ctc_weight=0.0))], eager=True)
    torch.cuda.synchronize()
    assert torch.equal(a.fp.grad, b.fp.grad) and torch.equal(a.fp.flat, b.fp.flat) and torch.equal(a._stats, b._stats)
    assert float(out["ctc_loss"]) == 0.0


def _text_batch(step, packed):
    from ofasys_amd.packing import build_pack_plan
    g = np.random.Generator(np.random.Philox(key=300 + step))
    B = 5
    sl = g.integers(9, 30, B)
    tl = g.integers(2, 12, B)
    sl[0], tl[0] = 29, 11                                                      # the same padded shape every step
    src = recipe.tokens(f"ctc.s{step}", (B, 29), V, sl.tolist())
    prev = recipe.tokens(f"ctc.p{step}", (B, 11), V, tl.tolist(), bos=0)
    lens = [int(min(n // 3, 7)) for n in sl]                                   # labels fit their sentence's encoder rows
    s = {"slots": make_slots([("TEXT", True, src, None), ("TEXT", False, prev, None)], DEV, torch.bfloat16),
         "target": make_target(prev).to(DEV), "encoder_target": _encoder_target(B, [7] + lens[1:], 50 + step, 1, 2).to(DEV),
         "ctc_range": f"{DS},{DE}", "ce_weight": 0.5, "ctc_weight": 0.5, "zero_infinity": False}
    if packed:
        s["pack"] = build_pack_plan(src.eq(1), prev.eq(1), bucket=256).to(DEV)
    return s


def test_packed_equals_padded_and_the_replayed_graph_equals_eager():
    """(c) bf16, three steps: the packed run against the padded run within the packed-versus-padded tolerance of
    tests/test_packing_gpu.py (2e-2 of the loss); eager against one captured graph replayed, bit for bit."""
    runs = {}
    for mode in ("padded", "packed-eager", "packed-graph"):
        tr = _engine(TEXT_CASE, torch.bfloat16, use_graph=mode == "packed-graph", graph_warmup=1)
        losses, ctcs = [], []
        for step in range(3):
            out = tr.train_step([_text_batch(step, mode != "padded")])
            losses.append(float(out["stats"][1]))
            ctcs.append(float(out["ctc_loss"]))
        torch.cuda.synchronize()
        runs[mode] = (losses, ctcs, tr.fp.flat.clone(), tr)
    print("\n", {k: (v[0], v[1]) for k, v in runs.items()})
    assert runs["packed-eager"][0] == runs["packed-graph"][0] and runs["packed-eager"][1] == runs["packed-graph"][1]
    assert torch.equal(runs["packed-eager"][2], runs["packed-graph"][2])
    assert sum(1 for e in runs["packed-graph"][3]._graphs.values() if "graphs" in e) == 1
    for a, b in zip(runs["padded"][0] + runs["padded"][1], runs["packed-eager"][0] + runs["packed-eager"][1]):
        assert np.isfinite(a) and a > 0 and abs(a - b) <= 2e-2 * abs(a)


def _oracle_on_encoder_output(tr, s, valid):
    """The float64 oracle (and torch's fp32 CPU result) on the CTC logits the engine's model computes for micro-batch s."""
    from ofasys_amd import ops
    import contextlib
    tr.model.train()
    with (tr._valid_mode(tr.model) if valid else contextlib.nullcontext()), torch.no_grad():
        _, _, enc = tr.model(s["slots"], return_encoder_out=True)
        x = ops.encoder_ctc_logits(enc["encoder_out"][0], tr.model.decoder.adaptor.embed_tokens.weight, DS, DE)
        lengths = (~enc["encoder_padding_mask"][0]).sum(1).cpu().numpy()
        xq = x.detach().cpu().contiguous()
    labels = [co.labels_of(r, DS, 1, 2) for r in s["encoder_target"].cpu().numpy()]
    ref = co.ctc_reference(xq.double().numpy(), lengths, labels, False)
    t32 = co.torch_reference(xq, lengths, labels, False, torch.float32)
    bound = 2 * abs(t32[0] - ref["loss"]) + float(np.finfo(np.float32).eps) * xq.shape[0]
    return ref, labels, bound


def test_bf16_step_is_finite_and_its_ctc_statistic_equals_the_oracle_on_the_encoder_output():
    """(d) the bound of tests/test_ctc_gpu.py for a loss: twice torch's fp32 CPU error against the float64 oracle on the same (bf16)
    logits, plus the absolute floor eps32 * T."""
    w = dict(ce_weight=1.0, ctc_weight=1.0, zero_infinity=False)
    tr = _engine(CASES["tiny_audio"], torch.bfloat16)
    s = _audio_sample(torch.bfloat16, w)
    ref, _, bound = _oracle_on_encoder_output(tr, s, valid=False)
    out = tr.train_step([s], eager=True)
    torch.cuda.synchronize()
    got = float(out["ctc_loss"])
    print(f"\nctc_loss {got:.9f}, oracle {ref['loss']:.9f}, error {abs(got - ref['loss']):.3g}, bound {bound:.3g}; "
          f"loss {float(out['stats'][1]):.4f}, gnorm {float(out['gnorm']):.4f}")
    assert np.isfinite(ref["loss"]) and abs(got - ref["loss"]) <= bound
    assert np.isfinite(float(out["stats"][1])) and np.isfinite(float(out["gnorm"])) and bool(torch.isfinite(tr.fp.grad.float()).all())
    assert float(out["skipped"][0]) == 0


def test_validation_reports_ctc_loss_and_unit_errors_and_changes_no_bit_of_training():
    """(e) two validation batches, eager and from captured graphs: ctc_loss within the bound of tests/test_ctc_gpu.py summed over the batches (twice torch's fp32 CPU
    error against the oracle on the same logits + eps32 * T each), c_errors / c_total equal to the oracle's greedy decode scored
    against the labels; and a validation pass between two train steps leaves the training bit for bit what it was."""
    from ofasys_amd import ops
    w = dict(ce_weight=1.0, ctc_weight=1.0, zero_infinity=False)
    batches = [_audio_sample(torch.float32, w, (3, 2), seed=3), _audio_sample(torch.float32, w, (2, 4), seed=4)]
    tr = _engine(CASES["tiny_audio"], torch.float32)
    want_loss = want_err = want_tot = bound = 0.0
    for s in batches:
        ref, labels, b = _oracle_on_encoder_output(tr, s, valid=True)
        want_loss, bound = want_loss + ref["loss"], bound + b
        want_err += sum(ops.edit_distance(h, l) for h, l in zip(ref["decode"], labels))
        want_tot += sum(len(l) for l in labels)
    tr.valid_begin()
    for s in batches:
        tr.valid_step([s], eager=True)
    res = tr.valid_result()
    print(f"\nvalidation: ctc_loss {res['ctc_loss']:.6f} vs oracle {want_loss:.6f} (bound {bound:.3g}); c_errors {res['c_errors']} / c_total {res['c_total']}")
    assert abs(res["ctc_loss"] - want_loss) <= bound and (res["c_errors"], res["c_total"]) == (want_err, want_tot) and want_tot == 11
    assert res["ntokens"] > 0 and np.isfinite(res["loss"])
    # the captured path: each batch structure is run eagerly once, then captured and replayed; every pass reports the eager figures
    g = _engine(CASES["tiny_audio"], torch.float32, use_graph=True, graph_warmup=1)
    for _ in range(3):
        g.valid_begin()
        for s in batches:
            g.valid_step([s])
        rg = g.valid_result()
        assert (rg["ctc_loss"], rg["c_errors"], rg["c_total"], rg["loss"]) == (res["ctc_loss"], res["c_errors"], res["c_total"], res["loss"])
    assert g.captured_valid_graphs() == 2
    tr.valid_begin()                                                            # a pass without such micro-batches reports what it always did
    tr.valid_step([_audio_sample(torch.float32)], eager=True)
    assert "ctc_loss" not in tr.valid_result()
    runs = []
    for with_valid in (False, True):
        e = _engine(CASES["tiny_audio"], torch.float32)
        e.train_step([batches[0]], eager=True)
        if with_valid:
            e.valid_begin()
            for s in batches:
                e.valid_step([s], eager=True)
            e.valid_result()
        e.train_step([batches[1]], eager=True)
        torch.cuda.synchronize()
        runs.append((e.fp.flat.clone(), e.exp_avg.clone(), e.fp.grad.clone(), e._stats.clone(), e._ctc_stat.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_fp16_step_with_a_loss_scale_scales_the_ctc_gradient_with_the_rest():
    """loss_scale (fp16): the backward seed is the scale, CtcLossFn.backward gets scale * ctc_weight.  The step is finite and not
    skipped, its ctc_loss statistic meets the oracle bound, and the arena of a step at scale 128, divided by 128, is the arena of
    the same step at scale 1 within 2e-2 of its norm (the packed-versus-padded figure of tests/test_packing_gpu.py: both steps round
    every activation gradient to fp16 once, at magnitudes 128 apart)."""
    arenas = {}
    for scale in (1.0, 128.0):
        tr = _engine(TEXT_CASE, torch.float16, loss_scale={"init_scale": scale})
        s = _text_batch(0, False)                                              # (token slots: no float input to cast)
        ref, _, bound = _oracle_on_encoder_output(tr, s, valid=False)
        out = tr.train_step([s], eager=True)
        torch.cuda.synchronize()
        assert abs(float(out["ctc_loss"]) - ref["loss"]) <= bound, (float(out["ctc_loss"]), ref["loss"], bound)
        assert float(out["skipped"][0]) == 0 and float(out["loss_scale"]) == scale and bool(torch.isfinite(tr.fp.grad.float()).all())
        arenas[scale] = tr.fp.grad.float().clone()
    a, b = arenas[1.0], arenas[128.0] / 128.0
    rel = float((a - b).norm() / a.norm())
    print(f"\nfp16 arena at scale 128 / 128 against scale 1: relative difference {rel:.3e}")
    assert float(a.norm()) > 0 and rel <= 2e-2
