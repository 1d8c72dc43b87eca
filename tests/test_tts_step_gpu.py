"""GPU: text-to-speech through the model and the step engine against tests/golden/tts.npz (the reference's own run on the CPU,
tools/gen_tts_golden.py).  fp32 is held to the project's parity bound 1e-3; bf16 to twice the reference's OWN bf16-vs-fp32 gap recorded
per tensor (max |a - b| / max |b| on the recorded tensor: the output, or a gradient's strided sample); the bf16 gradient comparison
covers the adaptor's own parameters, as the image_vit tests do.

Gradients that are zero by construction -- key-projection biases (softmax is shift invariant) and a convolution bias in front of a
train-mode BatchNorm (the batch mean takes it out) -- stand in the golden as rounding noise (norm < 1e-6 of the largest gradient norm).
For those the test asks for noise, not a live gradient: a norm below 1e-5 of the largest gradient norm in fp32; in bf16 below 2^-8 of
it -- such a gradient is a sum of cancelling terms, each rounded to bf16 at 2^-9 of its own size, and no term exceeds the live
gradients' size (the reference's own bf16 noise there is no yardstick: its kernels round at other points).  None of these
parameters belongs to the text-to-speech path except the postnet's convolution biases."""
import pytest
import torch

from oracle.cases import CASES, make_target, make_value
from tests import tts_case as C
from tests import tts_oracle as O
from tests.golden_util import load_golden, rel_err
from tests.model_util import build_model

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
FP32_BOUND = 1e-3
ZERO_NORM = 1e-6


@pytest.fixture(scope="module")
def golden():
    return load_golden("tts")


def _slots(golden, d, dtype, rows=None):
    from ofasys_amd import ModalityType, Slot
    sel = slice(None) if rows is None else slice(0, rows)
    prev = torch.from_numpy(golden["prev_outputs"])[sel].to(DEV).to(dtype)
    lengths = torch.from_numpy(golden["target_lengths"])[sel].to(DEV)
    target = torch.from_numpy(golden["target"])[sel].to(DEV).to(dtype)
    slots = [Slot(ModalityType.TEXT, True, C.source_tokens(len(d))[sel].to(DEV)),
             Slot(ModalityType.AUDIO, False, {"fbank": prev, "fbank_lengths": lengths})]
    return slots, target, lengths


def _sample(golden, d, dtype, rows=None):
    slots, target, lengths = _slots(golden, d, dtype, rows)
    return {"slots": slots, "target": target, "target_lengths": lengths, "bce_pos_weight": C.BCE_POS_WEIGHT, "task": "tts"}


def _check_grads(golden, grads, dtype):
    """fp32: every recorded gradient, norm and strided sample, at 1e-3.  bf16: the strided samples of the adaptor's own parameters
    (C.PREFIX, as the image_vit tests compare their adaptor's) at twice the reference's own bf16 gap for that sample; what lies upstream of
    the adaptor (the decoder and encoder stacks) is pinned in bf16 by the stacks' own tests.  -> the number of gradients compared."""
    keys = [str(k) for k in golden["gkeys"]]
    counts, norms, flat = golden["gcount"], golden["gnorm"], torch.from_numpy(golden["gsample"])
    top = float(norms.max())
    figs, bad, o = [], [], 0
    for k, n, want, gap in zip(keys, counts, norms, golden["gap_g"]):
        o += int(n)
        if grads.get(k) is None or (dtype != torch.float32 and not k.startswith(C.PREFIX)):
            continue
        g = grads[k].detach().float().cpu()
        norm = float(g.double().norm())
        if want < ZERO_NORM * top:                                             # zero by construction (see the module docstring)
            bound = 10 * ZERO_NORM * top if dtype == torch.float32 else 2.0 ** -8 * top
            figs.append((k, "zero by construction", norm, bound))
            if not norm <= bound:
                bad.append(figs[-1])
            continue
        e_norm, e_s = abs(norm - want) / want, rel_err(C.sample(g), flat[o - int(n):o])
        bound = FP32_BOUND if dtype == torch.float32 else 2 * float(gap)
        figs.append((k, f"norm {e_norm:.2e}", e_s, bound))
        if not (e_s <= bound and (dtype != torch.float32 or e_norm < FP32_BOUND)):
            bad.append(figs[-1])
    print(str(dtype), "gradients compared", len(figs))
    for f in figs:
        if f[0].startswith(C.PREFIX) or f in bad:
            print("   ", f[0], f[1], f"{f[2]:.3e}", "bound", f"{f[3]:.3e}")
    assert not bad, bad
    return len(figs)


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_model_against_the_golden(golden, dtype):
    from ofasys_amd import ops
    model, d = build_model(C.CASE, DEV, dtype)
    model.train()                                        # every dropout of the case is 0; BatchNorm takes batch statistics
    slots, target, lengths = _slots(golden, d, dtype)
    post, extra = model(slots)[:2]
    assert isinstance(extra["attn"], list) and len(extra["attn"]) == 1       # (None on the fused attention path: nothing to transpose)
    assert extra["eos_out"].shape == (C.B, 11, 1) and extra["feature_out"].shape == post.shape == (C.B, 11, C.F)
    loss, terms = ops.tacotron2_loss(extra["feature_out"], post, extra["eos_out"], target, lengths, C.BCE_POS_WEIGHT, "mean")
    loss.backward()
    torch.cuda.synchronize()
    figs = {k: (rel_err(t.detach().float().cpu(), torch.from_numpy(golden[k])), float(golden["gap_" + k][0]))
            for k, t in (("post", post), ("feature_out", extra["feature_out"]), ("eos_out", extra["eos_out"]))}
    got = torch.cat((loss.detach().reshape(1), terms)).double().cpu()
    figs["loss_mean"] = (rel_err(got, torch.from_numpy(golden["loss_mean"])), float(golden["gap_loss_mean"][0]))
    print(str(dtype), {k: (f"{e:.3e}", f"gap {g:.3e}") for k, (e, g) in figs.items()})
    for k, (e, gap) in figs.items():
        assert e < FP32_BOUND if dtype == torch.float32 else e <= 2 * gap, (k, e, gap)
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    for part in ("prenet.0.layers.1.0.weight", "prenet.1.bias", "feat_proj.weight", "eos_proj.weight", "postnet.convolutions.0.0.weight",
                 "postnet.convolutions.1.1.weight", "postnet.convolutions.2.0.weight", "embed_audio_positions.weight"):
        assert C.PREFIX + part in grads, part
    assert _check_grads(golden, grads, dtype) >= (250 if dtype == torch.float32 else 30)


def test_prenet_dropout_draws_in_eval_mode_too(golden):
    """The reference's prenet calls F.dropout with training=True always: an eval-mode forward with prenet_dropout > 0 depends on the
    Philox position, and the same position gives the same output."""
    from ofasys_amd import ops
    case = dict(C.CASE, adaptor_overrides={"audio_fbank": dict(C.CASE["adaptor_overrides"]["audio_fbank"], prenet_dropout=0.5)})
    model, d = build_model(case, DEV, torch.bfloat16)
    model.eval()
    slots, _, _ = _slots(golden, d, torch.bfloat16)
    outs = []
    with torch.no_grad():
        for seed in (1, 2, 1):
            ops.manual_seed(seed)
            outs.append(model(slots)[0].clone())
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------ TrainStep
def _engine(use_graph, case=C.CASE, **kw):
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    model, d = build_model(case, DEV, torch.bfloat16)
    ops.manual_seed(1234)
    return TrainStep(model, lr=1e-3, clip_norm=1.0, use_graph=use_graph, graph_warmup=1, **kw), d


def test_train_step_statistics_gradients_and_graph_replay(golden):
    runs = {}
    for mode in ("eager", "graph", "graph2"):
        tr, d = _engine(mode != "eager")
        sample = _sample(golden, d, torch.bfloat16)
        recs = []
        for step in range(3):
            last = tr.train_step([sample])
            recs.append([float(v) for v in (*last["stats"], last["l1_loss"], last["mse_loss"], last["eos_loss"], last["gnorm"])])
            if step == 0 and mode == "eager":
                # the first step ran on the recipe weights: its statistics and gradients are the golden's (bf16: the reference's gaps)
                n, loss_sum, ntok, l1, mse, eos, gnorm = recs[0]
                want = golden["loss_mean"]
                gap = 2 * float(golden["gap_loss_mean"][0])
                assert n == ntok == float(golden["ntokens"][0]) == 19.0
                assert rel_err(torch.tensor([loss_sum, l1, mse, eos]), torch.from_numpy(want)) <= gap
                assert abs(loss_sum - (l1 + mse + eos)) <= 1e-5 * loss_sum
                grads = {k: p.grad for k, p in tr.model.named_parameters() if p.grad is not None}
                assert _check_grads(golden, grads, torch.bfloat16) >= 30
                norms = golden["gnorm"]
                live = norms >= ZERO_NORM * norms.max()
                total = float((norms[live] ** 2).sum() ** 0.5) / 19.0          # the engine's norm is of g / sample_size
                assert abs(gnorm - total) <= 2 * float(golden["gap_gnorm"][live].max()) * total, (gnorm, total)
        torch.cuda.synchronize()
        runs[mode] = (recs, tr.fp.flat.clone())
        if mode == "graph":
            assert sum(1 for e in tr._graphs.values() if "graphs" in e) == 1
        assert {"l1_loss", "mse_loss", "eos_loss"} <= set(tr.last)
    print(runs["eager"][0])
    assert all(v == v for rec in runs["eager"][0] for v in rec)
    assert runs["eager"][0] == runs["graph"][0] and torch.equal(runs["eager"][1], runs["graph"][1])       # captured == eager, bit for bit
    assert runs["graph"][0] == runs["graph2"][0] and torch.equal(runs["graph"][1], runs["graph2"][1])     # two replayed runs are equal


def _caption_sample(d):
    from ofasys_amd import ModalityType, Slot
    vals, prev = [], None
    for mod, is_src, spec, attrs in CASES["tiny_text"]["slots"]:
        v = make_value(spec, len(d))
        vals.append(Slot(ModalityType[mod], is_src, v.to(DEV), attributes=attrs))
        if not is_src:
            prev = v
    return {"slots": vals, "target": make_target(prev).to(DEV), "task": "caption"}


def test_a_mixed_step_runs_and_a_step_without_tts_reports_what_it_did(golden):
    tr, d = _engine(False)
    cap, tts = _caption_sample(d), _sample(golden, d, torch.bfloat16)
    last = tr.train_step([cap])
    assert not {"l1_loss", "mse_loss", "eos_loss"} & set(last)
    n_cap = float(last["stats"][0])
    last = tr.train_step([cap, tts])
    torch.cuda.synchronize()
    stats = [float(v) for v in last["stats"]]
    assert stats[0] == n_cap + 19.0 and stats[2] == n_cap + 19.0 and stats[1] == stats[1] and float(last["gnorm"]) > 0
    assert float(last["l1_loss"]) > 0 and float(last["mse_loss"]) > 0 and float(last["eos_loss"]) > 0
    last = tr.train_step([dict(tts, sentence_avg=True)])
    assert float(last["stats"][0]) == 3.0 and float(last["stats"][2]) == 19.0


def test_refusals_fire_before_the_model_runs(golden):
    tr, d = _engine(False)
    tts = _sample(golden, d, torch.bfloat16)
    before = tr.fp.flat.clone()
    called = []
    h = tr.model.register_forward_pre_hook(lambda m, a: called.append(1))
    for extra, fragment in ((dict(use_guided_attention_loss=True), "use_guided_attention_loss"), (dict(ctc_weight=0.5), "ctc_weight > 0"),
                            (dict(pack=object()), "pack plan"), (dict(reward=torch.zeros(3, device=DEV)), "cannot carry reward")):
        with pytest.raises(NotImplementedError, match=fragment):
            tr.train_step([dict(tts, **extra)])
        with pytest.raises(NotImplementedError, match=fragment):
            tr.valid_step([dict(tts, **extra)])
    h.remove()
    assert not called and torch.equal(tr.fp.flat, before)


def test_validation_reports_the_weighted_terms_and_leaves_training_alone(golden):
    """valid_step on two batches (3 and 2 sentences): every value is the batches' mean weighted by sample_size (reduce_metrics), checked
    against the float64 oracle on the model's own eval-mode outputs.  And with prenet dropout 0.5 -- drawn in validation too -- a
    validation pass between two train steps changes no bit of the second."""
    tr, d = _engine(False)
    batches = [_sample(golden, d, torch.bfloat16), _sample(golden, d, torch.bfloat16, rows=2)]
    want, ss = torch.zeros(4, dtype=torch.float64), 0.0
    with tr._valid_mode(tr.model):
        for s in batches:
            post, extra = tr.model(s["slots"])[:2]
            out = torch.stack(O.tacotron2_loss(extra["feature_out"].double(), post.double(), extra["eos_out"].double(), s["target"].double(),
                                               s["target_lengths"], C.BCE_POS_WEIGHT, "mean")).cpu()
            n = float(s["target_lengths"].sum())
            want, ss = want + n * out, ss + n
    tr.valid_begin()
    for s in batches:
        tr.valid_step([s])
    res = tr.valid_result()
    got = torch.tensor([res["loss"], res["l1_loss"], res["mse_loss"], res["eos_loss"]], dtype=torch.float64)
    assert res["sample_size"] == res["ntokens"] == ss == 37.0
    assert rel_err(got, want / ss) <= 1e-5, (got, want / ss)

    case = dict(C.CASE, adaptor_overrides={"audio_fbank": dict(C.CASE["adaptor_overrides"]["audio_fbank"], prenet_dropout=0.5)})
    flats = []
    for validate in (False, True):
        tr, d = _engine(False, case)
        s = _sample(golden, d, torch.bfloat16)
        tr.train_step([s])
        if validate:
            tr.valid_begin()
            tr.valid_step([s])
            first = tr.valid_result()["loss"]
            tr.valid_begin()
            tr.valid_step([s])
            assert tr.valid_result()["loss"] == first                          # (the pass restores the position it found: it repeats)
        tr.train_step([s])
        torch.cuda.synchronize()
        flats.append(tr.fp.flat.clone())
    assert torch.equal(flats[0], flats[1])


# ------------------------------------------------------------------------------------------------------------------ Task / Trainer
def test_task_and_trainer_fit_then_validate():
    """The user surface end to end: Task(instruction "[TEXT:src] -> [AUDIO:fbank]", criterion ofa_tacotron2), Trainer().fit for a few steps
    on synthetic frames (the adaptor's defaults: prenet and postnet dropout 0.5, a 5 x 512 postnet), then Trainer.validate()."""
    import math

    from oracle import recipe
    from ofasys_amd import GeneralistModel, Task, TaskConfig, Trainer
    cfg = TaskConfig()
    cfg.criterion.name, cfg.criterion.bce_pos_weight = "ofa_tacotron2", 5.5
    task = Task(cfg, name="tts", instruction="[TEXT:src] -> [AUDIO:fbank]", micro_batch_size=2)
    lengths = [5, 8, 11, 14]
    rows = [{"src": f"sentence number {i} to be spoken", "fbank": {"fbank": recipe.floats(f"tts.fit.{i}", (n, C.F)), "fbank_lengths": n}}
            for i, n in enumerate(lengths)]
    task.add_dataset(rows, "train")
    task.add_dataset(rows[:3], "valid")
    model = GeneralistModel()
    model.cfg.arch = "tiny"
    model.__init__(model.cfg)
    trainer = Trainer(max_update=3, log_interval=1, lr=1e-4)
    history = trainer.fit(model=model, tasks=[task])
    assert len(history) == 3 and all(math.isfinite(r["loss"]) and math.isfinite(r["gnorm"]) and r["sample_size"] > 0 for r in history)
    last = trainer.step_engine.last
    assert all(float(last[k]) > 0 for k in ("l1_loss", "mse_loss", "eos_loss"))
    res = trainer.validate()["tts"]
    assert res["sample_size"] == res["ntokens"] == float(sum(lengths[:3]))
    assert all(math.isfinite(res[k]) and res[k] > 0 for k in ("loss", "l1_loss", "mse_loss", "eos_loss"))
    assert abs(res["loss"] - (res["l1_loss"] + res["mse_loss"] + res["eos_loss"])) <= 1e-5 * res["loss"]
