"""GPU: motion-diffusion training through the adaptor, the criterion route and the step engine on the tiny case of
tests/diffusion_case.py (2 + 2 layers, D = 64, 4 heads; a text source of 7 tokens; B = 3 target sentences of [9, 1, 6] frames, Dd = 18;
noise and levels supplied).  fp32 is held to the project's parity bound 1e-3 (max |a - b| / max |b|) against the float64 restatement in
tests/diffusion_oracle.py; what was measured stands in profiles/diffusion_parity_measured.txt."""
import math

import pytest
import torch

from oracle import recipe
from tests import diffusion_case as C
from tests import diffusion_oracle as O
from tests.golden_util import rel_err
from tests.model_util import build_model

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
FP32_BOUND = 1e-3


def _schedule(**kw):
    from ofasys_amd.diffusion import NoiseSchedule
    return NoiseSchedule(**dict(C.DIFFUSER_ARGS, **kw))


def _sample(d, sched, supplied=True, known_w=None, x0=None):
    from ofasys_amd import ModalityType, Slot
    x0 = (C.frames() if x0 is None else x0).to(DEV)
    value = {"value": x0, "masks": C.masks().to(DEV)}
    if known_w is not None:
        value["known_w"] = known_w.to(DEV)
    value["value_0"] = value["value"]
    slots = [Slot(ModalityType.TEXT, True, C.source_tokens(len(d)).to(DEV)),
             Slot(ModalityType.MOTION, False, value, attributes=["adaptor=motion_6d"])]
    mb = {"slots": slots, "diffusion": sched, "task": "t2m"}
    if supplied:
        mb["noise"], mb["noise_level"] = C.noise().to(DEV), C.levels().to(DEV)
    return mb


def _known_w():
    kw = torch.zeros(C.B, C.T)
    kw[:, 0] = 1.0
    kw[0, 5] = kw[0, 8] = 1.0
    return kw


# ------------------------------------------------------------------------------------------------------------------ the adaptor
@pytest.mark.parametrize("inbetween", (False, True), ids=("plain", "known_w"))
def test_adaptor_forward_and_gradients_against_the_float64_oracle(inbetween):
    from ofasys_amd import ModalityType, Slot, ops
    model, d = build_model(C.CASE, DEV, torch.float32)
    model.train()
    ad = model.decoder.adaptor.name2adaptor["motion_6d"]
    sched = _schedule()
    tab = sched.on(DEV)
    x0, noise, t, masks = C.frames(), C.noise(), C.levels(), C.masks()
    known_w = _known_w() if inbetween else None
    value = ops.diffusion_q_sample(x0.to(DEV), noise.to(DEV), t.to(DEV), sched, ad.max_data_dim, torch.float32,
                                   known_w=known_w.to(DEV) if inbetween else None, masks=masks.to(DEV))
    v = {"value": value, "masks": masks.to(DEV), "noise_level": t.to(DEV), "data_dim": C.DD}
    if inbetween:
        v["known_w"] = known_w.to(DEV)
    slot = Slot(ModalityType.MOTION, False, v, attributes=["adaptor=motion_6d"])
    out = ad.forward(slot)                                                  # (the adaptor's own forward: the shared post-hook is the text adaptor's)
    hidden = recipe.floats("input.diffusion.hidden", (C.B, C.T, 64))
    pred, extra = ad.forward_output(hidden.to(DEV), {}, slot)
    g1, g2 = recipe.floats("input.diffusion.g1", (C.B, C.T, 64)), recipe.floats("input.diffusion.g2", (C.B, C.T, C.DD))
    ((out.embed * g1.to(DEV)).sum() + (pred[..., :C.DD] * g2.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    # the oracle, float64, on the same fp32 tables
    params = {k: getattr_path(ad, k).detach().cpu().double().requires_grad_(True) for k in C.ADAPTOR_KEYS}
    value64 = O.adaptor_input(x0, noise, t, tab.sqrt_acp.cpu(), tab.sqrt_1m_acp.cpu(), ad.max_data_dim, known_w, masks)
    embed64 = O.adaptor_forward(params, value64, t, known_w)
    pred64 = O.adaptor_forward_output(params, hidden.double(), C.DD)
    ((embed64 * g1.double()).sum() + (pred64 * g2.double()).sum()).backward()
    figs = {"value": rel_err(value.cpu(), value64), "embed": rel_err(out.embed.detach().cpu(), embed64.detach()),
            "pred": rel_err(pred[..., :C.DD].detach().cpu(), pred64.detach())}
    assert extra["data_dim"] == C.DD and pred.shape == (C.B, C.T, ad.max_data_dim) and out.masks is v["masks"]
    assert out.pos_embed.shape == out.embed.shape == (C.B, C.T, 64)
    for k in C.ADAPTOR_KEYS:
        figs["grad " + k] = rel_err(getattr_path(ad, k).grad.cpu(), params[k].grad)
    print("diffusion parity", "known_w" if inbetween else "plain", {k: f"{e:.3e}" for k, e in figs.items()})
    assert all(e < FP32_BOUND for e in figs.values()), figs
    # the table's gradient is sparse: the three drawn levels (ids t + 1) and, in-betweening, level 0
    touched = getattr_path(ad, "noise_level_emb.weight").grad.abs().sum(1).gt(0).nonzero().view(-1).tolist()
    assert touched == sorted(([0] if inbetween else []) + [lv + 1 for lv in C.LEVELS])


def getattr_path(module, path):
    obj = module
    for part in path.split("."):
        obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
    return obj


# ------------------------------------------------------------------------------------------------------------------ the route
def _engine(use_graph, dtype=torch.bfloat16, lr=1e-3):
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    model, d = build_model(C.CASE, DEV, dtype)
    ops.manual_seed(1234)
    return TrainStep(model, lr=lr, clip_norm=1.0, use_graph=use_graph, graph_warmup=1), d


@pytest.mark.parametrize("prediction_type", ("sample", "epsilon"))
def test_step_loss_is_the_float64_criterion_on_the_models_own_output(prediction_type):
    from ofasys_amd import criterion
    tr, d = _engine(False, torch.float32)
    sched = _schedule(prediction_type=prediction_type)
    mb = dict(_sample(d, sched), scale_main_loss=0.5, criterion_weight=2.0, scale_aux_loss_1=0.0)
    assert criterion.route(mb, tr.criterion) == "diffusion"
    tr.model.train()
    with torch.no_grad():
        x = criterion.forward(tr.model, mb, "diffusion", tr.criterion)
    assert x.logits.shape == (C.B, C.T, 32) and torch.equal(x.extra["noise_level"], mb["noise_level"])
    assert "noise_level" not in mb["slots"][1].value and mb["slots"][1].value["value"].shape == (C.B, C.T, C.DD)      # a copy was noised
    want = float(O.criterion(x.logits.double().cpu()[..., :C.DD], C.frames(), C.noise(), C.levels(), sched.on(DEV).w.cpu().double(),
                             prediction_type, C.masks(), 1.0))
    last = tr.train_step([mb])
    torch.cuda.synchronize()
    got, stats = float(last["main_loss"]), [float(v) for v in last["stats"]]
    print("diffusion step", prediction_type, "loss", got, "oracle", want, "rel", abs(got - want) / want)
    assert abs(got - want) <= FP32_BOUND * want and stats[1] == got
    assert stats[0] == 1.0 and stats[2] == float(sum(C.LENGTHS))            # sample_size 1, ntokens = the unmasked frames
    assert float(last["gnorm"]) > 0 and math.isfinite(float(last["gnorm"]))
    grads = {k: p.grad for k, p in tr.model.named_parameters() if k.startswith(C.PREFIX) and k[len(C.PREFIX):] in C.ADAPTOR_KEYS}
    assert len(grads) == len(C.ADAPTOR_KEYS) and all(bool(g.abs().gt(0).any()) for g in grads.values())


def test_the_route_runs_the_decoder_without_a_causal_mask():
    """Changing the LAST target frame of sentence 0 changes the decoder's output at position 0 (a causal decoder could not see it)."""
    from ofasys_amd import criterion
    tr, d = _engine(False, torch.float32)
    sched = _schedule()
    outs = []
    x0 = C.frames()
    for delta in (0.0, 1.0):
        frames = x0.clone()
        frames[0, C.LENGTHS[0] - 1] += delta
        tr.model.eval()
        with torch.no_grad():
            outs.append(criterion.forward(tr.model, _sample(d, sched, x0=frames), "diffusion", tr.criterion).logits.clone())
    assert not torch.equal(outs[0][0, 0], outs[1][0, 0])
    assert torch.equal(outs[0][1:], outs[1][1:])                                # the other sentences saw nothing of it


def test_refusals_fire_before_the_model_runs():
    tr, d = _engine(False)
    mb = _sample(d, _schedule())
    before = tr.fp.flat.clone()
    called = []
    h = tr.model.register_forward_pre_hook(lambda m, a: called.append(1))
    for extra, kind, fragment in ((dict(pack=object()), NotImplementedError, "pack plan"),
                                  (dict(reward=torch.zeros(3, device=DEV)), NotImplementedError, "cannot carry reward"),
                                  (dict(target_lengths=torch.ones(3, device=DEV)), NotImplementedError, "cannot carry target_lengths"),
                                  (dict(scale_aux_loss_2=1.0), NotImplementedError, "scale_aux_loss_2 > 0")):
        with pytest.raises(kind, match=fragment):
            tr.train_step([dict(mb, **extra)])
        with pytest.raises(kind, match=fragment):
            tr.valid_step([dict(mb, **extra)])
    h.remove()
    assert not called and torch.equal(tr.fp.flat, before)
    small = _schedule(num_train_timesteps=64)                                   # 65 levels needed, the case's table has 64 rows
    with pytest.raises(ValueError, match="max_noise_levels 64 < num_train_timesteps \\+ 1 = 65"):
        tr.train_step([dict(_sample(d, small), noise_level=torch.zeros(3, dtype=torch.long, device=DEV))])
    assert torch.equal(tr.fp.flat, before)


# ------------------------------------------------------------------------------------------------------------------ the step engine
def test_eager_and_captured_steps_give_equal_bits():
    runs = {}
    for mode in ("eager", "graph", "graph2"):
        tr, d = _engine(mode != "eager")
        mb = _sample(d, _schedule(), known_w=_known_w())
        recs = []
        for _ in range(3):
            last = tr.train_step([mb])
            recs.append([float(v) for v in (*last["stats"], last["main_loss"], last["gnorm"])])
        torch.cuda.synchronize()
        runs[mode] = (recs, tr.fp.flat.clone())
        if mode != "eager":
            assert tr.captured_graphs() == 1
    print(runs["eager"][0])
    assert all(math.isfinite(v) for rec in runs["eager"][0] for v in rec)
    assert runs["eager"][0][0][3] != runs["eager"][0][1][3]                     # (the weights moved: the same draw gives another loss)
    assert runs["eager"][0] == runs["graph"][0] and torch.equal(runs["eager"][1], runs["graph"][1])
    assert runs["graph"][0] == runs["graph2"][0] and torch.equal(runs["graph"][1], runs["graph2"][1])


def test_a_replayed_step_draws_new_noise_and_the_seed_brings_it_back():
    """lr = 0 and no dropout: the weights never move, so the loss of a step depends on its draw alone.  The draws are torch's, from the
    device generator, inside the captured graph: two replays differ, and re-seeding the generator repeats the first."""
    tr, d = _engine(True, lr=0.0)
    mb = _sample(d, _schedule(), supplied=False)
    before = tr.fp.flat.clone()
    torch.manual_seed(7)
    for _ in range(2):                                                          # an eager visit, then the capture and its first replay
        tr.train_step([mb])
    assert tr.captured_graphs() == 1
    losses = []
    for seed in (11, None, 11):
        if seed is not None:
            torch.manual_seed(seed)
        losses.append(float(tr.train_step([mb])["main_loss"]))
    torch.cuda.synchronize()
    print("replayed draws", losses)
    assert torch.equal(tr.fp.flat, before)
    assert all(math.isfinite(v) and v > 0 for v in losses)
    assert losses[0] != losses[1] and losses[0] == losses[2]


def test_valid_step_returns_the_training_loss_of_the_same_draw_and_changes_no_weight():
    tr, d = _engine(False)
    mb = _sample(d, _schedule())
    before = tr.fp.flat.clone()
    tr.valid_begin()
    tr.valid_step([mb])
    res = tr.valid_result()
    assert torch.equal(tr.fp.flat, before)
    train = float(tr.train_step([mb])["main_loss"])                             # (its loss is of the weights before the update)
    torch.cuda.synchronize()
    print("valid", res["main_loss"], "train", train)
    assert abs(res["main_loss"] - train) <= 1e-5 * train and res["loss"] == res["main_loss"]
    assert res["sample_size"] == 1.0 and res["ntokens"] == float(sum(C.LENGTHS))
    assert not torch.equal(tr.fp.flat, before)
    tr.valid_begin()
    tr.valid_step([mb])
    tr.valid_step([mb])
    two = tr.valid_result()
    assert two["sample_size"] == 2.0 and math.isfinite(two["main_loss"]) and two["main_loss"] != res["main_loss"]


# ------------------------------------------------------------------------------------------------------------------ Task / Trainer
def test_task_and_trainer_fit_two_updates():
    """The user surface end to end: Task([TEXT] -> [MOTION:...,adaptor=motion_6d], diffusion_criterion, diffuser_args) and
    Trainer().fit for two updates on three hand-made samples; every step draws its own noise, so the two losses differ."""
    from ofasys_amd import GeneralistModel, Task, TaskConfig, Trainer
    cfg = TaskConfig()
    cfg.criterion.name = "diffusion_criterion"
    cfg.diffuser_args = '{"scheduler": "DDPMScheduler", "num_train_timesteps": 100}'
    cfg.dataset.shuffle = False
    task = Task(cfg, name="t2m", instruction="[TEXT:text] -> [MOTION:motion,preprocess=motion_6d,adaptor=motion_6d,min_length=1]",
                micro_batch_size=3)
    rows = [{"text": f"a person does motion number {i}", "motion": recipe.floats(f"diffusion.fit.{i}", (n, C.DD)).numpy()}
            for i, n in enumerate((4, 1, 6))]
    task.add_dataset(rows, "train")
    model = GeneralistModel()
    model.cfg.arch = "tiny"
    model.__init__(model.cfg)
    trainer = Trainer(max_update=2, log_interval=1, lr=1e-4)
    history = trainer.fit(model=model, tasks=[task])
    assert len(history) == 2 and all(math.isfinite(r["loss"]) and math.isfinite(r["gnorm"]) and r["sample_size"] == 1 for r in history)
    last = trainer.step_engine.last
    main = float(last["main_loss"])
    assert math.isfinite(main) and main > 0
    assert abs(history[1]["loss"] * math.log(2.0) - main) <= 1e-6 * main        # (the log line is base 2 per sample_size)
    assert history[0]["loss"] != history[1]["loss"]
    assert model.cfg.adaptor.motion_6d.is_active and float(last["stats"][2]) == 11.0
