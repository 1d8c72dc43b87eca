"""GPU: validation end to end -- TrainStep.valid_begin / valid_step / valid_result on the tiny text model of tests/model_util.py
(plain, packed, mask-form and node-form batches; eager and captured), against tests/criterion_eval_oracle.py applied to the very
logits the model produced; that a validation pass between train steps changes NOTHING of the training (bit for bit: parameters, Adam
moments, the statistics of every step -- eager, captured, and with dropout, where a moved Philox counter would show); validation with
the EMA weights; and Trainer.fit(validate_interval_updates=...) on the Task API."""
import numpy as np
import pytest
import torch

from tests import closed_set_train_case as cs
from tests import criterion_eval_oracle as eo
from tests.traverse_case import ANSWERS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
EPS = 0.1
SRC_LEN = [23, 9, 17, 12]
FORMS = (("plain", False), ("plain", True), ("masks", False), ("nodes", False), ("nodes", True))


def _case(dropout=0.0):
    return {"arch": "tiny", "active": {"text"}, "overrides": {"use_self_attn_bias": False, "entangle_position_embedding": True,
                                                              "dropout": dropout},
            "adaptor_overrides": {"text": {"entangle_position_embedding": True}}}


@pytest.fixture(scope="module")
def plan():
    from ofasys_amd.traverse import TraversePlan
    return TraversePlan(ANSWERS, 0, 2, 1)


@pytest.fixture(scope="module")
def trie(plan):
    return {"node_edge_off": torch.from_numpy(plan.node_edge_off).to(DEV), "edge_token": torch.from_numpy(plan.edge_token).to(DEV),
            "N": plan.N, "E": plan.E}


def _sample(which, plan, trie, form, V, pack=False):
    from oracle import recipe
    from ofasys_amd.packing import build_pack_plan
    from tests.model_util import make_slots
    b = cs.step_batch(which, plan, V)
    src = recipe.tokens(f"validation.src{which}", (4, 23), V, SRC_LEN)
    s = {"slots": make_slots([("TEXT", True, src, None), ("TEXT", False, b["prev"], None)], DEV, torch.bfloat16),
         "target": b["target"].to(DEV)}
    if form == "masks":
        s["constraint_masks"] = b["masks"].to(DEV)
    if form == "nodes":
        s["constraint_nodes"] = b["nodes"].to(DEV)
        s["constraint_trie"] = trie
    if pack:
        s["pack"] = build_pack_plan(src.eq(1), b["prev"].eq(1), bucket=64).to(DEV)
    return s


def _engine(dropout=0.0, **kw):
    from ofasys_amd import ops
    from ofasys_amd.trainer import TrainStep
    from tests.model_util import build_model
    model, d = build_model(_case(dropout), DEV, torch.bfloat16)
    ops.manual_seed(1234)
    return TrainStep(model, lr=kw.pop("lr", 1e-3), clip_norm=1.0, label_smoothing=EPS, **kw), len(d)


def _oracle(tr, model, samples):
    """The float64 oracle on the logits `model` gives these micro-batches in eval mode -> (sums over the batches, live rows); asserts
    the precondition: two eval-mode forwards (as validation runs the model: TrainStep._valid_mode) give bit-identical logits."""
    sums, live = [0.0] * 4, 0
    with tr._valid_mode(model):
        for s in samples:
            logits, target, cm, nodes, _ = tr._criterion_inputs(model, s)
            again = tr._criterion_inputs(model, s)[0]
            assert torch.equal(logits, again), "eval-mode forwards differ: the comparison below would not be one"
            V = logits.shape[-1]
            x, t = logits.reshape(-1, V), target.reshape(-1)
            A = eo.allowed_set(x.shape[0], V, None, None if cm is None else cm.reshape(-1, V).cpu(),
                               None if nodes is None else nodes.reshape(-1), s.get("constraint_trie"))
            ref = eo.eval_reference(x, t, A, EPS, cm is not None or nodes is not None, ignore=tr.pad)
            sums = [a + b for a, b in zip(sums, ref["sums"])]
            live += int((t != tr.pad).sum())
    return sums, live


def _agrees(res, sums, live):
    ln2 = 0.6931471805599453
    assert res["ntokens"] == sums[0] == res["total"] == res["sample_size"] and res["n_correct"] == sums[3], (res, sums)
    assert abs(res["loss"] * ln2 * sums[0] - sums[1]) <= live * eo.EVAL_TOL, (res, sums)
    assert abs(res["nll_loss"] * ln2 * sums[0] - sums[2]) <= live * eo.EVAL_TOL, (res, sums)
    assert res["ppl"] == pytest.approx(2.0 ** res["nll_loss"]) and res["accuracy"] == pytest.approx(100.0 * sums[3] / sums[0])


@pytest.mark.parametrize("form,pack", FORMS, ids=[f"{f}{'-packed' if p else ''}" for f, p in FORMS])
def test_valid_step_matches_the_oracle_eager_and_captured(plan, trie, form, pack):
    """Two batches of one structure: eager; then captured (graph_warmup = 0: the first visit records) with the second batch REPLAYED
    into the static inputs.  Counts exactly, loss / nll within the sum tolerance; eager and captured agree bit for bit."""
    accs = {}
    for mode in ("eager", "graph"):
        tr, V = _engine(use_graph=mode == "graph", graph_warmup=0)
        samples = [_sample(w, plan, trie, form, V, pack) for w in (0, 1)]
        sums, live = _oracle(tr, tr.model, samples)
        assert sums[0] == 30 and np.isfinite(sums[1])              # 2 x (11 answer tokens + 4 EOS)
        tr.valid_begin()
        for s in samples:
            tr.valid_step([s])
        res = tr.valid_result()
        _agrees(res, sums, live)
        assert tr.captured_valid_graphs() == (1 if mode == "graph" else 0) and tr.captured_graphs() == 0
        assert tr.model.training                                   # (put back as it was found)
        accs[mode] = tr._valid_acc.clone()
        # a second pass starts from zero and gives the same bits (fresh batches: a captured batch's tensors ARE the graph's static
        # inputs from then on, as in train_step, and the replay of another batch overwrites them)
        tr.valid_begin()
        for w in (0, 1):
            tr.valid_step([_sample(w, plan, trie, form, V, pack)])
        torch.cuda.synchronize()
        assert torch.equal(tr._valid_acc, accs[mode])
    print(f"\n{form} pack={pack}: {res}")
    assert torch.equal(accs["eager"], accs["graph"])


def test_valid_step_refusals(plan, trie):
    tr, V = _engine()
    s = _sample(0, plan, trie, "plain", V)
    s["reward"] = torch.ones(4, device=DEV)
    with pytest.raises(NotImplementedError, match="SCST"):
        tr.valid_step([s])
    with pytest.raises(RuntimeError, match="EMA"):
        tr.valid_step([_sample(0, plan, trie, "plain", V)], use_ema=True)
    with pytest.raises(NotImplementedError, match="pack plan"):
        tr.valid_step([_sample(0, plan, trie, "masks", V, pack=True)])
    s = _sample(0, plan, trie, "nodes", V)
    del s["constraint_trie"]
    with pytest.raises(ValueError, match="constraint_trie"):
        tr.valid_step([s])


def _state(tr):
    return [t.clone() for t in (tr.fp.flat, tr.master, tr.exp_avg, tr.exp_avg_sq, tr._step_t, tr._sched, tr._gsq)]


@pytest.mark.parametrize("use_graph,dropout", [(False, 0.0), (True, 0.0), (False, 0.1), (True, 0.1)],
                         ids=["eager", "graph", "eager-dropout", "graph-dropout"])
def test_validation_does_not_disturb_training(plan, trie, use_graph, dropout):
    """Four train steps; separately two train steps, a validation pass of two batches, two more train steps: parameters, master
    weights, Adam moments, the device counters and the returned statistics of every step are bit-identical."""
    from ofasys_amd import ops
    runs = {}
    for validated in (False, True):
        tr, V = _engine(dropout, use_graph=use_graph, graph_warmup=1)
        train = [_sample(w % 2, plan, trie, "nodes", V, True) for w in range(4)]
        valid = [_sample(w, plan, trie, "nodes", V, True) for w in (1, 0)]
        stats = []
        for i, s in enumerate(train):
            if validated and i == 2:
                tr.valid_begin()
                for v in valid:
                    tr.valid_step([v])
                res = tr.valid_result()
                assert res["ntokens"] == 30 and np.isfinite(res["loss"])
            out = tr.train_step([s])
            stats.append((out["stats"].clone(), out["gnorm"].clone()))
        torch.cuda.synchronize()
        runs[validated] = (_state(tr), stats, ops._Rng.offset, [b.clone() for b in ops._Rng.base.values()])
        if use_graph:
            assert tr.captured_graphs() == 1
    a, b = runs[False], runs[True]
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    for (s1, g1), (s2, g2) in zip(a[1], b[1]):
        assert torch.equal(s1, s2) and torch.equal(g1, g2)
    assert a[2] == b[2] and all(torch.equal(x, y) for x, y in zip(a[3], b[3]))          # the Philox position, host and device
    if dropout > 0:
        assert any(int(x) != 0 for x in a[3]) or a[2] != 0         # (dropout is on: the steps did draw)


def test_validation_with_the_ema_weights(plan, trie):
    tr, V = _engine(lr=1e-2, ema={"store_ema": True, "ema_decay": 0.5})
    for w in range(3):
        tr.train_step([_sample(w % 2, plan, trie, "plain", V)])
    samples = [_sample(w, plan, trie, "plain", V) for w in (0, 1)]
    results = {}
    for use_ema in (False, True):
        model = tr.ema.get_model() if use_ema else tr.model
        sums, live = _oracle(tr, model, samples)
        tr.valid_begin()
        for s in samples:
            tr.valid_step([s], use_ema=use_ema)
        results[use_ema] = tr.valid_result()
        _agrees(results[use_ema], sums, live)
    print("\nlive", results[False], "\nema ", results[True])
    assert results[True]["loss"] != results[False]["loss"]


def test_fit_validates_every_n_updates_and_trains_the_same():
    """Trainer.fit on the Task API's toy data: validate_interval_updates=2, max_update=4 -> valid_history at updates 2 and 4, finite
    losses, accuracy present (report_accuracy), and `history` identical to the same run without validation."""
    from ofasys_amd import GeneralistModel, Task, Trainer
    rows = [{"src": f"the {i}th book was written by a very careful author .", "tgt": f"book number {i}"} for i in range(12)]
    out = {}
    for interval in (0, 2):
        task = Task(name="echo", instruction="what is the title ? [TEXT:src] -> [TEXT:tgt]", micro_batch_size=4)
        task.cfg.criterion.report_accuracy = True
        task.add_dataset(rows, "train")
        task.add_valid_dataset(rows[:6])                           # 4 + a short batch of 2
        model = GeneralistModel()
        model.cfg.arch = "tiny"
        model.__init__(model.cfg)
        trainer = Trainer(max_update=4, log_interval=1, lr=1e-3, validate_interval_updates=interval)
        out[interval] = (trainer.fit(model=model, tasks=[task]), trainer)
    history, trainer = out[2]
    assert history == out[0][0] and len(history) == 4
    assert out[0][1].valid_history == []
    vh = trainer.valid_history
    assert [h["update"] for h in vh] == [2, 4]
    for h in vh:
        r = h["echo"]
        assert np.isfinite(r["loss"]) and np.isfinite(r["nll_loss"]) and r["ntokens"] > 0 and 0.0 <= r["accuracy"] <= 100.0
        assert r["total"] == r["ntokens"] and 0 <= r["n_correct"] <= r["total"]
    assert vh[0]["echo"]["ntokens"] == vh[1]["echo"]["ntokens"]
    # a task that does not ask for accuracy does not get it
    task.cfg.criterion.report_accuracy = False
    assert "accuracy" not in trainer.validate()["echo"] and len(trainer.valid_history) == 3
