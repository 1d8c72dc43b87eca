"""GPU: self-critical sequence training through the op, the step engine and the trainer, on the tiny text model with B = 2 sentences
and K = 3 hypotheses: ops.scst_loss against plain autograd; its seeded backward; TrainStep on an SCST micro-batch eager, captured and
replayed, padded and packed; generation after an update reading the updated weights; and Trainer.fit on a task with scst=True."""
import numpy as np
import pytest
import torch

from oracle.cases import CASES
from tests.golden_util import case_inputs, rel_err
from tests.model_util import build_model, make_slots
from tests.sampling_case import boost_eos

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
CASE = CASES["tiny_text"]
K = 3
HYPS = [[14, 15, 16, 17, 2], [14, 15, 33, 2], [40, 41, 2], [50, 51, 52, 53, 2], [50, 51, 60, 61, 2], [70, 2]]
REWARD = [1.25, -0.5, -0.75, 0.0, 2.0, -2.0]


def _batch(d, dtype, pad_to=1, hyps=HYPS, reward=REWARD):
    """The SCST micro-batch of the case's two source sentences with fixed hypotheses (what ScstRewardCriterion builds)."""
    from ofasys_amd.scst import hypothesis_batch, repeat_sources
    vals, _ = case_inputs(CASE)
    slots = make_slots(vals, DEV, dtype)
    prev, target = hypothesis_batch([torch.tensor(h) for h in hyps], d.pad(), d.bos(), pad_to)
    return {"slots": repeat_sources(slots, K, prev.to(DEV)), "target": target.to(DEV),
            "reward": torch.tensor(reward, dtype=torch.float32, device=DEV), "task": "caption"}


@pytest.mark.parametrize("crange", [None, (10, 150)], ids=["whole-vocabulary", "range"])
def test_scst_loss_matches_autograd(crange):
    """Value and parameter gradients of ops.scst_loss against autograd through the log-probabilities, the gather of the generated
    tokens and the reward (scst_loss.py:24-36): get_normalized_probs without a range; with one, the reference's -inf fill followed by
    torch's log-softmax.  fp32: within the project's 1e-3 relative bar."""
    from ofasys_amd import ops
    res = {}
    for mode in ("kernel", "autograd"):
        model, d = build_model(CASE, DEV, torch.float32)
        model.eval()
        mb = _batch(d, torch.float32)
        out = model(mb["slots"])
        pad = d.pad()
        if mode == "kernel":
            loss, ntok = ops.scst_loss(out[0], mb["target"], mb["reward"], pad, crange)
            assert int(ntok) == sum(len(h) for h in HYPS)
        else:
            if crange is None:
                lprobs = model.get_normalized_probs(out, log_probs=True)
            else:
                V = out[0].shape[-1]
                c = torch.arange(V, device=DEV)
                lprobs = torch.log_softmax(out[0].float().masked_fill(~((c < 4) | ((c >= crange[0]) & (c < crange[1]))), float("-inf")), -1)
            nll = -lprobs.gather(-1, mb["target"].unsqueeze(-1)).squeeze(-1) * mb["reward"].unsqueeze(-1)
            loss = nll.masked_fill(mb["target"].eq(pad), 0.0).sum()
        loss.backward()
        torch.cuda.synchronize()
        res[mode] = (float(loss.detach()), {k: p.grad.detach().float().cpu() for k, p in model.named_parameters() if p.grad is not None})
    (lk, gk), (la, ga) = res["kernel"], res["autograd"]
    assert abs(lk - la) <= 1e-3 * abs(la), (lk, la)
    assert set(gk) == set(ga) and len(ga) > 20
    scale = max(float(g.double().norm()) for g in ga.values())
    for k in ga:
        # (per element, with the floor tests/test_model_gpu.py gives its fp32 gradients: k_proj-like biases have mathematically zero
        #  gradient, so their 1e-9 of rounding noise is held against the global gradient scale)
        assert float((gk[k] - ga[k]).abs().max()) <= 1e-3 * float(ga[k].abs().max()) + 1e-7 * scale, (k, rel_err(gk[k], ga[k]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_seeded_backward(dtype):
    """The gradient precomputed at the seed's scale is what the backward seeded with that very tensor returns; another tensor of the
    same value, a second backward (retain_graph), and a seed written to since the forward all recompute -- to the same numbers, or to
    the new scale."""
    from ofasys_amd import ops
    g = torch.Generator().manual_seed(3)
    V = 204
    logits = (torch.randn(6, 8, V, generator=g) * 2).to(dtype).to(DEV).requires_grad_(True)
    target = torch.randint(4, V, (6, 8), generator=g)
    target[:, 6:] = 1
    target = target.to(DEV)
    reward = torch.tensor(REWARD, dtype=torch.float32, device=DEV)
    plain, _ = ops.scst_loss(logits, target, reward, 1)
    want, = torch.autograd.grad(plain, logits, torch.ones((), device=DEV))
    seed = torch.ones((), dtype=torch.float32, device=DEV)
    loss, ntok = ops.scst_loss(logits, target, reward, 1, seed=seed)
    assert float(loss) == float(plain) and int(ntok) == 36 and not ntok.requires_grad
    first, = torch.autograd.grad(loss, logits, seed, retain_graph=True)
    assert torch.equal(first, want) and float(first.float().abs().max()) > 0
    kept = first.clone()
    other, = torch.autograd.grad(loss, logits, torch.ones((), device=DEV), retain_graph=True)        # another tensor: recomputed
    assert torch.equal(other, want) and other.data_ptr() != first.data_ptr()
    again, = torch.autograd.grad(loss, logits, seed, retain_graph=True)                              # a second time: recomputed
    assert torch.equal(again, want) and again.data_ptr() != first.data_ptr() and torch.equal(first, kept)
    scaled, = torch.autograd.grad(loss, logits, torch.full((), 4.0, device=DEV), retain_graph=True)
    assert torch.equal(scaled.float(), want.float() * 4)
    # a seed changed in place between forward and backward: the stale gradient is not handed out
    seed2 = torch.ones((), dtype=torch.float32, device=DEV)
    loss2, _ = ops.scst_loss(logits, target, reward, 1, seed=seed2)
    seed2.mul_(2.0)
    changed, = torch.autograd.grad(loss2, logits, seed2)
    assert torch.equal(changed.float(), want.float() * 2)
    # rows and sentences that do not divide, and a map of the wrong length
    with pytest.raises(ValueError, match="sentences"):
        ops.scst_loss(logits, target, reward[:5], 1)
    with pytest.raises(ValueError, match="row_seq"):
        ops.scst_loss(logits, target, reward, 1, row_seq=torch.zeros(7, dtype=torch.int32, device=DEV))


def _steps(use_graph, pack=False, steps=4, dropout=None):
    from ofasys_amd import ops
    from ofasys_amd.packing import build_pack_plan
    from ofasys_amd.trainer import TrainStep
    case = CASE if dropout is None else dict(CASE, overrides=dict(CASE["overrides"], dropout=dropout))
    model, d = build_model(case, DEV, torch.bfloat16)
    tr = TrainStep(model, lr=1e-3, clip_norm=1.0, use_graph=use_graph, graph_warmup=1)
    ops.manual_seed(123)
    losses = []
    for step in range(steps):
        # a new reward and new targets of the same structure every step
        hyps = [[(t + 7 * step) % 190 + 4 for t in h[:-1]] + [2] for h in HYPS]
        reward = [r * (1 + 0.25 * step) for r in REWARD]
        mb = _batch(d, torch.bfloat16, pad_to=8, hyps=hyps, reward=reward)
        if pack:
            src = torch.cat([s.value for s in mb["slots"] if s.is_src], 1).cpu()
            prev = [s.value for s in mb["slots"] if not s.is_src][0].cpu()
            mb["pack"] = build_pack_plan(src.eq(d.pad()), prev.eq(d.pad()), bucket=64).to(DEV)
        out = tr.train_step([mb])
        losses.append(float(out["stats"][1]))
        assert float(out["stats"][0]) == float(out["stats"][2]) == sum(len(h) for h in hyps)
    torch.cuda.synchronize()
    return losses, tr.master.clone(), tr


def test_train_step_eager_captured_and_replayed_agree():
    """An SCST micro-batch through TrainStep: the eager steps and the captured step replayed with a new reward and new targets of the
    same structure walk the same trajectory, bit for bit (as the cross-entropy step does)."""
    l0, m0, _ = _steps(False)
    l1, m1, tr = _steps(True)
    assert tr.use_graph and sum(1 for e in tr._graphs.values() if "graphs" in e) == 1
    assert all(np.isfinite(l0)) and len(set(l0)) == len(l0)
    assert l0 == l1 and torch.equal(m0, m1)


def test_packed_and_padded_steps_give_the_same_loss():
    """With a pack plan the sentence of a packed decoder row comes from dec_index // Tt (row_seq); the loss equals the padded step's
    within bf16 rounding (dropout 0), eager and captured alike."""
    lp, _, _ = _steps(False, dropout=0.0)
    lk, _, _ = _steps(False, pack=True, dropout=0.0)
    lg, _, tr = _steps(True, pack=True, dropout=0.0)
    assert lk == lg and sum(1 for e in tr._graphs.values() if "graphs" in e) == 1
    for a, b in zip(lp, lk):
        assert abs(a - b) <= 2e-2 * abs(a), (lp, lk)


def test_reward_with_constraint_masks_is_refused():
    from ofasys_amd.trainer import TrainStep
    model, d = build_model(CASE, DEV, torch.bfloat16)
    tr = TrainStep(model, lr=1e-3)
    mb = _batch(d, torch.bfloat16)
    mb["constraint_masks"] = torch.ones(*mb["target"].shape, len(d), dtype=torch.bool, device=DEV)
    with pytest.raises(NotImplementedError, match="constraint_masks"):
        tr.train_step([mb], eager=True)


def _task(d, scst_args):
    from ofasys_amd import Task, TaskConfig
    cfg = TaskConfig()
    cfg.scst, cfg.scst_args = True, scst_args
    task = Task(cfg, name="caption", instruction="[TEXT:src] what does it describe? -> [TEXT:caption]")
    task.initialize(d)
    return task


def test_generation_after_a_step_reads_the_updated_weights():
    """Stale-state guard: generate, train one SCST step, generate again with the SAME generator (captured step graphs, re-packed decode
    projections): the second generation equals a freshly built generator's on the updated weights."""
    from ofasys_amd.scst import ScstRewardCriterion
    from ofasys_amd.trainer import TrainStep
    model, d = build_model(CASE, DEV, torch.float32)
    with torch.no_grad():
        boost_eos(model.state_dict()["decoder.adaptor.embed_tokens.weight"], d.eos())
    args = '{"beam": 3, "max_len": 6, "min_len": 2}'
    task = _task(d, args)
    crit = ScstRewardCriterion(task, task.cfg.criterion)
    vals, target = case_inputs(CASE)
    sample = {"net_input": {"slots": make_slots(vals, DEV)}, "target": target.to(DEV)}
    tr = TrainStep(model, lr=5e-2, clip_norm=1.0, use_graph=False)
    mb, log = crit(model, sample)
    assert mb["reward"].shape == (2 * K,) and mb["target"].shape[0] == 2 * K and np.isfinite(log["score"])
    mb["reward"] = torch.tensor(REWARD, dtype=torch.float32, device=DEV)      # (whatever the scores were: an update that moves the weights)
    before = [h.tokens.tolist() for hyps in task.scst_generator.generate(model, sample) for h in hyps]
    tr.train_step([mb])
    model.eval()
    after = [h.tokens.tolist() for hyps in task.scst_generator.generate(model, sample) for h in hyps]
    fresh = [h.tokens.tolist() for hyps in _task(d, args).scst_generator.generate(model, sample) for h in hyps]
    assert after == fresh
    assert len(after) == 2 * K and before != after                 # (lr 5e-2: the update really moves the hypotheses)


@pytest.mark.parametrize("scst_args", ['{"beam": 3, "max_len": 6, "min_len": 1}',
                                       '{"sampling": true, "sampling_topk": 20, "beam": 3, "max_len": 6, "seed": 5}'],
                         ids=["beam", "sampling"])
def test_trainer_fit_with_scst(scst_args, monkeypatch):
    from ofasys_amd import GeneralistModel, Task, TaskConfig, Trainer
    from ofasys_amd.scst import ScstRewardCriterion
    cfg = TaskConfig()
    cfg.scst, cfg.scst_args = True, scst_args
    task = Task(cfg, name="caption", instruction="[TEXT:src] what does it describe? -> [TEXT:caption]", micro_batch_size=2)
    task.add_dataset([{"src": f"picture number {i} of a small animal", "caption": f"a small animal number {i} sits"} for i in range(8)], "train")
    seen = []
    call = ScstRewardCriterion.__call__

    def recording(self, model, sample):
        mb, log = call(self, model, sample)
        assert mb["reward"].numel() == 2 * K == mb["target"].shape[0]
        seen.append((log["ntokens"], int(mb["target"].ne(self.task.global_dict.pad()).sum()), log["score"] / log["nsentences"]))
        return mb, log
    monkeypatch.setattr(ScstRewardCriterion, "__call__", recording)
    model = GeneralistModel()
    model.cfg.arch = "tiny"
    model.__init__(model.cfg)
    trainer = Trainer(max_update=3, log_interval=1, lr=1e-4)
    history = trainer.fit(model=model, tasks=[task])
    assert len(history) == 3 and len(seen) == 3
    for rec, (ntokens, nonpad, score) in zip(history, seen):
        assert np.isfinite(rec["loss"]) and np.isfinite(rec["score"]) and abs(rec["score"] - score) < 1e-12
        assert rec["sample_size"] == ntokens == nonpad > 0
