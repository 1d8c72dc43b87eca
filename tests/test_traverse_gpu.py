"""GPU: closed-set inference (csrc/closed_set_score.hip, ofasys_amd.traverse.TraverseTask).

1. The three kernels against the dense formulation of traverse_task.py:99-104 in fp32 torch (project onto V, mask, log_softmax,
   gather, sum) on the same, already rounded inputs.
2. TraverseTask.score / inference on the fp32 HIP `tiny_text` model against tests/golden/traverse.npz (the reference on the CPU).
3. Chunking the answers does not change the scores.
4. A second inference allocates nothing for the plan; the model stays in eval mode.
5. Beam-search generation, then a traverse pass, then a captured TrainStep, then a traverse pass again in one process.
"""
import numpy as np
import pytest
import torch

from oracle.cases import CASES, VOCAB_EXTRA, make_value
from tests.golden_util import case_inputs, load_golden
from tests.model_util import build_model, make_slots
from tests.traverse_case import ANSWERS, SCORE_TOL, random_answers, score_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOS, PAD, EOS = 0, 1, 2
V_OFA, D_OFA = 59457, 768
V_TINY = VOCAB_EXTRA + 4        # the model's dictionary as built; Task.initialize adds '<mask>' / '<bin>_k' symbols to it afterwards
_W = {}


def _proj(dtype):
    """One random output projection [V, D] (+ bias) per dtype, rounded to the dtype."""
    if dtype not in _W:
        g = torch.Generator().manual_seed(11)
        _W[dtype] = ((torch.randn(V_OFA, D_OFA, generator=g) * 0.05).to(DEV).to(dtype), torch.randn(V_OFA, generator=g).to(DEV).to(dtype))
    return _W[dtype]


def dense_scores(h, W, bias, plan, bsz):
    """traverse_task.py:99-104 in fp32 torch on the GPU: h [bsz, C, T, D] (any dtype, upcast), one sentence at a time."""
    C, T = plan.C, plan.Tmax
    rows, toks = [], []
    for c in range(C):
        for t in range(int(plan.lengths[c])):
            a = plan.allowed(c, t)
            rows += [c * T + t] * len(a)
            toks += a
    mask = torch.zeros(C * T, W.shape[0], dtype=torch.bool, device=DEV)
    mask[torch.tensor(rows, device=DEV), torch.tensor(toks, device=DEV)] = True
    tgt = torch.from_numpy(plan.target).to(DEV).reshape(-1)
    mask[tgt == PAD] = True                                   # (the reference pads its masks with True: those positions are zeroed)
    W32, b32 = W.float(), None if bias is None else bias.float()
    out = torch.empty(bsz, C, device=DEV)
    for b in range(bsz):
        logits = h[b].reshape(C * T, -1).float() @ W32.t()
        if b32 is not None:
            logits += b32
        logits.masked_fill_(~mask, float("-inf"))
        lp = torch.log_softmax(logits, -1).gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
        out[b] = lp.masked_fill(tgt == PAD, 0).view(C, T).sum(1)
    return out.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [1, 37, 700])
@pytest.mark.parametrize("with_bias", [False, True])
def test_kernels_match_dense_fp32(dtype, C, with_bias):
    """Bound: 1e-4 relative (floor 1e-4 absolute) for all three dtypes -- the kernels accumulate in fp32 on the same rounded
    inputs, so only the summation order differs from the dense formulation."""
    from ofasys_amd import TraversePlan
    from ofasys_amd import kernels as K
    rng = np.random.default_rng(C * 7 + int(with_bias))
    answers = random_answers(rng, C, V=V_OFA, p_dup=0.02, p_ext=0.15) if C == 700 else random_answers(rng, C, V=V_OFA)
    plan = TraversePlan(answers, BOS, EOS, PAD)
    if C == 700:
        assert plan.node_edge_off[1] > 512, int(plan.node_edge_off[1])          # the root is split over many workgroups
    bsz, T = 11, plan.Tmax                                                       # 11: a full tile of 8 sentences and a ragged one
    g = torch.Generator().manual_seed(C)
    h = torch.randn(bsz, C, T, D_OFA, generator=g)
    for c in range(C):                                        # a causal decoder: equal prefixes, equal hidden states
        for t in range(int(plan.lengths[c])):
            n = plan.node_of(c, t)
            h[:, c, t] = h[:, plan.rep_ans[n], plan.rep_pos[n]]
    h = h.to(DEV).to(dtype)
    W, bias = _proj(dtype)
    bias = bias if with_bias else None
    dev = plan.to_device(DEV)
    got = K.closed_set_score(h.reshape(-1, D_OFA), W, bias, dev, bsz)
    torch.cuda.synchronize()
    want = dense_scores(h, W, bias, plan, bsz)
    err = score_err(got.cpu().numpy(), want.numpy())                              # |d| / max(|want|, 1)
    print(f"closed_set kernels {dtype} C={C} bias={with_bias}: N={plan.N} E={plan.E} root={int(plan.node_edge_off[1])} max err {err:.3e}")
    assert torch.isfinite(got).all()
    assert err <= 1e-4, err
    # the chunked entry points give the same numbers: stage 1 per chunk of answers, stages 2-3 once
    if C > 1:
        ws = torch.empty((K.closed_set_ws_bytes(bsz, plan.E, plan.N) + 3) // 4, device=DEV)
        scores = torch.empty(bsz, C, device=DEV)
        per = 13
        for c0 in range(0, C, per):
            c1 = min(C, c0 + per)
            i0, i1, Tc = plan.chunk_items(c0, c1)
            if i1 > i0:
                hc = h[:, c0:c1, :Tc].reshape(-1, D_OFA)
                K.closed_set_edge_logits(hc, W, bias, dev, bsz, c1 - c0, Tc, c0, dev["items"][i0:i1], ws)
        K.closed_set_reduce(dev, bsz, ws, scores)
        assert torch.equal(scores, got)


def test_kernels_reject_mismatched_inputs():
    from ofasys_amd import TraversePlan
    from ofasys_amd import kernels as K
    from ofasys_amd.lib import OfaError
    plan = TraversePlan(ANSWERS, BOS, EOS, PAD)
    dev = plan.to_device(DEV)
    W = torch.zeros(204, 64, device=DEV)
    with pytest.raises(OfaError, match="feature rows"):
        K.closed_set_score(torch.zeros(7, 64, device=DEV), W, None, dev, 2)
    with pytest.raises(OfaError, match="dtype"):
        K.closed_set_score(torch.zeros(2 * plan.C * plan.Tmax, 64, device=DEV, dtype=torch.bfloat16), W, None, dev, 2)


# ------------------------------------------------------------------------------------------------ the task against the reference
def _task(d, **kw):
    from ofasys_amd import TraverseTask
    task = TraverseTask(name="vqa", instruction="[TEXT:src] what is it? -> [TEXT:tgt]", **kw)
    task.initialize(d, closed_set=[tuple(a) for a in ANSWERS])
    return task


def _sample(V=V_TINY, src=None):
    from ofasys_amd import ModalityType, Slot
    case = CASES["tiny_text"]
    slots = [Slot(ModalityType[m], True, (src if src is not None else make_value(spec, V)).to(DEV), attributes=a)
             for m, s, spec, a in case["slots"] if s]
    return {"net_input": {"slots": slots}}


def test_score_and_inference_match_reference_golden():
    """Bound: the standing fp32 bound against the reference, 1e-3 relative with a floor of 1e-3 absolute.  Measured maximum
    |score - reference| / max(|reference|, 1) on an MI355X: 1.27e-6 (profiles/traverse_parity.txt)."""
    g = load_golden("traverse")
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    task = _task(d)
    scores = task.score(model, _sample())
    assert scores.device.type == "cpu" and scores.dtype == torch.float32 and tuple(scores.shape) == (2, len(ANSWERS))
    err = score_err(scores.numpy(), g["scores"])
    print(f"traverse parity (tiny_text, fp32): max |score - reference| / max(|reference|, 1) = {err:.3e}")
    assert err <= SCORE_TOL, err
    hyps = task.inference(model, _sample())
    assert hyps == [tuple(ANSWERS[i]) for i in g["argmax"]]
    assert not model.training


def test_chunking_does_not_change_the_scores():
    """One answer per chunk against one chunk for all.  The edge logits of a node are computed from the decoder row of its
    representative answer in whichever chunk holds it; the decoder's kernels do not mix rows, so the arrangement is expected to
    be bit-identical.  Should a GEMM plan depend on the row count the sums could be reordered: the bound is then 1e-6
    (relative, floor absolute), fp32 rounding of a handful of sums."""
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    one, each, ragged = _task(d, max_rows=1 << 20), _task(d, max_rows=2), _task(d, max_rows=10)
    a, b, c = (t.score(model, _sample()) for t in (one, each, ragged))
    e1, e2 = score_err(b.numpy(), a.numpy()), score_err(c.numpy(), a.numpy())
    print(f"traverse chunking: one answer per chunk vs one chunk {e1:.3e} (bit-identical: {torch.equal(a, b)}), five per chunk {e2:.3e}")
    assert e1 <= 1e-6 and e2 <= 1e-6, (e1, e2)


def test_second_inference_allocates_nothing_and_model_stays_in_eval():
    from oracle import recipe
    model, d = build_model(CASES["tiny_text"], DEV, torch.float32)
    model.train()
    task = _task(d)
    V = V_TINY
    first = task.inference(model, _sample(V))
    assert not model.training and len(first) == 2
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in task._plan_on(torch.device(DEV, torch.cuda.current_device())).items() if torch.is_tensor(v)}
    nplans, nbufs = len(task._dev), len(task._buf)
    before = torch.cuda.memory_allocated()
    src = recipe.tokens("input.beam_src1", (2, 16), V, [16, 12])                  # another batch of the same shape
    second = task.inference(model, _sample(V, src))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert (len(task._dev), len(task._buf)) == (nplans, nbufs)
    for dev_plan in task._dev.values():
        assert {k: v.data_ptr() for k, v in dev_plan.items() if torch.is_tensor(v)} == ptrs
    assert len(second) == 2 and not model.training


def test_traverse_between_generation_and_a_captured_train_step():
    """scratch allocated inside the generator's captures belongs to the generator; the traverse pass runs eagerly
    on its own buffers and the shared eager cache, so a TrainStep captured afterwards addresses nothing of either."""
    from ofasys_amd.generator import SequenceGenerator
    from ofasys_amd.trainer import TrainStep
    case = CASES["tiny_text"]
    model, d = build_model(case, DEV, torch.float32)
    V = V_TINY
    gen = SequenceGenerator(d, beam_size=3, max_len=6)
    for _ in range(3):                                        # eager warm-up, capture, replay
        gen.generate(model, _sample(V))
    assert len(gen._dec._graphs) > 0
    task = _task(d)
    before = task.score(model, _sample(V))
    vals, target = case_inputs(case)
    model.train()
    tr = TrainStep(model, lr=0.0, clip_norm=0.0, use_graph=True, graph_warmup=1)
    for _ in range(3):
        stats = tr.train_step([{"slots": make_slots(vals, DEV), "target": target.to(DEV)}])["stats"]
    assert tr.captured_graphs() >= 1 and np.isfinite(float(stats[1]))
    after = task.score(model, _sample(V))                     # lr = 0: the same weights, now in the trainer's arenas
    assert not model.training
    assert score_err(after.numpy(), before.numpy()) <= 1e-6
    assert task.inference(model, _sample(V)) == [tuple(ANSWERS[i]) for i in load_golden("traverse")["argmax"]]
