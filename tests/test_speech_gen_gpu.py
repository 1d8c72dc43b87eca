"""GPU: autoregressive speech generation -- the fused step kernel (csrc/speech_step.hip) per element, its state machine and dropout, and
AutoRegressiveSpeechGenerator end to end against the reference's own run (tests/golden/speech_gen.npz).

The step kernel's tolerance is not a number chosen here: in the same test the UNFUSED composition of the existing kernels (ops.linear /
relu / dropout_add) is compared with the float64 restatement (tests/speech_gen_oracle.py `step`, on the same rounded inputs, the dtype's
roundings restated), and the fused kernel is held to 2 x that error per output (feat, p, embedding): the two differ in the summation
order of equally long dot products alone.  The error of an output is the root mean square, over its elements, of its distance from the
restatement's value BEFORE that output's own last rounding (feat and the embedding before their rounding to the model dtype, p as the
sigmoid of the unrounded logit); the embedding is restated from the arm's own stored feat, the rounded input its prenet read.  Why not
the distance from the ROUNDED restatement: in a 16-bit dtype both arms then agree with it in every bit -- measured: error exactly 0 in
most shapes -- except where an fp32 sum lands within ~1e-7 of a rounding boundary and the element flips to the neighbouring value, in
either arm, a few times per ten thousand elements (measured: bf16, B = 5, D = 768: the UNFUSED arm flipped one feat element and the
fused none; fp16, B = 1, D = 256: the other way round, 3.4e-06 against 0).  A bound of 2 x 0 tests the toss of that coin, not a kernel.
Against the unrounded value a flip moves an element's error from just under half an ulp to just over: the measure is continuous in
the summation error, which is what the factor 2 is about, and anything a kernel does wrong beyond rounding noise still shows.  Every
element is pinned exactly as well: on small-integer data every fp32 sum is exact, so fused, unfused and restatement must agree in every
bit, last rounding included.

End to end: fp32 within the project's parity bound 1e-3 (relative to the tensor's max), bf16 within twice the reference's own recorded
bf16-vs-fp32 gap per tensor; out_lens equal in both (the fixture's margin condition guarantees it for bf16)."""
import numpy as np
import pytest
import torch

from tests import speech_gen_case as C
from tests import speech_gen_oracle as O
from tests.golden_util import load_golden, rel_err
from tests.model_util import build_model

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
FP32_BOUND = 1e-3
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
SHAPES = [(D, F, P) for D in (256, 768) for F in (80, 160) for P in (256, 64)]      # embed_dim = D


@pytest.fixture(scope="module")
def golden():
    return load_golden("speech_gen")


# ------------------------------------------------------------------------------------------------------------------ step kernel helpers
def _weights(D, F, P, E, layers, dtype, gen, integer=False):
    def t(*shape, scale):
        if integer:                                             # {-1, 0, 1}, sparser where the inputs have grown: every fp32 sum stays exact
            keep = torch.rand(*shape, generator=gen) < scale
            return (torch.randint(-1, 2, shape, generator=gen) * keep).to(dtype).to(DEV)
        return (torch.randn(*shape, generator=gen) * scale).to(dtype).to(DEV)
    s = (lambda k: 1.0 / k ** 0.5) if not integer else (lambda k: 1.0)
    head = (t(F, D, scale=s(D)), t(F, scale=0.1 if not integer else 1.0), t(1, D, scale=s(D)), t(1, scale=0.1 if not integer else 1.0))
    prenet = [(t(P, F if i == 0 else P, scale=s(F if i == 0 else P) if not integer else (0.25 if i else 0.5)),
               t(P, scale=0.1 if not integer else 1.0)) for i in range(layers)]
    proj = (t(E, P, scale=s(P) if not integer else 1.0 / 16), t(E, scale=0.1 if not integer else 1.0))
    return head, prenet, proj


def _state(B, T_cap, F, E, dtype, threshold=0.5):
    i32 = dict(dtype=torch.int32, device=DEV)
    return {"feats": torch.zeros(B, T_cap, F, dtype=dtype, device=DEV), "eos_prob": torch.zeros(B, T_cap, dtype=torch.float32, device=DEV),
            "finished": torch.zeros(B, **i32), "out_lens": torch.full((B,), T_cap, **i32), "nfin": torch.zeros(1, **i32),
            "pad_next": torch.zeros(B, 1, dtype=torch.bool, device=DEV), "embed": torch.zeros(B, E, dtype=dtype, device=DEV),
            "threshold": torch.full((1,), threshold, dtype=torch.float32, device=DEV)}


def _cpu(ws):
    if torch.is_tensor(ws):
        return ws.detach().cpu()
    return type(ws)(_cpu(w) for w in ws)


def _rms(a, b):
    return float((a.double().cpu() - b.double().cpu()).pow(2).mean().sqrt())


def _both_arms(x, head, prenet, proj, dtype, step=1, T_cap=3, p_drop=0.0, threshold=0.5, seed=None):
    from ofasys_amd import ops
    B, F, E = x.shape[0], head[0].shape[0], proj[0].shape[0]
    out = {}
    for fused in (True, False):
        st = _state(B, T_cap, F, E, dtype, threshold)
        if seed is not None:
            ops.manual_seed(seed)
        with torch.no_grad():
            ops.speech_step(x, head, prenet, proj, st, step, p_drop, fused=fused)
        torch.cuda.synchronize()
        out[fused] = st
    return out[True], out[False]


@pytest.mark.parametrize("B", (1, 3, 5))                        # below the 4 rows of a workgroup; no multiple of them (a masked tail group)
@pytest.mark.parametrize("name", list(DTYPES))
def test_step_kernel_per_element(name, B):
    from ofasys_amd import kernels as K
    assert K.speech_step_rows() == 4
    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(100 + B)
    for D, F, P in SHAPES:
        assert K.speech_step_ok(D, F, P, D, 2, dtype)
        head, prenet, proj = _weights(D, F, P, D, 2, dtype, gen)
        x = torch.randn(B, D, generator=gen).to(dtype).to(DEV)
        fused, unfused = _both_arms(x, head, prenet, proj, dtype)
        ref = O.step(_cpu(x), _cpu(head), _cpu(prenet), _cpu(proj), dtype, torch.zeros(B, dtype=torch.bool), torch.full((B,), 3), 1, 0.5)
        figs = {}
        for key, get in (("feat", lambda st: st["feats"][:, 1]), ("p", lambda st: st["eos_prob"][:, 1]), ("embed", lambda st: st["embed"])):
            errs = []
            for arm in (fused, unfused):
                own = ref if key != "embed" else O.step(_cpu(x), _cpu(head), _cpu(prenet), _cpu(proj), dtype, torch.zeros(B, dtype=torch.bool),
                                                        torch.full((B,), 3), 1, 0.5, feat_in=arm["feats"][:, 1].cpu())
                errs.append(_rms(get(arm), own[key + "_exact"]))
            figs[key] = (errs[0], errs[1], float(ref[key].abs().max()))
        print(name, "B", B, "D F P", (D, F, P), {k: f"fused {a:.3e} unfused {b:.3e} (max |ref| {m:.2f})" for k, (a, b, m) in figs.items()})
        for key, (e_fused, e_unfused, _) in figs.items():
            # p is an fp32 tensor in every tier and holds B numbers: below one fp32 ulp of p (what one exponential and one division may
            # cost on the SAME logit, and more than p's own rounding) the two arms' errors are single draws, not a measure of anything
            floor = float(torch.finfo(torch.float32).eps * ref["p"].abs().max()) if key == "p" else 0.0
            assert e_fused <= 2 * max(e_unfused, floor), (name, B, (D, F, P), key, e_fused, e_unfused)
        assert torch.equal(fused["feats"][:, 0], torch.zeros_like(fused["feats"][:, 0])) and torch.equal(fused["feats"][:, 2], fused["feats"][:, 0])
        # exact data: every element, every bit
        head, prenet, proj = _weights(D, F, P, D, 2, dtype, gen, integer=True)
        x = torch.randint(-2, 3, (B, D), generator=gen).to(dtype).to(DEV)
        fused, unfused = _both_arms(x, head, prenet, proj, dtype)
        ref = O.step(_cpu(x), _cpu(head), _cpu(prenet), _cpu(proj), dtype, torch.zeros(B, dtype=torch.bool), torch.full((B,), 3), 1, 0.5)
        for key in ("feats", "embed", "finished", "out_lens", "pad_next", "nfin"):
            assert torch.equal(fused[key], unfused[key]), (name, B, (D, F, P), key)
        assert torch.equal(fused["feats"][:, 1].double().cpu(), ref["feat"]) and torch.equal(fused["embed"].double().cpu(), ref["embed"])
        assert float(ref["embed"].abs().max()) > 0 and bool(torch.isfinite(ref["embed"]).all())
        assert _rms(fused["eos_prob"][:, 1], ref["p"]) < 1e-6


def test_unserved_shapes_take_the_unfused_composition():
    from ofasys_amd import ops
    gen = torch.Generator().manual_seed(7)
    head, prenet, proj = _weights(256, 80, 64, 256, 5, torch.bfloat16, gen)         # five prenet layers: not built
    assert not ops.speech_step_fusable(torch.bfloat16, head, prenet, proj)
    assert ops.speech_step_fusable(torch.bfloat16, head, prenet[:4], proj)
    odd = (head[0][:, 4:], head[1], head[2], head[3])                                # a view that is neither contiguous nor aligned
    assert not ops.speech_step_fusable(torch.bfloat16, odd, prenet[:2], proj)
    assert not ops.speech_step_fusable(torch.float32, head, prenet[:2], proj)        # weights of another dtype than the rows


# ------------------------------------------------------------------------------------------------------------------ state machine
@pytest.mark.parametrize("fused", (True, False), ids=("fused", "unfused"))
def test_state_machine_is_bit_exact(fused):
    """Logits set exactly through x[:, 0] (eos_proj = the first unit vector, bias 0), threshold 0.5, B = 5 (two workgroups).
    Row 0 finishes at t = 0, row 1 at t = 1, row 2 sits exactly AT the threshold throughout (logit 0: p = 0.5, strict test), row 3 had
    finished before (out_len 7 kept whatever it does now), row 4 finishes at t = 0 in the second workgroup."""
    from ofasys_amd import ops
    dtype, B, D, F, P, T_cap = torch.bfloat16, 5, 256, 80, 64, 9
    gen = torch.Generator().manual_seed(3)
    head, prenet, proj = _weights(D, F, P, D, 2, dtype, gen)
    eos_w = torch.zeros(1, D, dtype=dtype, device=DEV)
    eos_w[0, 0] = 1
    head = (head[0], head[1], eos_w, torch.zeros(1, dtype=dtype, device=DEV))
    st = _state(B, T_cap, F, D, dtype)
    st["finished"][3], st["out_lens"][3], st["nfin"][0], st["pad_next"][3] = 1, 7, 1, True
    fin, lens = torch.tensor([0, 0, 0, 1, 0], dtype=torch.bool), torch.tensor([T_cap, T_cap, T_cap, 7, T_cap])
    logits = [[4.0, -4.0, 0.0, 4.0, 4.0], [-4.0, 4.0, 0.0, -4.0, 4.0], [4.0, 4.0, 0.0, 4.0, -4.0]]
    count, table = 1, []
    for t, z in enumerate(logits):
        x = torch.randn(B, D, generator=gen).to(dtype)
        x[:, 0] = torch.tensor(z)
        with torch.no_grad():
            ops.speech_step(x.to(DEV), head, prenet, proj, st, t, 0.0, fused=fused)
        ref = O.step(x, _cpu(head), _cpu(prenet), _cpu(proj), dtype, fin, lens, t, 0.5)
        fin, lens = ref["finished"], ref["out_lens"]
        count += int(ref["newly"].sum())
        table.append(ref["p"])
        assert st["finished"].cpu().bool().tolist() == fin.tolist() and st["out_lens"].cpu().tolist() == lens.tolist(), t
        assert st["pad_next"].view(-1).cpu().tolist() == fin.tolist(), t       # finished AFTER this step: the flag of position t + 1
        assert int(st["nfin"]) == count, t
        assert st["eos_prob"][2, t].item() == 0.5                              # exactly at the threshold: not finished
    assert lens.tolist() == [1, 2, T_cap, 7, 1] and count == 4
    # the flag a step leaves is the padding column of the NEXT position in the restated loop
    flags = O.padding_flags(torch.stack(table, 1)[[0, 1, 2, 4]], 0.5, 3)
    assert flags.tolist() == [[False, True, True], [False, False, True], [False, False, False], [False, True, True]]


# ------------------------------------------------------------------------------------------------------------------ dropout
def test_dropout_half_keeps_or_doubles_and_replays_draw_anew():
    """One prenet layer and an identity projection make the embedding the embedding's INPUT: at p = 0.5 every element is exactly 0 or
    bit-equal to twice its p = 0 value (large positive biases keep the ReLU out of the count); 8 x 512 = 4096 draws."""
    from ofasys_amd import ops
    dtype, B, D, F, P = torch.bfloat16, 8, 256, 80, 512
    gen = torch.Generator().manual_seed(11)
    head, prenet, _ = _weights(D, F, P, P, 1, dtype, gen)
    prenet = [(prenet[0][0], torch.full((P,), 8.0, dtype=dtype, device=DEV))]
    proj = (torch.eye(P, dtype=dtype, device=DEV), torch.zeros(P, dtype=dtype, device=DEV))
    x = torch.randn(B, D, generator=gen).to(dtype).to(DEV)
    base, base_u = _both_arms(x, head, prenet, proj, dtype, p_drop=0.0)
    assert bool((base["embed"] > 0).all())
    drop, drop_u = _both_arms(x, head, prenet, proj, dtype, p_drop=0.5, seed=5)
    for arm, ref in ((drop, base), (drop_u, base_u)):
        kept = arm["embed"] != 0
        assert torch.equal(arm["embed"][kept], (ref["embed"] * 2)[kept])
        frac = float(kept.float().mean())
        assert abs(frac - 0.5) <= 5 * (0.25 / kept.numel()) ** 0.5, frac
    assert torch.equal(drop["embed"] != 0, drop_u["embed"] != 0)               # ofa_dropout_add_fwd's element-to-counter mapping
    again, _ = _both_arms(x, head, prenet, proj, dtype, p_drop=0.5, seed=5)
    other, _ = _both_arms(x, head, prenet, proj, dtype, p_drop=0.5, seed=6)
    assert torch.equal(again["embed"], drop["embed"]) and not torch.equal(other["embed"], drop["embed"])
    # one captured step, replayed twice: the device-side stream position moves
    st = _state(B, 3, F, P, dtype)
    ops.manual_seed(5)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.no_grad(), torch.cuda.graph(g):
        ops.speech_step(x, head, prenet, proj, st, 0, 0.5, fused=True)
        ops.rng_advance()
    masks = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        masks.append((st["embed"] != 0).clone())
    assert torch.equal(masks[0], drop["embed"] != 0) and not torch.equal(masks[0], masks[1])


# ------------------------------------------------------------------------------------------------------------------ the generator
def _model(entry, dtype, prenet_dropout=None, golden=None):
    case = C.case(entry)
    if prenet_dropout is not None:
        case = dict(case, adaptor_overrides={"audio_fbank": dict(case["adaptor_overrides"]["audio_fbank"], prenet_dropout=prenet_dropout)})
    model, d = build_model(case)
    C.apply_eos_affine(model, torch.from_numpy(golden[f"{entry}.eos_scale"]), float(golden[f"{entry}.eos_bias"][0]))
    model = model.to(DEV)
    return (model if dtype == torch.float32 else model.to(dtype)).eval(), d


def _sample(entry, d, dtype, has_targ=False):
    from ofasys_amd import ModalityType, Slot
    sample = {"net_input": {"slots": [Slot(ModalityType.TEXT, True, C.source_tokens(len(d)).to(DEV)), Slot(ModalityType.AUDIO, False, None)]}}
    if has_targ:
        tgt, lens = C.target(entry)
        sample["target"], sample["target_lengths"] = tgt.to(dtype).to(DEV), lens.to(DEV)
    return sample


def _stats_file(tmp_path_factory):
    mean, std = C.gcmvn_stats()
    path = tmp_path_factory.mktemp("speech_gen") / "gcmvn_stats.npz"
    np.savez(path, mean=mean, std=std)
    return str(path)


@pytest.fixture(scope="module")
def stats_path(tmp_path_factory):
    return _stats_file(tmp_path_factory)


def _generator(entry, d, golden, stats_path, **kw):
    from ofasys_amd import AutoRegressiveSpeechGenerator
    kw.setdefault("eos_prob_threshold", float(golden[f"{entry}.threshold"][0]))
    return AutoRegressiveSpeechGenerator(d, stats_npz_path=stats_path, max_iter=C.ENTRIES[entry]["max_iter"], **kw)


def _lens(outs, n):
    return [int(o.eos_prob.shape[0]) // n for o in outs]


@pytest.mark.parametrize("entry", list(C.ENTRIES))
@pytest.mark.parametrize("name", ("fp32", "bf16"))
def test_generate_against_the_reference(golden, stats_path, name, entry):
    dtype, n = DTYPES[name], C.ENTRIES[entry]["n_frames_per_step"]
    g = lambda k: golden[f"{entry}.{k}"]                                        # noqa: E731
    model, d = _model(entry, dtype, golden=golden)
    gen = _generator(entry, d, golden, stats_path)
    for run in ("eager warm-up", "captured steps"):
        outs = gen.generate(model, _sample(entry, d, dtype, has_targ=True), has_targ=True)
        assert gen.fused is True and _lens(outs, n) == g("out_lens").tolist(), run
        whole = {"attn": C.batch(o.attn[:, :g(f"attn.{b}").shape[1]] for b, o in enumerate(outs))}
        for k in ("feature", "eos_prob", "targ_feature"):
            whole[k] = C.batch(getattr(o, k) for o in outs)
        for k, got in whole.items():                                           # bf16: over the batch, as the gaps were recorded
            err = rel_err(got, C.batch(g(f"{k}.{b}") for b in range(C.B)))
            bound = FP32_BOUND if dtype == torch.float32 else 2 * float(g("gap_" + k)[0])
            print(name, entry, run, k, f"{err:.3e} (bound {bound:.3e})")
            assert err <= bound, (run, k, err, bound)
        for b, o in enumerate(outs):
            L = int(g("out_lens")[b]) * n
            assert o.feature.shape == (L, C.RAW) and o.eos_prob.shape == (L,) and o.attn.shape == (C.TEXT_SHAPE[1], L)
            assert o.alignment.shape == (L,) and not o.feature.is_cuda and o.waveform is None
            cols = g(f"attn.{b}").shape[1]                                     # the reference keeps the first step's map: n columns
            figs = {"feature": rel_err(o.feature.float(), g(f"feature.{b}")), "eos_prob": rel_err(o.eos_prob.float(), g(f"eos_prob.{b}")),
                    "attn": rel_err(o.attn[:, :cols].float(), g(f"attn.{b}")), "targ_feature": rel_err(o.targ_feature.float(), g(f"targ_feature.{b}"))}
            print(name, entry, run, "row", b, {k: f"{v:.3e}" for k, v in figs.items()})
            if dtype == torch.float32:                                         # fp32: every row's tensors on their own as well
                assert all(v <= FP32_BOUND for v in figs.values()), (run, b, figs)
                assert o.alignment[:cols].tolist() == g(f"alignment.{b}").tolist()
            assert torch.equal(o.alignment, o.attn.argmax(dim=0))
            assert torch.equal(o.attn[:, ::n], o.attn[:, n - 1::n]) and torch.equal(o.eos_prob[::n], o.eos_prob[n - 1::n])
    assert len(gen._dec._graphs) == gen.steps_run == g("feature_out").shape[1]


def test_graph_eager_fused_unfused_agree_and_a_new_threshold_reuses_the_graphs(golden, stats_path):
    entry, dtype, n = "n1", torch.bfloat16, 1
    model, d = _model(entry, dtype, golden=golden)
    sample = _sample(entry, d, dtype)
    graph = _generator(entry, d, golden, stats_path)
    eager = _generator(entry, d, golden, stats_path, use_graph=False)
    unfused = _generator(entry, d, golden, stats_path, fused_step=False)
    graph.generate(model, sample)
    a, b = graph.generate(model, sample), eager.generate(model, sample)
    unfused.generate(model, sample)
    c = unfused.generate(model, sample)
    assert graph.fused and eager.fused and unfused.fused is False and len(eager._dec._graphs) == 0
    assert _lens(a, n) == _lens(b, n) == _lens(c, n) == golden["n1.out_lens"].tolist()
    for x, y in zip(a, b):
        for k in ("feature", "eos_prob", "attn", "alignment"):
            assert torch.equal(getattr(x, k), getattr(y, k)), k                # graph == eager, every bit (prenet_dropout 0)
    worst = rel_err(C.batch(z.feature for z in c), C.batch(x.feature for x in a))
    print("fused vs unfused feature, max relative difference over the batch", f"{worst:.3e}")
    assert worst <= 2 * float(golden["n1.gap_feature"][0])                     # inside the bf16 bound of the end-to-end test
    # another threshold: another finishing pattern, the same captured steps
    graphs = len(graph._dec._graphs)
    assert graphs == 12
    graph.eos_prob_threshold = eager.eos_prob_threshold = 1e-4
    a, b = graph.generate(model, sample), eager.generate(model, sample)
    assert len(graph._dec._graphs) == graphs and graph.steps_run < 12
    assert _lens(a, n) == _lens(b, n) != golden["n1.out_lens"].tolist()
    for x, y in zip(a, b):
        assert torch.equal(x.feature, y.feature) and torch.equal(x.eos_prob, y.eos_prob)
    for y in b:                                                                # the finish rule on the run's own probabilities
        assert bool((y.eos_prob[:-1] <= 1e-4).all()) and float(y.eos_prob[-1]) > 1e-4


def test_generate_is_reproducible_under_manual_seed(golden, stats_path):
    """prenet_dropout 0.5 draws in eval mode too: two whole generate calls after the same ops.manual_seed are bit-equal (the first runs
    eagerly, the second records and replays its steps), and another seed gives other frames."""
    from ofasys_amd import ops
    entry, dtype = "n1", torch.bfloat16
    model, d = _model(entry, dtype, prenet_dropout=0.5, golden=golden)
    sample = _sample(entry, d, dtype)
    gen = _generator(entry, d, golden, stats_path, eos_prob_threshold=2.0)     # nobody finishes: 12 steps each
    runs = []
    for seed in (21, 21, 22, 21):
        ops.manual_seed(seed)
        runs.append(gen.generate(model, sample))
    assert len(gen._dec._graphs) == 12
    for x, y, z, w in zip(*runs):
        assert torch.equal(x.feature, y.feature) and torch.equal(x.feature, w.feature) and not torch.equal(x.feature, z.feature)


def test_task_inference_returns_the_speech_outputs(golden, stats_path):
    from oracle import recipe
    from ofasys_amd import SpeechGeneratorOutput, Task
    from ofasys_amd.preprocessor import to_device
    entry = "n1"
    model, d = _model(entry, torch.float32, golden=golden)
    tokens = C.source_tokens(len(d)).to(DEV)                                  # (before initialize() adds the task's symbols to d)
    task = Task(name="tts", instruction="[TEXT:src] -> [AUDIO:fbank]", micro_batch_size=3)
    task.initialize(d)
    task.cfg.evaluation.generator_args = '{"max_iter": 12, "eos_prob_threshold": %r, "stats_npz_path": "%s"}' % (
        float(golden["n1.threshold"][0]), stats_path)
    rows = [{"src": f"sentence {i}", "fbank": {"fbank": recipe.floats(f"speech_gen.task.{i}", (4, C.RAW)), "fbank_lengths": 4}} for i in range(3)]
    task.add_dataset(rows, "valid")
    batch = to_device(task.get_sample("valid"), DEV)
    src = [s for s in batch["net_input"]["slots"] if s.is_src][0]
    src.value = tokens                                                        # the fixture's source tokens in the collated batch
    outs = task.inference(model, batch)
    assert len(outs) == 3 and all(isinstance(o, SpeechGeneratorOutput) for o in outs)
    assert [int(o.feature.shape[0]) for o in outs] == golden["n1.out_lens"].tolist()
    for b, o in enumerate(outs):
        assert rel_err(o.feature.float(), golden[f"n1.feature.{b}"]) <= FP32_BOUND
