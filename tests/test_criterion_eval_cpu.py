"""CPU: the validation oracle (tests/criterion_eval_oracle.py) is sound before a GPU is touched -- its float32 emulation stays within
1/8 of the tolerance the GPU tests use against the float64 reference over the whole table and agrees with it exactly on every hit and
every count; the table catches each named mutation of the emulation; the oracle reproduces what the reference's criterion recorded in
eval mode (tests/golden/validation.npz, written by tools/gen_validation_golden.py).  And the host side of validation that needs no
device: the header and the library carry the two entry points, which refuse bad arguments before any launch; Task.valid_batches;
the Trainer's options and refusals; the data-parallel reduction of the accumulator.
Run with -s for the measured figures."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import criterion_eval_oracle as eo
from tests import criterion_oracle as co

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
NAMES = {BF16: "bf16", FP16: "fp16", FP32: "fp32"}
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _built(i, dtype):
    case = eo.CASES[i]
    b = eo.build(case, dtype)
    ref = eo.eval_reference(b["x"], b["t"], b["A"], b["eps"], b["constrained"])
    return b, ref


def _emulate(i, dtype, mutation=None):
    b, ref = _built(i, dtype)
    em = eo.eval_emulate(b["x"], b["t"], b["A"], b["eps"], b["constrained"], b["fused"], mutation, leaks=b["leaks"])
    exact, err = eo.row_errors(em, ref)
    live = int((b["t"].cpu() != eo.IGNORE).sum())
    return exact, err, eo.sums_agree(em["sums"], ref["sums"], live), em, ref


ROUTE_IDX = [(eo.CASES.index(c), d) for c, d in eo.ROUTES]


# ------------------------------------------------------------------------------------------------------------------ the emulation
def test_constants_hang_together():
    assert eo.EVAL_TOL == 8 * eo.EVAL_WORST and eo.EVAL_TOL < 2e-5
    assert set(eo.MUTATIONS) == {"argmax_last_on_tie", "argmax_sees_disallowed", "argmax_sees_padding", "hit_counts_ignored",
                                 "nll_uses_smoothed", "drop_last_col", "drop_slab", "range_edge", "count_off", "node_sibling_leak"}
    for v in (eo.TARGET_FILL, eo.TIE_FILL, eo.FOREIGN_FILL, co.PAD_FILL):            # exact in both 16-bit types: ties stay ties
        for dt in (BF16, FP16):
            assert float(torch.tensor(v).to(dt)) == v


def test_emulation_stays_within_the_ceiling():
    """Hits, counts, zero rows and +inf rows agree exactly; row_loss / row_nll stay within EVAL_WORST = EVAL_TOL / 8 over every route."""
    worst = {}
    for i, dtype in ROUTE_IDX:
        exact, err, sums_ok, _, _ = _emulate(i, dtype)
        assert exact and sums_ok, (eo.CASES[i], dtype)
        k = (eo.CASES[i].form, NAMES[dtype])
        if err >= worst.get(k, (0.0, None))[0]:
            worst[k] = (err, eo.CASES[i][:7])
    print("\nworst |emulate - reference| of row_loss / row_nll:\n  " + "\n  ".join(f"{k}: {v[0]:.3g} at {v[1]}" for k, v in sorted(worst.items())))
    top = max(v[0] for v in worst.values())
    assert top <= eo.EVAL_WORST, top
    assert top >= eo.EVAL_WORST / 4, "EVAL_WORST is not the measured figure any more: measure again"


def _applies(m, case, b):
    if m == "range_edge":
        return case.form != "node" and case.crange is not None and case.crange[1] < case.V
    if m == "node_sibling_leak":
        return case.form == "node"
    if m == "drop_slab":
        return case.V > 8192
    if m == "argmax_sees_padding":
        return b["x"].stride(0) > case.V
    if m == "argmax_sees_disallowed":
        return b["constrained"]
    if m in ("count_off", "nll_uses_smoothed"):
        return case.eps > 0
    return True


@pytest.mark.parametrize("mutation", eo.MUTATIONS)
def test_table_catches_the_mutation(mutation):
    """Each subtly wrong variant of the emulation is caught -- an exact output differs or the tolerance of the GPU tests is exceeded --
    in at least one table entry of every form it applies to, while the unmutated emulation of that entry passes."""
    caught, seen = {}, {}
    for i, dtype in ROUTE_IDX:
        case = eo.CASES[i]
        if dtype == FP16:
            continue
        b, _ = _built(i, dtype)
        if not _applies(mutation, case, b):
            continue
        route = "regs" if b["fused"] else ("node" if case.form == "node" else "stream")
        seen[route] = seen.get(route, 0) + 1
        exact, err, sums_ok, _, _ = _emulate(i, dtype, mutation)
        if not exact or err > eo.EVAL_TOL or not sums_ok:
            c_exact, c_err, c_sums, _, _ = _emulate(i, dtype)
            assert c_exact and c_sums and c_err <= eo.EVAL_WORST
            caught[route] = caught.get(route, 0) + 1
    print(f"\n{mutation}: caught in {caught} of {seen} entries")
    assert seen and set(caught) == set(seen), (mutation, caught, seen)


def test_table_reaches_every_path():
    regs = [c for c in eo.CASES if c.form == "regs"]
    assert {co.nv_of(c.ld) for c in regs} == {1, 2, 4, 7, 8} and {c.ld for c in regs} >= set(co.FUSED_LD)
    for ld in co.FUSED_LD:
        assert {c.V for c in regs if c.ld == ld} >= {v for v in (ld, ld - 3, ld - 11) if v > 1}, ld
    assert any(c.ld == co.WIDE[1] and c.ld - c.V > 64 for c in regs), "a view of wider storage"
    assert any(c.variant == "range" and c.crange[0] % 8 and c.crange[1] % 8 for c in regs)
    assert any(c.variant == "range" and c.crange[0] < 8192 < c.crange[1] and c.crange[1] > 16384 for c in regs), "a range across slabs"
    stream = [c for c in eo.CASES if c.form == "stream"]
    for V in co.LS_V:
        assert {c.variant for c in stream if c.V == V} == {"none", "range", "mask", "both"}, V
    assert any(c.V > 65536 for c in stream) and any(c.ld is not None and c.ld % 4 for c in stream)
    assert {c.eps for c in eo.CASES} == {0.0, 0.1}
    node = [c for c in eo.CASES if c.form == "node"]
    assert [c.trie for c in node] == list(eo.cst.TRIE_CASES)
    kinds = set()
    for i, c in enumerate(eo.CASES):
        b, ref = _built(i, BF16)
        assert len(b["kinds"]) <= eo.MAX_ROWS and int((b["t"] == eo.IGNORE).sum()) >= 1
        kinds |= {(c.form, k, int(h)) for k, h in zip(b["kinds"], ref["row_hit"].tolist())}
        if c.form != "node":
            lay = eo.layout(c)
            planted = {col for p in lay["plant"] for col in p} | set(lay["t"])
            assert 0 in planted and (c.V - 1 in planted or c.crange is not None)
            if c.crange is not None:
                assert {c.crange[0], c.crange[1] - 1} <= planted, c
            for k in range(1, (c.V + 8191) // 8192):
                if c.crange is None:
                    assert 8192 * k - 1 in planted and (8192 * k in planted or 8192 * k >= c.V), (c, k)
            if c.V > 1536 and c.crange is None:
                assert {1535, 1536} <= planted
    for form in ("regs", "stream"):
        assert {(form, "seam", 1), (form, "tie_low", 1), (form, "tie_high", 0), (form, "ignored", 0), (form, "foreign", 1),
                (form, "dead", 0)} <= kinds, form
    assert {("node", "live", 1), ("node", "live", 0), ("node", "ignored", 0), ("node", "dead_node", 0), ("node", "not_child", 0),
            ("node", "cut_target", 0)} <= kinds
    ties = {eo.layout(c)["tie"][r] for c in regs for r in eo.layout(c)["tie"]}
    assert {(8, 24), (100, 1541), (40, 8232), (100, 9192)} <= ties, "equal maxima in two lanes, two waves, two slabs (same and other thread)"


def test_eps_zero_without_a_constraint_is_plain_cross_entropy():
    for i, c in enumerate(eo.CASES):
        if c.eps == 0.0 and c.variant == "none":
            _, _, _, em, ref = _emulate(i, BF16)
            assert torch.equal(em["row_loss"], em["row_nll"]) and torch.equal(ref["row_loss"], ref["row_nll"])


# ------------------------------------------------------------------------------------------------------------------ the reference's record
def test_oracle_reproduces_the_reference_criterion():
    """tests/golden/validation.npz: the reference's LabelSmoothedCrossEntropyCriterion in eval mode (compute_loss + compute_accuracy)."""
    g = np.load(os.path.join(HERE, "golden", "validation.npz"))
    pad = int(g["pad"][0])
    names = sorted(k[:-4] for k in g.files if k.endswith(".rec"))
    assert len(names) == 6
    for name in names:
        eps, cs, ce, loss, nll, ntok, n_correct, total = g[f"{name}.rec"].tolist()
        masked = name.startswith("mask")
        x = torch.from_numpy(g["logits_masked" if masked else "logits"])
        V = x.shape[-1]
        x = x.reshape(-1, V)
        t = torch.from_numpy(g[f"{name}.target"].astype(np.int64)).reshape(-1)
        crange = (int(cs), int(ce)) if cs >= 0 else None
        cmask = torch.from_numpy(np.unpackbits(g["mask"], axis=-1)[..., :V]).reshape(-1, V) if masked else None
        A = eo.allowed_set(x.shape[0], V, crange, cmask)
        constrained = crange is not None or masked
        for out in (eo.eval_reference(x, t, A, eps, constrained, ignore=pad), eo.eval_emulate(x, t, A, eps, constrained, False, ignore=pad)):
            s = out["sums"]
            assert s[0] == ntok == total and s[3] == n_correct, (name, s)
            assert s[1] == pytest.approx(loss, rel=1e-5) and s[2] == pytest.approx(nll, rel=1e-5), (name, s, loss, nll)
        if eps == 0.0:
            assert loss == nll
    assert 0 < g["none_eps00.rec"][6] < g["none_eps00.rec"][7]


# ------------------------------------------------------------------------------------------------------------------ header, library, arguments
def test_header_declares_and_library_exports_the_entry_points():
    from ofasys_amd.lib import lib, parse_header
    protos = parse_header()
    assert len(protos["ofa_criterion_eval"][1]) == 20 and len(protos["ofa_eval_stats_add"][1]) == 8
    h = lib()
    assert h.cdll.ofa_criterion_eval and h.cdll.ofa_eval_stats_add


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Status codes, no launch: every pointer here is a made-up address nothing may dereference (there is no device in this test)."""
    from ofasys_amd.lib import BF16 as DT_BF16, F32 as DT_F32, lib
    h = lib().cdll
    p = ctypes.c_void_p(4096)

    def call(**kw):
        a = dict(logits=p, target=p, cmask=None, node=None, off=None, tok=None, N=0, E=0, rl=p, rn=p, rh=p, rows=0, V=10, ld=16, ign=1,
                 eps=0.1, cs=-1, ce=-1, dt=DT_BF16, st=None)
        a.update(kw)
        return h.ofa_criterion_eval(*a.values())

    assert call() == 0 and call(dt=DT_F32) == 0                       # rows == 0 is a no-op
    assert call(cs=4, ce=10) == 0 and call(node=p, off=p, tok=p, N=3, E=5) == 0
    bad = [dict(V=1), dict(V=0), dict(ld=8), dict(rows=-1), dict(logits=None), dict(target=None), dict(rl=None), dict(rn=None),
           dict(rh=None), dict(dt=7), dict(eps=1.0), dict(eps=-0.1), dict(cs=2, ce=8), dict(cs=4, ce=4), dict(cs=4, ce=11),
           dict(node=p), dict(node=p, off=p, tok=p, N=0, E=5), dict(node=p, off=p, tok=None, N=3, E=5),
           dict(node=p, off=p, tok=p, N=3, E=5, cmask=p), dict(V=2 ** 31, ld=2 ** 31)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"criterion_eval" in h.ofa_last_error()
    assert h.ofa_eval_stats_add(p, None, None, None, None, 0, 1, None) == 0
    for args in ((None, p, p, p, p, 0), (p, None, p, p, p, 4), (p, p, None, p, p, 4), (p, p, p, None, p, 4), (p, p, p, p, None, 4),
                 (p, p, p, p, p, -1)):
        assert h.ofa_eval_stats_add(*args, 1, None) != 0, args


# ------------------------------------------------------------------------------------------------------------------ task / trainer, no device
def _cola_rows(n):
    return [{"sentence": f"the {i}th book was written by a very careful author .", "label": i % 2, "idx": i} for i in range(n)]


def _infill_task(**kw):
    from ofasys_amd import Task
    return Task(name="text_infilling", instruction='what is the complete text of " [TEXT:sentence,mask_ratio=0.3] "? -> [TEXT:sentence]',
                micro_batch_size=kw.pop("micro_batch_size", 3), **kw)


def test_valid_batches_cover_the_shard_once_in_order_with_the_short_tail():
    from ofasys_amd import Dictionary
    task = _infill_task()
    task.add_dataset(_cola_rows(5), "train")
    task.add_valid_dataset(_cola_rows(11))
    task.initialize(Dictionary())
    got = [np.asarray(b["idx"]).tolist() for b in task.valid_batches()]
    assert got == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10]]                      # finite, in order, the short tail included
    assert [np.asarray(b["idx"]).tolist() for b in task.valid_batches()] == got      # a second pass: the same, unshuffled
    d = task.global_dict
    for b in task.valid_batches():
        assert (b["net_input"]["slots"][0].value == d.index("<mask>")).sum() == 0    # no train-time noise
    for world in (2, 3, 4):                                                          # the shards are contiguous and cover every row once
        rows = [i for r in range(world) for b in task.valid_batches("valid", r, world) for i in np.asarray(b["idx"]).tolist()]
        assert rows == list(range(11)), world
    with pytest.raises(KeyError):
        next(task.valid_batches("test"))


def test_trainer_validation_options_and_refusals():
    from ofasys_amd import Trainer
    from ofasys_amd.task import CriterionConfig
    assert CriterionConfig().report_accuracy is False
    tr = Trainer()
    assert tr.cfg.common.validate_interval_updates == 0 and tr.cfg.common.max_valid_steps is None and not tr.cfg.common.validate_with_ema
    tr = Trainer(validate_interval_updates=2, max_valid_steps=3, validate_with_ema=True, store_ema=True)
    assert (tr.cfg.common.validate_interval_updates, tr.cfg.common.max_valid_steps, tr.cfg.common.validate_with_ema) == (2, 3, True)
    assert tr.valid_history == []
    with pytest.raises(RuntimeError, match="setup"):
        tr.validate()
    plain, scst, no_valid = _infill_task(), _infill_task(), _infill_task()
    plain.add_valid_dataset(_cola_rows(2))
    scst.add_valid_dataset(_cola_rows(2))
    scst.cfg.scst = True
    assert Trainer._valid_tasks([plain, no_valid], "valid") == [plain]              # a task without the split is skipped
    with pytest.raises(NotImplementedError, match="SCST"):
        Trainer._valid_tasks([plain, scst], "valid")
    assert Trainer._valid_tasks([plain, scst], "test") == []


def test_valid_metrics_fields_and_empty_pass():
    from ofasys_amd.trainer import valid_metrics
    ln2 = 0.6931471805599453
    r = valid_metrics(torch.tensor([8.0, 24.0, 16.0, 6.0], dtype=torch.float64))
    assert set(r) == {"loss", "nll_loss", "ppl", "ntokens", "sample_size", "n_correct", "total", "accuracy"}
    assert r["loss"] == pytest.approx(3.0 / ln2) and r["nll_loss"] == pytest.approx(2.0 / ln2) and r["ppl"] == pytest.approx(2 ** (2 / ln2))
    assert r["ntokens"] == r["sample_size"] == r["total"] == 8.0 and r["n_correct"] == 6.0 and r["accuracy"] == 75.0
    z = valid_metrics(torch.zeros(4, dtype=torch.float64))
    assert z["loss"] == 0.0 and z["accuracy"] == 0.0 and z["ppl"] == 1.0
    assert valid_metrics(torch.tensor([2.0, float("inf"), float("inf"), 0.0], dtype=torch.float64))["ppl"] == float("inf")


def _metrics_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ofasys_amd.trainer import valid_metrics
    acc = torch.tensor([[5.0, 10.0, 8.0, 3.0], [3.0, 14.0, 8.0, 1.0]][rank], dtype=torch.float64)
    keep = acc.clone()
    r = valid_metrics(acc, None, world)
    q.put((rank, r, bool(torch.equal(acc, keep))))
    dist.destroy_process_group()


def test_two_ranks_with_known_accumulators_give_the_summed_result():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 517) % 1000
    procs = [ctx.Process(target=_metrics_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ln2 = 0.6931471805599453
    for _, r, untouched in res:
        assert untouched                                          # the rank's own accumulator is reduced on a copy
        assert r["ntokens"] == 8.0 and r["n_correct"] == 4.0 and r["accuracy"] == 50.0
        assert r["loss"] == pytest.approx(24.0 / 8 / ln2) and r["nll_loss"] == pytest.approx(16.0 / 8 / ln2)
    assert res[0][1] == res[1][1]
