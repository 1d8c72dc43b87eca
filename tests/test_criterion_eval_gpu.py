"""GPU: the validation criterion kernels (ofa_criterion_eval: the registers form, the streaming form and the node form; and
ofa_eval_stats_add) against the float64 oracle of tests/criterion_eval_oracle.py over its whole table, in every dtype, through the
direct entry point (kernels.criterion_eval, output buffers NaN-poisoned) and through ops.criterion_eval.  row_hit, n_correct and
ntokens exactly; row_loss / row_nll within eo.EVAL_TOL (8 x the emulation's own error, measured on the CPU); the sums within
live rows x EVAL_TOL.  Then the accumulator: three calls add up, and two identical runs give the same bits.
Measured on an MI355X (printed with -s): see DESIGN.md 5r."""
import pytest
import torch

from tests import criterion_eval_oracle as eo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
WORST = {}


@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


def _poison(rows):
    """NaN / -1 filled tensors of the sizes the wrapper is about to torch.empty, freed again: the caching allocator hands those blocks
    straight back, so an element the kernel leaves unwritten reads as poison."""
    keep = [torch.full((rows,), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV),
            torch.full((rows,), -1, dtype=torch.int32, device=DEV)]
    torch.cuda.synchronize()
    del keep


def _args(b):
    cs, ce = b["crange"] if b["crange"] is not None else (-1, -1)
    return dict(eps=b["eps"], cstart=cs, cend=ce, cmask=b["cmask"], nodes=b["nodes"], trie=b["trie"])


def _check(got, ref, b, tag):
    exact, err = eo.row_errors(got, ref)
    assert exact, (tag, got["row_hit"].tolist(), ref["row_hit"].tolist(), got["row_loss"].tolist(), ref["row_loss"].tolist())
    assert err <= eo.EVAL_TOL, (tag, err)
    return err


@pytest.mark.parametrize("dtype", DTYPES, ids=[NAMES[d] for d in DTYPES])
def test_kernels_against_the_oracle_over_the_table(K, dtype):
    from ofasys_amd import ops
    worst, n = 0.0, 0
    for case, dt in eo.ROUTES:
        if dt != dtype:
            continue
        b = eo.build(case, dtype, DEV)
        ref = eo.eval_reference(b["x"], b["t"], b["A"], b["eps"], b["constrained"])
        live = int((b["t"] != eo.IGNORE).sum())
        rows, V = b["x"].shape
        tag = (tuple(case[:7]), NAMES[dtype])
        # the direct entry point
        _poison(rows)
        rl, rn, rh = K.criterion_eval(b["x"], b["t"], V, eo.IGNORE, **_args(b))
        acc = torch.zeros(4, dtype=torch.float64, device=DEV)
        K.eval_stats_add(acc, rl, rn, rh, b["t"], eo.IGNORE)
        torch.cuda.synchronize()
        assert set(rh.tolist()) <= {0, 1}, tag
        worst = max(worst, _check(dict(row_loss=rl, row_nll=rn, row_hit=rh), ref, b, tag))
        assert eo.sums_agree(acc.tolist(), ref["sums"], live), (tag, acc.tolist(), ref["sums"])
        # the op: the same rows, and its accumulator on top of what is there
        acc2 = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64, device=DEV)
        out, rl2, rn2, rh2 = ops.criterion_eval(b["x"][None], b["t"][None], eo.IGNORE, b["eps"], b["crange"],
                                                None if b["cmask"] is None else b["cmask"][None],
                                                None if b["nodes"] is None else b["nodes"][None], b["trie"], acc=acc2)
        torch.cuda.synchronize()
        assert out is acc2
        worst = max(worst, _check(dict(row_loss=rl2, row_nll=rn2, row_hit=rh2), ref, b, tag + ("op",)))
        added = (acc2 - torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64, device=DEV)).tolist()     # (exact: fp32 sums in fp64)
        assert eo.sums_agree(added, ref["sums"], live), (tag, added, ref["sums"])
        if b["x"].stride(0) % eo.NVEC[dtype] == 0:          # (else the op copies the rows to a vector-aligned stride: another route)
            assert torch.equal(rl2, rl) and torch.equal(rn2, rn) and torch.equal(rh2, rh) and added == acc.tolist(), tag
        n += 1
    WORST[NAMES[dtype]] = worst
    print(f"\n{NAMES[dtype]}: {n} table entries, worst |row_loss / row_nll - float64| {worst:.3g} against EVAL_TOL {eo.EVAL_TOL:.3g}")
    assert n > 0


def test_eps_zero_is_plain_cross_entropy_bit_for_bit(K):
    for case in eo.CASES:
        if case.eps == 0.0 and case.variant == "none":
            for dtype in eo.DTYPES[case.form]:
                b = eo.build(case, dtype, DEV)
                rl, rn, _ = K.criterion_eval(b["x"], b["t"], case.V, eo.IGNORE, **_args(b))
                assert torch.equal(rl, rn), (case, dtype)


def test_accumulator_adds_up_and_is_deterministic(K):
    """Three batches into one accumulator == the sum of three single accumulators (integers exactly, the fp64 sums of three fp32 batch
    sums exactly too: fp64 holds them); and the whole sequence run twice gives bit-identical accumulators.  2000 rows: several trips
    of the single block's loop."""
    from ofasys_amd import ops
    g = torch.Generator().manual_seed(3)
    batches = []
    for i, rows in enumerate((2000, 777, 1)):
        x = (torch.randn(rows, 520, generator=g) * 3).to(torch.bfloat16).to(DEV)
        t = torch.randint(0, 520, (rows,), generator=g).to(DEV)
        t[::7] = eo.IGNORE
        batches.append((x, t))
    runs = []
    for _ in range(2):
        acc = torch.zeros(4, dtype=torch.float64, device=DEV)
        singles = []
        for x, t in batches:
            ops.criterion_eval(x, t, eo.IGNORE, 0.1, (8, 500), acc=acc)
            singles.append(ops.criterion_eval(x, t, eo.IGNORE, 0.1, (8, 500))[0])
        torch.cuda.synchronize()
        runs.append((acc.clone(), [s.clone() for s in singles]))
    acc, singles = runs[0]
    assert torch.equal(acc, singles[0] + singles[1] + singles[2])
    assert float(acc[0]) == sum(int((t != eo.IGNORE).sum()) for _, t in batches)
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    # against the oracle, as a whole pass
    want = [0.0, 0.0, 0.0, 0.0]
    for x, t in batches:
        A = eo.allowed_set(x.shape[0], 520, (8, 500))
        s = eo.eval_reference(x, t, A, 0.1, True)["sums"]
        want = [a + b for a, b in zip(want, s)]
    assert want[1] == float("inf") or eo.sums_agree(acc.tolist(), want, int(want[0]))


def test_out_of_range_targets_are_never_dereferenced(K):
    """A live target far outside [0, V): +inf rows, no hit, counted as a token -- the existing kernels' convention."""
    x = torch.zeros(3, 16, dtype=torch.bfloat16, device=DEV)
    t = torch.tensor([2 ** 40, -5, 3], device=DEV)
    for xx in (x, x.float()):
        rl, rn, rh = K.criterion_eval(xx, t, 16, eo.IGNORE, 0.1)
        assert rl[:2].tolist() == [float("inf")] * 2 and rn[:2].tolist() == [float("inf")] * 2 and rh.tolist() == [0, 0, 0]
        assert torch.isfinite(rl[2])
