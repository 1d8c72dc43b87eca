"""CPU: the streaming / optimizer-step oracle (tests/stream_oracle.py) is sound before a GPU is touched -- the Philox restatement gives
the published known answers, every case lies where its name says against the restated grids (below, at, past), the float32 emulations
stay within the ceiling against float64 over every table and dtype, every named mutation is caught by a case of the table in every dtype
it can occur in (a figure over the kernel's limit, or a bit mismatch for the movers and the mask), and the exact-reduction inputs keep
every partial sum below 2^24.  Run with -s for the measured ceilings and the case that catches each mutation."""
import numpy as np
import pytest
import torch

from ofasys_amd import lib as L
from tests import stream_oracle as so

BF16, FP16, F32 = so.BF16, so.FP16, so.F32
IDS = [so.NAMES[d] for d in so.DTYPES3]


def test_philox_known_answers():
    for ctr, key, want in so.PHILOX_KAT:
        got = so.philox4x32_10(ctr, key)
        assert tuple(int(w[0]) for w in got) == want, [hex(int(w[0])) for w in got]
    assert so.philox_thresh(0.0) == 0 and so.philox_thresh(0.1) == 6554 and so.philox_thresh(0.5) == 32768
    # the counter is 64 bits wide: a low word that wraps during the launch carries into the high word
    m = so.dropout_mask(16000, 0.5, so.SEED, 2 ** 32 - 1000)
    hi = so.dropout_mask(8000, 0.5, so.SEED, 2 ** 32)
    assert torch.equal(m[8000:], hi) and not torch.equal(m[8000:], so.dropout_mask(8000, 0.5, so.SEED, 0))
    assert abs(float(m.double().mean()) - 0.5) < 0.02 and bool(so.dropout_mask(4099, 0.0, 1, 5).all())


def test_every_case_lies_where_its_name_says():
    """below / at / past against the restated grid of the launch, per dtype; the past cases make their second trip on blocks 0 and 1,
    block 1 on 44 threads only; the wide rows straddle the seam."""
    names = [c.name for c in so.CASES]
    assert len(set(names)) == len(names) and len({c.seed for c in so.CASES}) == len(names)
    for dt in so.DTYPES3:
        for c in so.CASES:
            assert so.case_where(c, dt) == so.case_pos(c, dt), (c.name, so.NAMES[dt], so.case_work(c, dt), so.case_grid(c, dt))
            assert so.case_numel(c, dt) <= 4.3e6, c.name
            if c.pos == "past" and c.kernel != "im2col_patch" and not dict(c.opt).get("D"):
                assert so.case_grid(c, dt) == so.STREAM_CAP
                over = so.case_work(c, dt) - so.STREAM_T
                assert 256 < over < 512, (c.name, over)                  # blocks 0 and 1 only
                if c.vpr != so.WIDE:
                    assert over - 256 == 44 + (c.kernel == "dropout_add" and c.tail > 0), (c.name, over)
                else:
                    assert so.STREAM_T % c.vpr != 0                      # a row straddles the seam
        for k in so.ONE_ROUNDING + so.MOVERS:
            assert {so.case_pos(c, dt) for c in so.cases_of(k)} == {"below", "at", "past"}, (k, so.NAMES[dt])
        for k in so.ROW_SHAPED:
            assert {c.vpr for c in so.cases_of(k) if c.pos == "past"} >= {1, so.WIDE}, k
        for k in so.HAS_TAIL:
            assert any(c.units == 0 and c.tail for c in so.cases_of(k)) and any(c.pos == "past" and c.tail for c in so.cases_of(k)), k
        # both im2col kernels, past their grids
        runs = {(so.im2col_runs(c, dt), so.case_pos(c, dt)) for c in so.cases_of("im2col_patch")}
        assert runs >= ({(True, "past"), (True, "at"), (False, "past"), (False, "at")} if dt != F32 else {(False, "past"), (False, "at")})
        assert {dict(c.opt)["lead"] for c in so.cases_of("im2col_patch")} == {0, 1}
        assert any(dict(c.opt)["Kpad"] > dict(c.opt)["C"] * dict(c.opt)["p"] ** 2 for c in so.cases_of("im2col_patch"))
        # the sumsq sizes against their own 1024-block grid
        for pos, u, t in so.SUMSQ_SIZES:
            n = so.sumsq_n(u, t, dt)
            assert so.where(n // so.NVEC[dt], so.sumsq_grid(n, dt) * 256) == pos, (pos, u, t)
    assert so.sumsq_n(*so.SUMSQ_SIZES[-1][1:], BF16) == 2_099_557
    assert [so.colsum_passes(r) for r in so.COLSUM_ROWS] == [8, 8, 9, 9] and so.colsum_slots(8193) == so.COLSUM_SLOT_CAP
    assert L.lib().cdll.ofa_colsum_slots(8193) == so.COLSUM_SLOT_CAP and L.lib().cdll.ofa_colsum_slots(100) == so.colsum_slots(100) == 2
    drops = [dict(c.opt) for c in so.cases_of("dropout_add")]
    assert {d["p"] for d in drops} == {0.0, 0.1, 0.5} and {d["offset"] for d in drops} >= {0, 77, 2 ** 32 - 1000}
    assert any(d["base"] for d in drops) and any(not d["res"] for d in drops)
    assert {dict(c.opt)["k"] for c in so.cases_of("add_n")} == {1, 2, 16}
    assert {(dict(c.opt)["batch"], dict(c.opt)["acc"]) for c in so.cases_of("batch_sum")} == {(1, 0), (1, 1), (5, 0), (5, 1)}
    assert {dict(c.opt)["parts"] for c in so.cases_of("gather_rows_parts") if c.pos == "past"} >= {3, 8}
    assert {dict(c.opt)["parts"] for c in so.cases_of("gather_rows_parts")} == {1, 3, 8}


def test_adam_cases_lie_where_their_names_say():
    """Default grid: no thread owns a second quad.  max_blocks = 1: a second quad on 10 threads; a second trip of 10 quads.  max_blocks = 2:
    a full first trip, a second trip whose second quad exists on 100 threads, and a tail.  The library's own host arithmetic agrees."""
    h = L.lib().cdll
    for n in so.ADAM_DEFAULT_N:
        assert so.adam_trips(n) == (0, 0, 0) and so.adam_grid(n) == so.cdiv(n, 256) == h.ofa_adam_step_blocks(n, 0)
    (n1, b1), (n2, b2), (n3, b3) = so.ADAM_CAPPED
    assert so.adam_trips(n1, b1) == (10, 0, 0) and n1 % 4 == 1
    assert so.adam_trips(n2, b2) == (256, 10, 0) and n2 % 4 == 2
    assert so.adam_trips(n3, b3) == (512, 512, 100) and n3 % 4 == 3 and n3 == 6547
    for n, mb in so.ADAM_CAPPED:
        assert h.ofa_adam_step_blocks(n, mb) == so.adam_grid(n, mb) == mb < so.cdiv(n, 256), (n, mb)      # the cap is what cut the grid
        assert so.where(n >> 2, mb * 256) == "past"
        assert len(so.adam_plant_positions(n, mb)) == 2
    assert h.ofa_adam_step_blocks(141_600_000, 0) == so.ADAM_CAP == so.adam_grid(141_600_000) and h.ofa_adam_step_blocks(5, -1) == -1
    assert so.adam_trips(67_108_864)[0] == 0 and so.adam_trips(67_108_868)[0] == 1 and so.adam_trips(134_217_732)[1] == 1
    capped = [c for c in so.ADAM_CASES if c.max_blocks]
    assert {(c.n, c.mode, c.wd) for c in capped if not c.skip} == {(n, m, w) for n, _ in so.ADAM_CAPPED for m in so.ADAM_MODES for w in (0.0, 0.01)}
    assert {c.second for c in capped} == {False, True} and sum(c.skip for c in so.ADAM_CASES) == 1
    assert {c.n for c in so.ADAM_CASES if not c.max_blocks} == set(so.ADAM_DEFAULT_N)
    for b in (0.9, 0.98, 0.999):
        assert float(np.float32(1.0) - np.float32(b)) == 1.0 - so.f32(b)
    with pytest.raises(L.OfaError, match="adam_step"):
        L.lib().call("ofa_adam_step_grid", 4096, 4096, 4096, 4096, 4096, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, L.BF16, -1, None)


# ------------------------------------------------------------------------------------------------------------------ emulations
def _eval(case, dtype, mutation=None):
    b = so.build(case, dtype)
    return so.figures(case, b, so.emulate(case, b, dtype, mutation), dtype)


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
@pytest.mark.parametrize("kernel", so.ONE_ROUNDING)
def test_emulation_stays_within_the_ceiling(kernel, dtype):
    worst = (-1.0, None)
    for case in so.cases_of(kernel):
        fig = _eval(case, dtype)
        assert fig.get("drop", 0.0) == 0.0, case.name
        if fig["y"] > worst[0]:
            worst = (fig["y"], case.name)
    print(f"\n{kernel} {so.NAMES[dtype]}: y {worst[0]:.3g} ({worst[1]})")
    assert worst[0] <= so.limit(kernel, "y", dtype, is_kernel=False), worst


def _applies(mutation, case, dtype):
    o = dict(case.opt)
    return {"second_trip_reads_first_trip": so.case_pos(case, dtype) == "past", "drop_tail": case.tail > 0, "drop_last_vector": case.units > 0,
            "philox_counter_is_thread_index": so.case_pos(case, dtype) == "past" and o.get("p", 0) > 0, "mask_halfword_swapped": o.get("p", 0) > 0,
            "keep_scale_missing": o.get("p", 0) > 0, "b_period_ignored": bool(o.get("period") and o.get("b")),
            "add_n_drops_last_input": o.get("k", 0) > 1, "batch_sum_overwrites": bool(o.get("acc")), "group_off_by_one": True}[mutation]


MUTANTS = [(k, m) for k in so.ONE_ROUNDING for m in so.MUTATIONS[k]]


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
@pytest.mark.parametrize("kernel,mutation", MUTANTS, ids=[f"{k}-{m}" for k, m in MUTANTS])
def test_table_and_metric_catch_the_mutation(kernel, mutation, dtype):
    """The mutated emulation exceeds what the GPU test allows a kernel in at least one case of the table, smallest first; the clean
    emulation of that case is within the ceiling."""
    tried = 0
    for case in sorted(so.cases_of(kernel), key=lambda c: so.case_numel(c, dtype)):
        if not _applies(mutation, case, dtype):
            continue
        tried += 1
        over = {n: v for n, v in _eval(case, dtype, mutation).items() if v > so.limit(kernel, n, dtype)}
        if over:
            assert all(v <= so.limit(kernel, n, dtype, is_kernel=False) for n, v in _eval(case, dtype).items()), case.name
            print(f"\n{kernel} {mutation} {so.NAMES[dtype]}: caught by [{case.name}] through " + ", ".join(f"{n} {v:.3g}" for n, v in over.items()))
            return
    pytest.fail(f"no case of the {kernel} table notices {mutation} in {so.NAMES[dtype]} ({tried} tried)")


@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
@pytest.mark.parametrize("kernel", so.MOVERS)
def test_mover_tables_catch_the_grid_mutations(kernel, dtype):
    """A mover's expected output with a wrong grid-stride loop applied differs in bits from the expected output in some case."""
    for mutation in so.MOVER_MUTATIONS:
        for case in sorted(so.cases_of(kernel), key=lambda c: so.case_numel(c, dtype)):
            if mutation == "second_trip_reads_first_trip" and so.case_pos(case, dtype) != "past":
                continue
            want = so.mover_expected(case, so.build(case, dtype))["out"]
            bad = so.grid_mutate(want.reshape(-1), so.vec_n(case, dtype), so.case_grid(case, dtype) * 256, mutation, float("nan"))
            if not so.same_bits(bad.view_as(want), want):
                print(f"\n{kernel} {mutation} {so.NAMES[dtype]}: caught by [{case.name}]")
                break
        else:
            pytest.fail(f"no case of the {kernel} table notices {mutation} in {so.NAMES[dtype]}")


def test_mask_mutations_change_the_mask():
    for c in so.cases_of("dropout_add"):
        o = dict(c.opt)
        n = so.case_numel(c, BF16)
        clean = so.dropout_mask(n, o["p"], so.SEED, o["offset"] + o["base"])
        if o["p"] > 0 and n >= 2048:
            assert not torch.equal(clean, so.dropout_mask(n, o["p"], so.SEED, o["offset"] + o["base"], "mask_halfword_swapped")), c.name
            assert so.case_pos(c, BF16) != "past" or not torch.equal(
                clean, so.dropout_mask(n, o["p"], so.SEED, o["offset"] + o["base"], "philox_counter_is_thread_index")), c.name


# ------------------------------------------------------------------------------------------------------------------ exact reductions
def test_exact_reduction_inputs_stay_below_two_to_the_24():
    for dt in so.DTYPES3:
        for i, (pos, u, t) in enumerate(so.SUMSQ_SIZES):
            x = so.small_ints(so.sumsq_n(u, t, dt), 100 + i, dt)
            assert so.same_bits(x.double().to(dt), x) and float(x.double().abs().max()) <= 2
            total = int((x.long() ** 2).sum())
            assert total + 7 < 2 ** 24 and float((x.float() ** 2).sum()) == total                  # (an upper bound on every partial sum)
            if pos == "past" and dt == BF16:
                assert 4.1e6 < total < 4.3e6
    assert max(so.COLSUM_ROWS) * 2 + 7 < 2 ** 24 and max(so.REDUCE_N) * 2 < 2 ** 24
    assert so.sumsq_chain(BF16) == 41 and so.sumsq_chain(F32) == 33 and so.COLSUM_CHAIN == 43


# ------------------------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("dtype", so.DTYPES3, ids=IDS)
def test_adam_emulation_stays_within_its_limits(dtype):
    worst = {}
    for case in so.ADAM_CASES:
        b = so.build_adam(case, dtype)
        for n, v in so.adam_figures(b, so.adam_emulate(b, dtype, case.max_blocks)).items():
            if v > worst.get(n, (-1.0, None))[0]:
                worst[n] = (v, case.name)
    print(f"\nadam {so.NAMES[dtype]}: " + "; ".join(f"{n} {v:.3g} ({w})" for n, (v, w) in sorted(worst.items())))
    for n, (v, w) in worst.items():
        assert v <= so.adam_limit(n, is_kernel=False), (n, v, w)


# (the fp32 gradient is loaded as one float4: it has no pair to unpack)
ADAM_MUTANTS = [(m, d) for m in so.ADAM_MUTATIONS for d in so.DTYPES3 if not (m == "quad_high_pair_takes_low_pair" and d == F32)]


@pytest.mark.parametrize("mutation,dtype", ADAM_MUTANTS, ids=[f"{m}-{so.NAMES[d]}" for m, d in ADAM_MUTANTS])
def test_adam_table_catches_the_mutation(mutation, dtype):
    for case in so.ADAM_CASES:
        if case.skip or (mutation == "tail_skips_weight_decay" and not (case.wd and case.n % 4)):
            continue
        b = so.build_adam(case, dtype)
        over = {n: v for n, v in so.adam_figures(b, so.adam_emulate(b, dtype, case.max_blocks, mutation)).items() if v > so.adam_limit(n)}
        if over:
            if mutation == "second_quad_takes_first_gradient":
                assert case.max_blocks, case.name                        # only a capped grid can see it
            print(f"\nadam {mutation} {so.NAMES[dtype]}: caught by [{case.name}] through " + ", ".join(f"{n} {v:.3g}" for n, v in over.items()))
            return
    pytest.fail(f"no Adam case notices {mutation} in {so.NAMES[dtype]}")
