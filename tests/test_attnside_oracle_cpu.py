"""CPU: the attention-side oracle (tests/attnside_oracle.py) is sound before a GPU is touched -- every case lies where its name says
against the restated launch arithmetic (the NI ladder, 4 rows per block, the 4096- and 1024-block caps, the decode keys per iteration
and the 64 KB LDS line, the 64-column / 32-head chunks, the V = 4 condition), the float32 emulations stay within the ceiling against
float64 over every table and dtype, and every named mutation is caught by a case of the table in every dtype it can occur in (a figure
over the kernel's limit, or a bit mismatch for the movers and the integer reductions).  Run with -s for the measured ceilings and the
case that catches each mutation."""
import pytest
import torch

from ofasys_amd import lib as L
from tests import attnside_oracle as ao

BF16, FP16, F32 = ao.BF16, ao.FP16, ao.F32
IDS = [ao.NAMES[d] for d in ao.DTYPES3]
D16 = (BF16, FP16)


def of(kernel):
    return [c for c in ao.SM_CASES if c.kernel == kernel]


# ------------------------------------------------------------------------------------------------------------------ where the cases lie
def test_softmax_cases_lie_where_their_names_say():
    assert [ao.sm_ni(sk) for sk in ao.SM_SK] == [1, 1, 1, 2, 4, 8, 16, 32, 32, 64, 64]
    assert [ao.sm_ni(sk) for sk in (64, 128, 256, 512, 1024, 2048, 4096)] == list(ao.SM_LADDER)      # the top of every rung
    names = [c.name for c in ao.SM_CASES]
    assert len(set(names)) == len(names) and len({c.seed for c in ao.SM_CASES}) == len(names)
    for k in ao.SM_FWD + ao.SM_BWD:
        causal = k in ("sm_causal", "sm_bwd_causal")
        assert {c.sk for c in of(k)} >= set(ao.SM_SK[:-1] if causal else ao.SM_SK), k
        assert {ao.sm_ni(c.sk) for c in of(k)} == set(ao.SM_LADDER), k                              # NI = 32 and NI = 64 run
        assert {c.regime for c in of(k)} == set(ao.REGIMES), k
        for c in of(k):
            assert f"NI{ao.sm_ni(c.sk)} " in c.name and c.sk <= 4096
            if not causal and not dict(c.opt).get("causal"):
                assert ao.sm_idle_waves(ao.sm_rows(c)) > 0, c.name                                  # waves of the last block return early
            if causal:
                assert c.sq == c.sk and c.np == 1
        if causal:
            big = [c for c in of(k) if c.sk in (1025, 2049)]
            assert len(big) == 2 and all(c.b == 1 and ao.sm_idle_waves(ao.sm_rows(c)) == 3 for c in big)
            assert any(c.b > 1 and c.sk > 1 for c in of(k))                                          # row % sq differs from the row
    assert all((c.b, c.np) in ((2, 3), (1, 5)) for c in of("sm_plain")) and {c.b for c in of("sm_plain")} == {1, 2}
    assert {dict(c.opt)["mask_b"] for c in of("sm_masked")} == {1, 2} and all(c.b == 2 and c.np == 3 for c in of("sm_masked"))
    assert any(c.sq > 1 and dict(c.opt)["mask_b"] == m for c in of("sm_masked") for m in (1, 2))
    assert {dict(c.opt)["inplace"] for c in of("sm_bwd")} == {0, 1} == {dict(c.opt)["inplace"] for c in of("sm_bwd_causal")}
    attn = [dict(c.opt) for c in of("sm_attn")]
    assert {(o["causal"], o["kpm"], o["bias"]) for o in attn} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert sorted(o["special"] for o in attn if "special" in o) == ["nan_score", "padded_batch"]
    assert all(c.b == 2 and c.np == 3 for c in of("sm_attn"))
    for dt in ao.DTYPES3:
        for c in of("sm_attn") + of("sm_masked"):
            b = ao.build_sm(c, dt)
            nanrow = ao.sm_reference(c, b)[2]
            if dict(c.opt).get("special") == "padded_batch":
                assert nanrow.tolist() == [False] * 9 + [True] * 9                                   # sample 1, all three heads
            else:
                assert not bool(nanrow.any()), c.name
            if dict(c.opt).get("special") == "nan_score":
                assert int(torch.isnan(b["x"]).sum()) == 3
            if c.kernel == "sm_masked" and dict(c.opt)["mask_b"] == 2:
                assert bool(b["mask"][1, 0].all()) and not bool(b["mask"][0, 0].all())              # one fully masked row
            if b["kpm"] is not None and c.sk > 1:
                assert not torch.equal(b["kpm"][0], b["kpm"][1])
        # fp32: finite t - max >= -80, so that expf's underflow stays out of it
        for c in ao.SM_CASES:
            if c.kernel in ao.SM_FWD:
                t, _, _ = ao._sm_scores(c, ao.build_sm(c, dt), torch.float64)
                t = torch.where(t <= -10000.0, torch.full_like(t, float("-inf")), t)                 # (the -10000 fill is meant to vanish)
                m = t.amax(-1, keepdim=True)
                gap = (t - m)[torch.isfinite(t - m)]
                assert gap.numel() == 0 or float(gap.min()) >= -80.0, (c.name, float(gap.min()))


def test_decode_cases_lie_where_their_names_say():
    assert (ao.dec_kpi(BF16), ao.dec_kpi(FP16), ao.dec_kpi(F32)) == (32, 32, 16)
    assert (ao.dec_last_under(BF16), ao.dec_last_under(FP16), ao.dec_last_under(F32)) == (14336, 14336, 15360)
    for dt in ao.DTYPES3:
        under, kpi = ao.dec_last_under(dt), ao.dec_kpi(dt)
        assert ao.dec_lds(under, dt) == ao.LDS_LINE < ao.dec_lds(under + 1, dt) == ao.LDS_LINE + 16
        assert ao.dec_lds(ao.DEC_CAP, dt) == (ao.DEC_CAP + kpi * 64) * 4 <= 160 * 1024               # the CU's 160 KB hold the cap
        S = [ao.dec_S(c, dt) for c in ao.DEC_CASES]
        assert set(S) >= {1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513, under, under + 1, ao.DEC_CAP}
        assert {s % kpi for s in S} >= {0, 1, kpi - 1} and {s % 256 for s in S} >= {0, 1, 255}     # key groups; the exp loop's stride
        assert {s % 4 for s in S} == {0, 1, 3} or {s % 4 for s in S} == {0, 1, 2, 3}                 # `red` sits at pad4(S)
        for c in ao.DEC_CASES:
            s = ao.dec_S(c, dt)
            assert (c.B, c.heads) == ((2, 3) if s <= 513 else (1, 1)), c.name
    cs = ao.DEC_CASES
    assert {c.c for c in cs} == {"none", "same", "f32"} and {c.bias for c in cs} == {True, False} == {c.kpm for c in cs} == {c.strided for c in cs}
    assert sum(c.special == "masked_row" for c in cs) == 1 and len({c.name for c in cs}) == len(cs)
    # S = 32 769 is refused before anything is launched (argument validation: runs without a GPU)
    for dt in (L.F32, L.BF16, L.F16):
        with pytest.raises(L.OfaError, match="exceeds the LDS score buffer"):
            L.lib().call("ofa_attn_decode", 4096, 4096, 4096, None, None, None, L.F32, 4096, None, 1, 1, 64, ao.DEC_CAP + 1, 64, 64 * (ao.DEC_CAP + 1),
                         0, 0.125, dt, None)


def test_bias_cases_lie_where_their_names_say():
    for c in ao.BLK_CASES:
        assert ao.where(ao.blk_work(c), ao.bias_grid(ao.blk_work(c)) * 256) == c.pos, c.name
        assert c.start + c.n <= c.T
    for k in ao.BLOCK_KERNELS:
        mine = [c for c in ao.BLK_CASES if c.kernel == k]
        assert {c.pos for c in mine} == {"below", "at", "past"}
        assert any(ao.blk_work(c) == ao.BIAS_T and c.A == 4 and c.n == 512 for c in mine)
        past = [c for c in mine if c.pos == "past"]
        assert [(c.B, c.A, c.n, c.T, c.start, ao.blk_work(c) - ao.BIAS_T) for c in past] == [(1, 1, 1025, 1030, 3, 2049)]
        assert any(c.start + c.n == c.T for c in mine) and any(c.start == 0 for c in mine) and any(c.B == 2 and c.A == 3 and c.n == 5 for c in mine)
    g = ao.GRAD_CASES
    assert {c.n for c in g} == {1, 63, 64, 65, 130} and {c.A for c in g} == {1, 12, 32, 33, 40} and {c.B for c in g} == {1, 3}
    assert all(c.start % 2 == 1 and c.T > c.start + c.n for c in g)
    assert {ao.grad_chunks(c.n, c.A) for c in g} >= {(1, 1, 1), (1, 63, 1), (1, 64, 1), (2, 1, 2), (3, 2, 2), (1, 64, 2), (2, 1, 1), (1, 1, 2)}
    for dt in ao.DTYPES3:
        v = [(ao.outer_case_v(c, dt), ao.outer_col_trips(c.P, ao.outer_case_v(c, dt))) for c in ao.OUTER_CASES]
        assert v == [(4, 1), (4, 2), (1, 1), (1, 2), (1, 1)], v
    by_shape, by_align = ao.OUTER_CASES[0], ao.OUTER_CASES[4]
    assert by_shape._replace(name="", offset=1, seed=0) == by_align._replace(name="", seed=0)       # all multiples of 4: only the pointer differs
    assert all(c.start + c.F * c.P <= c.T for c in ao.OUTER_CASES)
    # the existing P = 196 case (start 0, T 1600) is V = 4 with one trip: the V = 1 second trip never ran there
    assert ao.outer_v(0, 1600, 196, 0) == 4 and ao.outer_col_trips(196, 4) == 1


def test_aux_cases_lie_where_their_names_say():
    for c in ao.MEAN_CASES:
        assert ao.where(c.n, ao.mean_grid(c.n) * 256) == c.pos, c.name
    assert {c.pos for c in ao.MEAN_CASES} == {"below", "at", "past"} and {c.heads for c in ao.MEAN_CASES} == {1, 3, 16}
    assert any(c.n == ao.MEAN_T + 300 for c in ao.MEAN_CASES) and ao.MEAN_T == 262144
    t = ao.TR_CASES
    assert {c.T for c in t} == {1, 63, 64, 65} and {c.C for c in t} == {64, 65, 130}
    assert {c.ld - c.C for c in t} == {0, 3} and all(c.Tpad >= c.T for c in t)
    for T in (1, 63, 64, 65):
        assert {c.Tpad for c in t if c.T == T} == {T, ao.pad32(T), T + 70}
    assert any(ao.cdiv(c.Tpad, 64) > ao.cdiv(c.T, 64) for c in t)                                     # whole blocks with t0 >= T
    d = ao.DELTA_CASES
    assert all((c.B * c.T * c.heads) % 32 for c in d) and any(c.Tpad > c.T for c in d) and any(c.B * c.T * c.heads > 32 for c in d)
    assert [c.B * c.T for c in ao.CG_CASES] == [5, 1024, 1030, 2500] and [ao.cgrad_trips(c.B * c.T) for c in ao.CG_CASES] == [1, 1, 2, 3]
    assert any(c.ld > c.T for c in ao.CG_CASES) and {c.acc for c in ao.CG_CASES} == {0, 1}


# ------------------------------------------------------------------------------------------------------------------ emulations
def _sm_eval(case, dtype, mutation=None):
    b = ao.build_sm(case, dtype)
    got = (ao.sm_bwd_emulate if case.kernel in ao.SM_BWD else ao.sm_emulate)(case, b, dtype, mutation)
    return ao.sm_figures(case, b, got, dtype)


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
@pytest.mark.parametrize("kernel", ao.SM_FWD + ao.SM_BWD)
def test_softmax_emulation_stays_within_the_ceiling(kernel, dtype):
    worst = (-1.0, None)
    for case in of(kernel):
        fig = _sm_eval(case, dtype)["y"]
        if fig > worst[0]:
            worst = (fig, case.name)
    print(f"\n{kernel} {ao.NAMES[dtype]}: y {worst[0]:.3g} ({worst[1]})")
    assert worst[0] <= ao.limit(kernel, dtype, is_kernel=False), worst


SM_MUTANTS = [(k, m) for k in ao.SM_FWD + ao.SM_BWD for m in ao.SM_MUTATIONS[k]]


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
@pytest.mark.parametrize("kernel,mutation", SM_MUTANTS, ids=[f"{k}-{m}" for k, m in SM_MUTANTS])
def test_softmax_table_catches_the_mutation(kernel, mutation, dtype):
    tried = 0
    for case in sorted(of(kernel), key=lambda c: ao.sm_rows(c) * c.sk):
        if not ao.sm_applies(mutation, case, dtype):
            continue
        tried += 1
        fig = _sm_eval(case, dtype, mutation)["y"]
        if fig > ao.limit(kernel, dtype):
            assert _sm_eval(case, dtype)["y"] <= ao.limit(kernel, dtype, is_kernel=False), case.name
            print(f"\n{kernel} {mutation} {ao.NAMES[dtype]}: caught by [{case.name}] through y {fig:.3g}")
            return
    pytest.fail(f"no case of the {kernel} table notices {mutation} in {ao.NAMES[dtype]} ({tried} tried)")


def test_upper_registers_are_seen_at_every_rung():
    """Dropping the registers beyond NI / 2 is noticed at NI = 32 and NI = 64 themselves, forward and backward, not only at a small rung."""
    for k in ao.SM_FWD + ao.SM_BWD:
        for ni in (32, 64):
            case = next(c for c in of(k) if ao.sm_ni(c.sk) == ni)
            assert _sm_eval(case, BF16, "upper_registers_dropped")["y"] > ao.TOL, case.name


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_decode_emulation_and_mutations(dtype):
    worst, caught = {"out": (-1.0, None), "probs": (-1.0, None)}, {}
    for case in sorted(ao.DEC_CASES, key=lambda c: ao.dec_S(c, dtype)):
        b = ao.build_dec(case, dtype)
        for n, v in ao.dec_figures(case, b, ao.dec_emulate(case, b, dtype), dtype).items():
            if v > worst[n][0]:
                worst[n] = (v, case.name)
        for m in ao.DEC_MUTATIONS:
            if m in caught or not ao.dec_applies(m, case, dtype):
                continue
            over = {n: v for n, v in ao.dec_figures(case, b, ao.dec_emulate(case, b, dtype, m), dtype).items() if v > ao.limit("decode", dtype)}
            if over:
                caught[m] = (case.name, over)
    print(f"\ndecode {ao.NAMES[dtype]}: " + "; ".join(f"{n} {v:.3g} ({w})" for n, (v, w) in worst.items()))
    for m, (name, over) in caught.items():
        print(f"decode {m} {ao.NAMES[dtype]}: caught by [{name}] through " + ", ".join(f"{n} {v:.3g}" for n, v in over.items()))
    assert all(v <= ao.limit("decode", dtype, is_kernel=False) for v, _ in worst.values()), worst
    assert set(caught) == set(ao.DEC_MUTATIONS), set(ao.DEC_MUTATIONS) - set(caught)
    assert "out" in caught["c_attn_omitted"][1] and "probs" in caught["last_partial_key_group_dropped"][1]


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_bias_block_emulation_and_mutations(dtype):
    for k in ("block_add", "block_add_batch"):
        worst, caught = (-1.0, None), {}
        for case in [c for c in ao.BLK_CASES if c.kernel == k]:
            b = ao.build_blk(case, dtype)
            fig = ao.blk_figures(case, b, ao.blk_emulate(case, b, dtype), dtype)
            assert fig["rest"] == 0.0, case.name
            if fig["y"] > worst[0]:
                worst = (fig["y"], case.name)
            for m in ao.BLOCK_MUTATIONS[k]:
                if m not in caught and ao.blk_applies(m, case, dtype):
                    f = ao.blk_figures(case, b, ao.blk_emulate(case, b, dtype, m), dtype)
                    if f["y"] > ao.limit(k, dtype) or f["rest"] > 0:
                        caught[m] = case.name
        print(f"\n{k} {ao.NAMES[dtype]}: y {worst[0]:.3g} ({worst[1]}); caught: {caught}")
        assert worst[0] <= ao.limit(k, dtype, is_kernel=False), worst
        assert set(caught) == set(ao.BLOCK_MUTATIONS[k]), set(ao.BLOCK_MUTATIONS[k]) - set(caught)
        assert "past" in caught["second_trip_skipped"]


@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_mean_heads_and_delta_emulation_and_mutations(dtype):
    worst, caught = (-1.0, None), {}
    for case in ao.MEAN_CASES:
        b = ao.build_mean(case, dtype)
        ref, bd = ao.mean_reference(case, b)
        fig = ao.grad_excess(ao.mean_emulate(case, b, dtype), ref, bd, dtype)
        if fig > worst[0]:
            worst = (fig, case.name)
        for m in ao.MEAN_MUTATIONS:
            if m not in caught and ao.mean_applies(m, case) and ao.grad_excess(ao.mean_emulate(case, b, dtype, m), ref, bd, dtype) > ao.limit("mean_heads", dtype):
                caught[m] = case.name
    print(f"\nmean_heads {ao.NAMES[dtype]}: y {worst[0]:.3g} ({worst[1]}); caught: {caught}")
    assert worst[0] <= ao.limit("mean_heads", dtype, is_kernel=False) and set(caught) == set(ao.MEAN_MUTATIONS), (worst, caught)
    if dtype == F32:
        return                                                                                   # (attn_bwd_prep takes the 16-bit types only)
    worst, caught = (-1.0, None), {}
    for case in ao.DELTA_CASES:
        b = ao.build_delta(case, dtype)
        fig = ao.delta_figures(case, b, ao.delta_emulate(case, b))
        assert fig["tail"] == 0.0
        if fig["y"] > worst[0]:
            worst = (fig["y"], case.name)
        for m in ao.DELTA_MUTATIONS:
            f = ao.delta_figures(case, b, ao.delta_emulate(case, b, m))
            if m not in caught and (f["y"] > ao.limit("delta", dtype) or f["tail"] > 0):
                caught[m] = case.name
    print(f"delta {ao.NAMES[dtype]}: y {worst[0]:.3g} ({worst[1]}); caught: {caught}")
    assert worst[0] <= ao.limit("delta", dtype, is_kernel=False) and set(caught) == set(ao.DELTA_MUTATIONS), (worst, caught)


# ------------------------------------------------------------------------------------------------------------------ movers, exact reductions
@pytest.mark.parametrize("dtype", ao.DTYPES3, ids=IDS)
def test_mover_and_integer_tables_catch_their_mutations(dtype):
    """The expected bits with one mutation applied differ from the expected bits in some case of the table."""
    def sweep(label, mutations, cases, applies, clean, mutated):
        for m in mutations:
            hit = next((c.name for c in cases if applies(m, c) and not all(
                ao.same_bits(x, y) for x, y in zip(clean(c), mutated(c, m)))), None)
            assert hit, f"no case of the {label} table notices {m} in {ao.NAMES[dtype]}"
            print(f"\n{label} {m} {ao.NAMES[dtype]}: caught by [{hit}]")

    sl = [c for c in ao.BLK_CASES if c.kernel == "block_slice"]
    sweep("block_slice", ao.BLOCK_MUTATIONS["block_slice"], sl, lambda m, c: ao.blk_applies(m, c, dtype),
          lambda c: [ao.blk_slice_expected(c, ao.build_blk(c, dtype))], lambda c, m: [ao.blk_slice_expected(c, ao.build_blk(c, dtype), m)])
    sweep("transpose_heads", ao.TR_MUTATIONS, ao.TR_CASES, ao.tr_applies,
          lambda c: [ao.tr_expected(c, ao.build_tr(c, dtype))], lambda c, m: [ao.tr_expected(c, ao.build_tr(c, dtype), m)])
    sweep("block_grad", ao.GRAD_MUTATIONS, ao.GRAD_CASES, ao.grad_applies,
          lambda c: [ao.grad_expected(c, ao.build_grad(c, dtype), dtype)], lambda c, m: [ao.grad_expected(c, ao.build_grad(c, dtype), dtype, m)])
    sweep("outer_grad", ao.OUTER_MUTATIONS, ao.OUTER_CASES, lambda m, c: ao.outer_applies(m, c, dtype),
          lambda c: list(ao.outer_expected(c, ao.build_outer(c, dtype), dtype).values()),
          lambda c, m: list(ao.outer_expected(c, ao.build_outer(c, dtype), dtype, m).values()))
    sweep("c_attn_grad", ao.CG_MUTATIONS, ao.CG_CASES, ao.cg_applies,
          lambda c: [ao.cg_expected(c, ao.build_cg(c, dtype), dtype)], lambda c, m: [ao.cg_expected(c, ao.build_cg(c, dtype), dtype, m)])


def test_integer_reductions_are_exact_and_randn_ones_within_their_chain():
    """Integers in [-2, 2]: every partial sum stays below 2^24 and the fp32 sum is the integer sum; the expected 16-bit output is that
    integer rounded once.  The randn cases: the fp32 restatement against float64 within the chain bound."""
    for dt in ao.DTYPES3:
        for c in ao.GRAD_CASES:
            b = ao.build_grad(c, dt)
            blk = b["dbias"][:, :, c.start:c.start + c.n, c.start:c.start + c.n]
            assert float(blk.double().abs().max()) <= 2 and ao.same_bits(blk.double().to(dt), blk)
            assert ao.same_bits(ao.grad_expected(c, b, dt), blk.double().sum(0).permute(1, 2, 0).contiguous().to(dt))
            r = ao.build_grad(c, dt, randn=True)
            rb = r["dbias"][:, :, c.start:c.start + c.n, c.start:c.start + c.n].double()
            fig = ao.grad_excess(ao.grad_expected(c, r, dt), rb.sum(0).permute(1, 2, 0), rb.abs().sum(0).permute(1, 2, 0), dt)
            assert fig <= ao.reduction_limit(c.B, dt, is_kernel=False), (c.name, fig)
        for c in ao.OUTER_CASES:
            b, n = ao.build_outer(c, dt), c.F * c.P
            blk = b["G"][:, c.start:c.start + n, c.start:c.start + n].double().view(c.A, c.F, c.P, c.F, c.P)
            assert float(blk.abs().sum((2, 4)).max()) < 2 ** 24 and float(blk.abs().sum((1, 3)).max()) < 2 ** 24
            e = ao.outer_expected(c, b, dt)
            assert ao.same_bits(e["frames"], blk.sum((2, 4)).permute(1, 2, 0).contiguous().to(dt))
            assert ao.same_bits(e["patches"], blk.sum((1, 3)).permute(1, 2, 0).contiguous().to(dt))
        for c in ao.CG_CASES:
            b = ao.build_cg(c, dt)
            d = b["delta"].view(c.B, c.heads, c.ld)
            assert bool(torch.isnan(d[:, :, c.T:]).all()) and float(d[:, :, :c.T].abs().sum()) + 3 < 2 ** 24
            want = d[:, :, :c.T].double().sum((0, 2)) / b["c"].double() + (b["prev"].double() if c.acc else 0.0)
            assert ao.same_bits(ao.cg_expected(c, b, dt), want.to(dt)), c.name
            r = ao.build_cg(c, dt, randn=True)
            ref, bd = ao.cg_reference(c, r)
            assert ao.grad_excess(ao.cg_expected(c, r, dt), ref, bd, dt) <= ao.reduction_limit(ao.CG_CHAIN, dt, is_kernel=False), c.name
    assert ao.CG_CHAIN == 27 and ao.outer_chain(ao.OUTER_CASES[1], F32) == 65 * 2 * 4 + 9
