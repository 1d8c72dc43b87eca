"""CPU: the attention oracle (tests/attn_oracle.py) is sound before a GPU is touched -- the float32 emulation of the kernels' roundings
stays under EMUL_CEILING against the float64 reference over the whole table, the planted inputs reach the online softmax's branches by
construction, and the table + metric catch each named mutation of the emulation at the tolerance the GPU tests use."""
import pytest
import torch

from tests import attn_oracle as ao

DTYPES = [torch.bfloat16, torch.float16]
GROUPS = {f"T{T}": ao.seam_cases(T) for T in ao.SEAM_T}
GROUPS["regimes"] = ao.REGIME_CASES + ao.EXTRA_CASES


def _run(case, dtype, **emu):
    x, kw = ao.build_inputs(case, dtype)
    args = (x["q"], x["k"], x["v"], x["dout"], ao.HEADS, ao.SCALE)
    ref, bd, ones = ao.reference_and_bounds(*args, **kw)
    em = ao.emulate(*args, dtype=dtype, **kw, **emu)
    return args, kw, ref, bd, ones, em


def _fp32_errors(args, kw, ref, em):
    """|error| of the emulation's float32 lse / delta / shared dbias against float64 (delta and dbias with the SAME stored out)."""
    ref2 = ao.reference(*args, out=em["out"], **kw)
    e = dict(lse=float((em["lse"].double() - ref["lse"]).abs().max()), delta=float((em["delta"].double() - ref2["delta"]).abs().max()))
    if em["dbias"] is not None and em["dbias"].dtype == torch.float32:
        e["dbias32"] = float((em["dbias"].double() - ref2["dbias"]).abs().max())
    return e


def test_table_is_the_one_the_issue_asks_for():
    assert set(ao.CASES) >= set(c for T in ao.SEAM_T for c in ao.seam_cases(T)) and len(set(ao.CASES)) == len(ao.CASES)
    plain = {(c.T, c.S, c.causal) for c in ao.CASES if c.regime == "sharp" and c.bias == "none"}
    assert plain >= {(T, S, causal) for T in ao.SEAM_T for S in ao.SEAM_S for causal in (False, True)}
    for mode in ("dense", "shared", "shared_big"):
        have = {(c.T, c.S, c.causal) for c in ao.CASES if c.bias == mode}
        assert have >= {(T, S, causal) for T in ao.SEAM_T for S in (33, 65, 97) for causal in (False, True)}, mode
    assert all(c.kpm == (c.S >= 34) for T in ao.SEAM_T for c in ao.seam_cases(T))
    assert {c.c for c in ao.CASES} == set(ao.C_MODES)
    assert ao.TOL == 2 * ao.EMUL_CEILING


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_emulation_stays_within_the_ceiling(group, dtype):
    """excess(emulate, reference, bounds) <= EMUL_CEILING for every 16-bit output of every table entry, both types; the float32
    outputs of the emulation stay within 1/8 of the absolute tolerances the GPU tests use."""
    worst, w32 = {}, {}
    for case in GROUPS[group]:
        args, kw, ref, bd, ones, em = _run(case, dtype)
        for n, e in ao.check16(em, ref, bd, ones, dtype).items():
            if e > worst.get(n, (-1.0, None))[0]:
                worst[n] = (e, case)
        for n, e in _fp32_errors(args, kw, ref, em).items():
            w32[n] = max(w32.get(n, 0.0), e)
    print(group, dtype, {n: round(e, 3) for n, (e, _) in worst.items()}, {n: f"{e:.2e}" for n, e in w32.items()})
    for n, (e, case) in worst.items():
        assert e <= ao.EMUL_CEILING, (n, e, case)
    assert 8 * w32["lse"] <= ao.LSE_TOL and 8 * w32["delta"] <= ao.DELTA_TOL and 8 * w32.get("dbias32", 0.0) <= ao.DBIAS32_TOL, w32


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fp16_list_stays_within_the_ceiling_too(dtype):
    for case in ao.FP16_CASES:
        if case in GROUPS["regimes"] or case in GROUPS.get(f"T{case.T}", ()):
            continue                                # (already measured above)
        args, kw, ref, bd, ones, em = _run(case, dtype)
        for n, e in ao.check16(em, ref, bd, ones, dtype).items():
            assert e <= ao.EMUL_CEILING, (n, e, case)
        for n, e in _fp32_errors(args, kw, ref, em).items():
            assert 8 * e <= dict(lse=ao.LSE_TOL, delta=ao.DELTA_TOL, dbias32=ao.DBIAS32_TOL)[n], (n, e, case)


@pytest.mark.parametrize("regime,want", [("uniform", dict(norescale=0)), ("plant_first", dict(norescale=80)), ("stairs", dict(big=80)),
                                         ("plant_last", dict())])
def test_planted_inputs_reach_the_branches_by_construction(regime, want):
    """T = S = 160, B = heads = 2: 5 waves x 4 key blocks behind the first x 4 (sample, head) = 80 steps.  uniform never takes the
    no-rescale branch, plant_first takes it in every step of every wave, stairs rescales every row by >= 2^8 in every step; and the
    blockwise form computes what the one-shot form computes (within the ceiling, both against float64)."""
    case = ao.Case(regime, 160, 160, False, "none", False, "f32", 4000)
    args, kw, ref, bd, ones, em = _run(case, torch.bfloat16, blockwise=True)
    st = em["stats"]
    print(regime, st)
    assert st["steps"] == 80
    for n, v in want.items():
        assert st[n] == v, (regime, st)
    for n, e in ao.check16(em, ref, bd, ones, torch.bfloat16).items():
        assert e <= ao.EMUL_CEILING, (n, e)
    # the same inputs inside the table's regime cases (whatever bias they carry) keep the property the GPU run relies on
    for c in ao.REGIME_CASES:
        if c.regime == regime and not c.causal and c.bias == "none":
            s2 = _run(c, torch.bfloat16, blockwise=True)[5]["stats"]
            if regime == "plant_first":
                assert s2["norescale"] == s2["steps"] > 0, (c, s2)
            if regime == "stairs":
                assert s2["big"] == s2["steps"] > 0, (c, s2)


def _applies(mutation, case):
    if mutation == "drop_last_key":
        return not case.causal and not case.kpm and case.S > 1
    if mutation in ("diag_hidden", "diag_leak"):
        return case.causal and min(case.T, case.S) > 1 and (mutation == "diag_hidden" or min(case.T, case.S) % 32 != 1)
    if mutation == "skip_alpha":
        return case.S > 32
    if mutation == "kpm_shift":
        return case.kpm
    return case.bias in ("shared", "shared_big")     # lse_off


@pytest.mark.parametrize("mutation", ao.MUTATIONS)
def test_table_and_metric_catch_the_mutation(mutation):
    """Each subtly wrong variant of the emulation exceeds the GPU tolerance in at least one table entry (while the unmutated blockwise
    emulation of that entry stays under the ceiling).  lse_off -- one row's lse 1e-3 too large, fed to the backward -- moves P by a
    RELATIVE 1e-3 = 0.26 bf16 eps, which no 16-bit output can show against a bound it is itself relative to; the fp32 shared-bias
    gradient and its absolute tolerance are what catch it."""
    dtype, caught = torch.bfloat16, []
    for case in ao.CASES:
        if not _applies(mutation, case):
            continue
        args, kw, ref, bd, ones, em = _run(case, dtype, blockwise=True, mutation=mutation)
        ex = ao.check16(em, ref, bd, ones, dtype)
        over = {n: e for n, e in ex.items() if e > ao.TOL}
        if mutation == "lse_off":
            ref2 = ao.reference(*args, out=em["out"], **kw)
            e32 = float((em["dbias"].double() - ref2["dbias"]).abs().max())
            over = {"dbias32": e32} if e32 > ao.DBIAS32_TOL else {}
        if over:
            clean = ao.emulate(*args, dtype=dtype, blockwise=True, **kw)
            assert all(e <= ao.EMUL_CEILING for e in ao.check16(clean, ref, bd, ones, dtype).values()), case
            caught.append((case, over))
            if len(caught) >= 3:
                break
    print(mutation, caught[:1])
    assert caught, f"no table entry notices {mutation}: the table is missing a case"
